"""Helpers of the boundary tests (test_boundary_types_cpu.py,
test_boundary_python_cpu.py): include/lavish_dsp.h as the C compiler sees it,
and the reference's RTCD prototypes generated next to it.

Nothing here is kept: the reference's own build/cmake/rtcd.pl writes its two
RTCD headers and this module writes the config header they need into a
directory the caller names (a pytest temporary directory), and the checks are
C translation units compiled there with the host gcc.

* rtcd_headers(tmp)             config/aom_config.h, config/aom_dsp_rtcd.h and
                                config/av1_rtcd.h under tmp (reference needed)
* header_text() / preprocessed() the product header, its #include lines taken
                                out, after the C preprocessor
* structs(pre)                  every `typedef struct LavishX {...} LavishX;`
                                as (name, [(field, array lengths)])
* prototypes(pre)               every function prototype as
                                (name, return type, [argument types])
* check_prototypes(tmp, pre)    names whose `_c` and `_hip` types differ
* check_mirrors(tmp, pre)       field-by-field layout differences of the five
                                mirror structs
* probe_layout(tmp, pre)        size and per-field offset, size, array lengths
                                and kind of every struct, from a compiled probe
                                (header only: no reference needed)
* probe_scalar_types(tmp, ts)   kind and size of arithmetic C type names
"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "lavish_dsp.h")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")

# mirror struct of the header -> (the reference's type, the header defining it)
MIRRORS = {
    "LavishTxfmParam": ("TxfmParam", "aom_dsp/txfm_common.h"),
    "LavishConvolveParams": ("ConvolveParams", "av1/common/convolve.h"),
    "LavishInterpFilterParams": ("InterpFilterParams", "av1/common/filter.h"),
    "LavishDistWtdCompParams": ("DIST_WTD_COMP_PARAMS", "av1/common/blockd.h"),
    "LavishNNConfig": ("struct NN_CONFIG", "av1/encoder/ml.h"),
}


def have_reference():
    return os.path.isdir(os.path.join(REF, "av1"))


def _run(cmd, **kw):
    return subprocess.run(cmd, capture_output=True, text=True, **kw)


# ------------------------------------------------------------ the header --
def header_text():
    with open(HEADER) as f:
        return f.read()


def preprocessed(text=None):
    """The header's own declarations after the preprocessor (prototype macros
    expanded, comments gone); <stddef.h> / <stdint.h> are left to the unit
    that uses the text."""
    text = header_text() if text is None else text
    text = re.sub(r"(?m)^\s*#\s*include\s*<[^>]+>\s*$", "", text)
    r = _run(["gcc", "-E", "-P", "-x", "c", "-"], input=text)
    assert r.returncode == 0, r.stderr
    return r.stdout


_STRUCT_RE = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")


def structs(pre):
    """[(name, [(field, [array lengths]), ...])] of every struct the header
    defines, fields in declaration order, read from the struct's own body."""
    out = []
    for m in _STRUCT_RE.finditer(pre):
        assert m.group(1) == m.group(3), m.group(0)
        fields = []
        for decl in m.group(2).split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for k, d in enumerate(decl.split(",")):
                dm = re.search(r"(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)$", d.strip())
                assert dm, decl
                dims = [int(v, 0) for v in re.findall(r"\[\s*(\w+)\s*\]", dm.group(2))]
                fields.append((dm.group(1), dims))
        out.append((m.group(1), fields))
    return out


def _split_args(s):
    args, depth, cur = [], 0, ""
    for ch in s:
        if ch == "," and depth == 0:
            args.append(cur)
            cur = ""
            continue
        depth += ch in "(["
        depth -= ch in ")]"
        cur += ch
    if cur.strip():
        args.append(cur)
    return [a.strip() for a in args]


def prototypes(pre):
    """{name: (return type, [argument declarations])} of every function the
    header declares (no function-pointer arguments occur in it)."""
    body = _STRUCT_RE.sub(";", pre)
    body = re.sub(r"\benum\s*\{[^{}]*\}\s*;", ";", body)
    out = {}
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if "(" not in stmt:
            assert not stmt or stmt.startswith("typedef struct"), stmt
            continue
        m = re.fullmatch(r"(.*?)(\w+) ?\((.*)\)", stmt)
        assert m and "(" not in m.group(3), stmt
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in out, name
        out[name] = (ret, [] if args in ("void", "") else _split_args(args))
    return out


def hip_names(pre):
    """Reference names (no suffix) of the `_hip` shims the header declares."""
    return sorted(n[:-4] for n in prototypes(pre) if n.endswith("_hip"))


# ---------------------------------------------- the reference's RTCD side --
def _config_defines():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from cinterp import reference_defines
    d = reference_defines(REF)
    return {k: v for k, v in d.items() if isinstance(v, int) and not k.startswith("__") and
            k != "NDEBUG"}


def rtcd_headers(tmp):
    """Write tmp/config/{aom_config,aom_dsp_rtcd,av1_rtcd}.h the way the
    reference's build does for a generic (C only) target; returns the set of
    names that have a `_c` prototype."""
    cfg = os.path.join(str(tmp), "config")
    os.makedirs(cfg, exist_ok=True)
    conf = os.path.join(cfg, "aom_config.h")
    with open(conf, "w") as f:
        f.write("#ifndef AOM_CONFIG_H_\n#define AOM_CONFIG_H_\n")
        for k, v in sorted(_config_defines().items()):
            f.write("#define %s %d\n" % (k, v))
        f.write("#define INLINE inline\n#endif\n")
    names = set()
    for sym, defs in (("aom_dsp_rtcd", "aom_dsp/aom_dsp_rtcd_defs.pl"),
                      ("av1_rtcd", "av1/common/av1_rtcd_defs.pl")):
        r = _run(["perl", os.path.join(REF, "build/cmake/rtcd.pl"), "--arch=generic",
                  "--sym=" + sym, "--config=" + conf, os.path.join(REF, defs)])
        assert r.returncode == 0 and "eval failed" not in r.stderr, r.stderr
        with open(os.path.join(cfg, sym + ".h"), "w") as f:
            f.write(r.stdout)
        names.update(re.findall(r"\b(\w+)_c\s*\(", r.stdout))
    return names


def substitute_mirrors(pre):
    """The header with the five mirror structs' definitions dropped and the
    reference's type names in their place."""
    def drop(m):
        return "" if m.group(1) in MIRRORS else m.group(0)
    out = _STRUCT_RE.sub(drop, pre)
    for mine, (theirs, _) in MIRRORS.items():
        out = re.sub(r"typedef\s+struct\s+%s\s+%s\s*;" % (mine, mine), "", out)
        assert not re.search(r"struct\s+%s\b" % mine, out), mine
        out = re.sub(r"\b%s\b" % mine, theirs, out)
    return out


def _compile(tmp, name, src, run=False):
    path = os.path.join(str(tmp), name)
    with open(path, "w") as f:
        f.write(src)
    cmd = ["gcc", "-std=gnu11", "-w", "-I", str(tmp), "-I", REF]
    if not run:
        return _run(cmd + ["-fsyntax-only", "-fmax-errors=0", path])
    exe = path[:-2]
    r = _run(cmd + ["-o", exe, path])
    if r.returncode != 0:
        return r
    return _run([exe])


_UNIT_HEAD = """#include <stddef.h>
#include <stdint.h>
#include "config/aom_config.h"
#include "config/aom_dsp_rtcd.h"
#include "config/av1_rtcd.h"
%s
"""


def _ref_includes():
    return "\n".join('#include "%s"' % h for h in sorted({h for _, h in MIRRORS.values()}))


def check_prototypes(tmp, pre, c_names, unit="types.c"):
    """Compile one unit that holds the reference's `_c` prototypes and the
    header's `_hip` ones and asserts, per shared name, that the two function
    types are compatible.  Returns (shared names, names that are not)."""
    shared = [n for n in hip_names(pre) if n in c_names]
    src = _UNIT_HEAD % _ref_includes() + substitute_mirrors(pre) + "\n"
    for n in shared:
        src += ('_Static_assert(__builtin_types_compatible_p(__typeof__(%s_c), '
                '__typeof__(%s_hip)), "MISMATCH %s");\n' % (n, n, n))
    r = _compile(tmp, unit, src)
    bad = sorted(set(re.findall(r"MISMATCH (\w+)", r.stderr)))
    other = [l for l in r.stderr.splitlines() if "error" in l and "MISMATCH" not in l]
    assert not other, "\n".join(other[:20])
    assert (r.returncode == 0) == (not bad), r.stderr[-2000:]
    return shared, bad


def check_mirrors(tmp, pre, unit="mirrors.c"):
    """Build and run a program that prints sizeof and, per field of the
    mirror's own body, offsetof, size and type compatibility on both sides.
    Returns a list of differences ("LavishX.field: ..."), empty when the
    five layouts agree."""
    by_name = dict(structs(pre))
    src = "#include <stdio.h>\n" + _UNIT_HEAD % _ref_includes() + pre + "\nint main(void) {\n"
    for mine, (theirs, _) in MIRRORS.items():
        src += '  printf("%s - %%zu %%zu 1\\n", sizeof(%s), sizeof(%s));\n' % (mine, mine, theirs)
        for f, _dims in by_name[mine]:
            src += ('  printf("%s %s %%zu %%zu %%zu %%zu %%d\\n", offsetof(%s, %s), '
                    'offsetof(%s, %s), sizeof(((%s *)0)->%s), sizeof(((%s *)0)->%s), '
                    '__builtin_types_compatible_p(__typeof__(((%s *)0)->%s), '
                    '__typeof__(((%s *)0)->%s)));\n'
                    % (mine, f, mine, f, theirs, f, mine, f, theirs, f, mine, f, theirs, f))
    src += "  return 0;\n}\n"
    r = _compile(tmp, unit, src, run=True)
    if r.returncode != 0:  # e.g. a field the reference's struct does not have
        return ["does not compile: " + l for l in r.stderr.splitlines() if "error" in l] or \
            [r.stderr]
    diffs, seen = [], set()
    for line in r.stdout.splitlines():
        p = line.split()
        seen.add(p[0])
        if p[1] == "-":
            if p[2] != p[3]:
                diffs.append("%s: sizeof %s, reference %s" % (p[0], p[2], p[3]))
            continue
        if p[2] != p[3]:
            diffs.append("%s.%s: offset %s, reference %s" % (p[0], p[1], p[2], p[3]))
        if p[4] != p[5]:
            diffs.append("%s.%s: size %s, reference %s" % (p[0], p[1], p[4], p[5]))
        if p[6] != "1":
            diffs.append("%s.%s: type differs from the reference's" % (p[0], p[1]))
    assert seen == set(MIRRORS), seen
    return diffs


_KIND = ("_Generic((%s), signed char: 'i', short: 'i', int: 'i', long: 'i', long long: 'i', "
         "unsigned char: 'u', unsigned short: 'u', unsigned: 'u', unsigned long: 'u', "
         "unsigned long long: 'u', char: 'u', float: 'f', double: 'f', default: "
         "__builtin_classify_type(%s) == 5 ? 'p' : 's')")


def probe_layout(tmp, pre, unit="layout.c"):
    """Compile and run a program over the header alone (no reference needed):
    {struct: (sizeof, [(field, offset, element size, [array lengths], kind)])}
    with kind 'i' / 'u' (signed / unsigned integer), 'f', 'p' (pointer) or
    's' (nested struct) of the field's element."""
    src = "#include <stdio.h>\n#include <stddef.h>\n#include <stdint.h>\n" + pre
    src += "\nint main(void) {\n"
    st = structs(pre)
    for name, fields in st:
        src += '  printf("%s - %%zu\\n", sizeof(%s));\n' % (name, name)
        for f, dims in fields:
            e = "((%s *)0)->%s%s" % (name, f, "[0]" * len(dims))
            src += ('  printf("%s %s %%zu %%zu %%c\\n", offsetof(%s, %s), sizeof(%s), %s);\n'
                    % (name, f, name, f, e, _KIND % (e, e)))
    src += "  return 0;\n}\n"
    path = os.path.join(str(tmp), unit)
    with open(path, "w") as fh:
        fh.write(src)
    r = _run(["gcc", "-std=gnu11", "-w", "-o", path[:-2], path])
    assert r.returncode == 0, r.stderr
    r = _run([path[:-2]])
    assert r.returncode == 0, r.stderr
    dims = {(n, f): d for n, fs in st for f, d in fs}
    out = {}
    for line in r.stdout.splitlines():
        p = line.split()
        if p[1] == "-":
            out[p[0]] = (int(p[2]), [])
        else:
            out[p[0]][1].append((p[1], int(p[2]), int(p[3]), dims[(p[0], p[1])], p[4]))
    return out


def probe_scalar_types(tmp, types, unit="scalars.c"):
    """{type name: (kind, size)} of the given arithmetic C type names, from
    the compiler."""
    src = "#include <stdio.h>\n#include <stddef.h>\n#include <stdint.h>\nint main(void) {\n"
    for k, t in enumerate(types):
        e = "(%s)0" % t
        src += '  printf("%d %%c %%zu\\n", %s, sizeof(%s));\n' % (k, _KIND % (e, e), t)
    src += "  return 0;\n}\n"
    path = os.path.join(str(tmp), unit)
    with open(path, "w") as fh:
        fh.write(src)
    r = _run(["gcc", "-std=gnu11", "-w", "-o", path[:-2], path])
    assert r.returncode == 0, r.stderr
    r = _run([path[:-2]])
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        k, kind, size = line.split()
        out[types[int(k)]] = (kind, int(size))
    return out


def reference_field_counts():
    """Number of fields of each reference struct, counted from its own text
    (so a field the mirror lacks shows)."""
    out = {}
    for mine, (theirs, hdr) in MIRRORS.items():
        txt = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(REF, hdr)).read(), flags=re.S)
        tag = theirs.split()[-1]
        m = re.search(r"struct\s+%s\s*\{([^{}]*)\}\s*;" % tag, txt) if theirs.startswith("struct") \
            else re.search(r"typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*%s\s*;" % tag, txt)
        assert m, theirs
        out[mine] = sum(len(d.split(",")) for d in m.group(1).split(";") if d.strip())
    return out
