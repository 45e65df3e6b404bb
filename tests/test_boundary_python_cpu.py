"""The Python package's copies of include/lavish_dsp.h against the header
(CPU, no GPU, no reference needed):

* every ctypes.Structure subclass and every module-level *_DTYPE numpy record
  of lavish_dsp/*.py against the header struct it mirrors: item size, field
  names and order, offsets, element sizes, array lengths, signedness;
* every library function the package declares (argtypes / restype set) or
  names in its source: argument count, pointer against pointer,
  integer width and signedness, struct pointers against the paired struct,
  and the return type, against the header's prototype.

The header side comes from the C compiler: a probe program generated from
the preprocessed header prints each struct's layout (tests/_rtcd.py).  The
pairing tables below are explicit and complete in both directions, so a new
struct, mirror or dtype fails here until it is listed."""
import ctypes
import importlib
import os
import pkgutil
import re

import numpy as np
import pytest

import _rtcd as R

# Python mirror ("module.NAME", module relative to lavish_dsp) -> header struct
PAIRS = {
    ".TxfmParam": "LavishTxfmParam",
    ".QuantParams": "LavishQuantParams",
    ".PlaneQuant": "LavishPlaneQuant",
    ".BitDepthInfo": "LavishBitDepthInfo",
    ".INV_JOB_DTYPE": "LavishInvJob",
    ".RDO_DTYPE": "LavishRdoBlock",
    "blend.COMP_JOB_DTYPE": "LavishCompJob",   # (pixel.COMP_JOB_DTYPE re-exported)
    "blend.OBMC_JOB_DTYPE": "LavishObmcJob",
    "blend.WEDGE_JOB_DTYPE": "LavishWedgeJob",
    "compound.JOB_DTYPE": "LavishCompoundJob",
    "inter.INTER_JOB_DTYPE": "LavishInterPredJob",
    "inter.InterpFilterParams": "LavishInterpFilterParams",
    "inter.ConvolveParams": "LavishConvolveParams",
    "intra.INTRA_JOB_DTYPE": "LavishIntraJob",
    "motion.JOB_DTYPE": "LavishDiamondJob",
    "motion.RESULT_DTYPE": "LavishDiamondResult",
    "motion.MvCostParams": "LavishMvCostParams",
    "motion.RefTilesDesc": "LavishRefTiles",
    "motion.MeshParams": "LavishMeshParams",
    "motion.COMP_JOB_DTYPE": "LavishCompSearchJob",
    "motion.COMP_RESULT_DTYPE": "LavishCompSearchResult",
    "motion.SUBPEL_JOB_DTYPE": "LavishSubpelJob",
    "motion.SUBPEL_RESULT_DTYPE": "LavishSubpelResult",
    "motion.COMP_SUBPEL_JOB_DTYPE": "LavishCompSubpelJob",
    "pixel.JOB_DTYPE": "LavishPixJob",
    "pixel.DistWtdCompParams": "LavishDistWtdCompParams",
    "pixel.COMP_JOB_DTYPE": "LavishCompJob",
    "scale.JOB_DTYPE": "LavishScaleJob",
    "tpl.TPL_BLOCK_DTYPE": "LavishTplBlock",
    "tpl.TplMvParams": "LavishTplMvParams",
    "txprune.NNConfig": "LavishNNConfig",
    "warp.JOB_DTYPE": "LavishWarpJob",
}

# header structs the package builds no record of, one line of reason each
NO_PYTHON_MIRROR = {
    # txb.py holds these as flat int32 tensors, no per-field access; its cell
    # counts are compared with the structs' sizes below
    "LavishCoeffCost": "flat int32 cells in txb.py (COEFF_COST_CELLS)",
    "LavishEobCost": "flat int32 cells in txb.py (EOB_COST_CELLS)",
    "LavishCoeffCosts": "flat int32 cells in txb.py (COEFF_COSTS_CELLS)",
    "LavishTxbCtx": "an int32 [nblocks, 2] tensor in txb.py",
}


@pytest.fixture(scope="module")
def pkg():
    """lavish_dsp with every submodule imported: {"": package, "name": module}."""
    import lavish_dsp
    mods = {"": lavish_dsp}
    for mi in pkgutil.iter_modules(lavish_dsp.__path__):
        mods[mi.name] = importlib.import_module("lavish_dsp." + mi.name)
    return mods


@pytest.fixture(scope="module")
def pre():
    return R.preprocessed()


@pytest.fixture(scope="module")
def layout(tmp_path_factory, pre):
    return R.probe_layout(tmp_path_factory.mktemp("layout"), pre)


def _python_mirrors(pkg):
    out = {}
    for mname, m in pkg.items():
        for k, v in vars(m).items():
            if isinstance(v, type) and issubclass(v, (ctypes.Structure, ctypes.Union)) and \
                    v.__module__ == m.__name__:
                out["%s.%s" % (mname, k)] = v
            elif k.endswith("_DTYPE") and isinstance(v, np.dtype):
                out["%s.%s" % (mname, k)] = v
    return out


def _ctype_kind(t):
    """(kind, element size, [array lengths]) of a ctypes type."""
    dims = []
    while isinstance(t, type) and issubclass(t, ctypes.Array):
        dims.append(t._length_)
        t = t._type_
    if issubclass(t, (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_wchar_p,
                      ctypes._CFuncPtr)):
        return "p", ctypes.sizeof(t), dims
    if issubclass(t, (ctypes.Structure, ctypes.Union)):
        return "s", ctypes.sizeof(t), dims
    code = t._type_
    kind = "f" if code in "fdg" else "i" if code in "bhilq" else "u"
    return kind, ctypes.sizeof(t), dims


def _python_layout(v):
    """(item size, [(field, offset, element size, [array lengths], kind)])."""
    if isinstance(v, np.dtype):
        fields = []
        for n in v.names:
            sub, off = v.fields[n][:2]
            base, dims = (sub.subdtype[0], list(sub.shape)) if sub.subdtype else (sub, [])
            kind = {"i": "i", "u": "u", "f": "f", "V": "s"}[base.kind]
            fields.append((n, off, base.itemsize, dims, kind))
        return v.itemsize, fields
    fields = []
    for f in v._fields_:
        assert len(f) == 2, "bit field in %s" % v.__name__
        kind, size, dims = _ctype_kind(f[1])
        fields.append((f[0], getattr(v, f[0]).offset, size, dims, kind))
    return ctypes.sizeof(v), fields


def _compare_layout(tag, py, hdr):
    diffs = []
    if py[0] != hdr[0]:
        diffs.append("%s: item size %d, header %d" % (tag, py[0], hdr[0]))
    if [f[0] for f in py[1]] != [f[0] for f in hdr[1]]:
        diffs.append("%s: fields %s, header %s" % (tag, [f[0] for f in py[1]],
                                                   [f[0] for f in hdr[1]]))
        return diffs
    for p, h in zip(py[1], hdr[1]):
        # a pointer may be held as an 8-byte integer in a numpy record
        same_kind = p[4] == h[4] or (h[4] == "p" and p[4] in "iu" and p[2] == h[2])
        if p[1:4] != h[1:4] or not same_kind:
            diffs.append("%s.%s: (offset, size, dims, kind) %s, header %s" % (tag, p[0], p[1:],
                                                                            h[1:]))
    return diffs


# -------------------------------------------------------------- structs --
def test_pairing_tables_are_complete(pkg, layout):
    mirrors = _python_mirrors(pkg)
    assert set(mirrors) == set(PAIRS), (sorted(set(mirrors) - set(PAIRS)),
                                        sorted(set(PAIRS) - set(mirrors)))
    paired = set(PAIRS.values())
    assert paired <= set(layout), sorted(paired - set(layout))
    assert not paired & set(NO_PYTHON_MIRROR)
    assert paired | set(NO_PYTHON_MIRROR) == set(layout), \
        sorted(set(layout) - paired - set(NO_PYTHON_MIRROR))


def test_python_struct_mirrors_match_header(pkg, layout):
    mirrors = _python_mirrors(pkg)
    diffs = []
    for key, struct in sorted(PAIRS.items()):
        diffs += _compare_layout("%s (%s)" % (key, struct), _python_layout(mirrors[key]),
                                 layout[struct])
    assert not diffs, "\n".join(diffs)
    assert len(PAIRS) >= 30


def test_flat_cost_tables_match_header(pkg, layout):
    """txb.py's flat int32 forms of the coefficient-cost structs: every field
    is int32 and the cell counts equal the structs' sizes."""
    T = pkg["txb"]
    for name, cells in (("LavishCoeffCost", T.COEFF_COST_CELLS),
                        ("LavishEobCost", T.EOB_COST_CELLS),
                        ("LavishCoeffCosts", T.COEFF_COSTS_CELLS), ("LavishTxbCtx", 2)):
        size, fields = layout[name]
        assert size == 4 * cells, (name, size, cells)
        assert all(f[4] == "s" or (f[4] == "i" and f[2] == 4) for f in fields), (name, fields)
    (_, o0, s0, d0, _), (_, o1, s1, d1, _) = layout["LavishCoeffCosts"][1]
    assert (o0, s0, d0) == (0, 4 * T.COEFF_COST_CELLS, [5, 2])
    assert (o1, s1, d1) == (40 * T.COEFF_COST_CELLS, 4 * T.EOB_COST_CELLS, [7, 2])


def test_layout_comparison_rejects_doctored_mirrors(layout):
    """_compare_layout on records that differ from the header in one respect
    each: tail padding, a swapped pair, a widened field, signedness, an array
    length."""
    hdr = layout["LavishInvJob"]   # int64 dst_off, coeff_off; int32 tx_type, eob
    ok = np.dtype([("dst_off", "<i8"), ("coeff_off", "<i8"), ("tx_type", "<i4"), ("eob", "<i4")])
    assert _compare_layout("x", _python_layout(ok), hdr) == []
    f = [("dst_off", "<i8"), ("coeff_off", "<i8"), ("tx_type", "<i4"), ("eob", "<i4")]
    for bad in ([f[0], f[1], f[3], f[2]], f[:3] + [("eob", "<u4")], f[:3] + [("eob", "<i2")],
                f[:3] + [("eob", "<i4", (2,))], f + [("pad", "<i8")]):
        assert _compare_layout("x", _python_layout(np.dtype(bad, align=True)), hdr), bad
    hdr = layout["LavishDiamondResult"]   # 2 x int16, int32, 2 x int16: 12 bytes, no padding
    packed = np.dtype([("best_row", "<i2"), ("best_col", "<i2"), ("bestsme", "<i4"),
                       ("steps", "<i2"), ("searches", "<i2"), ("tail", "<i4")])
    assert _compare_layout("x", _python_layout(packed), hdr)

    class P(ctypes.Structure):
        _fields_ = [("bit_depth", ctypes.c_int), ("use_highbitdepth_buf", ctypes.c_uint)]
    assert _compare_layout("x", _python_layout(P), layout["LavishBitDepthInfo"])


# ------------------------------------------------------------ prototypes --
def _source_names(pkg):
    """Library functions the package's source names literally (`_lib.NAME`)."""
    names = set()
    d = os.path.dirname(pkg[""].__file__)
    for f in os.listdir(d):
        if f.endswith(".py"):
            src = open(os.path.join(d, f)).read()
            names.update(re.findall(r"\b_?lib(?:\(\))?\.((?:lavish|av1|aom)_\w+)", src))
    return names


def _touched_functions(pkg):
    """{name: function object} of the library functions the package has
    declared (argtypes or restype set) or names in its source.  A function
    that something else merely looked up on the package's handle (hasattr in
    another test) has neither and is left out, so the result does not depend
    on which tests ran before."""
    lib = pkg[""].lib()
    named = _source_names(pkg)
    out = {k: v for k, v in vars(lib).items() if isinstance(v, ctypes._CFuncPtr) and
           (v.argtypes is not None or v.restype is not ctypes.c_int or k in named)}
    for k in named - set(out):
        out[k] = getattr(lib, k)
    return out


def _header_arg(decl, scalars):
    """An argument (or return) declaration of the header -> ("p", pointee type
    name), ("s", struct name) or (kind, size)."""
    d = re.sub(r"\bconst\b", " ", decl)
    if "*" in d or "[" in d:
        return "p", re.split(r"[*\[]", d)[0].split()[0]
    toks = d.split()
    typ = " ".join(toks[:-1]) if len(toks) > 1 and toks[-1] not in ("int", "unsigned", "long") \
        else " ".join(toks)
    if typ.startswith("Lavish"):
        return "s", typ
    return scalars[typ]


def _header_scalar_types(protos):
    types = set()
    for ret, args in protos.values():
        for d in [ret] + args:
            d = re.sub(r"\bconst\b", " ", d)
            if "*" in d or "[" in d or d.strip() == "void":
                continue
            toks = d.split()
            if d is not ret and len(toks) > 1 and toks[-1] not in ("int", "unsigned", "long"):
                toks = toks[:-1]
            if not toks[0].startswith("Lavish"):
                types.add(" ".join(toks))
    return sorted(types)


def _compare_function(name, fn, proto, scalars, struct_of):
    ret, args = proto
    diffs = []
    if fn.argtypes is not None:
        if len(fn.argtypes) != len(args):
            return ["%s: %d argtypes, header has %d arguments" % (name, len(fn.argtypes),
                                                                len(args))]
        for k, (t, d) in enumerate(zip(fn.argtypes, args)):
            h = _header_arg(d, scalars)
            kind, size, dims = _ctype_kind(t)
            if h[0] == "p":
                ok = kind == "p" and not dims or bool(dims)  # (an array passes as a pointer)
                if ok and isinstance(t, type) and issubclass(t, ctypes._Pointer) and \
                        issubclass(t._type_, ctypes.Structure):
                    ok = struct_of.get(t._type_) == h[1]
            elif h[0] == "s":
                ok = kind == "s" and struct_of.get(t) == h[1]
            else:
                ok = (kind, size) == h and not dims
            if not ok:
                diffs.append("%s: argument %d is %s, header `%s`" % (name, k, t.__name__, d))
    r = fn.restype
    if ret.strip() == "void":
        ok = r is None or r is ctypes.c_int   # (c_int: ctypes' default, the value unused)
    elif "*" in ret:
        ok = r is not None and _ctype_kind(r)[0] == "p"
    else:
        ok = r is not None and _ctype_kind(r)[:2] == scalars[" ".join(
            re.sub(r"\bconst\b", " ", ret).split())]
    if not ok:
        diffs.append("%s: restype %s, header returns `%s`" % (
            name, getattr(r, "__name__", r), ret))
    return diffs


@pytest.fixture(scope="module")
def protos(pre):
    return R.prototypes(pre)


@pytest.fixture(scope="module")
def scalars(tmp_path_factory, protos):
    return R.probe_scalar_types(tmp_path_factory.mktemp("scalars"), _header_scalar_types(protos))


def _struct_of(pkg):
    m = _python_mirrors(pkg)
    return {v: PAIRS[k] for k, v in m.items() if not isinstance(v, np.dtype) and k in PAIRS}


def test_declared_prototypes_match_header(pkg, protos, scalars):
    fns = _touched_functions(pkg)
    unknown = sorted(set(fns) - set(protos))
    assert not unknown, "not in the header: %s" % unknown
    diffs = []
    for name, fn in sorted(fns.items()):
        diffs += _compare_function(name, fn, protos[name], scalars, _struct_of(pkg))
    assert not diffs, "\n".join(diffs)
    declared = [n for n, f in fns.items() if f.argtypes is not None or not protos[n][1]]
    assert len(declared) >= 1600, len(declared)


def test_functions_called_without_argtypes_report(pkg, protos):
    """Counts for the record (printed with -s); the gate is only that every
    such name exists in the header."""
    fns = _touched_functions(pkg)
    called = set(fns)
    assert called <= set(protos), sorted(called - set(protos))
    bare = sorted(n for n in called if protos[n][1] and fns[n].argtypes is None)
    unused = sorted(set(protos) - called)
    print("\nheader functions %d, touched by the package %d, with argtypes (or no arguments) %d, "
          "called without argtypes %d %s, never named by the package %d %s"
          % (len(protos), len(called), len(called) - len(bare), len(bare), bare, len(unused),
             unused))


def test_function_comparison_rejects_doctored_declarations(pkg, protos, scalars):
    """_compare_function on declarations that differ from the header in one
    respect each."""
    lib = ctypes.CDLL(pkg[""].LIB_PATH)   # a second handle: the package's stays as it is
    so = _struct_of(pkg)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    name = "aom_subtract_block_hip"   # (int, int, int16*, ptrdiff_t, u8*, ptrdiff_t, u8*, ptrdiff_t)
    good = [i32, i32, vp, ctypes.c_ssize_t, vp, ctypes.c_ssize_t, vp, ctypes.c_ssize_t]
    for args, res, n_bad in ((good, None, 0), (good[:-1] + [i32], None, 1), (good[:-1], None, 1),
                             ([ctypes.c_uint] + good[1:], None, 1),
                             (good[:2] + [ctypes.c_int64] + good[3:], None, 1),
                             (good, ctypes.c_int64, 1)):
        f = getattr(lib, name)
        f.argtypes, f.restype = args, res
        assert len(_compare_function(name, f, protos[name], scalars, so)) == n_bad, (args, res)
    f = lib.aom_sse_hip   # returns int64_t: ctypes' default restype would truncate it
    assert _compare_function("aom_sse_hip", f, protos["aom_sse_hip"], scalars, so)
    f = lib.av1_inv_txfm_add_hip   # (..., const LavishTxfmParam *)
    f.argtypes = [vp, vp, i32, ctypes.POINTER(pkg[""].QuantParams)]
    f.restype = None
    assert _compare_function("av1_inv_txfm_add_hip", f, protos["av1_inv_txfm_add_hip"], scalars, so)
