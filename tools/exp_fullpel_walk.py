#!/usr/bin/env python3
"""Two builds of the library on the full-pel diamond_search_sad walks: are
their outputs byte-identical, and is one slower?

One process measures one library (LAVISH_HIP_LIB selects it; default: the
tree's): the 13 calls of tools/exp_comp_search.py (16x16, 1080p job set), the
plain DIAMOND search untiled at 32x32 (LDS window) and 64x64 (no window,
source re-read through L2) and tiled at 8x8, plain NSTEP and NSTEP_8PT at
16x16 (all step_param 0, with cost lists), and tpl_motion_search with
search_method "diamond" on the 1080p x 7 frame of tests/test_gpu_tplmv.py.
Per call: the sha256 of every output buffer it writes, and --rounds windows
of --iters launches between two device events (exp_comp_search's window).
The batches of tests/test_gpu_mcomp.py::test_nstep_steps_and_cost_lists are
hashed too (not timed).

  python tools/exp_fullpel_walk.py --out run.json            one process
  python tools/exp_fullpel_walk.py --merge P1 N1 P2 N2 [--bench NAME=FILE ...] --out FILE
merges four runs made in the order parent, new, parent, new; each --bench
file holds the JSON line of one bench.py --no-cpu run (NAME such as
c3_parent), kept under "bench_no_cpu".  Per call the
new library passes when the mean of its two medians <= the mean of the
parent's two medians * (1 + m), m the larger of the relative difference of
the parent's two medians and the relative span (max - min) / median of the
rounds inside either parent run.
Needs a HIP device; there is no CPU fall-back."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("aom-av1-lavish_amd", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))


def sha(*tensors):
    import torch
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def plain_calls(M, E, cost):
    """name -> (call, output tensors) of the plain searches beyond exp_comp_search's."""
    import torch
    import lavish_dsp.synth as synth
    src, refs = synth.motion_planes(E.W, E.H, 1, E.BORDER)
    s, r = torch.from_numpy(src).cuda(), torch.from_numpy(refs).cuda()
    C = {}

    def add(name, bw, method, tiles=None):
        jobs = M.to_device(M.frame_jobs(E.W, E.H, src.shape[1], E.BORDER, src.size, bw, bw, 1))
        nj = jobs.numel() // M.JOB_DTYPE.itemsize
        out = torch.empty(nj * M.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        cl = torch.empty((nj, 5), dtype=torch.int32, device="cuda")
        C[name] = (lambda: M.full_pixel_search_batch(s, r, bw, bw, jobs, cost, method, 0, False,
                                                     True, out, cl, tiles=tiles), (out, cl))
    add("dia32_sp0", 32, "diamond")
    add("dia64_sp0", 64, "diamond")
    tiles = M.RefTiles(r, src.shape[1])
    tiles.build()
    add("dia8_tiled_sp0", 8, "diamond", tiles)
    add("nstep16_sp0", 16, "nstep")
    add("nstep8pt16_sp0", 16, "nstep_8pt")
    return C


def tpl_call(M):
    import torch
    import lavish_dsp.synth as synth
    import lavish_dsp.tpl as T
    W, H, R, border = 1920, 1072, 7, 288
    src, refs = synth.tpl_motion_planes(W, H, R, border, 5)
    jobs = M.to_device(M.frame_jobs(W, H, src.shape[1], border, src.size, 16, 16, R, mv_border=32))
    costs = M.MvCosts(*M.default_mv_cost_tables(True), device="cuda")
    cost = costs.cost_params(M.sad_per_bit(100), M.error_per_bit(1800), M.MV_COST_ENTROPY)
    s, r = torch.from_numpy(src).cuda(), torch.from_numpy(refs).cuda()
    out = T.tpl_motion_search(s, r, jobs, W // 16, H // 16, R, cost, "diamond", 6, False, 2, 2)
    keep = (out["mvs"], out["fp"], out["cl"], out["centers"])
    return (lambda: T.tpl_motion_search(s, r, jobs, W // 16, H // 16, R, cost, "diamond", 6,
                                        False, 2, 2, out=out), keep)


def nstep_test_hashes(M):
    import torch
    import lavish_dsp.synth as synth
    import test_gpu_mcomp as G
    src, refs = synth.motion_planes(480, 272, 3, G.BORDER, seed=77)
    planes = (480, 272, src, refs)
    s, r = torch.from_numpy(src).cuda(), torch.from_numpy(refs).cuda()
    mvj, mvc = M.default_mv_cost_tables(False)
    cost = M.MvCosts(mvj, mvc).cost_params(M.sad_per_bit(128), M.error_per_bit(1 << 14))
    H = {}
    for method in ("nstep", "nstep_8pt"):
        for bw, bh, skip in G.NSTEP_SHAPES:
            jobs = M.to_device(G.nstep_jobs(M, planes, bw, bh))
            for sp in (0, 13):
                out, cl = M.full_pixel_search_batch(s, r, bw, bh, jobs, cost, method, sp, skip,
                                                    cost_list=True)
                H["test_%s_%dx%d_skip%d_sp%d" % (method, bw, bh, skip, sp)] = sha(out, cl)
    return H


def run(args):
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    import exp_comp_search as E
    import lavish_dsp
    import lavish_dsp.motion as M
    D = E.build(M)
    costs = M.MvCosts(*M.default_mv_cost_tables(False), device="cuda")
    cost = costs.cost_params(M.sad_per_bit(128), M.error_per_bit(1 << 14))
    C13, out13 = E.calls(M, D, cost)
    C = {k: (f, (out13,)) for k, f in C13.items()}
    C.update(plain_calls(M, E, cost))
    C["tpl_diamond"] = tpl_call(M)
    hashes = {}
    for k, (f, outs) in C.items():  # warm-up; the outputs of one call, hashed
        for t in outs:
            t.zero_()
        for _ in range(3):
            rc = f()
            assert rc == 0 or not isinstance(rc, int), k
        hashes[k] = sha(*outs)
    hashes.update(nstep_test_hashes(M))
    t = {k: [] for k in C}
    for _ in range(args.rounds):
        for k, (f, _) in C.items():
            t[k].append(E.window_ms(f, args.iters if k != "tpl_diamond" else max(args.iters // 10, 5)))
    res = {"library": os.path.relpath(lavish_dsp.LIB_PATH, ROOT), "iters": args.iters,
           "rounds_ms": {k: [round(x, 5) for x in v] for k, v in t.items()}, "sha256": hashes}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: round(statistics.median(v), 5) for k, v in t.items()}))


def merge(args):
    runs = [json.load(open(p)) for p in args.merge]
    par, new = (runs[0], runs[2]), (runs[1], runs[3])
    calls = {}
    ok = True
    for k in runs[0]["rounds_ms"]:
        pm = [statistics.median(r["rounds_ms"][k]) for r in par]
        nm = [statistics.median(r["rounds_ms"][k]) for r in new]
        span = max((max(r["rounds_ms"][k]) - min(r["rounds_ms"][k])) / statistics.median(r["rounds_ms"][k])
                   for r in par)
        m = max(abs(pm[0] - pm[1]) / min(pm), span)
        good = statistics.mean(nm) <= statistics.mean(pm) * (1 + m)
        ok = ok and good
        calls[k] = {"parent_medians_ms": pm, "new_medians_ms": nm, "m": round(m, 4),
                    "new_over_parent": round(statistics.mean(nm) / statistics.mean(pm), 4),
                    "parent_rounds_ms": [r["rounds_ms"][k] for r in par],
                    "new_rounds_ms": [r["rounds_ms"][k] for r in new], "pass": good}
    same = {k: len({r["sha256"][k] for r in runs}) == 1 for k in runs[0]["sha256"]}
    res = {"order": "parent, new, parent, new", "iters": runs[0]["iters"], "unit": "ms per call",
           "timing": calls, "misses": sorted(k for k, v in calls.items() if not v["pass"]),
           "outputs_byte_identical": same, "all_identical": all(same.values()), "all_pass": ok}
    if args.bench:
        keys = ("workload", "value", "unit", "ms_per_step", "steps", "warmup")
        res["bench_no_cpu"] = {}
        for item in args.bench:
            name, path = item.split("=", 1)
            line = json.loads(open(path).read().strip().splitlines()[-1])
            res["bench_no_cpu"][name] = {k: line[k] for k in keys}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"all_identical": res["all_identical"], "all_pass": ok,
                      "ratio": {k: v["new_over_parent"] for k, v in calls.items()},
                      "m": {k: v["m"] for k, v in calls.items()}}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--merge", nargs=4, default=None)
    ap.add_argument("--bench", nargs="*", default=None)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    merge(a) if a.merge else run(a)
