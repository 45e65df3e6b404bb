#!/usr/bin/env python3
"""Timing of the compound / masked / OBMC sub-pel search batches
(csrc/subpel_comp.hip) against the plain
lavish_find_best_sub_pixel_tree_batch_ex, same jobs, same process,
alternating.

Workload: the 16x16 job set of one reference of a 1080p frame
(motion.frame_jobs over synth.motion_planes: 120 x 67 = 8,040 jobs), every
job starting at the plain DIAMOND search's full-pel best, one second_pred /
mask / wsrc block per job (second_pred and the OBMC neighbour are the source
plus a little noise, so the searches walk as they do on real content),
MV_COST_ENTROPY with the hp tables, allow_hp, EIGHTH_PEL, iters_per_step 2.
  tree8   SUBPEL_TREE with USE_8_TAPS (the speed 0..3 default)
  pm      SUBPEL_TREE_PRUNED_MORE (bilinear; the OBMC call has no pruned
          method: its bilinear run is USE_2_TAPS_ORIG)
  each for plain / average / masked / OBMC
Each figure is the median over --rounds rounds of one window of --iters
launches between two device events, after a warm-up of every call; the
rounds alternate the calls, so box drift hits all of them alike.  The ratio
to the plain search of the same kind is the figure of merit; `moved` (the
share of jobs that end off their start) shows the walks are not idle.  Before
timing, every form's records are compared with a second run of the same call
(the results do not depend on scheduling).

Usage: python tools/exp_comp_subpel.py [--iters 300] [--rounds 7] [--out FILE]
Needs a HIP device; there is no CPU fall-back."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aom-av1-lavish_amd"))

W, H, BW, BORDER = 1920, 1080, 16, 160


def build(M, cost, seed=7):
    import torch
    import lavish_dsp.synth as synth
    rng = np.random.default_rng(seed)
    src, refs = synth.motion_planes(W, H, 1, BORDER)
    jobs = M.frame_jobs(W, H, src.shape[1], BORDER, src.size, BW, BW, 1)
    nj, n = len(jobs), BW * BW
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ts, tr = t(src), t(refs)
    fp = M.results_numpy(M.full_pixel_search_batch(ts, tr, BW, BW, M.to_device(jobs), cost,
                                                   "diamond", 5)[0])
    sj = M.subpel_jobs(W, H, BORDER, BW, BW, jobs, fp)
    off = np.arange(nj) * n
    idx = np.arange(BW)[:, None] * src.shape[1] + np.arange(BW)[None, :]
    blocks = src.reshape(-1)[jobs["src_off"][:, None, None] + idx[None]].reshape(-1)
    blocks = blocks.astype(np.int64)
    om = rng.integers(1024, 4097, nj * n)
    nb = np.clip(blocks + rng.integers(-4, 5, nj * n), 0, 255)
    ws = blocks * 4096 - nb * (4096 - om)
    return dict(
        src=ts, ref=tr, nj=nj, starts=sj, jobs=M.to_device(sj),
        cjobs=M.to_device(M.comp_subpel_jobs(sj, off, off, rng.integers(0, 2, nj))),
        second=t(np.clip(blocks + rng.integers(-3, 4, nj * n), 0, 255).astype(np.uint8)),
        mask=t(rng.integers(0, 65, nj * n).astype(np.uint8)),
        wsrc=t(ws.astype(np.int32)), omask=t(om.astype(np.int32)))


def calls(M, D, cost):
    """The C calls themselves on preallocated outputs."""
    import torch
    L, st = M._lib, M._stream_ptr(None)
    d = lambda x: ctypes.c_void_p(x.data_ptr())
    nj = D["nj"]
    out = torch.empty(nj * 16, dtype=torch.uint8, device="cuda")
    s, r = D["src"], D["ref"]
    ss = s.stride(0)
    c = ctypes.byref(cost)
    C = {}
    # (method, search type) of the two kinds; the OBMC bilinear run is USE_2_TAPS_ORIG
    for kind, method, stype in (("tree8", 0, 3), ("pm", 2, 0)):
        C["plain_" + kind] = lambda method=method, stype=stype: \
            L.lavish_find_best_sub_pixel_tree_batch_ex(
                d(s), ss, d(r), ss, BW, BW, d(D["jobs"]), None, nj, method, stype, 0, 1, 2, c,
                None, d(out), st)
        C["avg_" + kind] = lambda method=method, stype=stype: \
            L.lavish_comp_find_best_sub_pixel_tree_batch(
                d(s), ss, d(r), ss, BW, BW, d(D["cjobs"]), None, 0, nj, method, stype, 0, 1, 2, c,
                d(D["second"]), None, 0, d(out), st)
        C["masked_" + kind] = lambda method=method, stype=stype: \
            L.lavish_comp_find_best_sub_pixel_tree_batch(
                d(s), ss, d(r), ss, BW, BW, d(D["cjobs"]), None, 0, nj, method, stype, 0, 1, 2, c,
                d(D["second"]), d(D["mask"]), BW, d(out), st)
        C["obmc_" + kind] = lambda stype=stype: L.lavish_obmc_find_best_sub_pixel_tree_batch(
            d(r), ss, BW, BW, d(D["cjobs"]), None, nj, stype, 0, 1, 2, c, d(D["wsrc"]),
            d(D["omask"]), d(out), st)
    return C, out


def records(M, fn, out):
    import torch
    assert fn() == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().view(M.SUBPEL_RESULT_DTYPE).copy()


def window_ms(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    import lavish_dsp.motion as M
    costs = M.MvCosts(*M.default_mv_cost_tables(True), device="cuda")
    cost = costs.cost_params(M.sad_per_bit(128), M.error_per_bit(1 << 14))
    D = build(M, cost)
    C, out = calls(M, D, cost)
    for k, f in C.items():  # warm-up; every call must accept its arguments
        for _ in range(3):
            assert f() == 0, k
    torch.cuda.synchronize()
    moved = {}
    for k, f in C.items():
        a, b = records(M, f, out), records(M, f, out)
        assert a.tobytes() == b.tobytes(), k
        moved[k] = round(float(((a["best_row"] != D["starts"]["start_row"]) |
                                (a["best_col"] != D["starts"]["start_col"])).mean()), 3)
    t = {k: [] for k in C}
    for _ in range(args.rounds):
        for k, f in C.items():
            t[k].append(window_ms(f, args.iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    basis = {k: "plain_" + k.split("_")[1] for k in C if not k.startswith("plain")}
    res = {"workload": "%d 16x16 jobs (1080p, one reference), MV_COST_ENTROPY (hp), allow_hp, "
                       "EIGHTH_PEL, iters_per_step 2; tree8 = SUBPEL_TREE USE_8_TAPS, pm = "
                       "SUBPEL_TREE_PRUNED_MORE (OBMC: the tree with USE_2_TAPS_ORIG)" % D["nj"],
           "iters": args.iters, "rounds": args.rounds, "unit": "ms per call (median of rounds)",
           "ms": {k: round(v, 5) for k, v in med.items()},
           "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in t.items()},
           "ratio_to_plain": {k: round(med[k] / med[b], 3) for k, b in basis.items()},
           "ns_per_job": {k: round(1e6 * v / D["nj"], 2) for k, v in med.items()},
           "moved": moved}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
