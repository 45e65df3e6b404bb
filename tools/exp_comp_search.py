#!/usr/bin/env python3
"""Timing of the compound / masked / OBMC full-pel search batches
(csrc/mcomp_comp.hip) against the plain full_pixel_search_batch (DIAMOND,
untiled), same jobs, same process, alternating.

Workload: the 16x16 job set of one reference of a 1080p frame
(motion.frame_jobs over synth.motion_planes: 120 x 67 = 8,040 jobs), one
second_pred / mask / wsrc block per job, MV_COST_ENTROPY.
  plain DIAMOND search               step_param 5 and 0
  compound average, masked           DIAMOND, step_param 5 and 0
  OBMC diamond and fast refinement   DIAMOND, step_param 5 and 0
  8-point refinement                 plain, average, masked
Each figure is the median over --rounds rounds of one window of --iters
launches between two device events, after a warm-up of every call; the
rounds alternate the calls, so box drift hits all of them alike.  The ratio
to the plain search at the same step_param is the figure of merit; the mean
`steps` of each call's records separates walk length from cost per step.

Usage: python tools/exp_comp_search.py [--iters 1000] [--rounds 7] [--out FILE]
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


def build(M, seed=7):
    import torch
    import lavish_dsp.synth as synth
    rng = np.random.default_rng(seed)
    src, refs = synth.motion_planes(W, H, 1, BORDER)
    jobs = M.frame_jobs(W, H, src.shape[1], BORDER, src.size, BW, BW, 1)
    nj, n = len(jobs), BW * BW
    off = np.arange(nj) * n
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    om = rng.integers(0, 4097, nj * n)
    idx = np.arange(BW)[:, None] * src.shape[1] + np.arange(BW)[None, :]
    blocks = src.reshape(-1)[jobs["src_off"][:, None, None] + idx[None]].reshape(-1)
    ws = blocks.astype(np.int64) * 4096 - rng.integers(0, 256, nj * n) * (4096 - om)
    return dict(
        src=t(src), ref=t(refs), nj=nj, jobs=M.to_device(jobs),
        cjobs=M.to_device(M.comp_jobs(jobs, off, off, rng.integers(0, 2, nj))),
        second=t(rng.integers(0, 256, nj * n).astype(np.uint8)),
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
    for sp in (5, 0):
        C["plain_sp%d" % sp] = lambda sp=sp: L.lavish_full_pixel_search_batch(
            d(s), ss, d(r), ss, BW, BW, d(D["jobs"]), nj, 0, sp, c, 0, d(out), None, st)
        C["avg_sp%d" % sp] = lambda sp=sp: L.lavish_comp_full_pixel_search_batch(
            d(s), ss, d(r), ss, BW, BW, d(D["cjobs"]), nj, 0, sp, c, d(D["second"]), None, 0,
            d(out), st)
        C["masked_sp%d" % sp] = lambda sp=sp: L.lavish_comp_full_pixel_search_batch(
            d(s), ss, d(r), ss, BW, BW, d(D["cjobs"]), nj, 0, sp, c, d(D["second"]),
            d(D["mask"]), BW, d(out), st)
        C["obmc_sp%d" % sp] = lambda sp=sp: L.lavish_obmc_full_pixel_search_batch(
            d(r), ss, BW, BW, d(D["cjobs"]), nj, 0, sp, c, 0, d(D["wsrc"]), d(D["omask"]),
            d(out), st)
    C["obmc_fast"] = lambda: L.lavish_obmc_full_pixel_search_batch(
        d(r), ss, BW, BW, d(D["cjobs"]), nj, 0, 0, c, 1, d(D["wsrc"]), d(D["omask"]), d(out), st)
    for name, sec, mask in (("plain", None, None), ("avg", D["second"], None),
                            ("masked", D["second"], D["mask"])):
        C["refine8_" + name] = lambda sec=sec, mask=mask: L.lavish_refining_search_8p_batch(
            d(s), ss, d(r), ss, BW, BW, d(D["cjobs"]), nj, c, d(sec) if sec is not None else None,
            d(mask) if mask is not None else None, BW, d(out), st)
    return C, out


def mean_steps(M, fn, name, out):
    """Mean step / round iterations per job of one call (its records' `steps`)."""
    import torch
    fn()
    torch.cuda.synchronize()
    dt = M.RESULT_DTYPE if name.startswith("plain") else M.COMP_RESULT_DTYPE
    return float(out.cpu().numpy().view(dt)["steps"].mean())


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
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    import lavish_dsp.motion as M
    D = build(M)
    costs = M.MvCosts(*M.default_mv_cost_tables(False), device="cuda")
    cost = costs.cost_params(M.sad_per_bit(128), M.error_per_bit(1 << 14))
    C, out = calls(M, D, cost)
    for k, f in C.items():  # warm-up; every call must accept its arguments
        for _ in range(3):
            assert f() == 0, k
    torch.cuda.synchronize()
    steps = {k: round(mean_steps(M, f, k, out), 2) for k, f in C.items()}
    t = {k: [] for k in C}
    for _ in range(args.rounds):
        for k, f in C.items():
            t[k].append(window_ms(f, args.iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    basis = {k: "plain_sp%s" % k[-1] for k in C if k[-3:-1] == "sp" and not k.startswith("plain")}
    res = {"workload": "%d 16x16 jobs (1080p, one reference), DIAMOND, MV_COST_ENTROPY" % D["nj"],
           "iters": args.iters, "rounds": args.rounds, "unit": "ms per call (median of rounds)",
           "ms": {k: round(v, 5) for k, v in med.items()},
           "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in t.items()},
           "ratio_to_plain": {k: round(med[k] / med[b], 3) for k, b in basis.items()},
           "mean_steps_per_job": steps,
           "ratio_per_step": {k: round(med[k] / steps[k] / (med[b] / steps[b]), 3)
                              for k, b in basis.items()}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
