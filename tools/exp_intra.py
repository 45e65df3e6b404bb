#!/usr/bin/env python3
"""Timing of lavish_intra_pred_batch (csrc/intra.hip).

Workload: the 16x16 grid (120 x 68 = 8,160 jobs) and the 64x64 grid (30 x 17 =
510 jobs) of a 1080p frame, u8 and 10-bit, every block predicted from the
plane's own pixels into a second plane, in four cases: DC, SMOOTH, one z2
angle with edge filtering (D135 + 3, both edges and the corner), and filter
intra (mode 0) on the 16x16 grid only.  Per case: ms per call and the bytes
counted (the block written plus the edge pixels read: w + h for DC and
SMOOTH, w + h + 1 for z2 and filter intra) over that time as a fraction of
8 TB/s.  Each figure is the median over --rounds rounds of one window of
--iters launches between two device events, after a warm-up of every call;
the rounds alternate the cases, so box drift hits all of them alike.

Usage: python tools/exp_intra.py [--iters 200] [--rounds 7] [--out FILE]
Needs a HIP device; there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aom-av1-lavish_amd"))

BORDER = 16
PEAK = 8e12  # bytes / s


def build(I, w, h, bd, seed=7):
    import torch
    rng = np.random.default_rng(seed)
    dt = np.uint16 if bd > 8 else np.uint8
    gw, gh = 1920 // w, 1088 // h
    ph, pw = gh * h + 2 * BORDER, gw * w + 2 * BORDER
    t = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    nj = gw * gh
    gy, gx = np.divmod(np.arange(nj), gw)
    base = (gy * h + BORDER) * pw + gx * w + BORDER
    tx = {(16, 16): 2, (64, 64): 4}[(w, h)]
    cases = {"dc": dict(mode=I.DC_PRED), "smooth": dict(mode=I.SMOOTH_PRED),
             "z2_filtered": dict(mode=I.D135_PRED, p_angle=138)}
    if w <= 32:
        cases["filter_intra"] = dict(mode=I.DC_PRED, filter_intra_mode=0)
    jobs = {k: I.intra_jobs_tensor(I.intra_jobs(base, base, tx, **kw), "cuda")
            for k, kw in cases.items()}
    plane = t(rng.integers(0, 1 << bd, (ph, pw)).astype(dt))
    return dict(plane=plane, dst=torch.zeros_like(plane), jobs=jobs, nj=nj)


def calls(I, D, w, h, bd):
    """The C call itself on preallocated planes; (call, bytes per job)."""
    L, d, st = I._lib, I._d, I._stream_ptr(None)
    px = 2 if bd > 8 else 1
    p, o, ps = D["plane"], D["dst"], D["plane"].stride(0)
    edge = {"dc": w + h, "smooth": w + h, "z2_filtered": w + h + 1, "filter_intra": w + h + 1}
    return {k: ((lambda j=j: L.lavish_intra_pred_batch(d(p), ps, d(o), ps, d(j), D["nj"], bd, st)),
                (w * h + edge[k]) * px) for k, j in D["jobs"].items()}


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    import lavish_dsp.intra as I
    res = {"workload": "the 16x16 (8160 jobs) and 64x64 (510 jobs) grids of a 1080p frame",
           "iters": args.iters, "rounds": args.rounds, "unit": "ms per call (median of rounds)",
           "peak_bytes_per_s": PEAK}
    for (w, h) in ((16, 16), (64, 64)):
        for bd in (8, 10):
            D = build(I, w, h, bd)
            C = calls(I, D, w, h, bd)
            for k, (f, _) in C.items():  # warm-up; every call must accept its arguments
                for _ in range(3):
                    assert f() == 0, k
            torch.cuda.synchronize()
            t = {k: [] for k in C}
            for _ in range(args.rounds):
                for k, (f, _) in C.items():
                    t[k].append(window_ms(f, args.iters))
            med = {k: statistics.median(v) for k, v in t.items()}
            res["%dx%d_bd%d" % (w, h, bd)] = {
                "ms": {k: round(v, 5) for k, v in med.items()},
                "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in t.items()},
                "bytes": {k: int(D["nj"] * C[k][1]) for k in C},
                "fraction_of_peak": {k: round(D["nj"] * C[k][1] / (med[k] * 1e-3) / PEAK, 4)
                                     for k in C}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
