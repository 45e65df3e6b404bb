#!/usr/bin/env python3
"""Timing of the compound pixel kernels (csrc/pixel_comp.hip) against the
existing rounded-average forms, same jobs, same process, alternating.

Workload: the 16x16 grid of a 1080p frame (120 x 68 = 8,160 jobs), 4
candidate references per job within +-16 pixels, u8 and 10-bit.
  masked SAD, distance-weighted SAD, OBMC SAD   vs lavish_sad_batch mode 2
  masked sub-pixel variance                     vs lavish_variance_batch kind 5
Each figure is the median over --rounds rounds of one window of --iters
launches between two device events, after a warm-up of every call; the
rounds alternate the calls, so box drift hits all of them alike.

Bytes per pixel read (the expectation printed next to each ratio): avg SAD
reads src + ref + second_pred = 3 streams, masked SAD adds the mask = 4;
OBMC reads pre (1 or 2 bytes) + wsrc (4) + mask (4).

Usage: python tools/exp_pixel_comp.py [--iters 400] [--rounds 7] [--out FILE]
Needs a HIP device; there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aom-av1-lavish_amd"))

W = H = 16
GW, GH = 1920 // 16, 1088 // 16
BORDER = 16


def build(P, bd, seed=7):
    import torch
    rng = np.random.default_rng(seed)
    dt = np.uint16 if bd > 8 else np.uint8
    ph, pw = GH * H + 2 * BORDER + 1, GW * W + 2 * BORDER + 1
    t = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    pix = lambda shape: rng.integers(0, 1 << bd, shape).astype(dt)
    nj, n = GW * GH, W * H
    gy, gx = np.divmod(np.arange(nj), GW)
    base = (gy * H + BORDER) * pw + gx * W + BORDER
    cj = np.zeros(nj, P.COMP_JOB_DTYPE)
    pj = np.zeros(nj, P.JOB_DTYPE)
    cj["src_off"] = pj["src_off"] = base
    for k in range(4):
        off = base + rng.integers(-16, 17, nj) * pw + rng.integers(-16, 17, nj)
        cj["ref_off"][:, k] = pj["ref_off"][:, k] = off
    cj["second_off"] = pj["aux_off"] = np.arange(nj) * n
    cj["mask_off"] = np.arange(nj) * n
    cj["xoff"] = pj["xoff"] = rng.integers(0, 8, nj)
    cj["yoff"] = pj["yoff"] = rng.integers(0, 8, nj)
    cj["invert_mask"] = rng.integers(0, 2, nj)
    mx = (1 << bd) - 1
    return dict(
        src=t(pix((ph, pw))), ref=t(pix((ph, pw))), second=t(pix(nj * n)),
        mask=t(rng.integers(0, 65, (nj * n // W, W)).astype(np.uint8)),
        wsrc=t(rng.integers(-mx * 4096, mx * 4096 + 1, nj * n).astype(np.int32)),
        omask=t(rng.integers(0, 4097, nj * n).astype(np.int32)),
        cjobs=P.comp_jobs_tensor(cj, "cuda"), pjobs=P.jobs_tensor(pj, "cuda"), nj=nj)


def calls(P, D, bd):
    """The C calls themselves on preallocated outputs (the Python wrappers
    widen their results with further kernels, which must stay out of the
    timed window)."""
    import torch
    L, d, st = P._lib, P._d, P._stream_ptr(None)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")
    nj, hb = D["nj"], int(bd > 8)
    o4, o1, o1b, o1c = i32(nj * 4), i32(nj), i32(nj), i32(nj)
    s, r, sec, mask = D["src"], D["ref"], D["second"], D["mask"]
    ss, rs = s.stride(0), r.stride(0)
    cj, pj = d(D["cjobs"]), d(D["pjobs"])
    return {
        "avg_sad": lambda: L.lavish_sad_batch(d(s), ss, d(r), rs, W, H, pj, nj, 4, 2, d(sec), hb,
                                              d(o4), st),
        "masked_sad": lambda: L.lavish_comp_sad_batch(d(s), ss, d(r), rs, W, H, cj, nj, 4, 0,
                                                      d(sec), d(mask), W, 0, 0, hb, d(o4), st),
        "dist_wtd_sad": lambda: L.lavish_comp_sad_batch(d(s), ss, d(r), rs, W, H, cj, nj, 4, 1,
                                                        d(sec), None, 0, 9, 7, hb, d(o4), st),
        "obmc_sad": lambda: L.lavish_obmc_batch(d(r), rs, W, H, cj, nj, 4, 0, bd, hb,
                                                d(D["wsrc"]), d(D["omask"]), d(o4), None, st),
        "avg_subpel_var": lambda: L.lavish_variance_batch(d(s), ss, d(r), rs, W, H, pj, nj, 5, bd,
                                                          hb, d(sec), d(o1), d(o1b), d(o1c), None,
                                                          st),
        "masked_subpel_var": lambda: L.lavish_comp_variance_batch(
            d(s), ss, d(r), rs, W, H, cj, nj, 0, bd, hb, d(sec), d(mask), W, 0, 0, d(o1), d(o1b),
            st),
    }


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
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    import lavish_dsp.pixel as P
    res = {"workload": "%d 16x16 jobs x 4 refs (1080p grid, +-16 px)" % (GW * GH),
           "iters": args.iters, "rounds": args.rounds, "unit": "ms per call (median of rounds)"}
    for bd in (8, 10):
        D = build(P, bd)
        C = calls(P, D, bd)
        for k, f in C.items():  # warm-up; every call must accept its arguments
            for _ in range(3):
                assert f() == 0, k
        torch.cuda.synchronize()
        t = {k: [] for k in C}
        for _ in range(args.rounds):
            for k, f in C.items():
                t[k].append(window_ms(f, args.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        px = 1 if bd == 8 else 2
        expect = {"masked_sad": (3 * px + 1) / (3 * px), "dist_wtd_sad": 1.0,
                  "obmc_sad": (px + 8) / (3 * px), "masked_subpel_var": (3 * px + 1) / (3 * px)}
        basis = {"masked_sad": "avg_sad", "dist_wtd_sad": "avg_sad", "obmc_sad": "avg_sad",
                 "masked_subpel_var": "avg_subpel_var"}
        res["bd%d" % bd] = {
            "ms": {k: round(v, 5) for k, v in med.items()},
            "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in t.items()},
            "ratio": {k: round(med[k] / med[b], 3) for k, b in basis.items()},
            "byte_ratio": {k: round(v, 3) for k, v in expect.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
