#!/usr/bin/env python3
"""Timing of the mask-building and blending kernels (csrc/blend.hip), and of
lavish_comp_pred_batch mode 2 on the jobs of the 2-D mask blend, same process,
alternating.

Workload: the 16x16 grid (120 x 68 = 8,160 jobs) and the 64x64 grid (30 x 17 =
510 jobs) of a 1080p frame, u8 and 10-bit.  Per kernel: ms per call and the
bytes it has to move (below) over that time as a fraction of 8 TB/s.
Each figure is the median over --rounds rounds of one window of --iters
launches between two device events, after a warm-up of every call; the
rounds alternate the calls, so box drift hits all of them alike.

Bytes per pixel counted (px = 1 or 2 bytes per pixel):
  blend_mask     src0 + src1 + mask + dst                     3 px + 1
  comp_pred_mask ref + pred + mask + comp_pred                3 px + 1
  blend_d16      two CONV_BUF + mask + dst                    5 + px
  diffwtd        src0 + src1 + mask out                       2 px + 1
  diffwtd_d16    two CONV_BUF + mask out                      5
  obmc_wsrc      src + the overlap halves of above and left
                 + wsrc + mask out (every neighbour visited)  2 px + 8
  obmc_blend     dst read and written where a neighbour
                 reaches (3/4 of the block) + the two halves  2.5 px
  wedge_sse      r1 + d + m                                   5
  wedge_sign     ds + m                                       3
  wedge_delta    a + b + d out                                6

Usage: python tools/exp_blend.py [--iters 200] [--rounds 7] [--out FILE]
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
# av1_get_obmc_mask(n), n = 1, 2, 4 .. 64: a caller's table.  Timing does not
# depend on the weights; any 127 bytes in 0..64 do.
TABLE = np.concatenate([np.linspace(33, 64, n).astype(np.uint8) for n in (1, 2, 4, 8, 16, 32, 64)])


def build(B, w, h, bd, seed=7):
    import torch
    rng = np.random.default_rng(seed)
    dt = np.uint16 if bd > 8 else np.uint8
    gw, gh = 1920 // w, 1088 // h
    ph, pw = gh * h + 2 * BORDER + 1, gw * w + 2 * BORDER + 1
    t = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    pix = lambda shape: rng.integers(0, 1 << bd, shape).astype(dt)
    nj, n = gw * gh, w * h
    gy, gx = np.divmod(np.arange(nj), gw)
    base = (gy * h + BORDER) * pw + gx * w + BORDER
    blk = np.arange(nj) * n
    bj = np.zeros(nj, B.COMP_JOB_DTYPE)       # blend: dst, src1, mask compact; src0 in the plane
    bj["src_off"], bj["mask_off"] = blk, blk
    bj["ref_off"][:, 0], bj["ref_off"][:, 1] = base, blk
    pj = np.zeros(nj, B.COMP_JOB_DTYPE)       # comp_pred: the same blocks
    pj["src_off"], pj["second_off"], pj["mask_off"] = blk, blk, blk
    pj["ref_off"][:, 0] = base
    dj = np.zeros(nj, B.COMP_JOB_DTYPE)       # d16: both inputs compact
    dj["src_off"], dj["mask_off"] = blk, blk
    dj["ref_off"][:, 0], dj["ref_off"][:, 1] = blk, blk
    oj = np.zeros(nj, B.OBMC_JOB_DTYPE)
    oj["src_off"], oj["above_off"], oj["left_off"] = base, base, base
    oj["wsrc_off"], oj["mask_off"] = blk, blk
    oj["above_mask"], oj["left_mask"] = (1 << (w // 4)) - 1, (1 << (h // 4)) - 1
    wj = np.zeros(nj, B.WEDGE_JOB_DTYPE)
    wj["a_off"], wj["b_off"], wj["m_off"], wj["out_off"], wj["n"] = blk, blk, blk, blk, n
    r0 = 3
    roff = (1 << (bd + 14 - r0 - 7)) + (1 << (bd + 13 - r0 - 7))
    conv = lambda: (roff + (rng.integers(0, 1 << bd, nj * n) << (7 - r0))).astype(np.uint16)
    return dict(
        plane=t(pix((ph, pw))), above=t(pix((ph, pw))), left=t(pix((ph, pw))), pred=t(pix(nj * n)),
        dst=t(pix(nj * n)), mask=t(rng.integers(0, 65, nj * n).astype(np.uint8)),
        conv0=t(conv()), conv1=t(conv()), res_a=t(rng.integers(-255, 256, nj * n).astype(np.int16)),
        res_b=t(rng.integers(-255, 256, nj * n).astype(np.int16)),
        wsrc=torch.empty(nj * n, dtype=torch.int32, device="cuda"),
        omask=torch.empty(nj * n, dtype=torch.int32, device="cuda"),
        table=t(TABLE), bjobs=B.comp_jobs_tensor(bj, "cuda"), pjobs=B.comp_jobs_tensor(pj, "cuda"),
        djobs=B.comp_jobs_tensor(dj, "cuda"), ojobs=B.obmc_jobs_tensor(oj, "cuda"),
        wjobs=B.wedge_jobs_tensor(wj, "cuda"), nj=nj, cp=B.conv_params(r0, 7))


def calls(B, D, w, h, bd):
    """The C calls themselves on preallocated outputs; (call, bytes per pixel)."""
    import ctypes
    import torch
    L, d, st = B._lib, B._d, B._stream_ptr(None)
    nj, hb, px = D["nj"], int(bd > 8), 2 if bd > 8 else 1
    p, ps = D["plane"], D["plane"].stride(0)
    cp = ctypes.byref(D["cp"])
    o64 = torch.empty(nj, dtype=torch.int64, device="cuda")
    o16 = torch.empty(nj * w * h, dtype=torch.int16, device="cuda")
    bjb, pjb, djb, ojb, wjb = (d(D[k]) for k in ("bjobs", "pjobs", "djobs", "ojobs", "wjobs"))
    return {
        "blend_mask": (lambda: L.lavish_blend_a64_batch(
            d(D["dst"]), w, d(p), ps, d(D["pred"]), w, d(D["mask"]), w, w, h, bjb, nj, 0, 0, 0, 0,
            hb, bd, None, st), 3 * px + 1),
        "comp_pred_mask": (lambda: L.lavish_comp_pred_batch(
            d(D["dst"]), d(D["pred"]), w, h, d(p), ps, pjb, nj, 2, d(D["mask"]), w, 0, 0, hb, st),
            3 * px + 1),
        "blend_d16": (lambda: L.lavish_blend_a64_batch(
            d(D["dst"]), w, d(D["conv0"]), w, d(D["conv1"]), w, d(D["mask"]), w, w, h, djb, nj, 0,
            0, 0, 1, hb, bd, cp, st), 5 + px),
        "diffwtd": (lambda: L.lavish_diffwtd_mask_batch(
            d(D["mask"]), d(p), ps, d(D["pred"]), w, w, h, bjb, nj, 0, hb, bd, None, st),
            2 * px + 1),
        "diffwtd_d16": (lambda: L.lavish_diffwtd_mask_batch(
            d(D["mask"]), d(D["conv0"]), w, d(D["conv1"]), w, w, h, djb, nj, 1, hb, bd, cp, st), 5),
        "obmc_wsrc": (lambda: L.lavish_obmc_wsrc_batch(
            d(p), ps, d(D["above"]), ps, d(D["left"]), ps, w, h, ojb, nj, d(D["table"]), hb,
            d(D["wsrc"]), d(D["omask"]), st), 2 * px + 8),
        "obmc_blend": (lambda: L.lavish_obmc_blend_batch(
            d(p), ps, d(D["above"]), ps, d(D["left"]), ps, w, h, 0, 0, ojb, nj, d(D["table"]), hb,
            st), 2.5 * px),
        "wedge_sse": (lambda: L.lavish_wedge_batch(d(D["res_a"]), d(D["res_b"]), d(D["mask"]), wjb,
                                                   nj, 1, d(o64), st), 5),
        "wedge_sign": (lambda: L.lavish_wedge_batch(d(D["res_a"]), None, d(D["mask"]), wjb, nj, 2,
                                                    d(o64), st), 3),
        "wedge_delta": (lambda: L.lavish_wedge_batch(d(D["res_a"]), d(D["res_b"]), None, wjb, nj,
                                                     0, d(o16), st), 6),
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    import lavish_dsp.blend as B
    res = {"workload": "the 16x16 (8160 jobs) and 64x64 (510 jobs) grids of a 1080p frame",
           "iters": args.iters, "rounds": args.rounds, "unit": "ms per call (median of rounds)",
           "peak_bytes_per_s": PEAK}
    for (w, h) in ((16, 16), (64, 64)):
        for bd in (8, 10):
            D = build(B, w, h, bd)
            C = calls(B, D, w, h, bd)
            for k, (f, _) in C.items():  # warm-up; every call must accept its arguments
                for _ in range(3):
                    assert f() == 0, k
            torch.cuda.synchronize()
            t = {k: [] for k in C}
            for _ in range(args.rounds):
                for k, (f, _) in C.items():
                    t[k].append(window_ms(f, args.iters))
            med = {k: statistics.median(v) for k, v in t.items()}
            npx = D["nj"] * w * h
            res["%dx%d_bd%d" % (w, h, bd)] = {
                "ms": {k: round(v, 5) for k, v in med.items()},
                "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in t.items()},
                "bytes": {k: int(npx * C[k][1]) for k in C},
                "fraction_of_peak": {k: round(npx * C[k][1] / (med[k] * 1e-3) / PEAK, 4) for k in C},
                "blend_mask_over_comp_pred_mask": round(med["blend_mask"] / med["comp_pred_mask"],
                                                        3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
