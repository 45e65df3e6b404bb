#!/usr/bin/env python3
"""Timing of the high-bit-depth upsampled sub-pel error (csrc/subpel_up_hbd.hip)
beside its 8-bit twins (csrc/subpel.hip, csrc/subpel_comp.hip) on the same jobs.

Workload: every 4x4 (130,560 jobs), 16x16 (8,160) and 64x64 (510) block of a
1920x1088 frame against one reference, tools/exp_mcomp_hbd.py's seeded 10-bit
plane pair and the same planes reduced to 8 bits (>> 2); SUBPEL_TREE with
USE_8_TAPS, allow_hp, iters_per_step 2, MV_COST_ENTROPY, every job starting at
the full-pel mv (3, -5) the reference was moved by.  Per size, four calls:
  hbd_plain   lavish_highbd_find_best_sub_pixel_tree_batch_ex, bit depth 10
  u8_plain    lavish_find_best_sub_pixel_tree_batch_ex, the same jobs
  hbd_avg     lavish_highbd_comp_find_best_sub_pixel_tree_batch_ex (no mask;
              second_pred the source plus seeded noise, one compact block a job)
  u8_avg      lavish_comp_find_best_sub_pixel_tree_batch, second_pred >> 2
Each figure is the median over --rounds rounds of one window of --iters
launches between two device events, after a warm-up of every call; the rounds
alternate the calls, so box drift hits all of them alike.  The ratios are
hbd / u8 of those medians.

Usage: python tools/exp_subpel_up_hbd.py [--iters 20] [--rounds 7] [--out FILE]
Needs a HIP device; there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aom-av1-lavish_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_mcomp_hbd import BORDER, H, W, planes, window_ms  # noqa: E402

START = (3, -5)     # full pel: where the reference matches


def second_blocks(src16, fj, bw, bh, stride, seed=3):
    """One compact bw x bh second_pred block per job: the source block plus
    noise of a few 10-bit steps."""
    rng = np.random.default_rng(seed)
    idx = np.arange(bh)[:, None] * stride + np.arange(bw)[None, :]
    blk = src16.reshape(-1)[fj["src_off"][:, None, None] + idx[None]].astype(np.int64)
    return np.clip(blk + rng.integers(-8, 9, blk.shape), 0, 1023).astype(np.uint16).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    import lavish_dsp.motion as M
    src16, ref16 = planes()
    t16 = lambda a: torch.from_numpy(a.view(np.int16).copy()).cuda()
    s16, r16 = t16(src16), t16(ref16)
    s8 = torch.from_numpy((src16 >> 2).astype(np.uint8)).cuda()
    r8 = torch.from_numpy((ref16 >> 2).astype(np.uint8)).cuda()
    stride = src16.shape[1]
    costs = M.MvCosts(*M.default_mv_cost_tables(True), device="cuda")
    cost = costs.cost_params(M.sad_per_bit(128, 10), M.error_per_bit(40000), M.MV_COST_ENTROPY)
    res = {"workload": "every 4x4 / 16x16 / 64x64 block of a 1920x1088 frame, one reference; "
                       "SUBPEL_TREE, USE_8_TAPS, allow_hp, iters_per_step 2, entropy mv cost, "
                       "start at full-pel (%d, %d)" % START,
           "iters": args.iters, "rounds": args.rounds, "unit": "ms per call (median of rounds)"}
    for bw, bh in ((4, 4), (16, 16), (64, 64)):
        fj = M.frame_jobs(W, H, stride, BORDER, src16.size, bw, bh, 1)
        fj["ref_off"] = fj["src_off"]       # (the reference is a plane of its own)
        nj = len(fj)
        fp = np.zeros(nj, M.RESULT_DTYPE)
        fp["best_row"], fp["best_col"] = START
        sj = M.subpel_jobs(W, H, BORDER, bw, bh, fj, fp)
        csj = M.comp_subpel_jobs(sj, np.arange(nj, dtype=np.int64) * bw * bh)
        jobs, cjobs = M.to_device(sj), M.to_device(csj)
        sec = second_blocks(src16, fj, bw, bh, stride)
        sec16 = torch.from_numpy(sec.view(np.int16).copy()).cuda()
        sec8 = torch.from_numpy((sec >> 2).astype(np.uint8)).cuda()
        out = {k: torch.empty(nj * M.SUBPEL_RESULT_DTYPE.itemsize, dtype=torch.uint8,
                              device="cuda")
               for k in ("hbd_plain", "u8_plain", "hbd_avg", "u8_avg")}
        kw = dict(method="tree", allow_hp=True, iters_per_step=2, search_type=M.USE_8_TAPS)
        calls = {
            "hbd_plain": lambda: M.highbd_find_best_sub_pixel_tree_batch(
                s16, r16, bw, bh, jobs, cost, bit_depth=10, out=out["hbd_plain"], **kw),
            "u8_plain": lambda: M.find_best_sub_pixel_tree_batch(
                s8, r8, bw, bh, jobs, cost, out=out["u8_plain"], **kw),
            "hbd_avg": lambda: M.highbd_comp_find_best_sub_pixel_tree_batch(
                s16, r16, bw, bh, cjobs, cost, sec16, bit_depth=10, out=out["hbd_avg"], **kw),
            "u8_avg": lambda: M.comp_find_best_sub_pixel_tree_batch(
                s8, r8, bw, bh, cjobs, cost, sec8, out=out["u8_avg"], **kw)}
        for f in calls.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, f in calls.items():
                t[k].append(window_ms(f, args.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        sp = {k: M.subpel_results_numpy(out[k]) for k in out}
        res["%dx%d" % (bw, bh)] = {
            "jobs": nj,
            "ms": {k: round(v, 5) for k, v in med.items()},
            "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in t.items()},
            "ratio_hbd_over_u8": {"plain": round(med["hbd_plain"] / med["u8_plain"], 3),
                                  "avg": round(med["hbd_avg"] / med["u8_avg"], 3)},
            # what the searches did (the two depths walk alike on these planes)
            "moved_fraction": {k: round(float(np.mean(
                (sp[k]["best_row"] != 8 * START[0]) | (sp[k]["best_col"] != 8 * START[1]))), 4)
                for k in sp},
            "same_mv_fraction": {f: round(float(np.mean(
                (sp["hbd_" + f]["best_row"] == sp["u8_" + f]["best_row"]) &
                (sp["hbd_" + f]["best_col"] == sp["u8_" + f]["best_col"]))), 4)
                for f in ("plain", "avg")}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
