#!/usr/bin/env python3
"""Timing of the high-bit-depth compound, masked and OBMC searches
(csrc/mcomp_comp_hbd.hip, csrc/subpel_comp_hbd.hip) beside their 8-bit twins
and beside the high-bit-depth plain searches, on the same jobs.

Workload: every 16x16 block (8,160 jobs) of a 1920x1088 frame against one
reference, a seeded 10-bit plane pair (a smooth field plus noise, the
reference moved by (3, -5) pixels) and the same planes reduced to 8 bits
(>> 2).  Per job a second_pred block (the source block off by a little noise;
>> 2 for the 8-bit calls), a random 0..64 mask block and an OBMC wsrc / mask
pair built from the job's source block at each depth.  The calls:
  comp_avg / comp_mask   lavish_[highbd_]comp_full_pixel_search_batch, NSTEP
  refine_avg             lavish_[highbd_]refining_search_8p_batch, the average
  obmc                   lavish_[highbd_]obmc_full_pixel_search_batch, NSTEP
  plain                  lavish_highbd_full_pixel_search_batch (no cost list)
  sub_avg / sub_mask     lavish_[highbd_]comp_find_best_sub_pixel_tree_batch
                         chained on the comp_avg / comp_mask records
                         (SUBPEL_TREE, USE_2_TAPS_ORIG, allow_hp, 2 iters)
  sub_obmc               lavish_[highbd_]obmc_find_best_sub_pixel_tree_batch
                         chained on the obmc records
  sub_plain              lavish_highbd_find_best_sub_pixel_tree_batch (tree)
Each figure is the median over --rounds rounds of one window of --iters
launches between two device events, after a warm-up of every call; the rounds
alternate the calls in one process, so drift hits all of them alike.

Usage: python tools/exp_mcomp_comp_hbd.py [--iters 50] [--rounds 7] [--out FILE]
Needs a HIP device; there is no CPU fall-back."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aom-av1-lavish_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from exp_mcomp_hbd import BORDER, H, W, planes, window_ms  # noqa: E402

BW = BH = 16
STEP_PARAM = 2


def invariants(src, fj, top, seed=11):
    """(second, mask, wsrc, omask) pools for jobs fj over plane src (values
    up to top): compact blocks, job k at k * 256."""
    rng = np.random.default_rng(seed)
    stride = src.shape[1]
    idx = (fj["src_off"][:, None, None] + (np.arange(BH) * stride)[None, :, None] +
           np.arange(BW)[None, None, :])
    blk = src.reshape(-1)[idx].astype(np.int64).reshape(len(fj), -1)
    second = np.clip(blk + rng.integers(-3, 4, blk.shape) * (top + 1) // 256, 0, top)
    mask = rng.integers(0, 65, blk.shape)
    om = rng.integers(1024, 4097, blk.shape)
    nb = np.clip(blk + rng.integers(-3, 4, blk.shape) * (top + 1) // 256, 0, top)
    ws = blk * 4096 - nb * (4096 - om)
    return second.reshape(-1), mask.reshape(-1), ws.reshape(-1), om.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    import lavish_dsp.motion as M
    src16, ref16 = planes()
    src8, ref8 = (src16 >> 2).astype(np.uint8), (ref16 >> 2).astype(np.uint8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pl = {"hbd": (dev(src16.view(np.int16)), dev(ref16.view(np.int16))),
          "u8": (dev(src8), dev(ref8))}
    stride = src16.shape[1]
    costs = M.MvCosts(*M.default_mv_cost_tables(True), device="cuda")
    cost = costs.cost_params(M.sad_per_bit(128, 10), M.error_per_bit(40000), M.MV_COST_ENTROPY)
    fj = M.frame_jobs(W, H, stride, BORDER, src16.size, BW, BH, 1)
    fj["ref_off"] = fj["src_off"]       # (the reference is a plane of its own)
    nj = len(fj)
    off = np.arange(nj) * BW * BH
    cj = M.to_device(M.comp_jobs(fj, off, off, 0))
    pj = M.to_device(fj)
    inv = {}
    s10, m, w10, o10 = invariants(src16, fj, 1023)
    s8, _, w8, o8 = invariants(src8, fj, 255)
    inv["hbd"] = (dev(s10.astype(np.uint16).view(np.int16)), dev(m.astype(np.uint8)),
                  dev(w10.astype(np.int32)), dev(o10.astype(np.int32)))
    inv["u8"] = (dev(s8.astype(np.uint8)), inv["hbd"][1], dev(w8.astype(np.int32)),
                 dev(o8.astype(np.int32)))
    rec = lambda: torch.empty(nj * 16, dtype=torch.uint8, device="cuda")
    kw = dict(method="nstep", step_param=STEP_PARAM)
    hb = dict(bit_depth=10)
    full, outs = {}, {}
    for d, (comp, refine, obmc, extra) in (
            ("hbd", (M.highbd_comp_full_pixel_search_batch, M.highbd_refining_search_8p_batch,
                     M.highbd_obmc_full_pixel_search_batch, hb)),
            ("u8", (M.comp_full_pixel_search_batch, M.refining_search_8p_batch,
                    M.obmc_full_pixel_search_batch, {}))):
        s, r = pl[d]
        sec, msk, ws, om = inv[d]
        o = outs[d] = {k: rec() for k in ("comp_avg", "comp_mask", "refine_avg", "obmc")}
        full[d + "_comp_avg"] = lambda s=s, r=r, sec=sec, o=o, f=comp, e=extra: f(
            s, r, BW, BH, cj, cost, sec, out=o["comp_avg"], **kw, **e)
        full[d + "_comp_mask"] = lambda s=s, r=r, sec=sec, msk=msk, o=o, f=comp, e=extra: f(
            s, r, BW, BH, cj, cost, sec, msk, BW, out=o["comp_mask"], **kw, **e)
        full[d + "_refine_avg"] = lambda s=s, r=r, sec=sec, o=o, f=refine, e=extra: f(
            s, r, BW, BH, cj, cost, sec, out=o["refine_avg"], **e)
        full[d + "_obmc"] = lambda r=r, ws=ws, om=om, o=o, f=obmc, e=extra: f(
            r, stride, BW, BH, cj, cost, ws, om, out=o["obmc"], **kw, **e)
    plain_out = rec()
    full["hbd_plain"] = lambda: M.highbd_full_pixel_search_batch(
        *pl["hbd"], BW, BH, pj, cost, out=plain_out, **kw, **hb)
    for f in full.values():     # warm-up, and the records the sub-pel jobs continue
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    sj = M.subpel_jobs(W, H, BORDER, BW, BH, fj, M.results_numpy(plain_out))
    csj = M.to_device(M.comp_subpel_jobs(sj, off, off, 0))
    psj = M.to_device(sj)
    skw = dict(forced_stop=0, allow_hp=True, iters_per_step=2)
    calls, souts = dict(full), {}
    for d, (comp, obmc, extra) in (
            ("hbd", (M.highbd_comp_find_best_sub_pixel_tree_batch,
                     M.highbd_obmc_find_best_sub_pixel_tree_batch, hb)),
            ("u8", (M.comp_find_best_sub_pixel_tree_batch,
                    M.obmc_find_best_sub_pixel_tree_batch, {}))):
        s, r = pl[d]
        sec, msk, ws, om = inv[d]
        o, so = outs[d], {k: rec() for k in ("avg", "mask", "obmc")}
        souts[d] = so
        calls[d + "_sub_avg"] = lambda s=s, r=r, sec=sec, o=o, so=so, f=comp, e=extra: f(
            s, r, BW, BH, csj, cost, sec, method="tree", fullpel=o["comp_avg"], out=so["avg"],
            **skw, **e)
        calls[d + "_sub_mask"] = lambda s=s, r=r, sec=sec, msk=msk, o=o, so=so, f=comp, e=extra: f(
            s, r, BW, BH, csj, cost, sec, msk, BW, method="tree", fullpel=o["comp_mask"],
            out=so["mask"], **skw, **e)
        calls[d + "_sub_obmc"] = lambda r=r, ws=ws, om=om, o=o, so=so, f=obmc, e=extra: f(
            r, stride, BW, BH, csj, cost, ws, om, fullpel=o["obmc"], out=so["obmc"], **skw, **e)
    plain_sout = rec()
    calls["hbd_sub_plain"] = lambda: M.highbd_find_best_sub_pixel_tree_batch(
        *pl["hbd"], BW, BH, psj, cost, method="tree", fullpel=plain_out, out=plain_sout, **skw,
        **hb)
    for k, f in calls.items():
        if "_sub_" in k:
            for _ in range(3):
                f()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, f in calls.items():
            t[k].append(window_ms(f, args.iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    names = ["comp_avg", "comp_mask", "refine_avg", "obmc", "sub_avg", "sub_mask", "sub_obmc"]
    plain_of = lambda n: "hbd_sub_plain" if n.startswith("sub_") else "hbd_plain"
    fp = {d: {k: M.comp_results_numpy(v) for k, v in outs[d].items()} for d in outs}
    res = {"workload": "every 16x16 block of a 1920x1088 frame (%d jobs), one reference, 10-bit "
                       "planes and the same >> 2; NSTEP step_param %d, entropy mv cost; "
                       "SUBPEL_TREE, allow_hp, 2 iters" % (nj, STEP_PARAM),
           "iters": args.iters, "rounds": args.rounds, "unit": "ms per call (median of rounds)",
           "ms": {k: round(v, 5) for k, v in med.items()},
           "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in t.items()},
           "ratio_hbd_over_u8": {n: round(med["hbd_" + n] / med["u8_" + n], 3) for n in names},
           "ratio_hbd_over_hbd_plain": {n: round(med["hbd_" + n] / med[plain_of(n)], 3)
                                        for n in names},
           # what the searches did (the two depths walk alike on these planes)
           "mean_steps": {d: {k: round(float(v["steps"].mean()), 2) for k, v in fp[d].items()}
                          for d in fp},
           "same_fullpel_mv_fraction": {k: round(float(np.mean(
               (fp["hbd"][k]["best_row"] == fp["u8"][k]["best_row"]) &
               (fp["hbd"][k]["best_col"] == fp["u8"][k]["best_col"]))), 4) for k in fp["hbd"]}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
