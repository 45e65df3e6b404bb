#!/usr/bin/env python3
"""Timing of the CfL alpha search (lavish_cfl_alpha_search_batch) for 8160 jobs
each of 8x8, 16x16 and 32x32 at 8 and 10 bits, and beside it, in the same
process, lavish_tpl_block_batch at the same block count with 33 prediction
planes: the same DCT + SATD per candidate (plus that call's quantization and
reconstruction of the best one), code that predates the CfL kernels.  Writes
profiles/cfl_timing.json; DESIGN.md section 5 quotes the ratios.

usage: python tools/exp_cfl.py [OUT_JSON]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aom-av1-lavish_amd"))

NJOBS, ITERS, ROUNDS = 8160, 20, 7


def _time(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / ITERS)
    return float(np.median(ms)), [float(min(ms)), float(max(ms))]


def main(out=None):
    import torch
    import lavish_dsp as L
    import lavish_dsp.cfl as K
    import lavish_dsp.tpl as T
    out = out or os.path.join(ROOT, "profiles", "cfl_timing.json")
    res = {"workload": "%d chroma blocks per size, 33 alphas each" % NJOBS, "iters": ITERS,
           "rounds": ROUNDS, "unit": "ms per call (median of rounds)"}
    rng = np.random.default_rng(3)
    for bd in (8, 10):
        dt = np.uint8 if bd == 8 else np.uint16
        maxv = (1 << bd) - 1
        for n in (8, 16, 32):
            tx = {8: 1, 16: 2, 32: 3}[n]
            bx = 96  # blocks per row of the plane
            by = NJOBS // bx
            W, H = bx * n, by * n
            src = rng.integers(0, maxv + 1, (H, W)).astype(dt)
            dc = np.full((H, W), maxv // 2, dt)
            cells = torch.from_numpy(rng.integers(-maxv, maxv + 1, (NJOBS, 32, 32)).astype(np.int16)).cuda()
            offs = [(b // bx) * n * W + (b % bx) * n for b in range(NJOBS)]
            jobs = K.cfl_jobs_tensor(K.cfl_search_jobs(np.arange(NJOBS), offs, offs, tx, ncells=NJOBS,
                                                       src_stride=W, src_elems=W * H, dc_stride=W,
                                                       dc_elems=W * H), "cuda")
            view = (lambda a: a.view(np.int16)) if bd > 8 else (lambda a: a)
            dsrc, ddc = torch.from_numpy(view(src)).cuda(), torch.from_numpy(view(dc)).cuda()
            cfl = _time(lambda: K.cfl_alpha_search_batch(cells, dsrc, ddc, jobs, bd))
            preds = torch.from_numpy(view(rng.integers(0, maxv + 1, (33, H, W)).astype(dt))).cuda()
            qp = L.build_quant_params(bd, 100, L.QUANT_FP)
            o, r, c = T.tpl_block_batch(dsrc, preds, n, bd, qp, ref_costs=True)
            tpl = _time(lambda: T.tpl_block_batch(dsrc, preds, n, bd, qp, out=o, recon=r, ref_costs=c))
            res["%dx%d_bd%d" % (n, n, bd)] = {
                "cfl_alpha_search_ms": round(cfl[0], 5), "cfl_min_max_ms": [round(v, 5) for v in cfl[1]],
                "tpl_block_batch_33_planes_ms": round(tpl[0], 5),
                "tpl_min_max_ms": [round(v, 5) for v in tpl[1]],
                "ratio_cfl_over_tpl": round(cfl[0] / tpl[0], 3)}
            print(n, bd, res["%dx%d_bd%d" % (n, n, bd)], flush=True)
    assert L.status()[0] == 0, L.status()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:])
