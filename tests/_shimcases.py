"""Per-call RTCD shim cases built from the reference's recorded outputs
(tests/golden/fix_*.npz): each builder yields (label, run) pairs, run() calls
the shim(s) on the fixture's inputs and asserts the outputs equal the
reference's bit for bit.

test_gpu_fixtures.py and test_gpu_warp.py run the cases one after another;
test_gpu_shim_threads.py runs the same cases from several host threads, and
(`python _shimcases.py first-use`) as the first library calls of a fresh
process.  Expected values are never taken from the code under test."""
import os
import sys
import threading
import time

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
BLOCK_SIZES = [(128, 128), (128, 64), (64, 128), (64, 64), (64, 32), (32, 64), (32, 32), (32, 16),
               (16, 32), (16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4), (4, 16),
               (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]
SUBPEL_OFFSETS = [(0, 0), (3, 0), (0, 5), (4, 4), (7, 2)]
SUBTRACT_SIZES = ((4, 4), (8, 4), (16, 16), (7, 5), (64, 64), (32, 8), (128, 128))


def load(name):
    return dict(np.load(os.path.join(GOLD, name)))


def tx_types(L, s):
    return [t for t in range(16) if L.tx_type_valid(s, t)]


# ------------------------------------------------------ forward transform --
def fwd_shim_cases(L, FT, s):
    """av1_fwd_txfm2d_{WxH}_hip: the whole W*H output buffer the reference
    writes (64-point sizes: zeroed + re-packed in place)."""
    W, H = TX_W[s], TX_H[s]
    fn = getattr(L, "av1_fwd_txfm2d_" + L.TX_SIZES[s])
    for t in tx_types(L, s):
        for k, (blk, exp, bd) in enumerate(zip(FT["in_%d_%d" % (s, t)], FT["out_%d_%d" % (s, t)],
                                               FT["bd_%d_%d" % (s, t)])):
            def run(blk=blk, exp=exp, bd=bd, t=t):
                padded = np.zeros((H, W + 3), np.int16)
                padded[:, :W] = blk
                got = np.full(W * H, 0x5A5A5A5A, np.int32)
                fn(padded, got, W + 3, t, int(bd))
                np.testing.assert_array_equal(got, exp, err_msg="size %d type %d" % (s, t))
            yield "fwd %s type %d block %d" % (L.TX_SIZES[s], t, k), run


# --------------------------------------------------------------- quantizers --
def quant_grid(FQ):
    for ci, (s, ls, hb, isb) in enumerate(FQ["cases"]):
        for q in (0, 32, 128, 255):
            yield ci, int(s), int(ls), bool(hb), bool(isb), 10 if hb else 8, q


def quant_shim_cases(L, FQ, G):
    """The per-call quantizer shims named like the reference's functions
    (av1_quantize_fp_hip, aom_quantize_b_32x32_hip, ...); G = fix_qparams."""
    for ci, s, ls, hb, isb, bd, q in quant_grid(FQ):
        name = str(FQ["case_names"][ci])[:-2]  # drop "_c"
        key = "%d_%d_q%d" % (ci, bd, q)
        n = L.max_eob(s)
        for k, c in enumerate(FQ["coeff_" + key]):
            def run(name=name, key=key, n=n, s=s, ls=ls, isb=isb, bd=bd, q=q, k=k, c=c):
                scan, iscan = L.scan_order(s, 0)
                row = lambda f: np.ascontiguousarray(G["%s_bd%d_sh0" % (f, bd)][q])
                rnd, qnt = (row("y_round"), row("y_quant")) if isb else (row("y_round_fp"),
                                                                          row("y_quant_fp"))
                qc = np.full(n, 99, np.int32)
                dq = np.full(n, 99, np.int32)
                eob = np.zeros(1, np.uint16)
                args = [np.ascontiguousarray(c), n, row("y_zbin"), rnd, qnt, row("y_quant_shift"),
                        qc, dq, row("y_dequant_QTX"), eob, scan, iscan]
                if name == "av1_highbd_quantize_fp":
                    args.append(ls)
                getattr(L, name)(*args)
                msg = "%s q %d block %d" % (name, q, k)
                np.testing.assert_array_equal(qc, FQ["qcoeff_" + key][k], err_msg=msg)
                np.testing.assert_array_equal(dq, FQ["dqcoeff_" + key][k], err_msg=msg)
                assert eob[0] == FQ["eob_" + key][k], msg
            yield "%s q %d block %d" % (name, q, k), run


# ------------------------------------------------------ inverse transform --
def inv_shim_cases(L, FI, s):
    """av1_inv_txfm2d_add_{WxH}_hip on the fixture's u16 destination (stride
    W + 5, only the W x H window may change)."""
    for t in tx_types(L, s):
        key = "%d_%d" % (s, t)
        for k, (c, dst, exp, bd) in enumerate(zip(FI["in_" + key], FI["dst_" + key],
                                                  FI["out_" + key], FI["bd_" + key])):
            def run(c=c, dst=dst, exp=exp, bd=bd, t=t):
                d = dst.copy()
                L.av1_inv_txfm2d_add(s, np.ascontiguousarray(c), d, d.shape[1], t, int(bd))
                np.testing.assert_array_equal(d, exp, err_msg="size %d type %d bd %d" % (s, t, bd))
            yield "inv %s type %d block %d" % (L.TX_SIZES[s], t, k), run


# ------------------------------------------------------------------- pixel --
def sad_variance_shim_case(PX, FP, W, H, bd):
    """SAD, skip SAD, x4d SAD, variance and five sub-pixel variances of one
    block size (10 shim calls)."""
    def run():
        k = "%dx%d_bd%d" % (W, H, bd)
        dt = np.uint8 if bd == 8 else np.uint16
        a, b = FP["src_" + k].astype(dt), FP["ref_" + k].astype(dt)
        hb = bd > 8
        ss, rs = a.shape[1], b.shape[1]
        assert PX.sad(W, H, a, ss, b, rs, highbd=hb) == FP["sad_" + k][0]
        assert PX.sad(W, H, a, ss, b, rs, highbd=hb, skip=True) == FP["sadskip_" + k][0]
        flat = b.reshape(-1)
        got4 = PX.sad_x4d(W, H, a, ss, [flat[o:] for o in (0, 1, 3, W + 2)], rs, highbd=hb)
        np.testing.assert_array_equal(got4, FP["sadx4d_" + k])
        assert list(PX.variance(W, H, a, ss, b, rs, bd, hb)) == list(FP["var_" + k])
        got = [PX.sub_pixel_variance(W, H, a, ss, xo, yo, b, rs, bd, hb)
               for xo, yo in SUBPEL_OFFSETS]
        np.testing.assert_array_equal(np.array(got, np.int64), FP["subvar_" + k])
    return "sad/variance %dx%d bd %d" % (W, H, bd), run


def subtract_sse_shim_case(PX, FP, w, h, bd):
    """subtract_block, sse, sum_squares_2d_i16, sum_sse_2d_i16 and
    get_blk_sse_sum of one (w, h, bd) (5 shim calls)."""
    def run():
        k = "%dx%d_bd%d" % (w, h, bd)
        dt = np.uint8 if bd == 8 else np.uint16
        src, prd = FP["s_src_" + k].astype(dt), FP["s_pred_" + k].astype(dt)
        exp = FP["sub_" + k]
        diff = np.full(exp.shape, 0x7777, np.int16)
        PX.subtract_block(h, w, diff, diff.shape[1], src, src.shape[1], prd, prd.shape[1],
                          highbd=bd > 8)
        np.testing.assert_array_equal(diff, exp, err_msg=k)
        assert PX.sse(src, src.shape[1], prd, prd.shape[1], w, h, highbd=bd > 8) == \
            FP["sse_" + k][0]
        assert PX.sum_squares_2d_i16(exp, exp.shape[1], w, h) == FP["sumsq_" + k][0]
        # the caller's *sum is accumulated into, as the reference does
        ss, sm = PX.sum_sse_2d_i16(exp, exp.shape[1], w, h, sum_in=7)
        assert [ss, sm - 7] == list(FP["sumsse_" + k])
        assert list(PX.get_blk_sse_sum(exp, exp.shape[1], w, h)) == list(FP["blksse_" + k])
    return "subtract/sse %dx%d bd %d" % (w, h, bd), run


# -------------------------------------------------------------------- warp --
def warp_row(F, r, J):
    g = lambda k: int(r[J[k]])
    W, H, RS, PS, DS = (int(v) for v in F["geom"])
    bd = g("bd")
    mode = g("mode")
    cp = dict(round_0=g("round_0"), round_1=g("round_1"), is_compound=int(mode > 0),
              do_average=int(mode >= 2), dist_wtd=int(mode == 3), fwd_offset=g("fwd_offset"),
              bck_offset=g("bck_offset"))
    return g, W, H, RS, PS, DS, bd, cp


def warp_shim_cases(Wp, F):
    """av1_warp_affine_hip / av1_highbd_warp_affine_hip on every third row of
    fix_warp: prediction and compound buffer."""
    J = {n: i for i, n in enumerate(F["row_fields"])}
    for k, r in enumerate(F["rows"]):
        if k % 3:
            continue

        def run(k=k, r=r):
            g, W, H, RS, PS, DS, bd, cp = warp_row(F, r, J)
            pdt = np.uint16 if bd > 8 else np.uint8
            ref = np.ascontiguousarray(F["refs"][g("ref_index")].astype(pdt))
            pred = F["pred_in"][k].astype(pdt).copy()
            dst = F["dst_in"][k].copy()
            c = Wp.conv_params(dst=dst, dst_stride=DS, **cp)
            Wp.warp_affine_shim([g("m%d" % i) for i in range(6)], ref, W, H, RS, pred, g("p_col"),
                                g("p_row"), g("p_width"), g("p_height"), PS, g("ss_x"), g("ss_y"),
                                c, tuple(g(f) for f in ("alpha", "beta", "gamma", "delta")), bd)
            np.testing.assert_array_equal(pred.astype(np.uint16), F["pred"][k],
                                          err_msg="row %d" % k)
            np.testing.assert_array_equal(dst, F["dst"][k], err_msg="row %d dst" % k)
        yield "warp row %d" % k, run


# ----------------------------------------------------------- thread runner --
def run_threads(case_lists, join_timeout):
    """Run case_lists[i] (a list of (label, run)) on host thread i, all
    released by one barrier; one pass, no retry.  Returns (mismatches,
    seconds, finished): a failed assertion of a case is one mismatch line and
    the thread goes on; any other exception ends that thread's list.
    finished is False if a thread was still running after join_timeout
    seconds (counted from the barrier) -- the caller must then start nothing
    more on the GPU."""
    barrier = threading.Barrier(len(case_lists))
    bad = [[] for _ in case_lists]

    def work(i):
        barrier.wait()
        for label, run in case_lists[i]:
            try:
                run()
            except AssertionError as e:
                bad[i].append("thread %d: %s: %s" % (i, label, str(e).strip()[:300]))
            except Exception as e:  # noqa: BLE001  (reported, not swallowed)
                bad[i].append("thread %d: %s: %r (thread stopped)" % (i, label, e))
                return

    threads = [threading.Thread(target=work, args=(i,), daemon=True)
               for i in range(len(case_lists))]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    deadline = time.monotonic() + join_timeout
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    finished = not any(t.is_alive() for t in threads)
    return [m for b in bad for m in b], time.perf_counter() - t0, finished


# ---------------------------------------------------- families for threads --
def family_pixel(PX, FP):
    """20 block-size cases, 200 calls: the small sizes at 8 and 10 bits."""
    sizes = sorted(BLOCK_SIZES, key=lambda wh: wh[0] * wh[1])[:10]
    return [sad_variance_shim_case(PX, FP, W, H, bd) for W, H in sizes for bd in (8, 10)]


def family_fwd_quant(L, FT, FQ, G):
    """69 forward transforms (every size, the first block of up to six
    types) and 100 quantizer calls (every named shim, q 0/32/128/255)."""
    out = []
    for s in range(19):
        cases = list(fwd_shim_cases(L, FT, s))
        per_type = len(cases) // len(tx_types(L, s))
        out += cases[::per_type][:6]
    q = list(quant_shim_cases(L, FQ, G))
    return out + q[::max(1, len(q) // 100)][:100]


def family_inv(L, FI):
    """185 inverse transforms: every size, up to ten cases spread over its
    types."""
    out = []
    for s in range(19):
        cases = list(inv_shim_cases(L, FI, s))
        out += cases[::max(1, len(cases) // 10)][:10]
    return out


def family_warp(Wp, FW):
    return list(warp_shim_cases(Wp, FW))


def pixel_growth_lists(PX, FP, nthreads=4):
    """Disjoint pixel cases for nthreads threads, ordered so that a thread's
    staging scratch grows mid-run: small SAD / variance blocks first (the
    pixel shims' fixed stage), then its share of the subtract / sse cases
    (which ask for more than the fixed stage; the 128x128 highbd one asks for
    the most), then the large SAD / variance blocks."""
    pix = [sad_variance_shim_case(PX, FP, W, H, bd)
           for W, H in sorted(BLOCK_SIZES, key=lambda wh: wh[0] * wh[1]) for bd in (8, 10)]
    sub = [subtract_sse_shim_case(PX, FP, w, h, bd) for w, h in SUBTRACT_SIZES for bd in (8, 10)]
    lists = []
    for i in range(nthreads):
        p, s = pix[i::nthreads], sub[i::nthreads]
        lists.append(p[:len(p) // 2] + s + p[len(p) // 2:])
    return lists


def first_use_lists():
    """One family per thread for the first-use race; imports only (no library
    call happens before the threads start)."""
    import lavish_dsp as L
    import lavish_dsp.pixel as PX
    import lavish_dsp.warp as Wp
    FP, FT, FQ, FI = (load(n) for n in ("fix_pixel.npz", "fix_txfm.npz", "fix_quant.npz",
                                        "fix_inv.npz"))
    G, FW = load("fix_qparams.npz"), load("fix_warp.npz")
    return L, [family_pixel(PX, FP)[:8], family_fwd_quant(L, FT, FQ, G)[::4],
               family_inv(L, FI)[::4], family_warp(Wp, FW)[::3]]


def _first_use_main():
    """Child process of test_gpu_shim_threads.py: the four threads' first
    calls are the process's first library calls.  Prints one line per
    mismatch and a summary; exit status 0 only when everything matched."""
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(os.path.dirname(here), "aom-av1-lavish_amd"), here]
    L, lists = first_use_lists()
    bad, secs, finished = run_threads(lists, float(sys.argv[2]) if len(sys.argv) > 2 else 60.0)
    for m in bad:
        print("MISMATCH " + m)
    if not finished:
        print("TIMEOUT a thread did not finish", flush=True)
        os._exit(3)   # a thread is stuck in a library call: do not wait for it
    st = L.status()
    print("first-use: %d calls lists, %d mismatches, status %d, %.2f s"
          % (sum(len(l) for l in lists), len(bad), st[0], secs), flush=True)
    return 0 if not bad and st[0] == 0 else 1


if __name__ == "__main__" and sys.argv[1:2] == ["first-use"]:
    sys.exit(_first_use_main())
