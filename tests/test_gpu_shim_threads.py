"""The per-call RTCD shims called the way the reference calls them: from
several host threads at once (its row workers), each with its own staging
scratch and stream (csrc/capi.hip), sharing the lazily uploaded tables.

Four host threads throughout; ctypes releases the GIL around every library
call.  Expected values are the reference's recorded outputs in
tests/golden/fix_*.npz (the cases of tests/_shimcases.py, the same ones
test_gpu_fixtures.py and test_gpu_warp.py run one after another), compared
bit for bit.  Each test is one pass over a fixed case list: no loop until
failure, no retry.  Every join carries a time limit; if a thread has not
finished the test fails and the rest of the module skips, so nothing more is
started on the GPU."""
import os
import subprocess
import sys
import time

import pytest

pytest.register_assert_rewrite("_shimcases")
import _shimcases as S  # noqa: E402

pytestmark = pytest.mark.gpu

JOIN_LIMIT = 60.0   # seconds, for a hang only: a pass takes well under one (see the docstrings)
_stuck = []         # set once a thread (or the child) did not finish


@pytest.fixture(autouse=True)
def _stop_after_a_hang():
    if _stuck:
        pytest.skip("an earlier test of this module left a thread running: %s" % _stuck[0])


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp
    return lavish_dsp


@pytest.fixture(scope="module")
def fixtures():
    return {n: S.load("fix_%s.npz" % n) for n in ("pixel", "txfm", "quant", "inv", "qparams",
                                                  "warp")}


def _run(lists, name):
    assert len(lists) == 4 and all(lists)
    bad, secs, finished = S.run_threads(lists, JOIN_LIMIT)
    print("\n%s: %s cases per thread, %.2f s" % (name, [len(l) for l in lists], secs))
    if not finished:
        _stuck.append(name)
        pytest.fail("%s: a thread was still running after %.0f s" % (name, JOIN_LIMIT))
    assert not bad, "\n".join(bad[:40])


def test_one_family_per_thread(L, fixtures):
    """SAD / variance / sub-pixel variance, forward transform + quantizers,
    av1_inv_txfm2d_add and the warp shims, one family per thread, started on
    a barrier; at most about 200 calls per thread.  (0.3 s on an MI355X.)"""
    import lavish_dsp.pixel as PX
    import lavish_dsp.warp as Wp
    F = fixtures
    lists = [S.family_pixel(PX, F["pixel"]),
             S.family_fwd_quant(L, F["txfm"], F["quant"], F["qparams"]),
             S.family_inv(L, F["inv"]), S.family_warp(Wp, F["warp"])]
    assert [len(l) for l in lists] == [20, 169, 185, 72]   # (20 pixel cases = 200 calls)
    _run(lists, "one family per thread")
    assert L.status()[0] == 0, L.status()


def test_same_family_disjoint_cases_scratch_grows(L, fixtures):
    """All four threads in the pixel family on disjoint cases: every block
    size at 8 and 10 bits, each thread going from 4x4-sized blocks through
    its share of the subtract / sse cases, whose stage request exceeds the
    scratch the thread holds by then (so it is freed and reallocated while
    the other threads' kernels run), to 128x128.  (0.3 s on an MI355X.)"""
    import lavish_dsp.pixel as PX
    lists = S.pixel_growth_lists(PX, fixtures["pixel"])
    labels = [[c[0] for c in l] for l in lists]
    assert len({x for l in labels for x in l}) == sum(len(l) for l in labels) == 44 + 14
    assert labels[0][0] == "sad/variance 4x4 bd 8"
    big = "subtract/sse 128x128 bd 10"
    owner = [l for l in labels if big in l]
    assert len(owner) == 1 and 0 < owner[0].index(big) < len(owner[0]) - 1
    for l in labels:   # small blocks, then a larger stage request, then large blocks
        first_sub = min(i for i, x in enumerate(l) if x.startswith("subtract"))
        assert 0 < first_sub < len(l) - 1 and l[-1].startswith("sad/variance")
    _run(lists, "same family, disjoint cases")
    assert L.status()[0] == 0, L.status()


def test_first_use_raced_in_fresh_process():
    """A fresh child process whose first library calls are made by the four
    threads at once: the scan tables, the per-thread streams and scratch and
    the HIP runtime itself are created under the race.  The child prints its
    mismatches; none, and exit status 0.  (2.4 s on an MI355X, nearly all of
    it the child's imports; the threads' pass takes 0.25 s.)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
        [os.path.abspath(S.__file__), "first-use", str(JOIN_LIMIT)]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=JOIN_LIMIT + 60)
    except subprocess.TimeoutExpired:
        _stuck.append("first use (child process)")
        pytest.fail("the child process did not finish")
    print("\nfirst use: %.2f s in all\n%s" % (time.perf_counter() - t0, r.stdout[-600:]))
    if r.returncode != 0:
        if "TIMEOUT" in r.stdout or r.returncode < 0:
            _stuck.append("first use (child: %d)" % r.returncode)
        pytest.fail("child exit status %d\n%s\n%s" % (r.returncode, r.stdout[-3000:],
                                                       r.stderr[-3000:]))
    assert "MISMATCH" not in r.stdout and " 0 mismatches, status 0" in r.stdout, r.stdout[-3000:]
