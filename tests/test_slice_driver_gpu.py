"""The host driver of jmhip_p_slice_search (me_wave.hip): what a call leaves in the context besides its results -- nothing when it is rejected,
a fresh EPZS map state when the search range changes, a closed me_int stage timer. The searches themselves are pinned by tests/test_slice_gpu.py;
here a context that has been through something is compared, record by record, with a fresh one (itself pinned on the oracle by run_synthetic)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_slice_gpu import compare, run_synthetic, slice_params, synth_clip

W, H, NREF, QP, SEED = 96, 64, 2, 28, 5          # 6x4 macroblocks: interior, edge and corner macroblocks, more than one row
NMB = (W // 16) * (H // 16)
LAM = int(65536 * np.sqrt(0.85 * 2 ** ((QP - 12) / 3.0)) + 0.5)
REF_COST1 = int(2 * np.sqrt(0.85 * 2 ** ((QP - 12) / 3.0)))


def open_context(pkg, ctx_range):
    """a context holding the first P picture of run_synthetic's clip (frame NREF against the NREF source frames before it)"""
    clip = synth_clip(np.random.default_rng(SEED), W, H, NREF + 1)
    ctx = pkg.Context(W, H, yuv_format=0, max_refs=NREF, search_range=ctx_range)
    ctx.slice_state_reset()
    for r in range(NREF):
        ctx.ref_upload(r, clip[NREF - 1 - r])
        ctx.interp_luma(r)
    ctx.cur_upload(clip[NREF])
    return ctx


def params(pkg, mode, R, **kw):
    p = slice_params(pkg, mode, R, NREF, [LAM] * 3, REF_COST1, W, mb_first=0, mb_count=NMB, qp_n=QP, **kw)
    if mode == 3:
        pocs = [2 * (NREF - 1 - r) for r in range(NREF)]
        pkg.load_library().jmhip_epzs_scales(p, 2 * NREF, (C.c_int * NREF)(*pocs), NREF)
    return p


def search(pkg, ctx, mode, R):
    if mode == 3:                                # the first P picture's co-located field is empty (run_synthetic: prev_field)
        ctx.epzs_colocated_upload(np.zeros((H // 4, W // 4, 2), np.int16))
    return ctx.p_slice_search(params(pkg, mode, R))


_fresh = {}


def fresh(pkg, mode, R, ctx_range):
    """the records of a fresh context searching this picture -- computed once per configuration, never modified"""
    key = (mode, R, ctx_range)
    if key not in _fresh:
        if ctx_range == R:                       # the same picture, parameters and state through the oracle's P-slice driver
            run_synthetic(pkg, mode, W, H, R, NREF, nframes=2, seed=SEED, qp=QP)
        ctx = open_context(pkg, ctx_range)
        _fresh[key] = search(pkg, ctx, mode, R)
        _fresh[key].setflags(write=False)
        ctx.close()
    return _fresh[key]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [-1, 3])
def test_rejected_call_leaves_no_trace(pkg, mode):
    ctx = open_context(pkg, 8)
    bad = params(pkg, mode, 8)
    bad.num_refs = 0
    with pytest.raises(pkg.JmhipError):
        ctx.p_slice_search(bad)
    bad = params(pkg, mode, 8)
    bad.mb_first, bad.mb_count = NMB - 3, 4
    with pytest.raises(pkg.JmhipError):
        ctx.p_slice_search(bad)
    got = search(pkg, ctx, mode, 8)
    ctx.close()
    compare(got, fresh(pkg, mode, 8, 8), NREF, "after two rejected calls")


@pytest.mark.gpu
def test_epzs_range_change_starts_from_a_fresh_map(pkg):
    """8 -> 16 -> 8 on one context: each change of range reallocates the EPZS map group (ep_state_ensure)"""
    ctx = open_context(pkg, 16)
    for k, R in enumerate((8, 16, 8)):
        ctx.slice_state_reset()
        got = search(pkg, ctx, 3, R)
        compare(got, fresh(pkg, 3, R, 16), NREF, "call %d, range %d" % (k, R))
    ctx.close()


# me_int begin / end pairs of one call on this picture, as the commit before the driver was split into steps (ddb086b) reports them:
# measured once on an MI355X by running this test against that commit's library. bench.py divides the stage time by this count.
ME_INT_LAUNCHES = {(-1, None): 1, (3, None): 1, (1, "wave"): 1}


@pytest.mark.gpu
@pytest.mark.parametrize("mode,sched", sorted(ME_INT_LAUNCHES, key=str))
def test_timing_stays_paired(pkg, mode, sched, monkeypatch):
    if sched:
        monkeypatch.setenv("JMHIP_SLICE_SCHED", sched)
    want = fresh(pkg, mode, 8, 8)
    ctx = open_context(pkg, 8)
    ctx.timing_enable()
    ctx.timing_select(["me_int"])
    got = search(pkg, ctx, mode, 8)
    ms, launches = ctx.timing_read()["me_int"]
    ctx.close()
    print("mode %d sched %s: me_int %.3f ms in %d launches" % (mode, sched, ms, launches))
    assert ms > 0
    assert launches == ME_INT_LAUNCHES[(mode, sched)]
    compare(got, want, NREF, "timed run")
