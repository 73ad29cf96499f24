"""Grow-on-demand device buffers of a context: every entry that sizes its arrays by the call runs on ONE context with the first 2 jobs, then
all 12, then the first 2 again, and each answer must equal the matching slice of what a fresh context returns for all 12 in one call (those
answers are pinned on the oracle by the tests whose job builders are used here). Then the plane swap of jmhip_recon_to_ref, and contexts
opened and closed in a row."""
import numpy as np
import pytest

from tests.test_bipred_chain import chain_params, make_jobs as chain_jobs
from tests.test_bipred_surface import make_jobs as bipred_surface_jobs
from tests.test_deblock import make_case
from tests.test_frame import synth
from tests.test_me import lambda_factors, make_mbs
from tests.test_state_guards import _params
from tests.test_tq import compare_lists, make_jobs as tq_jobs, quant_set

W, H, R, FMT = 64, 48, 8, 1
MBW, MBH = W // 16, H // 16
N = MBW * MBH                      # 12 macroblocks
STEPS = (2, N, 2)


def pictures():
    rng = np.random.default_rng(77)
    cur, ref0 = synth(rng, W, H, FMT)
    _, ref1 = synth(rng, W, H, FMT)
    return cur, ref0, tuple(np.roll(p, (1, -2), (0, 1)) for p in ref1)


def open_ctx(pkg, wide_slot1=False):
    """Two reference slots with all their sub-pel planes and the current picture. wide_slot1: slot 1 travels as 16-bit samples."""
    cur, ref0, ref1 = pictures()
    ctx = pkg.Context(W, H, yuv_format=FMT, max_refs=2, search_range=R)
    ctx.ref_upload(0, *ref0)
    ctx.ref_upload(1, *(tuple(p.astype(np.uint16) for p in ref1) if wide_slot1 else ref1))
    for s in (0, 1):
        ctx.interp_luma(s)
        ctx.interp_chroma(s)
    ctx.cur_upload(*cur)
    return ctx


def same(got, want, what):
    """structured arrays field by field, plain arrays whole"""
    if got.dtype.names:
        for k in got.dtype.names:
            assert np.array_equal(got[k], want[k]), (what, k)
    else:
        assert np.array_equal(got, want), what


def regrow(pkg, ctx, call, jobs, what):
    """call(context, jobs) on the shared context for 2, 12, 2 jobs against one call with all of them on a fresh context"""
    fresh = open_ctx(pkg)
    want = call(fresh, jobs)
    fresh.close()
    for k in STEPS:
        same(call(ctx, jobs[:k]), want[:k], (what, k))


def mb_tiles(planes, k):
    """the samples of macroblocks 0..k-1 (raster order) of a 4:2:0 picture: the frame stage writes no others"""
    out = []
    for i in range(k):
        x, y = i % MBW, i // MBW
        out.append(planes[0][16 * y:16 * y + 16, 16 * x:16 * x + 16])
        out += [p[8 * y:8 * y + 8, 8 * x:8 * x + 8] for p in planes[1:]]
    return np.concatenate([t.reshape(-1) for t in out])


def frame_stage(pkg, ctx, mbs, bi, monkeypatch, fused):
    """me_frame -> residual_frame -> downloads for the macroblocks given; bi: their second list, or None for P macroblocks"""
    monkeypatch.setenv("JMHIP_FRAME_FUSED", "1" if fused else "0")
    quants = np.array([pkg.flat_quant(28 + d, 342, adaptive_rounding=1, adapt_rnd_weight=4, cavlc=1) for d in (0, 0, 3)], dtype=pkg.QUANT_DTYPE)
    me = ctx.me_frame(_params(pkg, R), mbs)
    ctx.frame_bipred_set(bi)
    ctx.residual_frame(quants, None)
    res = ctx.residual_download(len(mbs))
    recon = ctx.recon_download()
    ctx.frame_bipred_set(None)
    return me, res, recon


def check_frame_stage(got, want, k, what):
    """what tests/test_frame.py pins on the oracle: the (level, run) lists up to their terminating zero, costs, modes, patterns, reconstruction"""
    for key in ("mv_int", "cost_int", "mv", "cost"):
        assert np.array_equal(got[0][key], want[0][key][:k]), (what, key)
    g, w = got[1], want[1]
    compare_lists(g["luma"]["levels"], g["luma"]["runs"], w["luma"]["levels"][:k], w["luma"]["runs"][:k], "%s: luma" % (what,))
    gc, wc = g["chroma"], w["chroma"][:2 * k]
    compare_lists(gc["levels"][:, :4, :16], gc["runs"][:, :4, :16], wc["levels"][:, :4, :16], wc["runs"][:, :4, :16], "%s: chroma AC" % (what,))
    compare_lists(gc["dc_levels"][:, None], gc["dc_runs"][:, None], wc["dc_levels"][:, None], wc["dc_runs"][:, None], "%s: chroma DC" % (what,))
    assert np.array_equal(g["luma"]["coeff_cost"], w["luma"]["coeff_cost"][:k]), (what, "coeff_cost")
    for key in ("modes", "cbp", "cbp_blk"):
        same(g[key], w[key][:k], (what, key))
    assert np.array_equal(mb_tiles(got[2], k), mb_tiles(want[2], k)), (what, "reconstruction")


@pytest.mark.gpu
def test_entries_regrow_on_one_context(pkg, monkeypatch):
    rng = np.random.default_rng(5)
    cur, ref0, ref1 = pictures()

    # the staging buffer of 16-bit samples: first a picture plane (slot 1 of this context), then the 16 quarter-pel planes, then a plane again
    ctx = open_ctx(pkg, wide_slot1=True)
    fresh = open_ctx(pkg)
    want_planes = fresh.download_luma_planes(1)
    fresh.close()
    assert np.array_equal(ctx.download_luma_planes(1), want_planes)
    assert np.array_equal(ctx.download_luma_planes(1, np.uint16), want_planes)
    ctx.ref_upload(1, *(p.astype(np.uint16) for p in ref1))
    ctx.interp_luma(1)
    ctx.interp_chroma(1)
    assert np.array_equal(ctx.download_luma_planes(1), want_planes)
    assert np.array_equal(ctx.download_chroma_planes(1, 1, np.uint16), ctx.download_chroma_planes(1, 1))

    # distortion surfaces of one reference: a window per macroblock, some of them across the picture's border
    sjobs = np.zeros(N, dtype=pkg.SURFACE_JOB_DTYPE)
    sjobs["mb_x"], sjobs["mb_y"], sjobs["R"] = np.arange(N) % MBW, np.arange(N) // MBW, 4
    sjobs["cx"], sjobs["cy"] = rng.integers(-14, 15, N), rng.integers(-14, 15, N)
    for kind in ("sad_rows", "satd_blocks"):
        regrow(pkg, ctx, lambda c, j: c.distortion_surface(kind, j), sjobs, "distortion_surface " + kind)

    # the bi-predictive chain and the bi-predictive surfaces over both slots
    cjobs = chain_jobs(pkg.BIPRED_CHAIN_JOB_DTYPE, rng, MBW - 1, MBH - 1, 0)          # two jobs per macroblock of a 3 x 2 corner: 12
    assert len(cjobs) == N
    cprm = chain_params(pkg, lambda_factors(30), 0, None, 3, R, 2)

    def chain(c, jobs):
        res = c.bipred_chain(cprm, jobs)
        assert (res["n_steps"] == 6).all()                  # 1 + 3 integer steps, 2 sub-pel steps; the trace's other two entries are not written
        for key in ("step_smv", "step_mv_in", "step_mv_out", "step_min_in", "step_cost"):
            res[key][:, 6:] = 0
        return res
    regrow(pkg, ctx, chain, cjobs, "bipred_chain")
    bjobs = np.tile(bipred_surface_jobs(None), N // 3)
    bjobs["cx"] += np.arange(N) // 3
    for kind in ("sad_rows", "satd_blocks"):
        regrow(pkg, ctx, lambda c, j: c.bipred_surface(kind, j), bjobs, "bipred_surface " + kind)

    # transform / quantisation batches: the job and result arrays grow with the jobs, the quantiser array with the quantisers
    quants = quant_set(pkg, [17, 28, 36], 342, adaptive_rounding=1, adapt_rnd_weight=4, cavlc=1)
    tjobs = tq_jobs(pkg, rng, N, len(quants), 12)
    tjobs["quant"][:2] = tjobs["quant_dc"][:2] = 0
    fresh = open_ctx(pkg)
    want = fresh.tq_batch("luma4x4", quants, tjobs)
    fresh.close()
    for k in STEPS:
        same(ctx.tq_batch("luma4x4", quants[:1] if k == 2 else quants, tjobs[:k]), want[:k], ("tq_batch", k))

    # deblocking: a band of two macroblock rows (every row is a slice of its own with idc 2: the band's rows are the whole picture's), then all rows
    planes, dmbs, dblks = make_case(pkg, rng, W, H, FMT, idc_mode="two")
    fresh = open_ctx(pkg)
    fresh.recon_upload(*planes)
    fresh.deblock_frame(dmbs, dblks)
    want = fresh.recon_download()
    fresh.close()
    assert any((wv != p).any() for wv, p in zip(want, planes)), "the case does not exercise the filter"
    for rows in (2, MBH, 2):
        ctx.recon_upload(*planes)
        ctx.deblock_frame(dmbs, dblks, 4, 0, rows)
        for g, wv, p, mb_h in zip(ctx.recon_download(), want, planes, (16, 8, 8)):
            assert np.array_equal(g[:rows * mb_h], wv[:rows * mb_h]) and np.array_equal(g[rows * mb_h:], p[rows * mb_h:]), ("deblock_frame", rows)

    # the frame stage after the search stage: the ME group regrows, then the frame group; through the separate kernels (whose result arrays are
    # zeroed when they are allocated) and through the fused one; then with a second list of 2 and of 12 macroblocks
    mbs = make_mbs(pkg, rng, MBW, MBH, 6)
    bi = np.zeros(N, dtype=pkg.MB_BIPRED_DTYPE)
    bi["pdir"], bi["ref1"], bi["mv1"] = rng.integers(0, 3, (N, 4)), 1, rng.integers(-40, 41, (N, 16, 2))
    want = {}
    for second_list in (None, bi):
        for fused in (False, True):
            fresh = open_ctx(pkg)
            want[second_list is not None, fused] = frame_stage(pkg, fresh, mbs, second_list, monkeypatch, fused)
            fresh.close()
    for k, fused in ((2, True), (N, False), (2, False), (N, True)):
        check_frame_stage(frame_stage(pkg, ctx, mbs[:k], None, monkeypatch, fused), want[False, fused], k, ("frame stage", k, fused))
    for k, fused in ((2, False), (N, True), (N, False)):
        check_frame_stage(frame_stage(pkg, ctx, mbs[:k], bi[:k], monkeypatch, fused), want[True, fused], k, ("B frame stage", k, fused))

    # the reconstruction becomes slot 1 (the planes trade places), and the frame stage runs again into what were the slot's planes
    p_stage = frame_stage(pkg, ctx, mbs, None, monkeypatch, True)
    ctx.recon_to_ref(1)
    with pytest.raises(pkg.JmhipError):
        ctx.recon_download()
    ctx.interp_luma(1)
    assert np.array_equal(ctx.download_luma_planes(1)[0][0][20:20 + H, 20:20 + W], p_stage[2][0])
    again = frame_stage(pkg, ctx, mbs, None, monkeypatch, True)
    check_frame_stage(again, want[False, True], N, "frame stage after the plane swap")
    assert np.array_equal(ctx.download_luma_planes(1)[0][0][20:20 + H, 20:20 + W], p_stage[2][0])
    ctx.close()


@pytest.mark.gpu
def test_contexts_open_and_close_in_a_row(pkg):
    """three contexts one after the other in one process, the second in 4:2:2: each frees all it owns, and the next one works"""
    planes = []
    for fmt in (1, 2, 1):
        cur, ref = synth(np.random.default_rng(3), W, H, fmt)
        ctx = pkg.Context(W, H, yuv_format=fmt, max_refs=2, search_range=R)
        ctx.ref_upload(0, *ref)
        ctx.interp_luma(0)
        ctx.interp_chroma(0)
        ctx.cur_upload(*cur)
        me = ctx.me_frame(_params(pkg, R), make_mbs(pkg, np.random.default_rng(4), MBW, MBH, 6))
        planes.append((ctx.download_luma_planes(0), ctx.download_chroma_planes(0, 1), me))
        ctx.close()
    assert planes[1][1].shape != planes[0][1].shape
    for a, b in zip(planes[0], planes[2]):
        same(a, b, "first and third context")
