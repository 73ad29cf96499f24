"""The 4:4:4 frame stage on the device (frame444.hip: frame_fused444_kernel) and the 6-tap Cb / Cr planes it predicts from
(jmhip_interp_chroma444), against tests/frame444_ref.py. The inputs of every case are built on the host alone and the branch coverage of the
parametrisation is asserted on the helper's output (tests/test_frame_444.py, no GPU); the device cases check that the device's motion search is
the oracle's, which makes that expectation theirs."""
import numpy as np
import pytest

from tests import frame444_ref, oracle
from tests.test_frame_444 import CASES, R, build_inputs, host_expectation, ref_stacks
from tests.test_me import lambda_factors
from tests.test_tq import compare_lists


def me_params(pkg, qp):
    prm = pkg.MeParams()
    prm.search_mode, prm.search_range, prm.rdopt = -1, R, 1
    prm.level_mv_min, prm.level_mv_max = -511, 511
    prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lambda_factors(qp)
    prm.subpel, prm.partition_mask = 1, (1 << 41) - 1
    return prm


def open_context(pkg, inp, planes444=True):
    ctx = pkg.Context(inp["w"], inp["h"], yuv_format=3, max_refs=max(inp["slots"]) + 1, search_range=R)
    for slot, ref in zip(inp["slots"], inp["refs"]):
        ctx.ref_upload(slot, *ref)
        ctx.interp_luma(slot)
        if planes444:
            ctx.interp_chroma444(slot)
    ctx.cur_upload(*inp["cur"])
    return ctx


def stage(pkg, ctx, inp, cur=None, modes="given"):
    """me_frame + residual_frame on the context's current references; everything the stage leaves behind."""
    n = len(inp["mbs"])
    if cur is not None:
        ctx.cur_upload(*cur)
    me = ctx.me_frame(me_params(pkg, inp["qp"][0]), inp["mbs"])
    ctx.frame_wp_set(inp["wp"])
    ctx.frame_keep_prediction()
    ctx.residual_frame(inp["quants"], inp["modes"] if modes == "given" else None)
    return {"me": me, "got": ctx.residual_download(n), "recon": ctx.recon_download(), "pred": ctx.pred_download(),
            "records": ctx.residual_records444(n), "records8": ctx.residual_records8_444(n)}


def check_stage(pkg, inp, out, want, ar):
    """Pictures, every byte of the records and side records, jmhip_residual_download's expansion, cbp / cbp_blk."""
    t8 = want["t8"]
    for pl, nm in enumerate("YUV"):
        assert np.array_equal(out["recon"][pl], want["recon"][pl]), "reconstruction %s" % nm
        assert np.array_equal(out["pred"][pl], want["predpic"][pl]), "prediction picture %s" % nm
    for f in out["records"].dtype.names:
        assert np.array_equal(out["records"][f], want["records"][f]), "jmhip_mb_residual444.%s" % f
    assert out["records"].tobytes() == want["records"].tobytes()
    for f in out["records8"].dtype.names:
        assert np.array_equal(out["records8"][f], want["records8"][f]), "jmhip_mb_residual8.%s" % f
    assert out["records8"].tobytes() == want["records8"].tobytes()
    got = out["got"]
    for pl in range(3):
        g = got["luma"] if pl == 0 else got["chroma"][pl - 1::2]
        w = want["planes"][pl]
        compare_lists(g["levels"], g["runs"], w["levels"], w["runs"], "plane %d 4x4 / interleaved 8x8 lists" % pl)
        compare_lists(g["levels8"][t8], g["runs8"][t8], w["levels8"][t8], w["runs8"][t8], "plane %d 8x8 lists" % pl)
        assert np.array_equal(g["coeff_cost"][~t8], w["coeff_cost"][~t8]) and np.array_equal(g["coeff_cost"][t8][:, :4], w["coeff_cost"][t8][:, :4])
        assert np.array_equal(g["nonzero"][~t8], want["nonzero_before"][pl][~t8]) and np.array_equal(g["nonzero"][t8][:, :4], want["nonzero_before"][pl][t8][:, :4])
        assert np.array_equal(g["recon"], w["recon"])
        if ar:
            assert np.array_equal(g["fadjust"], w["fadjust"])
        if pl:
            assert np.array_equal(g["ret"], want["plane_cbp"][:, pl]) and np.array_equal(g["cbp_blk"], want["plane_cbp_blk"][:, pl]) and not g["cbp_clear"].any()
    assert np.array_equal(got["cbp"], want["cbp"]) and np.array_equal(got["cbp_blk"], want["cbp_blk"])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(64, 48), (16, 16)])
def test_chroma444_planes(pkg, w, h):
    """jmhip_interp_chroma444: all 16 planes of Cb and Cr, ring included, equal the oracle's getSubImagesLuma of U / V (16x16: a picture that is
    all border); jmhip_interp_chroma afterwards restores the bilinear planes; each consumer refuses the other kind."""
    inp = build_inputs(pkg, seed=3, w=w, h=h, qp=(28, 28, 28), cavlc=1, ar=1, far=6, given=False, t8="none")
    ref = inp["refs"][0]
    ctx = open_context(pkg, inp, planes444=False)
    try:
        with pytest.raises(pkg.JmhipError, match="chroma sub-pel planes not built"):
            ctx.download_chroma_planes(0, 0)
        ctx.interp_chroma444(0)
        for uv in range(2):
            want = oracle.interp_luma(ref[1 + uv])
            assert np.array_equal(ctx.download_chroma_planes(0, uv), want), "6-tap planes of component %d" % uv
            assert np.array_equal(ctx.download_chroma_rows(0, uv), want), "6-tap planes of component %d through the row pointers" % uv
        assert np.array_equal(ctx.download_luma_planes(0), oracle.interp_luma(ref[0]))
        # the chroma term of the motion search reads the bilinear planes and says so
        prm = me_params(pkg, 28)
        prm.metric_set, prm.chroma_me, prm.chroma_me_weight = 1, 1, 1
        prm.metric[0], prm.metric[1], prm.metric[2] = 0, 2, 2
        with pytest.raises(pkg.JmhipError, match="jmhip_interp_chroma\\)"):
            ctx.me_frame(prm, inp["mbs"])
        ctx.interp_chroma(0)
        for uv in range(2):
            assert np.array_equal(ctx.download_chroma_planes(0, uv), oracle.interp_chroma(ref[1 + uv], 3)), "bilinear planes of component %d after the 6-tap ones" % uv
        ctx.me_frame(prm, inp["mbs"])                          # ... and takes them
        # the frame stage refuses bilinear planes, and missing ones
        ctx.me_frame(me_params(pkg, 28), inp["mbs"])
        with pytest.raises(pkg.JmhipError, match="jmhip_interp_chroma444"):
            ctx.residual_frame(inp["quants"], None)
        ctx.ref_upload(0, *ref)
        ctx.interp_luma(0)
        with pytest.raises(pkg.JmhipError, match="jmhip_interp_chroma444"):
            ctx.residual_frame(inp["quants"], None)
        ctx.interp_chroma444(0)
        ctx.residual_frame(inp["quants"], None)               # the context is still usable
        assert ctx.recon_download()[1].shape == (h, w)
    finally:
        ctx.close()
    ctx = pkg.Context(64, 48, yuv_format=1, search_range=R)
    try:
        with pytest.raises(pkg.JmhipError, match="4:4:4 contexts only"):
            ctx.interp_chroma444(0)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_stage_444(pkg, name):
    inp, me, modes, want = host_expectation(pkg, name)
    ctx = open_context(pkg, inp)
    try:
        out = stage(pkg, ctx, inp)
        ctx.frame_wp_set(None)
    finally:
        ctx.close()
    # the device's search is the oracle's, so the expectation is the one whose branch coverage the CPU test asserts
    for k in ("mv_int", "cost_int", "mv", "cost"):
        assert np.array_equal(out["me"][k], me[k]), "motion search field %s" % k
    gm = out["got"]["modes"]
    assert np.array_equal(gm["mode"], modes["mode"]) and np.array_equal(gm["pad"][:, 0], modes["pad"][:, 0])
    if inp["modes"] is None:
        assert np.array_equal(gm["b8mode"], modes["b8mode"])
    if CASES[name]["t8"] == "some" and len(inp["mbs"]) > 1:
        assert inp["t8"].any() and (~inp["t8"]).any()
    check_stage(pkg, inp, out, want, inp["ar"])


@pytest.mark.gpu
def test_y_plane_equals_the_420_stage_luma(pkg):
    """frame_fused444_kernel and frame_fused_kernel run one block body (frame_block.h) on their own views of it: on the same Y picture, vectors,
    given modes (8x8 transform on macroblock 0, off on 1, mixed after), CAVLC, adaptive rounding, explicit weights and Y quantisers, plane 0 of the
    4:4:4 records is the luma of the 4:2:0 records, byte for byte. 80x48: 15 macroblocks, a last workgroup of three live macroblocks and a spare."""
    inp = build_inputs(pkg, seed=41, w=80, h=48, qp=(28, 28, 28), cavlc=1, ar=1, far=6, given=True, t8="some", weighted=True)
    n, q = len(inp["mbs"]), inp["quants"]
    assert n == 15 and inp["t8"][0] and not inp["t8"][1]
    sub = lambda p: np.ascontiguousarray(p[::2, ::2])
    ctx = open_context(pkg, inp)
    try:
        out = stage(pkg, ctx, inp)
    finally:
        ctx.close()
    ctx = pkg.Context(inp["w"], inp["h"], yuv_format=1, max_refs=1, search_range=R)
    try:
        ref, cur = inp["refs"][0], inp["cur"]
        ctx.ref_upload(0, ref[0], sub(ref[1]), sub(ref[2]))
        ctx.interp_luma(0)
        ctx.interp_chroma(0)
        ctx.cur_upload(cur[0], sub(cur[1]), sub(cur[2]))
        me = ctx.me_frame(me_params(pkg, inp["qp"][0]), inp["mbs"])
        ctx.frame_wp_set(inp["wp"])
        ctx.frame_keep_prediction()
        chroma_dc = pkg.flat_quant(31, 342, adaptive_rounding=1, adapt_rnd_weight=4, cavlc=1)
        ctx.residual_frame(np.array([q[0], q[0], chroma_dc, q[3]], dtype=pkg.QUANT_DTYPE), inp["modes"])
        got, rec, rec8, recon, pred = ctx.residual_download(n, want_results=False), ctx.residual_records(n), ctx.residual_records8(n), ctx.recon_download(), ctx.pred_download()
    finally:
        ctx.close()
    assert np.array_equal(out["me"]["mv"], me["mv"]) and np.array_equal(out["me"]["cost"], me["cost"])
    r444 = out["records"]
    # the lists over their cnt entries: frame_fused_kernel does not zero its record first, so what follows a list there is not defined
    assert np.array_equal(r444["cnt"][:, 0], rec["cnt"][:, :16]), "plane 0 of jmhip_mb_residual444.cnt"
    listed = np.arange(16) < rec["cnt"][:, :16, None]
    for f in ("lev", "run"):
        assert np.array_equal(r444[f][:, 0][listed], rec[f][:, :16][listed]) and not r444[f][:, 0][~listed].any(), "plane 0 of jmhip_mb_residual444.%s" % f
    for f444, f420 in (("coeff_cost", "coeff_cost"), ("nonzero", "nonzero"), ("fadj", "fadj_y"), ("recon", "recon_y")):
        assert np.array_equal(r444[f444][:, 0], rec[f420]), "plane 0 of jmhip_mb_residual444.%s" % f444
    assert r444["lev"][:, 0].any() and r444["fadj"][:, 0].any() and rec8["lev"].any()
    assert out["records8"][:, 0].tobytes() == rec8.tobytes()
    assert np.array_equal(out["recon"][0], recon[0]) and np.array_equal(out["pred"][0], pred[0])
    assert np.array_equal(r444["plane_cbp"][:, 0], got["cbp"] & 15) and np.array_equal(r444["plane_cbp_blk"][:, 0], got["cbp_blk"] & 0xffff)


@pytest.mark.gpu
def test_chain_recon_becomes_the_reference(pkg):
    """jmhip_recon_to_ref after the stage, both interpolations again, a second picture's stage: equal to the helper run on the FIRST picture's
    expected reconstruction."""
    inp, me, modes, want = host_expectation(pkg, "planes_at_their_own_qp")
    cur2 = tuple(np.roll(p, (1, 2), (0, 1)) for p in inp["cur"])
    ctx = open_context(pkg, inp)
    try:
        first = stage(pkg, ctx, inp)
        ctx.recon_to_ref(0)
        with pytest.raises(pkg.JmhipError):                   # the slot's planes are stale until they are rebuilt
            ctx.download_chroma_planes(0, 0)
        ctx.interp_luma(0)
        ctx.interp_chroma444(0)
        second = stage(pkg, ctx, inp, cur=cur2)
    finally:
        ctx.close()
    for pl in range(3):
        assert np.array_equal(first["recon"][pl], want["recon"][pl])
    rec1 = tuple(want["recon"])
    me2 = oracle.me_frame(oracle.me_params(rdopt=1), [oracle.RefPic(rec1[0])], cur2[0], inp["mbs"], -1, R, lambda_factors(inp["qp"][0]))
    assert np.array_equal(second["me"]["mv"], me2["mv"]) and np.array_equal(second["me"]["cost"], me2["cost"])
    want2 = frame444_ref.residual_frame444(pkg, [frame444_ref.Ref444(*rec1)], cur2, inp["mbs"], me2["mv"], inp["modes"], inp["quants"])
    check_stage(pkg, inp, second, want2, inp["ar"])


@pytest.mark.gpu
def test_refusals_444(pkg):
    """Each case the stage does not take raises with its message and leaves the context usable."""
    inp, me, modes, want = host_expectation(pkg, "qp28_cavlc_ar_t8_some")
    n, q = len(inp["mbs"]), inp["quants"]
    ctx = open_context(pkg, inp)
    try:
        ctx.me_frame(me_params(pkg, 28), inp["mbs"])
        with pytest.raises(pkg.JmhipError, match="3 quantisers \\(Y, Cb, Cr\\) or 6"):
            ctx.residual_frame(q[:5], None)
        with pytest.raises(pkg.JmhipError, match="3 quantisers \\(Y, Cb, Cr\\) or 6"):
            ctx.residual_frame(q[:4], None)
        flagged = q[:3].copy()
        flagged[1]["transform8x8_flag"] = 1
        with pytest.raises(pkg.JmhipError, match="transform8x8_flag belongs to quants\\[3..5\\]"):
            ctx.residual_frame(flagged, None)
        with pytest.raises(pkg.JmhipError, match="bad macroblock mode"):      # flagged macroblocks need the six
            ctx.residual_frame(q[:3], inp["modes"])
        for bad in (-1, 32768):
            w = q.copy()
            w[2]["adapt_rnd_weight"] = bad
            with pytest.raises(pkg.JmhipError, match="not supported.*adapt_rnd_weight outside 0..32767"):
                ctx.residual_frame(w, inp["modes"])
        bi = np.zeros(n, dtype=pkg.MB_BIPRED_DTYPE)
        ctx.frame_bipred_set(bi)
        with pytest.raises(pkg.JmhipError, match="not supported.*jmhip_frame_bipred_set"):
            ctx.residual_frame(q, inp["modes"])
        ctx.frame_bipred_set(None)
        with pytest.raises(pkg.JmhipError):                   # no stage yet: nothing to download
            ctx.residual_records444(n)
        ctx.residual_frame(q, inp["modes"])                   # still usable: the stage runs and is right
        assert ctx.residual_records444(n).tobytes() == want["records"].tobytes()
        # the wrong record download after the stage; the loop filter fed from the device
        for call, msg in ((lambda: ctx.residual_records(n), "jmhip_residual_records444_download"), (lambda: ctx.residual_records422(n), "jmhip_residual_records444_download"),
                          (lambda: ctx.residual_records8(n), "jmhip_residual_records8_444_download"), (lambda: ctx.deblock_recon(28), "not supported.*three planes")):
            with pytest.raises(pkg.JmhipError, match=msg):
                call()
        with pytest.raises(pkg.JmhipError, match="more macroblocks requested"):
            ctx.residual_records444(n + 1)
        for pl in range(3):
            assert np.array_equal(ctx.recon_download()[pl], want["recon"][pl])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_slice_handover_refused_444(pkg):
    """Modes handed over from the slice search are out of scope for 4:4:4: refused, and a frame search afterwards feeds the stage again."""
    from tests.test_slice_gpu import slice_params
    inp, me, modes, want = host_expectation(pkg, "qp24_cavlc_ar_chosen")
    n = len(inp["mbs"])
    ctx = open_context(pkg, inp)
    try:
        ctx.slice_state_reset()
        lam = lambda_factors(24)[0]
        p = slice_params(pkg, -1, R, 1, [lam] * 3, 8, inp["w"], mb_first=0, mb_count=n, t8=0, qp_n=24)
        p.ref_slot[0] = 0
        ctx.p_slice_search(p)
        ctx.slice_to_frame([0])
        with pytest.raises(pkg.JmhipError, match="not supported.*jmhip_slice_to_frame"):
            ctx.residual_frame(inp["quants"], None)
        out = stage(pkg, ctx, inp, modes="chosen")
    finally:
        ctx.close()
    check_stage(pkg, inp, out, want, inp["ar"])


@pytest.mark.gpu
def test_other_formats_untouched_after_444(pkg):
    """A 4:2:0 context in the same process still runs its fused stage and its record download after a 4:4:4 context was used."""
    from tests.test_frame import synth
    from tests.test_me import make_mbs
    inp, me, modes, want = host_expectation(pkg, "qp24_cavlc_ar_chosen")
    ctx = open_context(pkg, inp)
    try:
        stage(pkg, ctx, inp, modes="chosen")
    finally:
        ctx.close()
    rng = np.random.default_rng(11)
    w, h, qp = 64, 48, 28
    cur, ref = synth(rng, w, h, 1)
    mbs = make_mbs(pkg, rng, w // 16, h // 16, 6)
    quants = np.array([pkg.flat_quant(qp + d, 342, adaptive_rounding=1, adapt_rnd_weight=4, cavlc=1) for d in (0, 0, 3)], dtype=pkg.QUANT_DTYPE)
    ctx = pkg.Context(w, h, yuv_format=1, max_refs=1, search_range=R)
    try:
        ctx.ref_upload(0, *ref)
        ctx.interp_luma(0)
        ctx.interp_chroma(0)
        ctx.cur_upload(*cur)
        got_me = ctx.me_frame(me_params(pkg, qp), mbs)
        ctx.residual_frame(quants, None)
        got, recon, records = ctx.residual_download(len(mbs)), ctx.recon_download(), ctx.residual_records(len(mbs))
        with pytest.raises(pkg.JmhipError, match="not a 4:4:4 one"):
            ctx.residual_records444(len(mbs))
    finally:
        ctx.close()
    rp = oracle.RefPic(*ref, yuv_format=1)
    yard = oracle.residual_frame(rp, cur, mbs, got_me["mv"], got["modes"], quants, pkg.TQ_JOB_DTYPE, yuv_format=1)
    for g, wv, name in zip(recon, yard["recon"], "YUV"):
        assert np.array_equal(g, wv), "4:2:0 reconstruction %s" % name
    assert np.array_equal(got["cbp"], yard["cbp"]) and np.array_equal(got["cbp_blk"], yard["cbp_blk"])
    assert np.array_equal(records["recon_y"], yard["luma"]["recon"])
