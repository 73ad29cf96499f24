"""The fused 4:2:0 frame stage with 8x8-transform macroblocks (luma_transform_size_8x8_flag): against the oracle's residual_frame and,
byte for byte, against the separate kernels (JMHIP_FRAME_FUSED=0) -- result structs, cbp, reconstruction, deblocked picture -- plus the
dense records, the 8x8 side records (jmhip_mb_residual8) and the prediction picture that only the fused stage leaves."""
import numpy as np
import pytest

from tests import oracle
from tests.test_frame import synth
from tests.test_me import lambda_factors, make_mbs
from tests.quant_tables import scaled_quant
from tests.test_tq import compare_lists

LUMA_FIELDS = ("levels", "runs", "levels8", "runs8", "coeff_cost", "nonzero", "recon", "fadjust")


def draw_quants(pkg, rng, qp, kw, scaling, qpc=None):
    """The frame stage's records: luma 4x4, chroma, chroma DC (qp + 3), luma 8x8. scaling True: the 8x8 record alone carries a scaling
    matrix; "all": each of the four gets a scaling matrix and per-position rounding offsets of its own (tests/quant_tables.py)."""
    flat = lambda d: pkg.flat_quant(qp + d, 342, **kw)
    if scaling == "all":
        qpc = qp if qpc is None else qpc                     # the chroma quantiser may sit below the luma one (chroma_qp_index_offset)
        quants = [scaled_quant(pkg, q, rng, False, **kw) for q in (qp, qpc, qpc + 3)] + [scaled_quant(pkg, qp, rng, True, transform8x8_flag=1, **kw)]
    elif scaling:
        quants = [flat(0), flat(0), flat(3), scaled_quant(pkg, qp, rng, True, offsets=False, transform8x8_flag=1, **kw)]
    else:
        quants = [flat(0), flat(0), flat(3), pkg.flat_quant(qp, 342, is8x8=True, transform8x8_flag=1, **kw)]
    return np.array(quants, dtype=pkg.QUANT_DTYPE)


def draw_inputs(pkg, *, w, h, qp, cavlc, ar, far, weighted, scaling, seed, all_t8=False, no_t8=False, qpc=None, **unused):
    """Everything a case feeds the frame stage with, drawn on the host (no device involved)."""
    rng = np.random.default_rng(seed)
    cur, ref = synth(rng, w, h, 1)
    mbs = make_mbs(pkg, rng, w // 16, h // 16, 4 * far)
    n = len(mbs)
    kw = dict(adaptive_rounding=ar, adapt_rnd_weight=4 if ar else 0, cavlc=cavlc)
    quants = draw_quants(pkg, rng, qp, kw, scaling, qpc)
    modes = np.zeros(n, dtype=pkg.MB_MODE_DTYPE)
    modes["mode"] = rng.choice([1, 2, 3, 8], n)
    modes["b8mode"] = rng.integers(4, 8, (n, 4))
    t8 = np.ones(n, bool) if all_t8 else rng.integers(0, 2, n).astype(bool)
    t8[0] = True
    if no_t8:                                                # a 4x4-only picture: the stage's 4x4 instantiation, three records
        t8[:] = False
        quants = quants[:3]
    modes["b8mode"][t8] = 4
    modes["pad"][:, 0] = t8
    wp = None
    if weighted:
        wp = {"luma_round": 16, "luma_denom": 5, "chroma_round": 4, "chroma_denom": 3, "weight": np.zeros((16, 3), int), "offset": np.zeros((16, 3), int)}
        wp["weight"][0], wp["offset"][0] = (29, 9, 7), (4, -2, 1)
    return dict(cur=cur, ref=ref, mbs=mbs, quants=quants, modes=modes, t8=t8, wp=wp)


def run_case(pkg, monkeypatch, *, fused, **case):
    """One frame stage on a fresh context; returns its inputs and everything it left behind."""
    if not fused:
        monkeypatch.setenv("JMHIP_FRAME_FUSED", "0")
    else:
        monkeypatch.delenv("JMHIP_FRAME_FUSED", raising=False)
    w, h, qp, R = case["w"], case["h"], case["qp"], 8
    out = draw_inputs(pkg, **case)
    n = len(out["mbs"])
    ctx = pkg.Context(w, h, yuv_format=1, max_refs=1, search_range=R)
    try:
        ctx.ref_upload(0, *out["ref"])
        ctx.interp_luma(0)
        if case["chroma_planes"]:
            ctx.interp_chroma(0)
        ctx.cur_upload(*out["cur"])
        lam = lambda_factors(qp)
        prm = pkg.MeParams()
        prm.search_mode, prm.search_range, prm.rdopt = -1, R, 1
        prm.level_mv_min, prm.level_mv_max = -511, 511
        prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lam
        prm.transform8x8_mode, prm.subpel, prm.partition_mask = 1, 1, (1 << 41) - 1
        out["me"] = ctx.me_frame(prm, out["mbs"])
        ctx.frame_wp_set(out["wp"])
        if fused:
            ctx.frame_keep_prediction()
        ctx.residual_frame(out["quants"], out["modes"])
        out.update(got=ctx.residual_download(n), recon=ctx.recon_download())
        if fused:
            out["records"], out["records8"], out["pred"] = ctx.residual_records(n), ctx.residual_records8(n), ctx.pred_download()
        else:
            with pytest.raises(pkg.JmhipError):
                ctx.residual_records8(n)
        ctx.deblock_recon(qp)
        out["deblocked"] = ctx.recon_download()
    finally:
        ctx.close()
    return out


def check_against_oracle(pkg, o, ar, check_records=True):
    mbs, t8, quants = o["mbs"], o["t8"], o["quants"]
    got, recon = o["got"], o["recon"]
    rp = oracle.RefPic(o["ref"][0], o["ref"][1], o["ref"][2], yuv_format=1)
    n = len(mbs)
    want = oracle.residual_frame([rp], o["cur"], mbs, o["me"]["mv"], o["modes"], quants, pkg.TQ_JOB_DTYPE, yuv_format=1,
                                 blk_ref=np.zeros((n, 4), int), wp=o["wp"])
    wl = want["luma"]
    compare_lists(got["luma"]["levels"], got["luma"]["runs"], wl["levels"], wl["runs"], "luma 4x4 / interleaved 8x8 lists")
    compare_lists(got["luma"]["levels8"][t8], got["luma"]["runs8"][t8], wl["levels8"][t8], wl["runs8"][t8], "luma 8x8 lists")
    assert np.array_equal(got["luma"]["coeff_cost"][~t8], wl["coeff_cost"][~t8])
    assert np.array_equal(got["luma"]["coeff_cost"][t8][:, :4], wl["coeff_cost"][t8][:, :4])
    assert np.array_equal(got["luma"]["recon"], wl["recon"])
    if ar:
        assert np.array_equal(got["luma"]["fadjust"], wl["fadjust"])
    assert np.array_equal(got["cbp"], want["cbp"])
    assert np.array_equal(got["cbp_blk"], want["cbp_blk"])
    for g, wv, name in zip(recon, want["recon"], "YUV"):
        assert np.array_equal(g, wv), "recon %s" % name
    if not check_records:
        return want
    recs, recs8, pred = o["records"], o["records8"], o["pred"]
    for i, mb in enumerate(mbs):
        r, r8, x, y = recs[i], recs8[i], 16 * int(mb["mb_x"]), 16 * int(mb["mb_y"])
        assert np.array_equal(pred[0][y:y + 16, x:x + 16], want["jobs_y"][i]["pred"]), "luma prediction of macroblock %d" % i
        for uv in range(2):
            assert np.array_equal(pred[1 + uv][y // 2:y // 2 + 8, x // 2:x // 2 + 8], want["jobs_c"][2 * i + uv]["pred"][:8, :8]), "chroma prediction of macroblock %d" % i
        assert np.array_equal(r["recon_y"], wl["recon"][i])
        if ar:
            assert np.array_equal(r["fadj_y"], wl["fadjust"][i])
        if not t8[i]:
            assert not r8.tobytes().strip(b"\0"), "side record of 4x4-transform macroblock %d is not zero" % i
            continue
        # 8x8 transform: the jmhip_mb_residual luma lists / costs / nonzero read 0, the side record holds dct_8x8's results
        assert int(r["nonzero"]) == 0 and not r["cnt"][:16].any() and not r["coeff_cost"].any() and not r["lev"][:16].any()
        assert int(r8["transform8x8"]) == 1 and int(r8["interleaved"]) == int(quants[3]["cavlc"])
        for b8 in range(4):
            assert int(r8["coeff_cost"][b8]) == int(wl["coeff_cost"][i, b8]) and int(r8["nonzero"][b8]) == int(wl["nonzero"][i, b8])
            if r8["interleaved"]:
                for k in range(4):
                    c = int(r8["cnt"][b8, k])
                    assert np.array_equal(r8["lev"][b8, 16 * k:16 * k + c], wl["levels"][i, 4 * b8 + k, :c]) and wl["levels"][i, 4 * b8 + k, c] == 0
                    assert np.array_equal(r8["run"][b8, 16 * k:16 * k + c], wl["runs"][i, 4 * b8 + k, :c])
            else:
                c = int(r8["cnt"][b8, 0])
                assert np.array_equal(r8["lev"][b8, :c], wl["levels8"][i, b8, :c]) and wl["levels8"][i, b8, c] == 0
                assert np.array_equal(r8["run"][b8, :c], wl["runs8"][i, b8, :c])
    return want


def check_against_separate(a, b):
    """The fused stage (a) and the separate kernels (b) on the same inputs: identical downloads, pictures and deblocked pictures."""
    for f in LUMA_FIELDS:
        assert np.array_equal(a["got"]["luma"][f], b["got"]["luma"][f]), "luma %s" % f
    ca, cb = a["got"]["chroma"], b["got"]["chroma"]
    compare_lists(ca["levels"][:, :4, :16], ca["runs"][:, :4, :16], cb["levels"][:, :4, :16], cb["runs"][:, :4, :16], "chroma AC")
    compare_lists(ca["dc_levels"][:, None], ca["dc_runs"][:, None], cb["dc_levels"][:, None], cb["dc_runs"][:, None], "chroma DC")
    for f in ("ret", "cbp_blk", "cbp_clear"):
        assert np.array_equal(ca[f], cb[f]), "chroma %s" % f
    assert np.array_equal(ca["recon"][:, :8, :8], cb["recon"][:, :8, :8])
    for f in ("cbp", "cbp_blk"):
        assert np.array_equal(a["got"][f], b["got"][f]), f
    assert a["got"]["modes"].tobytes() == b["got"]["modes"].tobytes()
    for pa, pb, name in zip(a["recon"], b["recon"], "YUV"):
        assert np.array_equal(pa, pb), "recon %s" % name
    for pa, pb, name in zip(a["deblocked"], b["deblocked"], "YUV"):
        assert np.array_equal(pa, pb), "deblocked %s" % name


CASES = {
    "cavlc_ar": dict(w=64, h=48, qp=28, cavlc=1, ar=1, far=6, chroma_planes=True, weighted=False, scaling=False),
    "cabac_ar": dict(w=64, h=48, qp=22, cavlc=0, ar=1, far=6, chroma_planes=True, weighted=False, scaling=False),
    "cavlc_no_ar": dict(w=64, h=48, qp=30, cavlc=1, ar=0, far=6, chroma_planes=True, weighted=False, scaling=False),
    "cabac_no_ar_low_qp": dict(w=64, h=48, qp=12, cavlc=0, ar=0, far=6, chroma_planes=True, weighted=False, scaling=False),
    "far_planes": dict(w=64, h=48, qp=34, cavlc=1, ar=1, far=45, chroma_planes=True, weighted=False, scaling=False),
    "far_no_planes": dict(w=64, h=48, qp=26, cavlc=0, ar=1, far=90, chroma_planes=False, weighted=False, scaling=False),
    "weighted": dict(w=64, h=48, qp=26, cavlc=1, ar=1, far=6, chroma_planes=True, weighted=True, scaling=False),
    "scaling_matrix": dict(w=64, h=48, qp=24, cavlc=0, ar=1, far=6, chroma_planes=True, weighted=False, scaling=True),
    "scaling_matrix_cavlc": dict(w=64, h=48, qp=20, cavlc=1, ar=0, far=6, chroma_planes=True, weighted=False, scaling=True),
    "high_qp": dict(w=64, h=48, qp=44, cavlc=1, ar=1, far=6, chroma_planes=True, weighted=False, scaling=False),
    "tail_wave": dict(w=80, h=48, qp=26, cavlc=0, ar=1, far=6, chroma_planes=False, weighted=False, scaling=False),   # 15 macroblocks
    "tail_wave_one": dict(w=48, h=48, qp=28, cavlc=1, ar=1, far=6, chroma_planes=True, weighted=True, scaling=False),  # 9 macroblocks
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_t8_frame_stage(pkg, monkeypatch, name):
    kw = CASES[name]
    seed = 100 + sorted(CASES).index(name)
    a = run_case(pkg, monkeypatch, fused=True, seed=seed, **kw)
    b = run_case(pkg, monkeypatch, fused=False, seed=seed, **kw)
    assert a["t8"].any() and (~a["t8"]).any()
    check_against_separate(a, b)
    check_against_oracle(pkg, a, kw["ar"])
    # the thresholds and the 8x8 lists are exercised somewhere across the parametrisation
    assert (a["got"]["cbp"][a["t8"]] & 15).max() > 0 or kw["qp"] >= 34


# Scaling matrices AND per-position rounding offsets, asymmetric, a set of their own for each of luma 4x4, chroma, chroma DC and luma 8x8
# (the stage takes one chroma quantiser per call, so Cb and Cr share theirs). no_t8: a 4x4-only picture, the stage's 4x4 instantiation.
# qpc: synth's chroma carries a quarter of the luma's amplitude; at the luma QP its AC levels are too few for the chroma tables to show.
TABLE_CASES = {
    "tables_t8_cabac_ar": dict(w=64, h=48, qp=24, cavlc=0, ar=1, far=6, chroma_planes=True, weighted=False, scaling="all", qpc=10, seed=311),
    "tables_t8_cavlc": dict(w=64, h=48, qp=20, cavlc=1, ar=0, far=6, chroma_planes=False, weighted=False, scaling="all", qpc=10, seed=312),
    "tables_4x4_only_cavlc_ar": dict(w=64, h=48, qp=26, cavlc=1, ar=1, far=6, chroma_planes=True, weighted=False, scaling="all", qpc=10, no_t8=True, seed=313),
    "tables_4x4_only_cabac": dict(w=64, h=48, qp=18, cavlc=0, ar=0, far=6, chroma_planes=False, weighted=True, scaling="all", qpc=10, no_t8=True, seed=314),
    "tables_tail_wave": dict(w=80, h=48, qp=22, cavlc=1, ar=1, far=6, chroma_planes=True, weighted=False, scaling="all", qpc=10, seed=315),   # 15 macroblocks
}


def frame_differences(got, recon, want, t8, ar):
    """What check_against_oracle compares of the downloads, as the list of names that differ; got / recon: the device's, or a second oracle run's
    (its "luma" / "chroma" dicts and "recon" pictures)."""
    bad = []

    def lists(name, *a):
        try:
            compare_lists(*a, name)
        except AssertionError:
            bad.append(name)
    gl, wl, gc, wc = got["luma"], want["luma"], got["chroma"], want["chroma"]
    lists("luma levels", gl["levels"], gl["runs"], wl["levels"], wl["runs"])
    lists("luma levels8", gl["levels8"][t8], gl["runs8"][t8], wl["levels8"][t8], wl["runs8"][t8])
    lists("chroma levels", gc["levels"][:, :4, :16], gc["runs"][:, :4, :16], wc["levels"][:, :4, :16], wc["runs"][:, :4, :16])
    lists("chroma dc_levels", gc["dc_levels"][:, None], gc["dc_runs"][:, None], wc["dc_levels"][:, None], wc["dc_runs"][:, None])
    same = lambda name, a, b: None if np.array_equal(a, b) else bad.append(name)
    same("luma coeff_cost", gl["coeff_cost"][~t8], wl["coeff_cost"][~t8])
    same("luma coeff_cost", gl["coeff_cost"][t8][:, :4], wl["coeff_cost"][t8][:, :4])
    same("luma recon", gl["recon"], wl["recon"])
    same("chroma recon", gc["recon"][:, :8, :8], wc["recon"][:, :8, :8])
    same("chroma ret", gc["ret"], wc["ret"])
    if ar:
        same("luma fadjust", gl["fadjust"], wl["fadjust"])
        same("chroma fadjust", gc["fadjust"][:, :8, :8], wc["fadjust"][:, :8, :8])
    same("cbp", got["cbp"], want["cbp"])
    same("cbp_blk", got["cbp_blk"], want["cbp_blk"])
    for g, wv, name in zip(recon, want["recon"], "YUV"):
        same("picture recon %s" % name, g, wv)
    return bad


_table_refs = {}


def table_reference(pkg, name):
    """Inputs, the oracle's motion search and its expectation for a TABLE_CASES entry -- built once, checked for the tables to bite, shared."""
    if name not in _table_refs:
        from tests.quant_tables import is_asymmetric, mutated, table_size
        from tests.test_tq import assert_tables_bite
        kw = TABLE_CASES[name]
        inp = draw_inputs(pkg, **kw)
        for q in inp["quants"]:
            assert all(is_asymmetric(q[t], table_size(q)) for t in ("levelscale", "invlevelscale", "leveloffset"))
        rp = oracle.RefPic(*inp["ref"], yuv_format=1)
        me = oracle.me_frame(oracle.me_params(rdopt=1, transform8x8_mode=1), [rp], inp["cur"][0], inp["mbs"], -1, 8, lambda_factors(kw["qp"]))
        n = len(inp["mbs"])
        run = lambda quants: oracle.residual_frame([rp], inp["cur"], inp["mbs"], me["mv"], inp["modes"], quants, pkg.TQ_JOB_DTYPE, yuv_format=1,
                                                   blk_ref=np.zeros((n, 4), int), wp=inp["wp"])
        want = run(inp["quants"])
        # 4:2:0 reads its chroma DC from the chroma record at (0, 0) and never opens record 2 (block.c:1094-1107), so no mutation of it can show
        groups = {"luma4x4": ([0], False), "chroma": ([1], False)}
        if inp["t8"].any():
            groups["luma8x8"] = ([3], False)
        if inp["t8"].all():
            del groups["luma4x4"]

        def differ(ks, how):
            other = run(mutated(inp["quants"], ks, how))
            return frame_differences(other, other["recon"], want, inp["t8"], kw["ar"])
        assert_tables_bite(differ, groups, name)
        _table_refs[name] = (inp, me, want)
    return _table_refs[name]


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_tables_are_asymmetric_where_it_matters(pkg, name):
    """No GPU: on the oracle, each of the luma 4x4, chroma and luma 8x8 records of every TABLE_CASES entry changes a compared output when its
    levelscale, invlevelscale or leveloffset is transposed or its leveloffset flattened to the mean (tests/test_tq.py assert_tables_bite)."""
    inp, me, want = table_reference(pkg, name)
    assert TABLE_CASES[name].get("no_t8") or (inp["t8"].any() and (~inp["t8"]).any())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_frame_stage_asymmetric_tables(pkg, monkeypatch, name):
    """The fused 4:2:0 stage (4x4-only and mixed with 8x8-transform macroblocks) and the separate kernels on asymmetric scaling matrices and
    rounding offsets: against each other and against the oracle -- result structs, cbp, cbp_blk, reconstruction, dense records, side records,
    prediction picture."""
    kw = TABLE_CASES[name]
    inp, me, want = table_reference(pkg, name)              # asserts that the tables bite before anything is compared
    a = run_case(pkg, monkeypatch, fused=True, **kw)
    b = run_case(pkg, monkeypatch, fused=False, **kw)
    for o in (a, b):
        assert np.array_equal(o["me"]["mv"], me["mv"]) and o["quants"].tobytes() == inp["quants"].tobytes()
        assert frame_differences(o["got"], o["recon"], want, inp["t8"], kw["ar"]) == []
    check_against_separate(a, b)
    check_against_oracle(pkg, a, kw["ar"])
    check_against_oracle(pkg, b, kw["ar"], check_records=False)


@pytest.mark.gpu
def test_fused_t8_frame_stage_1080p(pkg, monkeypatch):
    """One full-size picture whose every macroblock uses the 8x8 transform."""
    kw = dict(w=1920, h=1088, qp=28, cavlc=0, ar=1, far=20, chroma_planes=True, weighted=False, scaling=False, all_t8=True)
    a = run_case(pkg, monkeypatch, fused=True, seed=7, **kw)
    b = run_case(pkg, monkeypatch, fused=False, seed=7, **kw)
    assert a["t8"].all()
    check_against_separate(a, b)
    check_against_oracle(pkg, a, 1, check_records=False)
    assert int(a["records8"]["transform8x8"].sum()) == len(a["mbs"])
    assert np.array_equal(a["records8"]["coeff_cost"], a["got"]["luma"]["coeff_cost"][:, :4])


@pytest.mark.gpu
def test_records8_zero_for_4x4_only_pictures(pkg, monkeypatch):
    """A 4x4-only picture keeps the 4x4 kernel; its side records read zero."""
    monkeypatch.delenv("JMHIP_FRAME_FUSED", raising=False)
    rng = np.random.default_rng(3)
    w, h, R, qp = 64, 48, 8, 28
    cur, ref = synth(rng, w, h, 1)
    ctx = pkg.Context(w, h, yuv_format=1, max_refs=1, search_range=R)
    try:
        ctx.ref_upload(0, *ref)
        ctx.interp_luma(0)
        ctx.interp_chroma(0)
        ctx.cur_upload(*cur)
        mbs = make_mbs(pkg, rng, w // 16, h // 16, 6)
        prm = pkg.MeParams()
        prm.search_mode, prm.search_range, prm.rdopt = -1, R, 1
        prm.level_mv_min, prm.level_mv_max = -511, 511
        prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lambda_factors(qp)
        prm.subpel, prm.partition_mask = 1, (1 << 41) - 1
        ctx.me_frame(prm, mbs)
        quants = np.array([pkg.flat_quant(qp + d, 342, adaptive_rounding=1, adapt_rnd_weight=4, cavlc=1) for d in (0, 0, 3)], dtype=pkg.QUANT_DTYPE)
        ctx.residual_frame(quants, None)
        r8 = ctx.residual_records8(len(mbs))
    finally:
        ctx.close()
    assert not r8.tobytes().strip(b"\0")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,t8,slot_of", [(3, 1, (1, 0)), (-1, 1, (9, 0)), (3, 2, (0, 11)), (-1, 2, (1, 0))])
def test_slice_search_with_8x8_transform_feeds_the_fused_stage(pkg, monkeypatch, mode, t8, slot_of):
    """A Transform8x8Mode 1 / 2 slice search (EPZS, FullSearch; two references) hands its decided picture to the frame stage on the device
    (jmhip_slice_to_frame): the modes it leaves carry luma_transform_size_8x8_flag, so the fused stage's 8x8 instantiation runs. Records,
    side records, prediction picture, reconstruction and cbp against the oracle fed with the slice records. Reference slots 9 and 11:
    jmhip_slice_to_frame takes every allocated slot (the chroma planes are built, so no 0..7 limit applies)."""
    from tests.test_slice_gpu import slice_params, synth_clip, upsampled_chroma
    monkeypatch.delenv("JMHIP_FRAME_FUSED", raising=False)
    W, H, R, nref, qp = 176, 144, 16, 2, 28
    rng = np.random.default_rng(31 + t8)
    clip = synth_clip(rng, W, H, 3)
    clip[0] = np.clip(clip[0].astype(int) + 9, 0, 255).astype(np.uint8)        # a brightness step, so that reference 1 wins for some blocks
    cur, refs = clip[2], [clip[1], clip[0]]
    cur_c = upsampled_chroma(rng, cur)
    refs_c = [upsampled_chroma(rng, r) for r in refs]
    nmb = (W // 16) * (H // 16)
    ctx = pkg.Context(W, H, yuv_format=1, max_refs=max(slot_of) + 1, search_range=R)
    try:
        ctx.slice_state_reset()
        for r in range(nref):
            ctx.ref_upload(slot_of[r], refs[r], *refs_c[r])
            ctx.interp_luma(slot_of[r])
            ctx.interp_chroma(slot_of[r])
        ctx.cur_upload(cur, *cur_c)
        if mode == 3:
            ctx.epzs_colocated_upload(np.zeros((H // 4, W // 4, 2), np.int16))
        lam = int(65536 * np.sqrt(0.85 * 2 ** ((qp - 12) / 3.0)) + 0.5)
        lib = pkg.load_library()
        p = slice_params(pkg, mode, R, nref, [lam] * 3, 8, W, mb_first=0, mb_count=nmb, t8=t8, qp_n=qp)
        p.ref_slot[0], p.ref_slot[1] = slot_of
        if mode == 3:
            import ctypes as C
            lib.jmhip_epzs_scales(p, 4, (C.c_int * 2)(2, 0), 2)
        rec = ctx.p_slice_search(p)
        ctx.frame_keep_prediction()
        ctx.slice_to_frame(list(slot_of))
        ar = 0                                             # Transform8x8Mode in the slice search: no adaptive rounding
        quants = np.array([pkg.flat_quant(qp + d, 342, adaptive_rounding=ar, adapt_rnd_weight=4, cavlc=1) for d in (0, 0, 3)] +
                          [pkg.flat_quant(qp, 342, is8x8=True, adaptive_rounding=ar, adapt_rnd_weight=4, cavlc=1, transform8x8_flag=1)], dtype=pkg.QUANT_DTYPE)
        ctx.residual_frame(quants, None)
        got = ctx.residual_download(nmb)
        recon = ctx.recon_download()
        records, records8, pred = ctx.residual_records(nmb), ctx.residual_records8(nmb), ctx.pred_download()
    finally:
        ctx.close()

    t8mb = rec["transform8x8_flag"] == 1
    assert t8mb.any() and (t8 == 2 or (~t8mb).any())
    modes = np.zeros(nmb, dtype=pkg.MB_MODE_DTYPE)
    mbs = np.zeros(nmb, dtype=pkg.ME_MB_DTYPE)
    mv = np.zeros((nmb, 41, 2), np.int16)
    blk_ref = np.zeros((nmb, 4), int)
    parts = pkg.partition_table()
    for i in range(nmb):
        mbs[i]["mb_x"], mbs[i]["mb_y"] = i % (W // 16), i // (W // 16)
        modes[i]["mode"] = rec[i]["best_mode"]
        modes[i]["b8mode"] = rec[i]["b8mode"] if rec[i]["best_mode"] == 8 else 4
        modes[i]["pad"][0] = rec[i]["transform8x8_flag"]
        blk_ref[i] = [slot_of[int(r)] for r in rec[i]["b8ref"]]
        for pi in range(41):
            x4, y4 = parts[pi][1], parts[pi][2]
            rr = int(rec[i]["b8ref"][2 * (y4 >> 1) + (x4 >> 1)])
            mv[i, pi] = rec[i]["mv"][rr, pi]
            if rec[i]["best_mode"] == 8 and rec[i]["transform8x8_flag"] and 5 <= pi < 9:       # the 8x8-transform pass's vectors
                mv[i, pi] = rec[i]["mv8ts"][rr, pi - 5]
    assert np.array_equal(got["modes"]["mode"], modes["mode"]) and np.array_equal(got["modes"]["pad"][:, 0], modes["pad"][:, 0])
    by_slot = [None] * (max(slot_of) + 1)
    for r in range(nref):
        by_slot[slot_of[r]] = oracle.RefPic(refs[r], *refs_c[r], yuv_format=1)
    want = oracle.residual_frame(by_slot, (cur,) + cur_c, mbs, mv, modes, quants, pkg.TQ_JOB_DTYPE, yuv_format=1, blk_ref=blk_ref)
    assert np.array_equal(got["cbp"], want["cbp"]) and np.array_equal(got["cbp_blk"], want["cbp_blk"])
    for k in range(3):
        assert np.array_equal(recon[k], want["recon"][k]), "plane %d" % k
    assert (got["cbp"] != 0).any()
    wl = want["luma"]
    for i in range(nmb):
        x, y = 16 * (i % (W // 16)), 16 * (i // (W // 16))
        assert np.array_equal(pred[0][y:y + 16, x:x + 16], want["jobs_y"][i]["pred"]), "luma prediction of macroblock %d" % i
        assert np.array_equal(records[i]["recon_y"], wl["recon"][i])
        r8 = records8[i]
        if not t8mb[i]:
            assert not r8.tobytes().strip(b"\0")
            for b in range(16):
                n = int(records[i]["cnt"][b])
                assert np.array_equal(records[i]["lev"][b, :n], wl["levels"][i, b, :n]) and wl["levels"][i, b, n] == 0
            continue
        assert int(r8["transform8x8"]) == 1 and int(r8["interleaved"]) == 1 and int(records[i]["nonzero"]) == 0
        for b8 in range(4):
            assert int(r8["coeff_cost"][b8]) == int(wl["coeff_cost"][i, b8]) and int(r8["nonzero"][b8]) == int(wl["nonzero"][i, b8])
            for k in range(4):
                c = int(r8["cnt"][b8, k])
                assert np.array_equal(r8["lev"][b8, 16 * k:16 * k + c], wl["levels"][i, 4 * b8 + k, :c]) and wl["levels"][i, 4 * b8 + k, c] == 0
                assert np.array_equal(r8["run"][b8, 16 * k:16 * k + c], wl["runs"][i, 4 * b8 + k, :c])
