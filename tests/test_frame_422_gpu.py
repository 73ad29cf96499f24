"""The fused 4:2:2 frame stage (frame_fused_kernel's 4:2:2 instantiations): against the oracle's residual_frame(yuv_format=2) and, byte for
byte, against the separate kernels (JMHIP_FRAME_FUSED=0); the dense records (jmhip_mb_residual422), the 8x8 side records and the prediction
picture that only the fused stage leaves. The inputs of every small case are built on the host alone (build_inputs), so that the branch
coverage of the parametrisation is asserted on the ORACLE's output (test_cases_cover_the_branches_of_dct_chroma_422, no GPU): the device cases
then check that the device's motion search agrees with the oracle's, which makes that expectation theirs."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import oracle
from tests.test_frame import synth
from tests.test_me import lambda_factors, make_mbs
from tests.quant_tables import scaled_quant
from tests.test_tq import compare_lists

R = 8
LUMA_FIELDS = ("levels", "runs", "levels8", "runs8", "coeff_cost", "nonzero", "recon", "fadjust")
CHROMA_FIELDS = ("levels", "runs", "dc_levels", "dc_runs", "recon", "fadjust", "ret", "cbp_blk", "cbp_clear")

# QP 12: the DC quantiser (qp + 3 = 15) has qp_per_dc = 2 < 4; QP 24 / 28 / 40: qp_per_dc >= 4 (block.c:1303-1316)
CASES = {
    "qp12_cabac_ar": dict(w=64, h=48, qp=12, cavlc=0, ar=1, far=6, planes=True, given=True, t8="none"),
    "qp12_cavlc_t8_some": dict(w=64, h=48, qp=12, cavlc=1, ar=0, far=6, planes=False, given=True, t8="some"),
    "qp24_cavlc_ar_chosen": dict(w=64, h=48, qp=24, cavlc=1, ar=1, far=6, planes=True, given=False, t8="none"),
    "qp24_cabac_fly_chosen": dict(w=64, h=48, qp=24, cavlc=0, ar=0, far=6, planes=False, given=False, t8="none"),
    "qp28_cavlc_ar_t8_some": dict(w=64, h=48, qp=28, cavlc=1, ar=1, far=6, planes=True, given=True, t8="some"),
    "qp28_cabac_t8_all": dict(w=64, h=48, qp=28, cavlc=0, ar=1, far=6, planes=False, given=True, t8="all"),
    "qp28_weighted": dict(w=64, h=48, qp=28, cavlc=1, ar=1, far=6, planes=True, given=True, t8="none", weighted=True),
    "qp28_far_fly": dict(w=64, h=48, qp=28, cavlc=0, ar=1, far=90, planes=False, given=True, t8="some"),
    "qp34_far_planes": dict(w=64, h=48, qp=34, cavlc=1, ar=1, far=45, planes=True, given=True, t8="none"),
    "qp40_cavlc": dict(w=64, h=48, qp=40, cavlc=1, ar=1, far=6, planes=True, given=True, t8="none"),
    "qp40_cabac_t8_some": dict(w=64, h=48, qp=40, cavlc=0, ar=0, far=6, planes=False, given=True, t8="some"),
    "tail_15_mbs": dict(w=80, h=48, qp=26, cavlc=0, ar=1, far=6, planes=False, given=True, t8="some"),       # 15 macroblocks: spare groups in the last wave
    "tail_9_mbs_weighted": dict(w=48, h=48, qp=28, cavlc=1, ar=1, far=6, planes=True, given=False, t8="none", weighted=True),
    # luma at QP 36, chroma at QP 22: macroblocks whose luma falls to _LUMA_MB_COEFF_COST_ while the chroma is coded (seed found on the host)
    "qp36_luma_mb_threshold": dict(w=96, h=64, qp=36, qpc=22, cavlc=1, ar=1, far=6, planes=True, given=True, t8="some", seed=901),
    "b_macroblocks": dict(w=64, h=48, qp=26, cavlc=1, ar=1, far=6, planes=True, given=True, t8="none", bipred=True),
    "b_macroblocks_weighted_fly": dict(w=64, h=48, qp=30, cavlc=0, ar=1, far=6, planes=False, given=True, t8="some", bipred=True, weighted=True),
}


def build_inputs(pkg, *, w, h, qp, cavlc, ar, far, planes, given, t8, seed, weighted=False, bipred=False, fmt=2, qpc=None, tables=False):
    """Everything a case feeds the frame stage with, drawn on the host (no device involved)."""
    rng = np.random.default_rng(seed)
    cur, ref = synth(rng, w, h, fmt)
    refs = [ref]
    if bipred:                                            # a second reference: the first one shifted and dimmed
        refs.append(tuple(np.clip(np.roll(p, (1, -2), (0, 1)).astype(int) - 6, 0, 255).astype(np.uint8) for p in ref))
    mbs = make_mbs(pkg, rng, w // 16, h // 16, 4 * far)
    n = len(mbs)
    kw = dict(adaptive_rounding=ar, adapt_rnd_weight=4 if ar else 0, cavlc=cavlc)
    qpc = qp if qpc is None else qpc                        # the chroma quantiser may sit below the luma one (chroma_qp_index_offset)
    quants = [pkg.flat_quant(qp, 342, **kw), pkg.flat_quant(qpc, 342, **kw), pkg.flat_quant(qpc + 3, 342, **kw)]
    if t8 != "none":
        quants.append(pkg.flat_quant(qp, 342, is8x8=True, transform8x8_flag=1, **kw))
    if tables:                                            # a scaling matrix and per-position offsets of its own for every record, none symmetric
        quants = [scaled_quant(pkg, q, rng, False, **kw) for q in (qp, qpc, qpc + 3)]
        if t8 != "none":
            quants.append(scaled_quant(pkg, qp, rng, True, transform8x8_flag=1, **kw))
    quants = np.array(quants, dtype=pkg.QUANT_DTYPE)
    modes = None
    flags = np.zeros(n, bool)
    if given:
        modes = np.zeros(n, dtype=pkg.MB_MODE_DTYPE)
        modes["mode"] = rng.choice([1, 2, 3, 8], n)
        modes["b8mode"] = rng.integers(4, 8, (n, 4))
        if t8 != "none":
            flags = np.ones(n, bool) if t8 == "all" else rng.integers(0, 2, n).astype(bool)
            flags[0] = True
            if t8 == "some":
                flags[1] = False
            modes["b8mode"][flags] = 4
            modes["pad"][:, 0] = flags
    wp = bw = bi = None
    if weighted:
        wp = {"luma_round": 16, "luma_denom": 5, "chroma_round": 4, "chroma_denom": 3, "weight": np.zeros((16, 3), int), "offset": np.zeros((16, 3), int)}
        wp["weight"][0], wp["offset"][0] = (29, 9, 7), (4, -2, 1)
    if bipred:
        bi = np.zeros(n, dtype=pkg.MB_BIPRED_DTYPE)
        bi["pdir"] = rng.integers(0, 3, (n, 4))
        bi["pdir"][0] = (0, 1, 2, 2)
        bi["ref1"] = 1
        bi["mv1"] = rng.integers(-40, 41, (n, 16, 2))
        bi["mv1"][0] = [[-300, -200]] * 16                  # far outside the picture: the UMV clamps
        if weighted:
            bw = {"w0": rng.integers(10, 40, (4, 4, 3)), "w1": rng.integers(10, 40, (4, 4, 3)), "weight1": rng.integers(5, 12, (4, 3)), "offset1": rng.integers(-4, 5, (4, 3))}
            bw["weight1"][:, 0] += 22
    return dict(w=w, h=h, qp=qp, ar=ar, planes=planes, cur=cur, refs=refs, mbs=mbs, quants=quants, modes=modes, t8=flags, wp=wp, bi=bi, bw=bw, fmt=fmt, qpc=qpc)


def oracle_search(inp):
    rp = oracle.RefPic(*inp["refs"][0], yuv_format=inp["fmt"])
    return oracle.me_frame(oracle.me_params(rdopt=1), [rp], inp["cur"][0], inp["mbs"], -1, R, lambda_factors(inp["qp"]))


def expectation(pkg, inp, mv, modes):
    rps = [oracle.RefPic(*r, yuv_format=inp["fmt"]) for r in inp["refs"]]
    return oracle.residual_frame(rps, inp["cur"], inp["mbs"], mv, modes, inp["quants"], pkg.TQ_JOB_DTYPE, yuv_format=inp["fmt"],
                                 blk_ref=np.zeros((len(inp["mbs"]), 4), int), wp=inp["wp"], bi=inp["bi"], bw=inp["bw"])


def run_device(pkg, monkeypatch, inp, fused, deblock=True):
    """One frame stage on a fresh context; returns everything it left behind."""
    if not fused:
        monkeypatch.setenv("JMHIP_FRAME_FUSED", "0")
    else:
        monkeypatch.delenv("JMHIP_FRAME_FUSED", raising=False)
    w, h, n = inp["w"], inp["h"], len(inp["mbs"])
    ctx = pkg.Context(w, h, yuv_format=inp["fmt"], max_refs=len(inp["refs"]), search_range=R)
    try:
        for slot, ref in enumerate(inp["refs"]):
            ctx.ref_upload(slot, *ref)
            ctx.interp_luma(slot)
            if inp["planes"]:
                ctx.interp_chroma(slot)
        ctx.cur_upload(*inp["cur"])
        prm = pkg.MeParams()
        prm.search_mode, prm.search_range, prm.rdopt = inp.get("search_mode", -1), R, 1
        prm.level_mv_min, prm.level_mv_max = -511, 511
        prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lambda_factors(inp["qp"])
        prm.subpel, prm.partition_mask = 1, (1 << 41) - 1
        me = ctx.me_frame(prm, inp["mbs"])
        ctx.frame_wp_set(inp["wp"])
        if inp["bi"] is not None:
            ctx.frame_bipred_set(inp["bi"], inp["bw"])
        if fused:
            ctx.frame_keep_prediction()
        ctx.residual_frame(inp["quants"], inp["modes"])
        out = {"me": me, "got": ctx.residual_download(n), "recon": ctx.recon_download()}
        if fused:
            out["records"], out["records8"], out["pred"] = ctx.residual_records422(n), ctx.residual_records8(n), ctx.pred_download()
            with pytest.raises(pkg.JmhipError):              # the 4:2:0 record cannot hold 4:2:2 chroma
                ctx.residual_records(n)
        else:
            for call in (lambda: ctx.residual_records422(n), lambda: ctx.residual_records8(n), ctx.pred_download):
                with pytest.raises(pkg.JmhipError):
                    call()
        if deblock and inp["bi"] is None:
            ctx.deblock_recon(inp["qp"])
            out["deblocked"] = ctx.recon_download()
        if inp["bi"] is not None:
            ctx.frame_bipred_set(None)
        ctx.frame_wp_set(None)
    finally:
        ctx.close()
    return out


def lists_differ(gl, gr, wl, wr):
    """(level, run) lists compared up to and including the terminating zero level, vectorised over all rows (the full-size pictures)"""
    w = wl.reshape(-1, wl.shape[-1])
    g, r_g, r_w = gl.reshape(w.shape), gr.reshape(w.shape), wr.reshape(w.shape)
    k = np.where((w == 0).any(axis=1), np.argmax(w == 0, axis=1), w.shape[1] - 1)[:, None]
    idx = np.arange(w.shape[1])[None, :]
    return bool((np.where(idx <= k, g != w, False)).any() or (np.where(idx < k, r_g != r_w, False)).any())


def check_download(got, recon, want, t8, ar, mbs=None, vectorised=False):
    """jmhip_residual_download and the recon picture against the oracle's expectation: every field the separate kernels write."""
    gl, wl, gc, wc = got["luma"], want["luma"], got["chroma"], want["chroma"]
    if vectorised:
        assert not lists_differ(gl["levels"], gl["runs"], wl["levels"], wl["runs"]), "luma 4x4 / interleaved 8x8 lists"
        assert not lists_differ(gl["levels8"][t8], gl["runs8"][t8], wl["levels8"][t8], wl["runs8"][t8]), "luma 8x8 lists"
        assert not lists_differ(gc["levels"][:, :8, :16], gc["runs"][:, :8, :16], wc["levels"][:, :8, :16], wc["runs"][:, :8, :16]), "chroma AC lists"
        assert not lists_differ(gc["dc_levels"], gc["dc_runs"], wc["dc_levels"], wc["dc_runs"]), "chroma DC lists"
    else:
        compare_lists(gl["levels"], gl["runs"], wl["levels"], wl["runs"], "luma 4x4 / interleaved 8x8 lists")
        compare_lists(gl["levels8"][t8], gl["runs8"][t8], wl["levels8"][t8], wl["runs8"][t8], "luma 8x8 lists")
        compare_lists(gc["levels"][:, :8, :16], gc["runs"][:, :8, :16], wc["levels"][:, :8, :16], wc["runs"][:, :8, :16], "chroma AC lists")
        compare_lists(gc["dc_levels"][:, None], gc["dc_runs"][:, None], wc["dc_levels"][:, None], wc["dc_runs"][:, None], "chroma DC lists")
    assert np.array_equal(gl["coeff_cost"][~t8], wl["coeff_cost"][~t8]) and np.array_equal(gl["coeff_cost"][t8][:, :4], wl["coeff_cost"][t8][:, :4])
    assert np.array_equal(gl["nonzero"][~t8], wl["nonzero"][~t8]) and np.array_equal(gl["nonzero"][t8][:, :4], wl["nonzero"][t8][:, :4])
    assert np.array_equal(gl["recon"], wl["recon"]) and np.array_equal(gc["recon"][:, :, :8], wc["recon"][:, :, :8])
    for f in ("ret", "cbp_blk", "cbp_clear"):
        assert np.array_equal(gc[f], wc[f]), "chroma %s" % f
    if ar:
        assert np.array_equal(gl["fadjust"], wl["fadjust"]) and np.array_equal(gc["fadjust"][:, :, :8], wc["fadjust"][:, :, :8])
    assert np.array_equal(got["cbp"], want["cbp"]) and np.array_equal(got["cbp_blk"], want["cbp_blk"])
    if mbs is None:
        for g, wv, name in zip(recon, want["recon"], "YUV"):
            assert np.array_equal(g, wv), "recon %s" % name
    else:                                                 # a subset of the macroblocks: their tiles of the pictures
        for k, mb in enumerate(mbs):
            x, y = 16 * int(mb["mb_x"]), 16 * int(mb["mb_y"])
            assert np.array_equal(recon[0][y:y + 16, x:x + 16], want["recon"][0][y:y + 16, x:x + 16]), ("luma recon", k)
            for p in (1, 2):
                assert np.array_equal(recon[p][y:y + 16, x // 2:x // 2 + 8], want["recon"][p][y:y + 16, x // 2:x // 2 + 8]), ("chroma recon", p, k)


def check_records(recs, recs8, pred, want, mbs, t8, ar, cavlc):
    """Every field of jmhip_mb_residual422 / jmhip_mb_residual8 and the prediction picture against the same expectation."""
    wl = want["luma"]
    for i, mb in enumerate(mbs):
        r, r8, x, y = recs[i], recs8[i], 16 * int(mb["mb_x"]), 16 * int(mb["mb_y"])
        assert np.array_equal(pred[0][y:y + 16, x:x + 16], want["jobs_y"][i]["pred"]), "luma prediction of macroblock %d" % i
        assert np.array_equal(r["recon_y"], wl["recon"][i])
        if ar:
            assert np.array_equal(r["fadj_y"], wl["fadjust"][i])
        for uv in range(2):
            wc = {k: v[2 * i + uv] for k, v in want["chroma"].items()}
            # chroma tiles are 16 rows x 8 columns at (16 * mb_y, 8 * mb_x)
            assert np.array_equal(pred[1 + uv][y:y + 16, x // 2:x // 2 + 8], want["jobs_c"][2 * i + uv]["pred"][:16, :8]), "chroma prediction of macroblock %d" % i
            zeroed = int(r["ac_zeroed"][uv])
            for b in range(8):
                k = int(r["cnt"][16 + 8 * uv + b])
                lev = r["lev"][16 + 8 * uv + b, :k]
                assert np.array_equal(np.zeros_like(lev) if zeroed else lev, wc["levels"][b, :k]) and wc["levels"][b, k] == 0, (i, uv, b)
                assert np.array_equal(r["run"][16 + 8 * uv + b, :k], wc["runs"][b, :k]), (i, uv, b)
            if zeroed:
                assert not wc["levels"][:8, :16].any()
            k = int(r["dc_cnt"][uv])
            assert np.array_equal(r["dc_lev"][uv, :k], wc["dc_levels"][:k]) and np.array_equal(r["dc_run"][uv, :k], wc["dc_runs"][:k]) and wc["dc_levels"][k] == 0
            assert int(r["ret"][uv]) == int(wc["ret"]) and int(r["cbp_blk"][uv]) == int(wc["cbp_blk"]) and int(r["cbp_clear"][uv]) == int(wc["cbp_clear"])
            assert np.array_equal(r["recon_c"][uv], wc["recon"][:16, :8])
            if ar:
                assert np.array_equal(r["fadj_c"][uv], wc["fadjust"][:16, :8])
        if not t8[i]:
            assert not r8.tobytes().strip(b"\0"), "side record of 4x4-transform macroblock %d is not zero" % i
            for b in range(16):
                k = int(r["cnt"][b])
                assert np.array_equal(r["lev"][b, :k], wl["levels"][i, b, :k]) and np.array_equal(r["run"][b, :k], wl["runs"][i, b, :k]) and wl["levels"][i, b, k] == 0
                assert ((int(r["nonzero"]) >> b) & 1) == int(wl["nonzero"][i, b]) and int(r["coeff_cost"][b]) == int(wl["coeff_cost"][i, b])
            continue
        # 8x8 transform: the luma lists / costs / nonzero of the main record read 0, the side record holds dct_8x8's results
        assert int(r["nonzero"]) == 0 and not r["cnt"][:16].any() and not r["coeff_cost"].any() and not r["lev"][:16].any()
        assert int(r8["transform8x8"]) == 1 and int(r8["interleaved"]) == int(cavlc)
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


def check_against_separate(a, b):
    """The fused stage (a) and the separate kernels (b) on the same inputs: byte-identical downloads and pictures."""
    for f in LUMA_FIELDS:
        assert np.array_equal(a["got"]["luma"][f], b["got"]["luma"][f]), "luma %s" % f
    for f in CHROMA_FIELDS:
        assert np.array_equal(a["got"]["chroma"][f], b["got"]["chroma"][f]), "chroma %s" % f
    assert a["got"]["luma"].tobytes() == b["got"]["luma"].tobytes() and a["got"]["chroma"].tobytes() == b["got"]["chroma"].tobytes()
    for f in ("cbp", "cbp_blk"):
        assert np.array_equal(a["got"][f], b["got"][f]), f
    assert a["got"]["modes"].tobytes() == b["got"]["modes"].tobytes()
    for key in ("recon", "deblocked"):
        for pa, pb, name in zip(a.get(key, ()), b.get(key, ()), "YUV"):
            assert np.array_equal(pa, pb), "%s %s" % (key, name)


def coverage(want, t8):
    """Which branches of dct_chroma's 4:2:2 path and of the luma thresholds the oracle's output shows."""
    wc, wl = want["chroma"], want["luma"]
    ac = wc["levels"][:, :8, :16]
    any_run = (wc["runs"][:, :8, :16] != 0).any(axis=(1, 2))         # the runs stay when the threshold zeroes the levels
    dc = wc["dc_levels"][:, 0] != 0
    zeroed = ~ac.any(axis=(1, 2)) & any_run                            # levels gone, runs left: _CHROMA_COEFF_COST_ hit
    # _LUMA_MB_COEFF_COST_ decides: some 8x8 block survives _LUMA_COEFF_COST_ (cost > 4) and the survivors sum to 5 or less (macroblock.c:1386)
    cc = wl["coeff_cost"].astype(np.int64)
    cost8 = np.where(t8[:, None], cc[:, :4], cc.reshape(-1, 4, 4).sum(axis=2))
    kept = cost8 > 4
    luma_mb_hit = kept.any(axis=1) & ((cost8 * kept).sum(axis=1) <= 5)
    chroma_coded = (want["cbp"] >> 4) > 0
    return {
        "threshold_hit_no_dc": bool((wc["cbp_clear"] != 0).any()),
        "threshold_hit_dc_coded": bool((zeroed & dc & (wc["cbp_clear"] == 0)).any()),
        "cr_dc_sign_extended": bool((dc[1::2] & (wc["cbp_blk"][1::2] < 0)).any()),
        "ac_in_rows_8_15": bool(ac[:, 4:8].any()),
        "ac_in_rows_0_7": bool(ac[:, 0:4].any()),
        "luma_mb_zeroed_chroma_coded": bool((luma_mb_hit & chroma_coded & ((want["cbp"] & 15) == 0)).any()),
    }


def case_inputs(pkg, name):
    kw = dict(CASES[name])
    seed = kw.pop("seed", 400 + sorted(CASES).index(name))
    return build_inputs(pkg, seed=seed, **kw)


def test_cases_cover_the_branches_of_dct_chroma_422(pkg):
    """No GPU: the expectation of every small case from the oracle alone (its own motion search), and over the parametrisation each branch the
    4:2:2 path has must occur IN THE ORACLE'S OUTPUT: both DC dequantisation branches with coded DC levels, the coefficient-cost threshold with
    and without a coded DC, the sign-extended Cr cbp_blk, AC levels in the transformed (rows 0..7) and the untransformed (rows 8..15) half, a
    macroblock whose luma falls to _LUMA_MB_COEFF_COST_ while its chroma is coded."""
    seen = {}
    for name in sorted(CASES):
        inp = case_inputs(pkg, name)
        me = oracle_search(inp)
        modes = inp["modes"] if inp["modes"] is not None else oracle.pick_modes(me["cost"])
        want = expectation(pkg, inp, me["mv"], modes)
        cov = coverage(want, inp["t8"])
        dc_coded = bool((want["chroma"]["dc_levels"][:, 0] != 0).any())
        cov["dc_dequant_qp_per_below_4"] = dc_coded and (inp["qp"] + 3) // 6 < 4
        cov["dc_dequant_qp_per_4_and_above"] = dc_coded and (inp["qp"] + 3) // 6 >= 4
        for k, v in cov.items():
            seen[k] = seen.get(k, False) or v
    assert all(seen.values()), "branches the cases do not reach: %s" % [k for k, v in seen.items() if not v]


def run_and_check(pkg, monkeypatch, kw, inp):
    a = run_device(pkg, monkeypatch, inp, fused=True)
    b = run_device(pkg, monkeypatch, inp, fused=False)
    check_against_separate(a, b)
    # the device's search is the oracle's, so the expectation below is the one whose branch coverage the CPU test asserts
    me = oracle_search(inp)
    assert np.array_equal(a["me"]["mv"], me["mv"]) and np.array_equal(a["me"]["cost"], me["cost"])
    modes = inp["modes"] if inp["modes"] is not None else oracle.pick_modes(me["cost"])
    assert np.array_equal(a["got"]["modes"]["mode"], modes["mode"]) and np.array_equal(a["got"]["modes"]["pad"][:, 0], modes["pad"][:, 0])
    if inp["modes"] is None:
        assert np.array_equal(a["got"]["modes"]["b8mode"], modes["b8mode"])
    if kw["t8"] == "some":
        assert inp["t8"].any() and (~inp["t8"]).any()
    want = expectation(pkg, inp, a["me"]["mv"], a["got"]["modes"])
    for o in (a, b):
        check_download(o["got"], o["recon"], want, inp["t8"], kw["ar"])
    check_records(a["records"], a["records8"], a["pred"], want, inp["mbs"], inp["t8"], kw["ar"], kw["cavlc"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_422_frame_stage(pkg, monkeypatch, name):
    run_and_check(pkg, monkeypatch, CASES[name], case_inputs(pkg, name))


# Scaling matrices and per-position rounding offsets, asymmetric, a set of their own for each of luma 4x4, chroma, chroma DC (qp + 3, which
# the 4:2:2 DC path does read) and luma 8x8; the stage takes one chroma quantiser per call, so Cb and Cr share theirs.
# qpc: synth's chroma carries a quarter of the luma's amplitude; at the luma QP its AC levels are too few for the chroma tables to show.
TABLE_CASES = {
    "tables_cabac_ar_t8_some": dict(w=64, h=48, qp=24, qpc=10, cavlc=0, ar=1, far=6, planes=True, given=True, t8="some", tables=True, seed=611),
    "tables_cavlc_4x4_chosen": dict(w=64, h=48, qp=20, qpc=10, cavlc=1, ar=0, far=6, planes=False, given=False, t8="none", tables=True, seed=612),
    "tables_tail_15_mbs": dict(w=80, h=48, qp=26, qpc=10, cavlc=1, ar=1, far=6, planes=False, given=True, t8="some", tables=True, seed=613),
}


def download_differences(got, recon, want, t8, ar):
    """check_download's comparisons as the list of names that differ; got / recon: a second oracle run's "luma" / "chroma" / "recon"."""
    gl, wl, gc, wc = got["luma"], want["luma"], got["chroma"], want["chroma"]
    bad = []
    for name, d in (("luma levels", lists_differ(gl["levels"], gl["runs"], wl["levels"], wl["runs"])),
                    ("luma levels8", bool(t8.any()) and lists_differ(gl["levels8"][t8], gl["runs8"][t8], wl["levels8"][t8], wl["runs8"][t8])),
                    ("chroma levels", lists_differ(gc["levels"][:, :8, :16], gc["runs"][:, :8, :16], wc["levels"][:, :8, :16], wc["runs"][:, :8, :16])),
                    ("chroma dc_levels", lists_differ(gc["dc_levels"], gc["dc_runs"], wc["dc_levels"], wc["dc_runs"]))):
        if d:
            bad.append(name)
    same = lambda name, a, b: None if np.array_equal(a, b) else bad.append(name)
    same("luma coeff_cost", gl["coeff_cost"][~t8], wl["coeff_cost"][~t8])
    same("luma coeff_cost", gl["coeff_cost"][t8][:, :4], wl["coeff_cost"][t8][:, :4])
    same("luma recon", gl["recon"], wl["recon"])
    same("chroma recon", gc["recon"][:, :, :8], wc["recon"][:, :, :8])
    for f in ("ret", "cbp_blk", "cbp_clear"):
        same("chroma %s" % f, gc[f], wc[f])
    if ar:
        same("luma fadjust", gl["fadjust"], wl["fadjust"])
        same("chroma fadjust", gc["fadjust"][:, :, :8], wc["fadjust"][:, :, :8])
    same("cbp", got["cbp"], want["cbp"])
    same("cbp_blk", got["cbp_blk"], want["cbp_blk"])
    for g, wv, name in zip(recon, want["recon"], "YUV"):
        same("picture recon %s" % name, g, wv)
    return bad


_table_inputs = {}


def table_inputs(pkg, name):
    """The inputs of a TABLE_CASES entry, built once and checked on the oracle alone for the tables to bite (tests/test_tq.py assert_tables_bite)."""
    if name not in _table_inputs:
        from tests.quant_tables import is_asymmetric, mutated, table_size
        from tests.test_tq import assert_tables_bite
        kw = dict(TABLE_CASES[name])
        inp = build_inputs(pkg, **kw)
        for q in inp["quants"]:
            assert all(is_asymmetric(q[t], table_size(q)) for t in ("levelscale", "invlevelscale", "leveloffset"))
        me = oracle_search(inp)
        modes = inp["modes"] if inp["modes"] is not None else oracle.pick_modes(me["cost"])
        want = expectation(pkg, inp, me["mv"], modes)

        def differ(ks, how):
            other = expectation(pkg, dict(inp, quants=mutated(inp["quants"], ks, how)), me["mv"], modes)
            return download_differences(other, other["recon"], want, inp["t8"], kw["ar"])
        # the DC set: dct_chroma's 4:2:2 DC path reads its offset and inverse scale at (0, 0) and nothing else (block.c:1263)
        groups = {"luma4x4": ([0], False), "chroma": ([1], False), "chroma_dc": ([2], True)}
        if inp["t8"].any():
            groups["luma8x8"] = ([3], False)
        assert_tables_bite(differ, groups, name)
        _table_inputs[name] = inp
    return _table_inputs[name]


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_tables_are_asymmetric_where_it_matters(pkg, name):
    """No GPU: on the oracle, each record of every TABLE_CASES entry changes a compared output when its levelscale, invlevelscale or leveloffset
    is transposed or its leveloffset flattened to the mean; the qp + 3 DC record, read at (0, 0) alone, when its offset is."""
    table_inputs(pkg, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_fused_422_frame_stage_asymmetric_tables(pkg, monkeypatch, name):
    """The fused 4:2:2 stage and the separate kernels on asymmetric scaling matrices and rounding offsets: everything test_fused_422_frame_stage
    checks -- fused against separate, both against the oracle, records, side records, prediction picture."""
    inp = table_inputs(pkg, name)                           # asserts that the tables bite before anything is compared
    run_and_check(pkg, monkeypatch, TABLE_CASES[name], inp)


def full_size_inputs(pkg, W, H, qp=28):
    from tests.test_fullsize import clip
    cur, ref = clip(W, H)
    mk = lambda img, s: np.clip(np.round(128 + s * 0.25 * (img[:, ::2].astype(float) - 128)), 0, 255).astype(np.uint8)
    mbw, mbh = W // 16, H // 16
    n = mbw * mbh
    rng = np.random.default_rng(9)
    mbs = np.zeros(n, dtype=pkg.ME_MB_DTYPE)
    mbs["mb_x"], mbs["mb_y"], mbs["ref_is_0"] = np.arange(n) % mbw, np.arange(n) // mbw, 1
    mbs["pred_mv"] = (np.array([16, -16]) + rng.integers(-8, 9, (n, 1, 2))) + np.zeros((n, 41, 2), int)
    kw = dict(adaptive_rounding=1, adapt_rnd_weight=4, cavlc=1)
    quants = np.array([pkg.flat_quant(qp, 342, **kw), pkg.flat_quant(qp, 342, **kw), pkg.flat_quant(qp + 3, 342, **kw),
                       pkg.flat_quant(qp, 342, is8x8=True, transform8x8_flag=1, **kw)], dtype=pkg.QUANT_DTYPE)
    modes = np.zeros(n, dtype=pkg.MB_MODE_DTYPE)
    modes["mode"] = rng.choice([1, 2, 3, 8], n)
    modes["b8mode"] = rng.integers(4, 8, (n, 4))
    flags = rng.integers(0, 2, n).astype(bool)             # 4x4- and 8x8-transform macroblocks mixed
    modes["b8mode"][flags] = 4
    modes["pad"][:, 0] = flags
    return dict(w=W, h=H, qp=qp, ar=1, planes=True, cur=(cur, mk(cur, 1), mk(cur, -1)), refs=[(ref, mk(ref, 1), mk(ref, -1))], mbs=mbs, quants=quants,
                modes=modes, t8=flags, wp=None, bi=None, bw=None, fmt=2, search_mode=0)


def expectation_threaded(pkg, inp, mv, modes, sel):
    """The oracle over the selected macroblocks, dealt to host threads in chunks (its C functions release the GIL); the sub-pel planes are built once."""
    rps = [oracle.RefPic(*r, yuv_format=2) for r in inp["refs"]]
    chunks = np.array_split(sel, 32)

    def one(idx):
        return oracle.residual_frame(rps, inp["cur"], inp["mbs"][idx], mv[idx], modes[idx], inp["quants"], pkg.TQ_JOB_DTYPE, yuv_format=2,
                                     blk_ref=np.zeros((len(idx), 4), int))
    with ThreadPoolExecutor(max_workers=14) as ex:
        return list(zip(chunks, ex.map(one, chunks)))


def check_full_size(pkg, monkeypatch, W, H, step):
    inp = full_size_inputs(pkg, W, H)
    n = len(inp["mbs"])
    a = run_device(pkg, monkeypatch, inp, fused=True, deblock=False)
    b = run_device(pkg, monkeypatch, inp, fused=False, deblock=False)
    check_against_separate(a, b)                           # all macroblocks
    assert inp["t8"].any() and (~inp["t8"]).any()
    assert (a["got"]["cbp"] & 15).max() > 0 and ((a["got"]["cbp"] & 15) == 0).any()
    for idx, want in expectation_threaded(pkg, inp, a["me"]["mv"], a["got"]["modes"], np.arange(0, n, step)):
        csel = np.stack([2 * idx, 2 * idx + 1], axis=1).reshape(-1)
        got = {"luma": a["got"]["luma"][idx], "chroma": a["got"]["chroma"][csel], "cbp": a["got"]["cbp"][idx], "cbp_blk": a["got"]["cbp_blk"][idx]}
        check_download(got, a["recon"], want, inp["t8"][idx], 1, mbs=inp["mbs"][idx], vectorised=True)
        for k, i in enumerate(idx):
            x, y = 16 * int(inp["mbs"][i]["mb_x"]), 16 * int(inp["mbs"][i]["mb_y"])
            assert np.array_equal(a["pred"][0][y:y + 16, x:x + 16], want["jobs_y"][k]["pred"])
            for uv in range(2):
                assert np.array_equal(a["pred"][1 + uv][y:y + 16, x // 2:x // 2 + 8], want["jobs_c"][2 * k + uv]["pred"][:16, :8])
                assert np.array_equal(a["records"][i]["recon_c"][uv], want["chroma"]["recon"][2 * k + uv][:16, :8])


@pytest.mark.gpu
def test_fused_422_frame_stage_1080p(pkg, monkeypatch):
    """1920x1088 4:2:2, 4x4- and 8x8-transform macroblocks mixed: every macroblock against the oracle, and fused equals separate."""
    check_full_size(pkg, monkeypatch, 1920, 1088, 1)


@pytest.mark.gpu
def test_fused_422_frame_stage_2160p(pkg, monkeypatch):
    """3840x2160 4:2:2 (BASELINE config 5's picture): fused equals separate on all 32 400 macroblocks, every 9th against the oracle."""
    check_full_size(pkg, monkeypatch, 3840, 2160, 9)


def slice_case(pkg, monkeypatch, mode, t8, slot_of, weighted, fused, handover="decision"):
    """jmhip_p_slice_search in a 4:2:2 context -> jmhip_slice_to_frame (or a candidate form) -> jmhip_residual_frame."""
    from tests.test_slice_gpu import slice_params, synth_clip
    if not fused:
        monkeypatch.setenv("JMHIP_FRAME_FUSED", "0")
    else:
        monkeypatch.delenv("JMHIP_FRAME_FUSED", raising=False)
    W, H, SR, nref, qp = 176, 144, 16, 2, 28
    rng = np.random.default_rng(31 + t8)
    clip = synth_clip(rng, W, H, 3)
    clip[0] = np.clip(clip[0].astype(int) + 9, 0, 255).astype(np.uint8)        # a brightness step, so that reference 1 wins for some blocks
    chroma = lambda Y: (np.clip(Y[:, ::2].astype(int) // 2 + 60 + rng.integers(-3, 4, (H, W // 2)), 0, 255).astype(np.uint8),
                        np.clip(200 - Y[:, 1::2].astype(int) // 2 + rng.integers(-3, 4, (H, W // 2)), 0, 255).astype(np.uint8))
    cur, refs = clip[2], [clip[1], clip[0]]
    cur_c = chroma(cur)
    refs_c = [chroma(r) for r in refs]
    nmb = (W // 16) * (H // 16)
    ctx = pkg.Context(W, H, yuv_format=2, max_refs=max(slot_of) + 1, search_range=SR)
    try:
        ctx.slice_state_reset()
        for r in range(nref):
            ctx.ref_upload(slot_of[r], refs[r], *refs_c[r])
            ctx.interp_luma(slot_of[r])
            ctx.interp_chroma(slot_of[r])                      # slots 8 and above need their eighth-pel chroma planes
        ctx.cur_upload(cur, *cur_c)
        lam = int(65536 * np.sqrt(0.85 * 2 ** ((qp - 12) / 3.0)) + 0.5)
        p = slice_params(pkg, mode, SR, nref, [lam] * 3, 8, W, mb_first=0, mb_count=nmb, t8=t8, qp_n=qp)
        p.ref_slot[0], p.ref_slot[1] = slot_of
        wp = None
        if weighted:
            p.wp_pred, p.wp_round, p.wp_denom = 1, 16, 5
            p.wp_weight[0], p.wp_offset[0], p.wp_weight[1], p.wp_offset[1] = 30, 2, 34, -3
            wp = {"luma_round": 16, "luma_denom": 5, "chroma_round": 8, "chroma_denom": 4, "weight": np.zeros((16, 3), int), "offset": np.zeros((16, 3), int)}
            wp["weight"][slot_of[0]], wp["offset"][slot_of[0]] = (30, 17, 15), (2, -1, 0)
            wp["weight"][slot_of[1]], wp["offset"][slot_of[1]] = (34, 16, 14), (-3, 1, 2)
        rec = ctx.p_slice_search(p)
        ctx.frame_wp_set(wp)
        if fused:
            ctx.frame_keep_prediction()
        if handover == "decision":
            ctx.slice_to_frame(list(slot_of))
        elif handover == "candidates":
            ctx.slice_to_frame_candidates(list(slot_of), 0, nmb)
        else:
            ctx.slice_to_frame_candidates8(list(slot_of), 0, nmb)
        ar = 0 if t8 else 1                                    # Transform8x8Mode in the slice search: no adaptive rounding
        quants = [pkg.flat_quant(qp + d, 342, adaptive_rounding=ar, adapt_rnd_weight=4, cavlc=1) for d in (0, 0, 3)]
        if t8:
            quants.append(pkg.flat_quant(qp, 342, is8x8=True, adaptive_rounding=ar, adapt_rnd_weight=4, cavlc=1, transform8x8_flag=1))
        quants = np.array(quants, dtype=pkg.QUANT_DTYPE)
        ctx.residual_frame(quants, None)
        out = {"got": ctx.residual_download(nmb), "recon": ctx.recon_download()}
        if fused:
            out["records"], out["records8"], out["pred"] = ctx.residual_records422(nmb), ctx.residual_records8(nmb), ctx.pred_download()
        ctx.frame_wp_set(None)
    finally:
        ctx.close()
    out.update(rec=rec, cur=(cur,) + cur_c, refs=[(refs[r],) + refs_c[r] for r in range(nref)], quants=quants, wp=wp, ar=ar, nmb=nmb, W=W)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode,t8,slot_of,weighted", [(-1, 0, (1, 0), False), (-1, 1, (9, 0), False), (1, 0, (9, 0), True), (1, 1, (1, 0), True)])
def test_slice_search_feeds_the_fused_422_stage(pkg, monkeypatch, mode, t8, slot_of, weighted):
    """An exhaustive search and UMHexagonS with explicit weights (BASELINE config 5's tools), two references in non-adjacent slots, with and
    without Transform8x8Mode: the decided picture goes to the frame stage on the device, every 8x8 block predicts from the slot ITS decision
    chose. Downloads, records, side records, prediction picture and reconstruction against the oracle fed with the search's records; and the
    separate kernels give the same bytes."""
    o = slice_case(pkg, monkeypatch, mode, t8, slot_of, weighted, fused=True)
    s = slice_case(pkg, monkeypatch, mode, t8, slot_of, weighted, fused=False)
    check_against_separate(o, s)
    rec, nmb, W = o["rec"], o["nmb"], o["W"]
    t8mb = rec["transform8x8_flag"] == 1
    assert (rec["b8ref"] == 1).any() and (rec["b8ref"] == 0).any()
    if t8:
        assert t8mb.any()
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
    assert np.array_equal(o["got"]["modes"]["mode"], modes["mode"]) and np.array_equal(o["got"]["modes"]["pad"][:, 0], modes["pad"][:, 0])
    by_slot = [None] * (max(slot_of) + 1)
    for r in range(2):
        by_slot[slot_of[r]] = oracle.RefPic(*o["refs"][r], yuv_format=2)
    want = oracle.residual_frame(by_slot, o["cur"], mbs, mv, modes, o["quants"], pkg.TQ_JOB_DTYPE, yuv_format=2, blk_ref=blk_ref, wp=o["wp"])
    assert (o["got"]["cbp"] != 0).any()
    check_download(o["got"], o["recon"], want, t8mb, o["ar"])
    check_records(o["records"], o["records8"], o["pred"], want, mbs, t8mb, o["ar"], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("handover,t8", [("candidates", 0), ("candidates8", 1)])
def test_candidate_handovers_fused_equals_separate_422(pkg, monkeypatch, handover, t8):
    """jmhip_slice_to_frame_candidates / _candidates8 in a 4:2:2 context: the fused stage and the separate kernels leave the same bytes."""
    o = slice_case(pkg, monkeypatch, -1, t8, (1, 0), False, fused=True, handover=handover)
    s = slice_case(pkg, monkeypatch, -1, t8, (1, 0), False, fused=False, handover=handover)
    check_against_separate(o, s)
    assert (o["got"]["cbp"] != 0).any()
    if t8:
        assert int(o["records8"]["transform8x8"].sum()) == o["nmb"] and o["got"]["modes"]["pad"][:, 0].all()
    else:
        assert not o["records8"].tobytes().strip(b"\0") and (o["got"]["modes"]["mode"] == 8).all()


@pytest.mark.gpu
def test_422_records_refusals(pkg, monkeypatch):
    """Which download serves which frame stage: the 4:2:0 record refuses after a fused 4:2:2 stage, the 4:2:2 record after a 4:2:0 one, and the
    separate kernels leave neither records nor a prediction picture."""
    for fmt in (2, 1):
        inp = build_inputs(pkg, seed=5, w=64, h=48, qp=28, cavlc=1, ar=1, far=6, planes=True, given=False, t8="none", fmt=fmt)
        n = len(inp["mbs"])
        monkeypatch.delenv("JMHIP_FRAME_FUSED", raising=False)
        ctx = pkg.Context(64, 48, yuv_format=fmt, max_refs=1, search_range=R)
        try:
            ctx.ref_upload(0, *inp["refs"][0])
            ctx.interp_luma(0)
            ctx.interp_chroma(0)
            ctx.cur_upload(*inp["cur"])
            prm = pkg.MeParams()
            prm.search_mode, prm.search_range, prm.rdopt = -1, R, 1
            prm.level_mv_min, prm.level_mv_max = -511, 511
            prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lambda_factors(28)
            prm.subpel, prm.partition_mask = 1, (1 << 41) - 1
            ctx.me_frame(prm, inp["mbs"])
            ctx.residual_frame(inp["quants"], None)
            good, bad = (ctx.residual_records422, ctx.residual_records) if fmt == 2 else (ctx.residual_records, ctx.residual_records422)
            assert len(good(n)) == n
            with pytest.raises(pkg.JmhipError, match="residual_records"):
                bad(n)
            with pytest.raises(pkg.JmhipError):              # jmhip_frame_keep_prediction was not switched on
                ctx.pred_download()
            ctx.frame_keep_prediction()
            ctx.residual_frame(inp["quants"], None)
            assert ctx.pred_download()[1].shape == ((48, 32) if fmt == 2 else (24, 32))
            monkeypatch.setenv("JMHIP_FRAME_FUSED", "0")
            ctx.residual_frame(inp["quants"], None)
            for call in (lambda: good(n), lambda: bad(n), ctx.pred_download):
                with pytest.raises(pkg.JmhipError):
                    call()
        finally:
            ctx.close()
