"""The 8x8-transform P8x8 candidate of a Transform8x8Mode slice search on the device (jmhip_slice_to_frame_candidates8): the reference each
8x8 block settled on in that pass (jmhip_slice_ref8ts_download), and the fused frame stage fed with every macroblock in that form -- sub-mode 4,
luma_transform_size_8x8_flag, the pass's vectors -- which is what JM's LumaResidualCoding8x8 codes inside submacroblock_mode_decision(...,
transform8x8 = 1) (src/md_low.c:226-251). Records, side records, prediction picture and reconstruction against the oracle's residual-frame
restatement, and against the decided hand-over where the decision IS that pass. Same synthetic two-reference clip and slot permutation as
tests/test_slice_gpu.py::test_slice_search_feeds_the_frame_stage."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle


def search(pkg, mode, t8, weighted, qp=28):
    from tests.test_slice_gpu import slice_params, synth_clip, upsampled_chroma
    W, H, R, nref = 176, 144, 16, 2
    rng = np.random.default_rng(23)
    clip = synth_clip(rng, W, H, 3)
    clip[0] = np.clip(clip[0].astype(int) + 9, 0, 255).astype(np.uint8)        # a brightness step, so that reference 1 wins for some blocks
    cur, refs = clip[2], [clip[1], clip[0]]
    cur_c = upsampled_chroma(rng, cur)
    refs_c = [upsampled_chroma(rng, r) for r in refs]
    slot_of = [1, 0]                                                          # list-0 index -> reference slot, deliberately not the identity
    nmb = (W // 16) * (H // 16)
    ctx = pkg.Context(W, H, yuv_format=1, max_refs=2, search_range=R)
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
    recs, prms = [], []
    for first, count in ((0, 40), (40, nmb - 40)):                            # two slices: the second must not overwrite the first's references
        p = slice_params(pkg, mode, R, nref, [lam] * 3, 8, W, mb_first=first, mb_count=count, t8=t8, qp_n=qp)
        p.ref_slot[0], p.ref_slot[1] = slot_of
        if weighted and t8:
            p.wp_pred, p.wp_round, p.wp_denom = 1, 16, 5
            p.wp_weight[0], p.wp_offset[0], p.wp_weight[1], p.wp_offset[1] = 30, 2, 34, -3
        if mode == 3:
            lib.jmhip_epzs_scales(p, 4, (C.c_int * 2)(2, 0), 2)
        recs.append(ctx.p_slice_search(p))
        prms.append(p)
    wp = None
    if weighted:
        wp = {"luma_round": 16, "luma_denom": 5, "chroma_round": 8, "chroma_denom": 4, "weight": np.zeros((16, 3), int), "offset": np.zeros((16, 3), int)}
        wp["weight"][0], wp["offset"][0] = (30, 17, 15), (2, -1, 0)
        wp["weight"][1], wp["offset"][1] = (34, 16, 14), (-3, 1, 2)
    ctx.frame_wp_set(wp)
    quants = [pkg.flat_quant(qp + d, 342, adaptive_rounding=0, adapt_rnd_weight=4, cavlc=1) for d in (0, 0, 3)]
    quants.append(pkg.flat_quant(qp, 342, is8x8=True, adaptive_rounding=0, adapt_rnd_weight=4, cavlc=1, transform8x8_flag=1))
    quants = np.array(quants, dtype=pkg.QUANT_DTYPE)
    d = dict(ctx=ctx, W=W, H=H, nmb=nmb, rec=np.concatenate(recs), ref_cost1=int(prms[0].ref_cost1), slot_of=slot_of, refs=refs, refs_c=refs_c,
             cur=cur, cur_c=cur_c, wp=wp, quants=quants)
    return d


def frame_pass(ctx, nmb, quants, handover):
    ctx.frame_keep_prediction()
    handover()
    ctx.residual_frame(quants, None)
    return dict(got=ctx.residual_download(nmb), recon=ctx.recon_download(), records=ctx.residual_records(nmb), records8=ctx.residual_records8(nmb),
                pred=ctx.pred_download())


@pytest.mark.gpu
@pytest.mark.parametrize("mode,t8,weighted", [(3, 1, False), (-1, 1, True), (3, 2, True), (-1, 2, False)])
def test_t8_candidate_pass_feeds_the_frame_stage(pkg, mode, t8, weighted):
    d = search(pkg, mode, t8, weighted)
    ctx, nmb, rec, slot_of, quants = d["ctx"], d["nmb"], d["rec"], d["slot_of"], d["quants"]
    try:
        ref8 = ctx.slice_ref8ts(0, nmb)
        ref8_tail = ctx.slice_ref8ts(40, nmb - 40)
        cand = frame_pass(ctx, nmb, quants, lambda: ctx.slice_to_frame_candidates8(slot_of, 0, nmb))
        dec = frame_pass(ctx, nmb, quants, lambda: ctx.slice_to_frame(slot_of))
    finally:
        ctx.frame_wp_set(None)
        ctx.close()
    assert np.array_equal(ref8_tail, ref8[40:])

    # ref8ts: the decided reference where the decision is that pass; everywhere else list0_cost's first strict minimum over the references of
    # (ref ? ref_cost1 : 0) + the pass's motion cost (oracle/jmo_lowcplx.c:349, mode_decision.c:255)
    assert ((ref8 == 0) | (ref8 == 1)).all()
    t8p8 = (rec["best_mode"] == 8) & (rec["transform8x8_flag"] == 1)
    assert (~t8p8).any() and (t8 == 1 or t8p8.any())          # (Transform8x8Mode 2: every P8x8 decision is the 8x8-transform pass)
    assert np.array_equal(ref8[t8p8], rec["b8ref"][t8p8])
    for i in range(nmb):
        for k in range(4):
            best, best_ref = None, 0
            for r in range(2):
                c = (d["ref_cost1"] if r else 0) + int(rec[i]["cost8ts"][r, k])
                if best is None or c < best:
                    best, best_ref = c, r
            assert ref8[i, k] == best_ref, (i, k, rec[i]["cost8ts"][:2, k].tolist())
    assert (ref8 == 1).any() and (ref8 == 0).any()

    # the hand-over: mode 8, sub-mode 4 and the 8x8 transform everywhere
    got = cand["got"]
    assert (got["modes"]["mode"] == 8).all() and (got["modes"]["b8mode"] == 4).all() and (got["modes"]["pad"][:, 0] == 1).all()
    r8 = cand["records8"]
    assert (r8["transform8x8"] == 1).all() and (r8["interleaved"] == 1).all()

    # against the oracle fed with those fields
    W = d["W"]
    modes = np.zeros(nmb, dtype=pkg.MB_MODE_DTYPE)
    mbs = np.zeros(nmb, dtype=pkg.ME_MB_DTYPE)
    mv = np.zeros((nmb, 41, 2), np.int16)
    blk_ref = np.zeros((nmb, 4), int)
    parts = pkg.partition_table()
    for i in range(nmb):
        mbs[i]["mb_x"], mbs[i]["mb_y"] = i % (W // 16), i // (W // 16)
        modes[i]["mode"], modes[i]["b8mode"], modes[i]["pad"][0] = 8, 4, 1
        blk_ref[i] = [slot_of[int(r)] for r in ref8[i]]
        for pi in range(41):
            x4, y4 = parts[pi][1], parts[pi][2]
            rr = int(ref8[i, 2 * (y4 >> 1) + (x4 >> 1)])
            mv[i, pi] = rec[i]["mv8ts"][rr, pi - 5] if 5 <= pi < 9 else rec[i]["mv"][rr, pi]
    by_slot = [None, None]
    for r in range(2):
        by_slot[slot_of[r]] = oracle.RefPic(d["refs"][r], *d["refs_c"][r], yuv_format=1)
    want = oracle.residual_frame(by_slot, (d["cur"],) + d["cur_c"], mbs, mv, modes, quants, pkg.TQ_JOB_DTYPE, yuv_format=1, blk_ref=blk_ref, wp=d["wp"])
    assert np.array_equal(got["cbp"], want["cbp"]) and np.array_equal(got["cbp_blk"], want["cbp_blk"])
    for k in range(3):
        assert np.array_equal(cand["recon"][k], want["recon"][k]), "plane %d" % k
    assert (got["cbp"] != 0).any()
    wl = want["luma"]
    records, pred = cand["records"], cand["pred"]
    for i in range(nmb):
        x, y = 16 * (i % (W // 16)), 16 * (i // (W // 16))
        assert np.array_equal(pred[0][y:y + 16, x:x + 16], want["jobs_y"][i]["pred"]), "candidate prediction of macroblock %d" % i
        assert np.array_equal(records[i]["recon_y"], wl["recon"][i]) and int(records[i]["nonzero"]) == 0
        for b8 in range(4):
            assert int(r8[i]["coeff_cost"][b8]) == int(wl["coeff_cost"][i, b8]) and int(r8[i]["nonzero"][b8]) == int(wl["nonzero"][i, b8])
            for k in range(4):
                c = int(r8[i]["cnt"][b8, k])
                assert np.array_equal(r8[i]["lev"][b8, 16 * k:16 * k + c], wl["levels"][i, 4 * b8 + k, :c]) and wl["levels"][i, 4 * b8 + k, c] == 0
                assert np.array_equal(r8[i]["run"][b8, 16 * k:16 * k + c], wl["runs"][i, 4 * b8 + k, :c])

    # where the decision is the 8x8-transform pass, the decided hand-over codes the very same blocks: byte-identical luma
    for i in np.nonzero(t8p8)[0]:
        x, y = 16 * (i % (W // 16)), 16 * (i // (W // 16))
        assert dec["records8"][i].tobytes() == r8[i].tobytes(), "side record of macroblock %d" % i
        assert np.array_equal(dec["records"][i]["recon_y"], records[i]["recon_y"])          # (fadj_y: adaptive rounding is off)
        assert np.array_equal(dec["pred"][0][y:y + 16, x:x + 16], pred[0][y:y + 16, x:x + 16])
        assert np.array_equal(dec["recon"][0][y:y + 16, x:x + 16], cand["recon"][0][y:y + 16, x:x + 16])


@pytest.mark.gpu
def test_t8_candidate_pass_needs_a_t8_search(pkg):
    d = search(pkg, -1, 0, False)
    ctx, nmb = d["ctx"], d["nmb"]
    try:
        assert (ctx.slice_ref8ts(0, nmb) == -1).all()        # the pass did not run
        with pytest.raises(pkg.JmhipError):
            ctx.slice_to_frame_candidates8(d["slot_of"], 0, nmb)
    finally:
        ctx.frame_wp_set(None)
        ctx.close()
