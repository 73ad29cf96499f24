"""jmhip_p_slice_search (me_wave.hip): a whole P slice on the device -- predictors, FullSearch / FastFull / UMHexagonS / EPZS integer search,
sub-pel refinement, skip shortcut and the low-complexity inter decision as a macroblock wavefront -- bit-exact against
  (1) the REAL JM: the frame-level fixtures tests/golden/field_*.npz (every BlockMotionSearch call + the final field of each P picture),
  (2) the oracle's driver (oracle/jmo_lowcplx.c, itself pinned on those fixtures) on larger synthetic pictures, several references, slices."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import oracle
from tests.test_golden_field import CASES, GOLD, QP_N, part_index

FIELDS = ("pred", "mv_int", "cost_int", "mv", "cost")


def slice_params(pkg, *args, **kw):
    """the package's host helper (h.264_amd/slice_host.py); the flat 8x8 tables it takes from jmhip_flat_quant equal the oracle's (tests/test_tq.py)"""
    return pkg.slice_host.slice_params(*args, **kw)


def compare(got, want, nref, what):
    for f in ("pred8ts", "mv_int8ts", "mv8ts", "cost_int8ts", "cost8ts"):
        if not np.array_equal(got[f][:, :nref], want[f][:, :nref]):
            i = int(np.argwhere(np.any((got[f][:, :nref] != want[f][:, :nref]).reshape(len(got), -1), axis=1))[0][0])
            raise AssertionError("%s: %s differs at macroblock %d: device %s oracle %s" % (what, f, i, got[f][i, :nref].tolist(), want[f][i, :nref].tolist()))
    for f in ("best_mode", "min_cost", "b8mode", "b8ref", "final_mv", "skip_mv", "transform8x8_flag", "cbp8ts", "p8mode", "p8ref"):
        if not np.array_equal(got[f], want[f]):
            i = int(np.argwhere(np.any((got[f] != want[f]).reshape(len(got), -1), axis=1))[0][0])
            raise AssertionError("%s: %s differs at macroblock %d: device %s oracle %s" % (what, f, i, got[f][i].tolist(), want[f][i].tolist()))
    for f in FIELDS:
        g, w = got[f][:, :nref], want[f][:, :nref]
        if not np.array_equal(g, w):
            idx = np.argwhere((g != w).reshape(len(got), nref, 41, -1).any(axis=3))[0]
            raise AssertionError("%s: %s differs at macroblock %d ref %d partition %d: device %s oracle %s" % (what, f, idx[0], idx[1], idx[2], g[tuple(idx)].tolist(), w[tuple(idx)].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_pictures_match_the_real_jm(pkg, name):
    case = CASES[name] if isinstance(CASES[name], tuple) else (CASES[name], 0, 1)
    mode, t8, cavlc = case[:3]
    metric = case[3] if len(case) > 3 else (0, 2, 2)
    md_metric = case[4] if len(case) > 4 else 2
    z = np.load(os.path.join(GOLD, name + ".npz"))
    n = int(z["n_frames"])
    W, H = int(z["f0_head"][0]), int(z["f0_head"][1])
    R = 16
    ctx = pkg.Context(W, H, yuv_format=0, max_refs=2, search_range=R)
    ctx.slice_state_reset()
    epzs = oracle.Epzs(W, H, R, 2) if mode == 3 else None         # only its EPZSSliceInit: the co-located field is an INPUT of the device call
    lib = pkg.load_library()
    for k in range(n):
        head = z["f%d_head" % k]
        nref = int(head[3])
        refinfo = z["f%d_refinfo" % k]
        for r in range(nref):
            ctx.ref_upload(r, z["f%d_refs" % k][r])
            ctx.interp_luma(r)
        ctx.cur_upload(z["f%d_cur" % k])
        p = slice_params(pkg, mode, R, nref, [int(v) for v in head[6:9]], int(head[9]), W, H=H, t8=t8, cavlc=cavlc, metric=metric, md_metric=md_metric,
                         **(dict(qp_n=int(head[2])) if t8 else {}))
        if mode == 3:
            ids = (refinfo[:, 1].astype(np.int64) & 0xffffffff) | (refinfo[:, 2].astype(np.int64) << 32)
            epzs.slice_init(int(head[10]), [int(v) for v in refinfo[:, 0]], ids, z["f%d_col_mv" % k], z["f%d_col_ref_id" % k], num_ref_idx_l0_active=int(head[11]))
            ctx.epzs_colocated_upload(oracle.epzs_colocated(epzs, W, H))
            pocs = [int(v) for v in refinfo[:, 0]]
            lib.jmhip_epzs_scales(p, int(head[10]), (C.c_int * nref)(*pocs), nref)
        got = ctx.p_slice_search(p)
        bad = 0
        seen = set()
        for (mb, ref, bt, bx, by, px, py, mx, my, cost, rng, lam) in z["f%d_calls" % k]:
            pi = part_index(int(bt), int(bx), int(by))
            g = got[int(mb)]
            first8 = t8 and int(bt) == 4 and (int(mb), int(ref), pi) not in seen          # the 8x8-transform P8x8 pass searches the 8x8 blocks first
            seen.add((int(mb), int(ref), pi))
            if first8:
                t = (int(g["pred8ts"][ref, pi - 5, 0]), int(g["pred8ts"][ref, pi - 5, 1]), int(g["mv8ts"][ref, pi - 5, 0]), int(g["mv8ts"][ref, pi - 5, 1]), int(g["cost8ts"][ref, pi - 5]))
            else:
                t = (int(g["pred"][ref, pi, 0]), int(g["pred"][ref, pi, 1]), int(g["mv"][ref, pi, 0]), int(g["mv"][ref, pi, 1]), int(g["cost"][ref, pi]))
            if t != (px, py, mx, my, cost):
                if not bad:
                    first = "picture %d mb %d ref %d blocktype %d block (%d,%d): JM pred (%d,%d) mv (%d,%d) cost %d, device %s" % (k, mb, ref, bt, bx, by, px, py, mx, my, cost, t)
                bad += 1
        assert bad == 0, "%d of %d BlockMotionSearch calls differ from JM; first: %s" % (bad, len(z["f%d_calls" % k]), first)
        ref_idx, mv = ctx.slice_field()
        fld = z["f%d_field" % k]
        assert np.array_equal(ref_idx, fld[..., 0]) and np.array_equal(mv, fld[..., 1:]), "picture %d: final field differs from JM" % k
    if epzs:
        epzs.close()
    ctx.close()


def synth_clip(rng, W, H, nframes):
    from tests.conftest import load_pkg
    return load_pkg().slice_host.synth_clip(rng, W, H, nframes)


def run_synthetic(pkg, mode, W, H, R, nref, slices=1, nframes=3, seed=5, metric=(0, 2, 2), qp=28, max_mbs=None, t8=0, cavlc=1, wp=None, one_call=False, rdopt=0, map_log=None, map_init=None, what_if=None, ideal_map=False, first_touch=None, md_metric=2, q8=None, lambda_mf=None, clip=None, oracle_only=False):
    """Frames 1.. are coded as P pictures against the previous `nref` SOURCE frames (the search does not care where a reference came from).
    lambda_mf: the three factors when they are to differ (tests/lambda_cases.py); clip: the frames, for pictures other than synth_clip's.
    oracle_only (with what_if): no device is touched and `pkg` is not used -- the oracle's records alone, for tests that run without a GPU."""
    assert not oracle_only or (what_if is not None and map_init is None and not one_call)
    rng = np.random.default_rng(seed)
    if clip is None:
        clip = synth_clip(rng, W, H, nframes + nref - 1)
    lam = int(65536 * np.sqrt(0.85 * 2 ** ((qp - 12) / 3.0) * (4 if False else 1)) + 0.5)     # any positive factor does
    lam3 = [lam, lam, lam] if lambda_mf is None else list(lambda_mf)
    ref_cost1 = int(2 * np.sqrt(0.85 * 2 ** ((qp - 12) / 3.0)))
    nmb = (W // 16) * (H // 16)
    ctx = None if oracle_only else pkg.Context(W, H, yuv_format=0, max_refs=nref, search_range=R)
    if ctx:
        ctx.slice_state_reset()
    epzs = oracle.Epzs(W, H, R, nref) if mode == 3 else None
    if map_init is not None:                             # EPZSMap / EPZSBlkCount of an encoder that is already running
        ctx.epzs_map_upload(map_init[0], R, map_init[1])
        epzs.map_set(map_init[0], map_init[1])
    if ideal_map:                                        # NOT JM: the oracle's what-if with a map cleared per search (with what_if: oracle only, collecting the records)
        epzs.ideal_map()
    umhex = oracle.Umhex(W, H, R, nref, qp) if mode == 1 else None
    all_mv_state = np.zeros((4, 4, oracle.MAX_REFS, 9, 2), np.int16)
    prev_field = [(np.zeros((H // 4, W // 4, 2), np.int16), np.full((H // 4, W // 4), -1, np.int64))] * 2
    lib = None if oracle_only else pkg.load_library()
    passes = []
    for f in range(nref, nref + nframes - 1):
        cur = clip[f]
        refs = [clip[f - 1 - r] for r in range(nref)]
        pocs = [2 * (f - 1 - r) for r in range(nref)]
        orefs = [oracle.RefPic(r, yuv_format=0) for r in refs]
        for r in range(nref if ctx else 0):
            ctx.ref_upload(r, refs[r])
            ctx.interp_luma(r)
        if ctx:
            ctx.cur_upload(cur)
        if epzs:
            epzs.slice_init(2 * f, pocs, pocs, [prev_field[0][0], prev_field[1][0]], [prev_field[0][1], prev_field[1][1]])
            if ctx:
                ctx.epzs_colocated_upload(oracle.epzs_colocated(epzs, W, H))
        ref_idx = np.full((H // 4, W // 4), -1, np.int8)
        mvf = np.zeros((H // 4, W // 4, 2), np.int16)
        per = (nmb + slices - 1) // slices
        wants = []
        for s in range(slices):
            first, count = s * per, min(per, nmb - s * per)
            q = oracle.lowcplx_params(mode, R, nref, lam3, ref_cost1, W, H, epzs=epzs, umhex=umhex, all_mv_state=all_mv_state, metric=metric,
                                      transform8x8_mode=t8, qp=qp, cavlc=cavlc, rdopt=rdopt, md_metric=md_metric, q8=q8)
            if wp:                                       # explicit weighted prediction, used in the search too (UseWeightedReferenceME): (denominator, [(weight, offset)] per reference)
                q.wp_pred, q.me.apply_weights = 1, 1
                q.me.luma_log_weight_denom, q.me.wp_luma_round = wp[0], (1 << (wp[0] - 1)) if wp[0] else 0
                for r in range(nref):
                    q.wp_weight[r], q.wp_offset[r] = wp[1][r]
            sid = (np.arange(nmb) // per).astype(np.int32)
            q._sid = sid
            q.slice_id = sid.ctypes.data
            want, _, _ = oracle.lowcplx_p_slice(q, orefs, cur, ref_idx, mvf, mb_first=first, mb_count=count)
            if what_if is not None:
                what_if.append(want)
                continue
            if one_call:                                 # the device searches all slices of the picture in ONE call (slice_mbs) below
                wants.append(want)
                continue
            p = slice_params(pkg, mode, R, nref, lam3, ref_cost1, W, mb_first=first, mb_count=count, metric=metric, qp_n=qp, t8=t8, cavlc=cavlc, rdopt=rdopt, md_metric=md_metric, q8=q8)
            if mode == 3:
                lib.jmhip_epzs_scales(p, 2 * f, (C.c_int * nref)(*pocs), nref)
            if wp:
                p.wp_me, p.wp_pred, p.wp_denom, p.wp_round = 1, 1, wp[0], (1 << (wp[0] - 1)) if wp[0] else 0
                for r in range(nref):
                    p.wp_weight[r], p.wp_offset[r] = wp[1][r]
            got = ctx.p_slice_search(p)
            passes.append(ctx.slice_passes())
            compare(got, want, nref, "frame %d slice %d" % (f, s))
            if map_log is not None:                      # EPZS: (aliased map tests of this slice, searches so far) on the device and in the oracle
                map_log.append((ctx.epzs_map_info(), (epzs.alias_events() - sum(m[1][0] for m in map_log), epzs.search_count())))
        if one_call:
            p = slice_params(pkg, mode, R, nref, lam3, ref_cost1, W, mb_first=0, mb_count=nmb, metric=metric, qp_n=qp, t8=t8, cavlc=cavlc, rdopt=rdopt, md_metric=md_metric, q8=q8)
            p.slice_mbs = per
            if mode == 3:
                lib.jmhip_epzs_scales(p, 2 * f, (C.c_int * nref)(*pocs), nref)
            got = ctx.p_slice_search(p)
            passes.append(ctx.slice_passes())
            compare(got, np.concatenate(wants), nref, "frame %d, %d slices in one call" % (f, slices))
        if what_if is None:
            gref, gmv = ctx.slice_field()
            assert np.array_equal(gref, ref_idx) and np.array_equal(gmv, mvf), "frame %d: final field" % f
        # what EPZS will read of this picture when it is the co-located one: its vectors and, as reference ids, the POCs of what they point to
        ids = np.where(ref_idx >= 0, np.array(pocs, np.int64)[np.clip(ref_idx, 0, None)], -1)
        prev_field = [(mvf.copy(), ids), prev_field[0]]
    if epzs:
        if first_touch is not None:
            first_touch.append(epzs.first_touch())
        epzs.close()
    if umhex:
        umhex.close()
    if ctx:
        ctx.close()
    return passes


@pytest.mark.gpu
@pytest.mark.parametrize("mode,W,H,R,nref,slices", [
    (-1, 96, 64, 8, 1, 1),          # FullSearch: per-partition centres from the true predictors
    (-1, 96, 64, 8, 2, 2),
    (0, 96, 64, 8, 2, 1),           # FastFullSearch
    (3, 176, 144, 16, 2, 1),        # EPZS, two references
    (3, 320, 192, 32, 3, 3),        # EPZS, +-32, three references, three slices (the last two begin mid-row)
    (1, 176, 144, 16, 2, 1),        # UMHexagonS with the dynamic search range
    (1, 320, 192, 32, 3, 3),
    (2, 176, 144, 16, 2, 1),        # the simplified UMHexagonS (me_umhexsmp.c)
    (2, 320, 192, 32, 3, 3),
    (3, 176, 144, 16, 5, 1),        # five references (JMHIP_SLICE_REFS): EPZS, UMHexagonS, simplified UMHexagonS
    (1, 176, 144, 16, 5, 2),
    (2, 176, 144, 16, 5, 1),
])
def test_synthetic_clip_matches_the_oracle(pkg, mode, W, H, R, nref, slices):
    run_synthetic(pkg, mode, W, H, R, nref, slices=slices)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,metric,md,t8", [
    (3, (1, 1, 1), 1, 0),           # EPZS: SSE at every level and in the decision costs
    (1, (1, 1, 1), 1, 0),           # UMHexagonS (its thresholds are then fed squared errors, as in JM)
    (2, (0, 1, 2), 0, 0),           # simplified UMHexagonS: SAD integer, SSE half-pel, Hadamard SAD quarter-pel
    (-1, (0, 1, 1), 1, 1),          # FullSearch: SAD at integer positions (the only metric the exhaustive modes take there), SSE refinement, SSE transform decision
    (0, (0, 2, 1), 1, 0),           # FastFull
])
def test_sse_metric_in_the_slice_search(pkg, mode, metric, md, t8):
    """computeSSE (me_distortion.c:1042) through the computeUniPred dispatch of mv-search.c:400-424 and as ModeDecisionMetric (distortion4x4 of the skip
    cost, TransformDecision): the walkers at every level, the exhaustive searches' refinements, the decision costs."""
    run_synthetic(pkg, mode, 176, 144, 16, 2, metric=metric, md_metric=md, t8=t8, qp=30)


@pytest.mark.gpu
def test_epzs_visited_map_aliases(pkg):
    """EPZSMap is never cleared and EPZSBlkCount has 16 bits (me_epzs.c:49,1550,1598,1757,1840): a map test also reads "visited" from the stamp
    a search 65536 k calls earlier left. 720x576 = 1620 macroblocks x 41 searches x 2 references = 132840 searches per picture, so the counter
    wraps twice a picture; on this clip (picked with tools/find_epzs_alias.py) the oracle's shadow map counts such tests in the fifth P
    picture. The device must report the same number of them, slice by slice, the same search count -- and the same searches."""
    log = []
    run_synthetic(pkg, 3, 720, 576, 32, 2, nframes=6, seed=5, map_log=log)
    assert len(log) == 5
    for dev, orc in log:
        assert dev == orc, "device (aliased tests, searches) %s, oracle %s" % (dev, orc)
    assert sum(orc[0] for _, orc in log) > 0, "the clip no longer produces an aliased map test: pick another (tools/find_epzs_alias.py)"


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,R,nref,slices", [(352, 288, 16, 2, 1), (320, 192, 32, 3, 3)])
def test_epzs_map_of_a_running_encoder(pkg, W, H, R, nref, slices):
    """The same mechanism under load: the search starts from the map and the counter of an encoder in mid-stream (jmhip_epzs_map_upload). The
    map is the worst one: every cell carries the stamp of the search that, with a map cleared per search, would be the first to test it (taken
    from a what-if run of the oracle) -- so the first test of most cells is answered from the old stamp, in most macroblocks, and that changes
    what the searches find. The counter also wraps within the first picture."""
    start = 65000
    probe, ideal = [], []
    run_synthetic(pkg, 3, W, H, R, nref, slices=slices, map_init=(None, start), what_if=ideal, ideal_map=True, first_touch=probe)
    first = probe[0]
    stamps = np.where(first > 0, first & 0xffff, start).astype(np.uint16).view(np.int16)
    log, jm = [], []
    run_synthetic(pkg, 3, W, H, R, nref, slices=slices, map_init=(stamps, start), map_log=log)
    assert all((dev[0], dev[1] & 0xffff) == (orc[0], orc[1] & 0xffff) for dev, orc in log), log
    assert sum(orc[0] for _, orc in log) > 100, log
    run_synthetic(pkg, 3, W, H, R, nref, slices=slices, map_init=(stamps, start), what_if=jm)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(ideal, jm)), "the aliased tests of this clip change nothing: the test does not show the mechanism"


@pytest.mark.gpu
@pytest.mark.parametrize("mode,W,H,R,nref,slices", [
    (-1, 176, 144, 16, 1, 1),       # FullSearch: one work item per distinct window centre of a macroblock
    (-1, 176, 144, 16, 2, 2),
    (0, 176, 144, 16, 2, 1),        # FastFullSearch: one window per macroblock and reference, centred on the 16x16 predictor
    (0, 320, 192, 32, 3, 3),        # +-32, three references, three slices (the last two begin mid-row)
    (-1, 320, 192, 32, 4, 3),
    (0, 176, 144, 20, 4, 1),        # a range between the kernel's column groupings (2R+1 = 41)
    (-1, 176, 144, 40, 1, 1),       # the largest range of the pair-lane kernel
    (0, 176, 144, 16, 5, 2),        # five references: what every cfg the reference ships asks for (NumberReferenceFrames = 5)
    (-1, 176, 144, 16, 5, 1),
])
def test_exhaustive_searches_as_sweeps_over_the_frame_kernels(pkg, mode, W, H, R, nref, slices):
    """16 <= search_range <= 40, JM's default metrics, the 4x4 transform: FullSearch / FastFullSearch slices run as relaxation sweeps whose
    searches are the frame kernels over device-built work lists (me_xslice.hip): replay of the decision on call records -> integer search of the
    records whose predictor changed -> their refinement -> skip costs, until a sweep asks for nothing and changes nothing."""
    passes = run_synthetic(pkg, mode, W, H, R, nref, slices=slices)
    print("sweeps per slice call:", passes)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,nref,sweeps", [(-1, 2, "1"), (0, 2, "2"), (-1, 1, "3")])
def test_exhaustive_sweeps_hand_over_to_the_macroblock_kernels(pkg, mode, nref, sweeps, monkeypatch):
    """The sweeps are capped; when they have not settled, the one-wave-per-macroblock schedules of me_wave.hip finish from the field they left
    (any state is a legal first guess). JMHIP_SLICE_SWEEPS caps both; JMHIP_SLICE_X=0 switches the frame-kernel sweeps off altogether."""
    monkeypatch.setenv("JMHIP_SLICE_SWEEPS", sweeps)
    run_synthetic(pkg, mode, 176, 144, 16, nref, nframes=2)
    monkeypatch.delenv("JMHIP_SLICE_SWEEPS")
    monkeypatch.setenv("JMHIP_SLICE_X", "0")
    run_synthetic(pkg, mode, 176, 144, 16, nref, nframes=2)


@pytest.mark.gpu
@pytest.mark.parametrize("sched,sweeps", [("wave", None), ("relax", "1"), ("relax", "3")])
@pytest.mark.parametrize("mode,W,H,R,nref,slices", [(3, 320, 192, 32, 3, 3), (1, 176, 144, 16, 2, 1), (0, 96, 64, 8, 2, 1), (-1, 96, 64, 8, 2, 2)])
def test_schedules_agree(pkg, mode, W, H, R, nref, slices, sched, sweeps, monkeypatch):
    """The default schedule is relaxation (every macroblock of the slice at once, sweep after sweep until nothing changes; me_wave.hip
    p_slice_relax_kernel). JMHIP_SLICE_SCHED=wave forces the coding-order wavefront; JMHIP_SLICE_SWEEPS caps the sweeps, after which the
    wavefront takes over from whatever state the sweeps left (1: after a single sweep). Every combination must give JM's result."""
    monkeypatch.setenv("JMHIP_SLICE_SCHED", sched)
    if sweeps:
        monkeypatch.setenv("JMHIP_SLICE_SWEEPS", sweeps)
    run_synthetic(pkg, mode, W, H, R, nref, slices=slices, nframes=3)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [3, 1, 2])
def test_sad_everywhere_and_satd_everywhere(pkg, mode):
    run_synthetic(pkg, mode, 176, 144, 16, 2, metric=(0, 0, 0), nframes=2)
    run_synthetic(pkg, mode, 176, 144, 16, 2, metric=(2, 2, 2), nframes=2)     # SATD at full-pel positions too (BASELINE config 3: "EPZS + SATD cost")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [3, 1])
def test_1080p_walkers_match_the_oracle(pkg, mode):
    """BASELINE configs 3 / 5 at their picture width: one 1920x1088 P picture, +-32, two references, every macroblock against the oracle."""
    passes = run_synthetic(pkg, mode, 1920, 1088, 32, 2, nframes=2, seed=11)
    print("passes per slice call:", passes)


@pytest.mark.gpu
def test_1080p_config3_tools_match_the_oracle(pkg):
    """BASELINE config 3 as it is worded -- EPZS, Hadamard SAD cost at every level, 8x8 transform enabled (Transform8x8Mode 1) -- on one 1920x1088 P
    picture, +-32, two references: every BlockMotionSearch call, the transform decisions, both P8x8 passes and the final field of every macroblock
    against the oracle (coarse quantiser, so that the coded-block-pattern fallback of the 8x8-transform pass occurs)."""
    passes = run_synthetic(pkg, 3, 1920, 1088, 32, 2, nframes=2, seed=13, metric=(2, 2, 2), t8=1, qp=34)
    print("passes per slice call:", passes)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,t8", [(-1, 0), (0, 0), (3, 0), (1, 0), (2, 0), (3, 1), (1, 2)])
def test_weighted_prediction_in_the_search(pkg, mode, t8):
    """Explicit weights per reference in every evaluation of the search (computeSADWP / computeSATDWP), in the skip cost and -- with the 8x8
    transform -- in the transform decision's predictions (LumaPrediction): all four search modes against the oracle."""
    run_synthetic(pkg, mode, 176, 144, 16, 2, nframes=3, seed=17, wp=(5, [(30, 2), (35, -4)]), t8=t8, qp=32)


@pytest.mark.gpu
def test_2160p_config5_search_matches_the_oracle(pkg):
    """BASELINE config 5's search at its picture size: UMHexagonS with explicit weighted prediction used in ME, 3840x2160, +-32, two references,
    every macroblock of one P picture against the oracle (the 4:2:2 of that config concerns the frame stage, not the luma search)."""
    passes = run_synthetic(pkg, 1, 3840, 2160, 32, 2, nframes=2, seed=19, wp=(6, [(60, 3), (70, -5)]))
    print("passes per slice call:", passes)


def upsampled_chroma(rng, Y):
    H, W = Y.shape
    U = np.clip(Y[::2, ::2].astype(int) // 2 + 60 + rng.integers(-3, 4, (H // 2, W // 2)), 0, 255).astype(np.uint8)
    V = np.clip(200 - Y[1::2, 1::2].astype(int) // 2 + rng.integers(-3, 4, (H // 2, W // 2)), 0, 255).astype(np.uint8)
    return U, V


@pytest.mark.gpu
@pytest.mark.parametrize("mode,weighted,planes,t8,candidates", [(3, False, True, 0, 0), (3, True, False, 0, 0), (-1, True, True, 0, 0), (1, False, False, 0, 0),
                                                                (3, False, False, 1, 0), (-1, True, True, 1, 0), (0, False, True, 2, 0),
                                                                # jmhip_slice_to_frame_candidates: every macroblock in its P8x8 candidate form (what JM codes inside
                                                                # submacroblock_mode_decision before it decides, src/mode_decision.c:874), whatever mode won
                                                                (-1, False, False, 0, 1), (3, True, True, 0, 1), (0, False, False, 0, 1)])
def test_slice_search_feeds_the_frame_stage(pkg, mode, weighted, planes, t8, candidates):
    """The searched picture goes to jmhip_residual_frame without leaving the device (jmhip_slice_to_frame): every 8x8 block predicts from the
    reference ITS decision chose (LumaPrediction's l0_ref_idx), optionally with explicit weighted prediction; reconstruction, cbp and cbp_blk of
    every macroblock against the oracle's LumaResidualCoding / ChromaResidualCoding restatement fed with the same records."""
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
        if planes:
            ctx.interp_chroma(slot_of[r])
    ctx.cur_upload(cur, *cur_c)
    if mode == 3:
        ctx.epzs_colocated_upload(np.zeros((H // 4, W // 4, 2), np.int16))
    lam = int(65536 * np.sqrt(0.85 * 2 ** ((28 - 12) / 3.0)) + 0.5)
    lib = pkg.load_library()
    recs = []
    for first, count in ((0, 40), (40, nmb - 40)):
        p = slice_params(pkg, mode, R, nref, [lam] * 3, 8, W, mb_first=first, mb_count=count, t8=t8, qp_n=28)
        p.ref_slot[0], p.ref_slot[1] = slot_of
        if weighted and t8:                                # LumaPrediction's explicit weights take part in the transform decision's predictions
            p.wp_pred, p.wp_round, p.wp_denom = 1, 16, 5
            p.wp_weight[0], p.wp_offset[0], p.wp_weight[1], p.wp_offset[1] = 30, 2, 34, -3
        if mode == 3:
            lib.jmhip_epzs_scales(p, 4, (C.c_int * 2)(2, 0), 2)
        recs.append(ctx.p_slice_search(p))
    rec = np.concatenate(recs)
    assert (rec["b8ref"] == 1).any() and (rec["b8ref"] == 0).any() and (rec["best_mode"] == 8).any()
    wp = None
    if weighted:
        wp = {"luma_round": 16, "luma_denom": 5, "chroma_round": 8, "chroma_denom": 4, "weight": np.zeros((16, 3), int), "offset": np.zeros((16, 3), int)}
        wp["weight"][0], wp["offset"][0] = (30, 17, 15), (2, -1, 0)
        wp["weight"][1], wp["offset"][1] = (34, 16, 14), (-3, 1, 2)
    ctx.frame_wp_set(wp)
    if candidates:
        assert (rec["best_mode"] != 8).any() and (rec["p8mode"] >= 4).all()
        ctx.frame_keep_prediction()
        ctx.slice_to_frame_candidates(slot_of, 0, nmb)
    else:
        ctx.slice_to_frame(slot_of)
    ar = 0 if t8 else 1                                    # Transform8x8Mode 1 in the slice search: no adaptive rounding
    quants = [pkg.flat_quant(28 + d, 342, adaptive_rounding=ar, adapt_rnd_weight=4, cavlc=1) for d in (0, 0, 3)]
    if t8:
        quants.append(pkg.flat_quant(28, 342, is8x8=True, adaptive_rounding=ar, adapt_rnd_weight=4, cavlc=1, transform8x8_flag=1))
    quants = np.array(quants, dtype=pkg.QUANT_DTYPE)
    ctx.residual_frame(quants, None)
    got = ctx.residual_download(nmb)
    recon = ctx.recon_download()
    records, pred = (ctx.residual_records(nmb), ctx.pred_download()) if candidates else (None, None)
    ctx.frame_wp_set(None)
    ctx.close()

    modes = np.zeros(nmb, dtype=pkg.MB_MODE_DTYPE)
    mbs = np.zeros(nmb, dtype=pkg.ME_MB_DTYPE)
    mv = np.zeros((nmb, 41, 2), np.int16)
    blk_ref = np.zeros((nmb, 4), int)
    parts = pkg.partition_table()
    for i in range(nmb):
        mbs[i]["mb_x"], mbs[i]["mb_y"] = i % (W // 16), i // (W // 16)
        cand = candidates
        modes[i]["mode"] = 8 if cand else rec[i]["best_mode"]
        modes[i]["b8mode"] = rec[i]["p8mode"] if cand else (rec[i]["b8mode"] if rec[i]["best_mode"] == 8 else 4)
        modes[i]["pad"][0] = 0 if cand else rec[i]["transform8x8_flag"]
        refs8 = rec[i]["p8ref"] if cand else rec[i]["b8ref"]
        blk_ref[i] = [slot_of[int(r)] for r in refs8]
        for pi in range(41):
            x4, y4 = parts[pi][1], parts[pi][2]
            rr = int(refs8[2 * (y4 >> 1) + (x4 >> 1)])
            mv[i, pi] = rec[i]["mv"][rr, pi]
            if not cand and rec[i]["best_mode"] == 8 and rec[i]["transform8x8_flag"] and 5 <= pi < 9:       # the 8x8-transform pass's vectors
                mv[i, pi] = rec[i]["mv8ts"][rr, pi - 5]
    assert np.array_equal(got["modes"]["mode"], modes["mode"]) and np.array_equal(got["modes"]["b8mode"], modes["b8mode"])
    if t8:
        assert (rec["transform8x8_flag"] == 1).any() and (t8 == 2 or (rec["transform8x8_flag"] == 0).any())
    by_slot = [None, None]
    for r in range(nref):
        by_slot[slot_of[r]] = oracle.RefPic(refs[r], *refs_c[r], yuv_format=1)
    want = oracle.residual_frame(by_slot, (cur,) + cur_c, mbs, mv, modes, quants, pkg.TQ_JOB_DTYPE, yuv_format=1, blk_ref=blk_ref, wp=wp)
    assert np.array_equal(got["cbp"], want["cbp"]) and np.array_equal(got["cbp_blk"], want["cbp_blk"])
    for k in range(3):
        assert np.array_equal(recon[k], want["recon"][k]), "plane %d" % k
    assert (got["cbp"] != 0).any()
    if candidates:                                         # what the JM binding answers the candidate pass from: the prediction picture and the dense records
        for i in range(nmb):
            x, y = 16 * (i % (W // 16)), 16 * (i // (W // 16))
            assert np.array_equal(pred[0][y:y + 16, x:x + 16], want["jobs_y"][i]["pred"]), "candidate prediction of macroblock %d" % i
            assert np.array_equal(records[i]["recon_y"], want["luma"]["recon"][i]) and np.array_equal(records[i]["coeff_cost"], want["luma"]["coeff_cost"][i])
            for b in range(16):
                n = int(records[i]["cnt"][b])
                assert np.array_equal(records[i]["lev"][b, :n], want["luma"]["levels"][i, b, :n]) and want["luma"]["levels"][i, b, n] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode,W,H,R,nref,slices,t8,qp,cavlc", [
    (3, 176, 144, 16, 2, 1, 1, 36, 1),      # EPZS, both transform sizes, coarse quantiser: 8x8-transform P8x8 winners without a coded block fall back
    (-1, 96, 64, 8, 2, 2, 1, 30, 0),        # FullSearch, CABAC cost counting, two slices
    (0, 96, 64, 8, 2, 1, 2, 28, 1),         # FastFullSearch, 8x8 transform only
    (1, 176, 144, 16, 2, 1, 1, 40, 1),      # UMHexagonS
    (3, 320, 192, 32, 3, 3, 1, 34, 1),
    (2, 176, 144, 16, 2, 1, 1, 34, 1),      # simplified UMHexagonS
])
def test_transform8x8_modes_match_the_oracle(pkg, mode, W, H, R, nref, slices, t8, qp, cavlc):
    """Transform8x8Mode 1 / 2 in the slice search: the 8x8 Hadamard for block types 1..4, TransformDecision after modes 1..3 (with the references
    it writes into the picture array), the 8x8-transform P8x8 pass, GetBestTransformP8x8 on ties, and the coded-block pattern of that pass
    (prediction, dct_8x8, coefficient cost) deciding between the two passes' partitionings."""
    run_synthetic(pkg, mode, W, H, R, nref, slices=slices, t8=t8, qp=qp, cavlc=cavlc)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,W,H,slices,t8", [(-1, 176, 144, 3, 0), (0, 320, 192, 8, 0), (2, 320, 192, 5, 0), (-1, 320, 192, 4, 1)])
def test_several_slices_in_one_call(pkg, mode, W, H, slices, t8):
    """slice_mbs: the slices of a picture (input->slice_mode 1: fixed macroblock count, most of them beginning mid-row) searched in ONE call --
    neighbours across slice boundaries unavailable, img->all_mv running on from slice to slice -- against the oracle run slice by slice."""
    run_synthetic(pkg, mode, W, H, 16, 2, slices=slices, one_call=True, t8=t8, qp=32)


@pytest.mark.gpu
def test_2160p_config4_eight_slices_in_one_call(pkg):
    """BASELINE config 4's picture and slice layout on ONE GPU: 3840x2160, FullSearch +-32, eight slices of 4050 macroblocks, one call."""
    passes = run_synthetic(pkg, -1, 3840, 2160, 32, 1, slices=8, nframes=2, seed=23, one_call=True)
    print("sweeps of the one call:", passes)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,slices", [(3, 5), (1, 5), (3, 2), (1, 3)])
def test_walkers_with_memories_several_slices_in_one_call(pkg, mode, slices):
    """EPZS and UMHexagonS keep picture-level memories (EPZSDistortion / EPZSMotion row arrays, the UMHexagonS cost maps) that JM carries on from
    slice to slice in coding order: the stored rows of the relaxation hold exactly that, so their slices go in one call too."""
    run_synthetic(pkg, mode, 320, 192, 16, 2, slices=slices, one_call=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,slices,t8", [(-1, 1, 0), (0, 2, 0), (2, 1, 0), (-1, 3, 1), (0, 1, 2)])
def test_call_records_for_the_high_complexity_modes(pkg, mode, slices, t8):
    """rdopt != 0: BlockMotionSearch without what JM does only with RDOptimization off (centre clamp, zero-vector bonuses, pos_00 pre-check, skip
    shortcut) -- the records the JM binding answers from, speculatively, when the encoder runs its rate-distortion decision."""
    run_synthetic(pkg, mode, 176, 144, 16, 2, slices=slices, rdopt=1, t8=t8, qp=30, one_call=slices > 1)


# ------------------------------------------------------------------ the transform decision on a position-dependent, asymmetric 8x8 quantiser

T8_TABLE_W, T8_TABLE_H, T8_TABLE_R, T8_TABLE_NREF = 96, 64, 8, 2           # the smallest clip of test_transform8x8_modes_match_the_oracle


def oracle_slices(mode, q8, qp, seed=5, nframes=3):
    """run_synthetic's oracle half alone (no device): the records of every P picture of the clip, one slice each, Transform8x8Mode 1 with q8."""
    W, H, R, nref = T8_TABLE_W, T8_TABLE_H, T8_TABLE_R, T8_TABLE_NREF
    rng = np.random.default_rng(seed)
    clip = synth_clip(rng, W, H, nframes + nref - 1)
    lam = int(65536 * np.sqrt(0.85 * 2 ** ((qp - 12) / 3.0)) + 0.5)
    ref_cost1 = int(2 * np.sqrt(0.85 * 2 ** ((qp - 12) / 3.0)))
    epzs = oracle.Epzs(W, H, R, nref) if mode == 3 else None
    umhex = oracle.Umhex(W, H, R, nref, qp) if mode == 1 else None
    all_mv_state = np.zeros((4, 4, oracle.MAX_REFS, 9, 2), np.int16)
    prev_field = [(np.zeros((H // 4, W // 4, 2), np.int16), np.full((H // 4, W // 4), -1, np.int64))] * 2
    out = []
    for f in range(nref, nref + nframes - 1):
        pocs = [2 * (f - 1 - r) for r in range(nref)]
        orefs = [oracle.RefPic(clip[f - 1 - r], yuv_format=0) for r in range(nref)]
        if epzs:
            epzs.slice_init(2 * f, pocs, pocs, [prev_field[0][0], prev_field[1][0]], [prev_field[0][1], prev_field[1][1]])
        ref_idx = np.full((H // 4, W // 4), -1, np.int8)
        mvf = np.zeros((H // 4, W // 4, 2), np.int16)
        q = oracle.lowcplx_params(mode, R, nref, [lam] * 3, ref_cost1, W, H, epzs=epzs, umhex=umhex, all_mv_state=all_mv_state,
                                  transform8x8_mode=1, qp=qp, cavlc=1, q8=q8)
        sid = np.zeros((W // 16) * (H // 16), np.int32)
        q._sid = sid
        q.slice_id = sid.ctypes.data
        out.append(oracle.lowcplx_p_slice(q, orefs, clip[f], ref_idx, mvf)[0])
        ids = np.where(ref_idx >= 0, np.array(pocs, np.int64)[np.clip(ref_idx, 0, None)], -1)
        prev_field = [(mvf.copy(), ids), prev_field[0]]
    for o in (epzs, umhex):
        if o:
            o.close()
    return np.concatenate(out)


# The quantiser enters the decision in one place: a P8x8 macroblock whose 8x8-transform pass won keeps it only if dct_8x8 leaves a coded block
# (coefficient cost > 4, md_low.c:547). That is a handful of macroblocks of a 48-macroblock picture, and a swap of row and column moves a cost
# across 4 only under a coarse quantiser: (qp, clip seed) per search mode below were found on the oracle alone (the table seed is 53 for all).
# Third entry: each of levelscale^T and leveloffset^T ALONE moves a decision. For EPZS no such input was found among 4 qp x 79 clip seeds;
# there only the two transposed together are shown to bite, so a kernel that mis-indexes one of the two tables alone could pass mode 3.
T8_TABLE_CASES = {-1: (38, 10, True), 0: (38, 10, True), 1: (38, 10, True), 3: (44, 36, False)}


def t8_table_case(pkg, mode):
    from tests.quant_tables import scaled_quant
    qp, clip_seed = T8_TABLE_CASES[mode][:2]
    return qp, clip_seed, scaled_quant(pkg, qp, np.random.default_rng(53), True, transform8x8_flag=1, cavlc=1)


T8_DECISION = ("transform8x8_flag", "best_mode", "b8mode", "cbp8ts")


def assert_t8_tables_bite(pkg, mode):
    """On the oracle: the decision takes the 8x8 transform for some macroblocks and the 4x4 one for others, and the transposed table -- levelscale
    and leveloffset read at [i][j], which is what the slice parameters carry of the quantiser -- changes it for at least one macroblock; where
    T8_TABLE_CASES says so, each of the two transposed alone does as well."""
    from tests.quant_tables import is_asymmetric, mutated
    qp, clip_seed, q8 = t8_table_case(pkg, mode)
    assert is_asymmetric(q8["levelscale"], 8) and is_asymmetric(q8["leveloffset"], 8)
    want = oracle_slices(mode, q8, qp, seed=clip_seed)
    flag = want["transform8x8_flag"]
    assert (flag == 1).any() and (flag == 0).any()
    one = lambda how, q: mutated(np.array([q], dtype=pkg.QUANT_DTYPE), [0], how)[0]
    variants = {"levelscale^T and leveloffset^T": one("leveloffset^T", one("levelscale^T", q8))}
    if T8_TABLE_CASES[mode][2]:
        variants.update({how: one(how, q8) for how in ("levelscale^T", "leveloffset^T")})
    for how, swapped in variants.items():
        other = oracle_slices(mode, swapped, qp, seed=clip_seed)
        changed = np.zeros(len(want), bool)
        for f in T8_DECISION:
            changed |= (other[f] != want[f]).reshape(len(want), -1).any(axis=1)
        assert changed.any(), "SearchMode %d: %s changes no macroblock's decision" % (mode, how)


@pytest.mark.parametrize("mode", [-1, 0, 1, 3])
def test_tables_are_asymmetric_where_it_matters(pkg, mode):
    """No GPU: the input condition of test_transform_decision_on_asymmetric_tables, on the oracle alone."""
    assert_t8_tables_bite(pkg, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [-1, 0, 1, 3])
def test_transform_decision_on_asymmetric_tables(pkg, mode):
    """Transform8x8Mode 1 with an inter 8x8 luma quantiser whose scaling matrix and rounding offsets depend on (j, i) and are not symmetric:
    the coded-block pattern of the 8x8-transform P8x8 pass (dct_8x8's quantisation in the search kernel) and with it the decision, per search
    mode, against the oracle."""
    assert_t8_tables_bite(pkg, mode)
    qp, clip_seed, q8 = t8_table_case(pkg, mode)
    run_synthetic(pkg, mode, T8_TABLE_W, T8_TABLE_H, T8_TABLE_R, T8_TABLE_NREF, t8=1, qp=qp, q8=q8, seed=clip_seed)
