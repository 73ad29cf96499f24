"""Reference slots above 0: every search kernel, the frame stage and the lazily patched pointer table on job lists whose macroblocks draw
`ref` from {0, 1, 3} of a four-slot context and `ref_is_0` independently of it, device against oracle, bit-exact on (mv_int, cost_int, mv,
cost) of all 41 partitions (frame stage: reconstruction, cbp, cbp_blk, prediction picture).

The three slots hold the same scene under three translations; in a third of the macroblocks every slot is the current picture plus its own
small noise, so the zero vector wins there and the zero-vector bonuses (check_for_00, me_fullsearch.c:75; check_position0, :361) decide.
Slot 2 is never uploaded. Macroblock (0, 0) -- the one place where JM's early-exit bound wraps (me_fullsearch.c:129-138) -- is on slot 3
with ref_is_0 = 1 in some cases and on slot 0 with ref_is_0 = 0 in others.

Without a GPU: on the oracle alone, a search that read slot 0 for every job, exchanged slots 1 and 3, inverted ref_is_0 or exchanged the
weights of two slots changes a compared output in every macroblock concerned, so such a device cannot agree with the expected values."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import oracle
from tests.conftest import load_pkg
from tests.test_me import lambda_factors, make_mbs

load_pkg()                                             # make_mbs imports the binding's record layouts
SLOTS = (0, 1, 3)
MAX_REFS = 4
FIELDS = ("mv_int", "cost_int", "mv", "cost")
FULL, FASTFULL = -1, 0
ALL_PARTS = (1 << 41) - 1
ORIGINS = {"A": (3, 1), "B": (0, 0)}                   # (ref, ref_is_0) of macroblock (0, 0)
CUR_AT = (21, 13)                                      # origin (x, y) of the current picture in the scene
SLOT_AT = {0: (16, 16), 1: (25, 11), 3: (19, 18)}      # ... of each slot's picture: motion (-5, 3), (4, -2), (-2, 5)
QP = 28
# luma (weight, offset) per slot at denominator 5: one above 1, one negative, one whose offset saturates bright samples; [2] is a sentinel
WP_DENOM = 5
WP_LUMA = {0: (48, -9), 1: (-24, 200), 3: (40, 90)}
WP_CR = {0: ((40, 4), (27, -6)), 1: ((-20, 190), (36, 60)), 3: ((25, -11), (44, 70))}
WP_SENTINEL = (127, -128)


def case(size=(64, 48), R=8, mode=FULL, rdopt=1, one_pred=False, spread=8, origin="A", far=False, mixed=False, is_b=0, subpel=1, t8=0,
         wp=False, metric=None, chroma_me=0, fmt=0, seed=1):
    return dict(size=size, R=R, mode=mode, rdopt=rdopt, one_pred=one_pred, spread=spread, origin=origin, far=far, mixed=mixed, is_b=is_b,
                subpel=subpel, t8=t8, wp=wp, metric=metric, chroma_me=chroma_me, fmt=fmt, seed=seed)


BIG = dict(size=(96, 64), R=32, one_pred=True)
CASES = {
    # me_int_kernel (2R+1 < 32): the union window of 41 centres, two macroblocks with predictors far outside the picture
    "union_full_rd0": case(rdopt=0, far=True, seed=2),
    "union_full_rd1": case(rdopt=1, far=True, origin="B", seed=3),
    "union_fastfull_rd0": case(mode=FASTFULL, rdopt=0, origin="B", seed=4),
    # 2R+1 = 65, one predictor per macroblock: me_int_pair_kernel (one-predictor body), JMHIP_ME_KERNEL=single / pers
    "one_full_rd0": case(rdopt=0, seed=5, **BIG),
    "one_full_rd0_B": case(rdopt=0, origin="B", seed=6, **BIG),
    "one_full_rd1": case(rdopt=1, origin="B", seed=7, **BIG),
    "one_fastfull_rd0": case(mode=FASTFULL, rdopt=0, origin="B", seed=8, **BIG),
    "one_fastfull_rd1": case(mode=FASTFULL, rdopt=1, seed=9, **BIG),
    # every other macroblock with 41 predictors (several centres: the table body), the rest with one
    "mixed_rd0": case(size=(96, 64), R=32, rdopt=0, mixed=True, seed=10),
    "mixed_rd1": case(size=(96, 64), R=32, rdopt=1, mixed=True, origin="B", seed=11),
    "b_slice": case(rdopt=0, is_b=1, seed=12, **BIG),
    # (rdopt on: without the refinement the flag reaches macroblock (0, 0) alone, too little for the input condition on rdopt-0 cases)
    "integer_only": case(rdopt=1, subpel=0, seed=13, **BIG),
    "integer_only_union": case(rdopt=1, subpel=0, origin="B", seed=14),
    # UseWeightedReferenceME with one (weight, offset) per slot
    "wp_union": case(rdopt=1, wp=True, seed=15),
    "wp_one_full_rd0": case(rdopt=0, wp=True, seed=16, **BIG),
    "wp_tables_fastfull_t8": case(size=(96, 64), R=32, mode=FASTFULL, rdopt=1, t8=1, wp=True, origin="B", seed=17),
    # me_metric.hip on a 4:2:0 context
    "metric_022_c2": case(metric=(0, 2, 2), chroma_me=2, fmt=1, seed=18),
    "metric_111_c1": case(mode=FASTFULL, metric=(1, 1, 1), chroma_me=1, fmt=1, origin="B", seed=19),
    "metric_wp": case(metric=(0, 0, 2), chroma_me=2, fmt=1, wp=True, seed=20),
    "metric_rd0": case(rdopt=0, metric=(1, 2, 2), chroma_me=2, fmt=1, seed=21),
    # the search in front of the frame stage
    "frame": case(fmt=1, spread=6, seed=22),
}
WEIGHTED = sorted(k for k, c in CASES.items() if c["wp"])


def frozen(a):
    a.flags.writeable = False
    return a


def chroma_of(Y, sign):
    """a 4:2:0 chroma plane that follows the luma picture (tests/test_frame.py::synth)"""
    return np.clip(np.round(128 + sign * 0.25 * (Y[::2, ::2].astype(float) - 128)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pictures(w, h, fmt, seed, wp=False):
    """-> (cur, {slot: ref}), each a tuple of planes (Y alone when fmt = 0), and the macroblocks in which every slot is cur + noise -- wp: in
    which the slot's picture, once weighted with WP_LUMA[slot], is cur + noise (as far as the sample range allows)"""
    rng = np.random.default_rng(1000 + seed)
    mbw, n = w // 16, (w // 16) * (h // 16)
    yy, xx = np.mgrid[0:h + 32, 0:w + 32]
    scene = ((np.sin(xx / 6.0) * np.cos(yy / 9.0)) * 70 + 128 + rng.normal(0, 12, (h + 32, w + 32))).clip(0, 255)
    cut = lambda at: scene[at[1]:at[1] + h, at[0]:at[0] + w]
    curY = (cut(CUR_AT) + rng.normal(0, 2, (h, w))).clip(0, 255).astype(np.uint8)
    still = np.zeros(n, bool)
    still[0] = True
    still[rng.permutation(np.arange(1, n))[:n // 3 - 1]] = True
    refs = {}
    for s in SLOTS:
        Y = cut(SLOT_AT[s]).astype(np.uint8)
        for i in np.nonzero(still)[0]:
            x, y = 16 * (i % mbw), 16 * (i // mbw)
            blk = curY[y:y + 16, x:x + 16].astype(int) + rng.integers(-2, 3, (16, 16))
            if wp:
                blk = np.round((blk - WP_LUMA[s][1]) * float(1 << WP_DENOM) / WP_LUMA[s][0])
            Y[y:y + 16, x:x + 16] = blk.clip(0, 255)
        refs[s] = (frozen(Y),) if fmt == 0 else (frozen(Y), frozen(chroma_of(Y, 1)), frozen(chroma_of(Y, -1)))
    cur = (frozen(curY),) if fmt == 0 else (frozen(curY), frozen(chroma_of(curY, 1)), frozen(chroma_of(curY, -1)))
    return cur, refs, frozen(still)


@functools.lru_cache(maxsize=None)
def refpics(w, h, fmt, seed, wp=False):
    """[rp0, rp1, None, rp3]: what the device's four slots hold"""
    _, refs, _ = pictures(w, h, fmt, seed, wp)
    return [oracle.RefPic(*refs[s], yuv_format=fmt) if s in SLOTS else None for s in range(MAX_REFS)]


def inputs(name):
    c = CASES[name]
    return pictures(c["size"][0], c["size"][1], c["fmt"], c["seed"], c["wp"])


def slot_pics(name):
    c = CASES[name]
    return refpics(c["size"][0], c["size"][1], c["fmt"], c["seed"], c["wp"])


@functools.lru_cache(maxsize=None)
def jobs(name):
    """make_mbs, then: the six (ref, ref_is_0) pairs dealt over the macroblocks, macroblock (0, 0) as the case says, an all-zero predictor in
    four macroblocks out of ten (every `still` one among them, so that the zero vector is both the best match and free)"""
    c = CASES[name]
    rng = np.random.default_rng(2000 + c["seed"])
    mbw, mbh = c["size"][0] // 16, c["size"][1] // 16
    mbs = make_mbs(None, rng, mbw, mbh, c["spread"], per_partition=not c["one_pred"])
    n = len(mbs)
    pairs = [(s, f) for s in SLOTS for f in (0, 1)]
    for k, i in enumerate(rng.permutation(n)):
        mbs[i]["ref"], mbs[i]["ref_is_0"] = pairs[k % len(pairs)]
    mbs[0]["ref"], mbs[0]["ref_is_0"] = ORIGINS[c["origin"]]
    if c["mixed"]:
        mbs["pred_mv"][::2] = mbs["pred_mv"][::2, :1]
    if c["far"]:                                       # two windows that leave the picture and its padding ring (rdopt 0 clips the centre to +-R)
        for i, (fx, fy) in ((n - 1, (300, 260)), (mbw + 1, (-340, -280))):
            mbs[i]["pred_mv"] = mbs[i]["pred_mv"] + np.array([fx, fy], np.int16)
    zero = inputs(name)[2] | (rng.random(n) < 0.15)
    if c["far"]:
        zero[[n - 1, mbw + 1]] = False
    mbs["pred_mv"][zero] = 0
    return frozen(mbs)


def weights_of(name, swap=None, chroma_only=False):
    """None, or {"luma": {slot: (w, o)}, "cr": {slot: ((w, o), (w, o))}} -- with the entries of the two slots `swap` exchanged"""
    if not CASES[name]["wp"]:
        return None
    wts = {"luma": dict(WP_LUMA), "cr": dict(WP_CR)}
    if swap:
        a, b = swap
        for key in ("cr",) if chroma_only else ("luma", "cr"):
            wts[key][a], wts[key][b] = wts[key][b], wts[key][a]
    return wts


def oracle_params(c, wts, slot):
    p = oracle.me_params(rdopt=c["rdopt"], is_b_slice=c["is_b"], transform8x8_mode=c["t8"], metric=c["metric"] or (0, 2, 2),
                         chroma_me=c["chroma_me"], chroma_me_weight=1)
    if wts:
        p.apply_weights = 1
        p.weight_luma, p.offset_luma = wts["luma"][slot]
        p.luma_log_weight_denom = p.chroma_log_weight_denom = WP_DENOM
        p.wp_luma_round = p.wp_chroma_round = 1 << (WP_DENOM - 1)
        for k in range(2):
            p.weight_cr[k], p.offset_cr[k] = wts["cr"][slot][k]
    return p


def run_oracle(name, mbs, wts, subpel=None):
    """oracle.me_frame on the four slots; weighted: once per slot on that slot's jobs with that slot's weights, scattered back"""
    c = CASES[name]
    cur = inputs(name)[0]
    rps, lam = slot_pics(name), lambda_factors(QP)
    kw = dict(subpel=bool(c["subpel"] if subpel is None else subpel), cur_uv=cur[1:] if c["chroma_me"] else None)
    if not wts:
        return oracle.me_frame(oracle_params(c, None, 0), rps, cur[0], mbs, c["mode"], c["R"], lam, **kw)
    n = len(mbs)
    out = {"mv": np.zeros((n, 41, 2), np.int16), "cost": np.zeros((n, 41), np.int32), "mv_int": np.zeros((n, 41, 2), np.int16), "cost_int": np.zeros((n, 41), np.int32)}
    for s in sorted(set(int(r) for r in mbs["ref"])):
        idx = np.nonzero(mbs["ref"] == s)[0]
        part = oracle.me_frame(oracle_params(c, wts, s), rps, cur[0], mbs[idx], c["mode"], c["R"], lam, **kw)
        for key in FIELDS:
            out[key][idx] = part[key]
    return out


MUTATIONS = ("slot->0", "1<->3", "flip", "tied")


def mutated_jobs(mbs, how):
    """The ways of getting the slot or the flag wrong: every job from slot 0; slots 1 and 3 exchanged; ref_is_0 inverted; ref_is_0 = (ref == 0)"""
    out = mbs.copy()
    if how == "slot->0":
        out["ref"] = 0
    elif how == "1<->3":
        out["ref"] = np.where(mbs["ref"] == 1, 3, np.where(mbs["ref"] == 3, 1, mbs["ref"]))
    elif how == "flip":
        out["ref_is_0"] = 1 - mbs["ref_is_0"]
    elif how == "tied":
        out["ref_is_0"] = mbs["ref"] == 0
    return out


@functools.lru_cache(maxsize=None)
def expected(name, how=None, swap=None, chroma_only=False):
    mbs = jobs(name) if how is None else mutated_jobs(jobs(name), how)
    return {k: frozen(v) for k, v in run_oracle(name, mbs, weights_of(name, swap, chroma_only)).items()}


def changed_mbs(a, b, fields=FIELDS, parts=slice(None)):
    """per macroblock: does any of `fields` differ in the partitions `parts`"""
    n = len(a["cost"])
    return np.array([any(not np.array_equal(a[f][i][parts], b[f][i][parts]) for f in fields) for i in range(n)])


# ------------------------------------------------------------------ without a GPU: do the inputs let a mistake show?

@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_tell_the_slots_apart(name):
    mbs, c = jobs(name), CASES[name]
    assert (int(mbs[0]["ref"]), int(mbs[0]["ref_is_0"])) == ORIGINS[c["origin"]] and not mbs[0]["pred_mv"].any()
    seen = {(int(m["ref"]) == 0, int(m["ref_is_0"])) for m in mbs}
    assert seen == {(True, 0), (True, 1), (False, 0), (False, 1)} and set(int(r) for r in mbs["ref"]) == set(SLOTS)
    assert (mbs["pred_mv"].reshape(len(mbs), -1) == 0).all(axis=1).sum() >= 3
    true = expected(name)
    moved = changed_mbs(true, expected(name, "slot->0"))
    assert moved[mbs["ref"] != 0].all() and not moved[mbs["ref"] == 0].any()
    moved = changed_mbs(true, expected(name, "1<->3"))
    assert moved[mbs["ref"] != 0].all() and not moved[mbs["ref"] == 0].any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_tell_ref_is_0_apart(name):
    """rdopt off in a P slice: inverting ref_is_0 moves the 16x16 result of at least three macroblocks -- in FullSearch one of them in cost_int
    with mv_int = (0, 0) (check_for_00: the run that has the flag set takes the bonus at macroblock (0, 0)), and with sub-pel refinement one in
    cost with mv = (0, 0) (check_position0). The other partitions, rdopt on and B slices: nothing moves. A flag tied to ref == 0 shows as well."""
    mbs, c = jobs(name), CASES[name]
    true, flipped, tied = expected(name), expected(name, "flip"), expected(name, "tied")
    if c["rdopt"] or c["is_b"]:
        assert not changed_mbs(true, flipped).any() and not changed_mbs(true, tied).any()
        return
    assert not changed_mbs(true, flipped, parts=slice(1, None)).any()
    moved = changed_mbs(true, flipped, parts=slice(0, 1))
    assert moved.sum() >= 3
    with_flag = lambda i: true if mbs[i]["ref_is_0"] else flipped
    if c["mode"] == FULL:
        assert any(true["cost_int"][i, 0] != flipped["cost_int"][i, 0] and not with_flag(i)["mv_int"][i, 0].any() for i in np.nonzero(moved)[0])
        assert true["cost_int"][0, 0] != flipped["cost_int"][0, 0]
    if c["subpel"]:
        hits = [i for i in np.nonzero(moved)[0] if true["cost"][i, 0] != flipped["cost"][i, 0] and not true["mv"][i, 0].any() and not flipped["mv"][i, 0].any()]
        assert hits and any(true["cost_int"][i, 0] == flipped["cost_int"][i, 0] for i in hits)
    assert changed_mbs(true, tied, parts=slice(0, 1)).any()


@pytest.mark.parametrize("name", WEIGHTED)
def test_inputs_tell_the_weights_apart(name):
    mbs = jobs(name)
    true = expected(name)
    for a, b in ((0, 1), (1, 3), (0, 3)):
        on = (mbs["ref"] == a) | (mbs["ref"] == b)
        moved = changed_mbs(true, expected(name, swap=(a, b)))
        assert moved[on].all() and not moved[~on].any(), (a, b)
        if CASES[name]["chroma_me"]:                   # wp_weight_cr / wp_offset_cr alone
            moved = changed_mbs(true, expected(name, swap=(a, b), chroma_only=True))
            assert moved[on].all() and not moved[~on].any(), (a, b, "chroma")


# ------------------------------------------------------------------ device side

def open_context(pkg, name, luma=SLOTS, chroma=SLOTS, R=None):
    c = CASES[name]
    cur, refs, _ = inputs(name)
    ctx = pkg.Context(c["size"][0], c["size"][1], yuv_format=c["fmt"], max_refs=MAX_REFS, search_range=R or c["R"])
    for s in SLOTS:
        ctx.ref_upload(s, *refs[s])
        if s in luma:
            ctx.interp_luma(s)
        if c["fmt"] and s in chroma:
            ctx.interp_chroma(s)
    ctx.cur_upload(*cur)
    return ctx


def me_params(pkg, name, **over):
    c = dict(CASES[name], **over)
    prm = pkg.MeParams()
    prm.search_mode, prm.search_range, prm.rdopt, prm.is_b_slice = c["mode"], c["R"], c["rdopt"], c["is_b"]
    prm.level_mv_min, prm.level_mv_max = -511, 511
    prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lambda_factors(QP)
    prm.transform8x8_mode, prm.subpel, prm.partition_mask = c["t8"], c["subpel"], ALL_PARTS
    if c["metric"]:
        prm.metric_set = 1
        prm.metric[0], prm.metric[1], prm.metric[2] = c["metric"]
        prm.chroma_me, prm.chroma_me_weight = c["chroma_me"], 1
    if c["wp"]:
        prm.wp_enable, prm.wp_denom, prm.wp_round = 1, WP_DENOM, 1 << (WP_DENOM - 1)
        prm.wp_chroma_denom, prm.wp_chroma_round = WP_DENOM, 1 << (WP_DENOM - 1)
        prm.wp_weight[2], prm.wp_offset[2] = WP_SENTINEL
        for k in range(2):
            prm.wp_weight_cr[2][k], prm.wp_offset_cr[2][k] = WP_SENTINEL
        for s in SLOTS:
            prm.wp_weight[s], prm.wp_offset[s] = WP_LUMA[s]
            for k in range(2):
                prm.wp_weight_cr[s][k], prm.wp_offset_cr[s][k] = WP_CR[s][k]
    return prm


def assert_me_equal(got, want, mbs, where):
    for key in FIELDS:
        if not np.array_equal(got[key], want[key]):
            i, q = np.argwhere((got[key] != want[key]).reshape(len(mbs), 41, -1).any(axis=2))[0]
            raise AssertionError("%s: %s differs at mb %d (slot %d, ref_is_0 %d) partition %d: device %s oracle %s" % (
                where, key, i, mbs[i]["ref"], mbs[i]["ref_is_0"], q, got[key][i, q], want[key][i, q]))


def device_me(pkg, name, monkeypatch=None, kernel=None, grid=None, luma=SLOTS, resident=False):
    if kernel:
        monkeypatch.setenv("JMHIP_ME_KERNEL", kernel)
    if grid:
        monkeypatch.setenv("JMHIP_ME_PERS_GRID", str(grid))
    ctx = open_context(pkg, name, luma=luma)
    try:
        prm, mbs = me_params(pkg, name), jobs(name)
        got = ctx.me_frame(prm, mbs)
        assert_me_equal(got, expected(name), mbs, name)
        if resident:                                   # the job array that stayed on the device: slots and flags are read from it again
            ctx.me_frame_async(prm, None, len(mbs))
            assert_me_equal(ctx.me_results(len(mbs)), expected(name), mbs, name + " (resident)")
    finally:
        ctx.close()


# Which integer kernel a parameter set launches (jmhip_me_frame_async, me_int.hip): a macroblock is a "fast" item when every partition is searched and
# 2R+1 >= 32 (64 under JMHIP_ME_KERNEL=single); fast items go to me_int_pair_kernel, or me_int_fast_kernel (single), or me_int_pers_kernel (pers,
# unweighted, every used slot interpolated); everything else -- here all of R = 8 -- to me_int_kernel.
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["union_full_rd0", "union_full_rd1", "union_fastfull_rd0", "one_full_rd0", "one_full_rd0_B", "one_full_rd1",
                                  "one_fastfull_rd0", "one_fastfull_rd1", "b_slice"])
def test_me_frame_mixed_slots_default_kernels(pkg, name):
    device_me(pkg, name)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,grid", [("single", None), ("pers", None), ("pers", 8)])
@pytest.mark.parametrize("name", ["one_full_rd0", "one_full_rd0_B", "one_full_rd1", "one_fastfull_rd0", "one_fastfull_rd1"])
def test_me_frame_mixed_slots_selectable_kernels(pkg, name, kernel, grid, monkeypatch):
    """grid 8: 24 one-predictor items on 8 workgroups -- each walks three items of different slots and flags back to back, staging the
    next one's window (from its slot) while it finishes the last one (ref and ref_is_0 packed into one word per item)."""
    device_me(pkg, name, monkeypatch, kernel, grid)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed_rd0", "mixed_rd1"])
def test_me_frame_mixed_slots_both_item_bodies_and_resident_rerun(pkg, name):
    device_me(pkg, name, resident=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["integer_only", "integer_only_union"])
def test_integer_search_from_a_slot_without_sub_pel_planes(pkg, name):
    """subpel = 0 needs the uploaded picture alone: slot 3 has had no jmhip_interp_luma"""
    device_me(pkg, name, luma=(0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wp_union", "wp_one_full_rd0", "wp_tables_fastfull_t8"])
def test_weighted_reference_search_per_slot(pkg, name):
    """wp_weight[ref] / wp_offset[ref]: a negative weight on slot 1, an offset that saturates on slot 3, a sentinel in the unused [2]; at
    macroblock (0, 0) of the rdopt-0 case the wrapped bound's one row is weighted with slot 3's pair."""
    device_me(pkg, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["metric_022_c2", "metric_111_c1", "metric_wp", "metric_rd0"])
def test_metric_kernel_mixed_slots(pkg, name):
    """me_metric.hip: chroma planes and wp_weight_cr[slot][uv] / wp_offset_cr[slot][uv] by slot; rdopt 0: its own copies of check_for_00, the
    wrapped bound and check_position0"""
    device_me(pkg, name)


# ------------------------------------------------------------------ jmhip_me_subpel alone

SUBPEL_CASE = "union_full_rd0"


@functools.lru_cache(maxsize=None)
def subpel_vectors():
    """arbitrary integer vectors; (0, 0) on the 16x16 block of every other macroblock"""
    mbs = jobs(SUBPEL_CASE)
    mv_int = np.random.default_rng(31).integers(-14, 15, (len(mbs), 41, 2)).astype(np.int16)
    mv_int[::2, 0] = 0
    return frozen(mv_int)


@functools.lru_cache(maxsize=None)
def subpel_expected(rdopt, how=None):
    """jmo_subpel_search per block as tests/test_dist.py::test_me_subpel_alone calls it, on the job's slot and with the job's flag"""
    c = dict(CASES[SUBPEL_CASE], rdopt=rdopt)
    mbs = jobs(SUBPEL_CASE) if how is None else mutated_jobs(jobs(SUBPEL_CASE), how)
    mv_int, rps = subpel_vectors(), slot_pics(SUBPEL_CASE)
    L = oracle._setup_search_protos()
    p = oracle_params(c, None, 0)
    cur16 = inputs(SUBPEL_CASE)[0][0].astype(np.uint16)
    lam_a = (C.c_int * 3)(*lambda_factors(QP))
    out = {"mv": np.zeros((len(mbs), 41, 2), np.int16), "cost": np.zeros((len(mbs), 41), np.int32)}
    for i, mb in enumerate(mbs):
        ox, oy = int(mb["mb_x"]) * 16, int(mb["mb_y"]) * 16
        for q, (bt, x4, y4, w4, h4) in enumerate(oracle.PARTS):
            px, py, bsx, bsy = ox + 4 * x4, oy + 4 * y4, 4 * w4, 4 * h4
            orig = np.zeros(768, np.uint16)
            orig[: bsx * bsy] = cur16[py:py + bsy, px:px + bsx].reshape(-1)
            mvq = (mv_int[i, q] * 4).copy()
            out["cost"][i, q] = L.jmo_subpel_search(C.byref(p), C.byref(rps[int(mb["ref"])].ref), orig.ctypes.data, int(mb["ref_is_0"]), px, py, bt,
                                                    int(mb["pred_mv"][q][0]), int(mb["pred_mv"][q][1]), mvq.ctypes.data, mvq[1:].ctypes.data, 9, 9, 2147483647, lam_a)
            out["mv"][i, q] = mvq
    return {k: frozen(v) for k, v in out.items()}


@pytest.mark.parametrize("rdopt", [0, 1])
def test_subpel_inputs_tell_slots_and_flag_apart(rdopt):
    mbs, true = jobs(SUBPEL_CASE), subpel_expected(rdopt)
    for how in ("slot->0", "1<->3"):
        moved = changed_mbs(true, subpel_expected(rdopt, how), ("mv", "cost"))
        assert moved[mbs["ref"] != 0].all() and not moved[mbs["ref"] == 0].any(), how
    moved = changed_mbs(true, subpel_expected(rdopt, "flip"), ("mv", "cost"))
    if rdopt:
        assert not moved.any()
    else:                                              # check_position0 where the 16x16 block starts from (0, 0), nowhere else
        assert moved.sum() >= 3 and not moved[1::2].any()
        assert not changed_mbs(true, subpel_expected(rdopt, "flip"), ("mv", "cost"), slice(1, None)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("rdopt", [0, 1])
def test_me_subpel_alone_mixed_slots(pkg, rdopt):
    mbs = jobs(SUBPEL_CASE)
    ctx = open_context(pkg, SUBPEL_CASE)
    try:
        res = np.zeros(len(mbs), dtype=pkg.ME_RESULT_DTYPE)
        res["mv_int"] = subpel_vectors()
        got = ctx.me_subpel(me_params(pkg, SUBPEL_CASE, rdopt=rdopt), mbs, res)
    finally:
        ctx.close()
    want = subpel_expected(rdopt)
    for key in ("mv", "cost"):
        assert np.array_equal(got[key], want[key]), (key, np.argwhere((got[key] != want[key]).reshape(len(mbs), 41, -1).any(axis=2))[0])


# ------------------------------------------------------------------ frame stage after a mixed-slot search

FRAME_WP = {"luma_round": 16, "luma_denom": 5, "chroma_round": 4, "chroma_denom": 3}
FRAME_WEIGHTS = {0: ((30, 9, 7), (3, -2, 1)), 1: ((36, 6, 10), (-5, 4, -3)), 3: ((27, 11, 5), (8, -6, 2))}      # slot: (weight, offset) of Y, Cb, Cr


def frame_wp(swap=None):
    wp = dict(FRAME_WP, weight=np.full((16, 3), 127, int), offset=np.full((16, 3), -100, int))      # unused slots: sentinels
    table = dict(FRAME_WEIGHTS)
    if swap:
        table[swap[0]], table[swap[1]] = table[swap[1]], table[swap[0]]
    for s, (w, o) in table.items():
        wp["weight"][s], wp["offset"][s] = w, o
    return wp


def frame_quants(pkg):
    return np.array([pkg.flat_quant(QP + d, 342, adaptive_rounding=1, adapt_rnd_weight=4, cavlc=1) for d in (0, 0, 3)], dtype=pkg.QUANT_DTYPE)


@functools.lru_cache(maxsize=None)
def frame_expected(weighted, how=None, swap=None):
    """oracle.residual_frame on the oracle's own vectors and mode choice, each 8x8 block from its macroblock's slot"""
    pkg = load_pkg()
    mbs, me = jobs("frame"), expected("frame")
    if how:
        mbs = mutated_jobs(mbs, how)
    modes = oracle.pick_modes(me["cost"])
    return oracle.residual_frame(slot_pics("frame"), inputs("frame")[0], mbs, me["mv"], modes, frame_quants(pkg), pkg.TQ_JOB_DTYPE, yuv_format=1,
                                 blk_ref=np.repeat(mbs["ref"][:, None], 4, axis=1), wp=frame_wp(swap) if weighted else None), modes


def recon_changed(a, b, mbs):
    """per macroblock: does the reconstruction differ"""
    out = []
    for mb in mbs:
        x, y = 16 * int(mb["mb_x"]), 16 * int(mb["mb_y"])
        out.append(any(not np.array_equal(p[y // d:y // d + 16 // d, x // d:x // d + 16 // d], q[y // d:y // d + 16 // d, x // d:x // d + 16 // d])
                       for p, q, d in zip(a["recon"], b["recon"], (1, 2, 2))))
    return np.array(out)


@pytest.mark.parametrize("weighted", [False, True])
def test_frame_inputs_tell_slots_and_weights_apart(weighted):
    mbs = jobs("frame")
    true = frame_expected(weighted)[0]
    assert (true["cbp"] != 0).any()
    for how in ("slot->0", "1<->3"):
        moved = recon_changed(true, frame_expected(weighted, how)[0], mbs)
        assert moved[mbs["ref"] != 0].all() and not moved[mbs["ref"] == 0].any(), how
    if weighted:
        for a, b in ((0, 1), (1, 3), (0, 3)):
            on = (mbs["ref"] == a) | (mbs["ref"] == b)
            moved = recon_changed(true, frame_expected(True, swap=(a, b))[0], mbs)
            assert moved[on].all() and not moved[~on].any(), (a, b)


def assert_frame_equal(pkg, ctx, want, modes, n, pred=True):
    got = ctx.residual_download(n)
    assert np.array_equal(got["modes"]["mode"], modes["mode"]) and np.array_equal(got["modes"]["b8mode"], modes["b8mode"])
    assert np.array_equal(got["cbp"], want["cbp"]) and np.array_equal(got["cbp_blk"], want["cbp_blk"])
    for g, wv, plane in zip(ctx.recon_download(), want["recon"], "YUV"):
        assert np.array_equal(g, wv), "reconstruction %s" % plane
    if pred:
        P = ctx.pred_download()
        for i, mb in enumerate(jobs("frame")):
            x, y = 16 * int(mb["mb_x"]), 16 * int(mb["mb_y"])
            assert np.array_equal(P[0][y:y + 16, x:x + 16], want["jobs_y"][i]["pred"]), "luma prediction of macroblock %d" % i
            for uv in range(2):
                assert np.array_equal(P[1 + uv][y // 2:y // 2 + 8, x // 2:x // 2 + 8], want["jobs_c"][2 * i + uv]["pred"][:8, :8]), "chroma prediction of macroblock %d" % i


@pytest.mark.gpu
@pytest.mark.parametrize("planes,fused,weighted", [(True, True, False), (False, True, False), (True, False, False), (False, False, True), (True, True, True)])
def test_frame_stage_after_a_mixed_slot_search(pkg, planes, fused, weighted, monkeypatch):
    """s_ref[] = mb.ref: prediction from each macroblock's slot -- eighth-pel chroma planes of every slot or computed on the fly, fused kernel
    and separate kernels, jmhip_frame_wp weight[slot][component]"""
    if not fused:
        monkeypatch.setenv("JMHIP_FRAME_FUSED", "0")
    mbs = jobs("frame")
    want, modes = frame_expected(weighted)
    ctx = open_context(pkg, "frame", chroma=SLOTS if planes else ())
    try:
        assert_me_equal(ctx.me_frame(me_params(pkg, "frame"), mbs), expected("frame"), mbs, "frame")
        ctx.frame_wp_set(frame_wp() if weighted else None)
        if fused:
            ctx.frame_keep_prediction()
        ctx.residual_frame(frame_quants(pkg), None)
        assert_frame_equal(pkg, ctx, want, modes, len(mbs), pred=fused)
    finally:
        ctx.close()


# ------------------------------------------------------------------ a reconstruction that becomes slot 1 and is searched from

def two_slot_jobs(name, slots):
    mbs = jobs(name).copy()
    mbs["ref"] = np.where(mbs["ref"] == 3, slots[-1], np.where(mbs["ref"] == 1, slots[len(slots) // 2], slots[0]))
    return mbs


@pytest.mark.gpu
@pytest.mark.parametrize("flush_by_search", [False, True])
def test_search_from_a_reconstruction_that_became_slot_1(pkg, flush_by_search):
    """jmhip_recon_to_ref(1) trades planes and leaves ONE pending entry of the device's pointer table. Either the next jmhip_interp_luma launch
    carries it along, or -- flush_by_search: an integer-only search of slot-1 jobs comes first -- jm_ensure_ref_table writes it. Expected: the
    oracle on [slot 0's picture, the reconstruction of picture 1 as downloaded before the swap]."""
    name = "frame"
    cur, refs, _ = inputs(name)
    mbs = two_slot_jobs(name, (0, 1))
    ctx = pkg.Context(64, 48, yuv_format=1, max_refs=MAX_REFS, search_range=8)
    try:
        for s in (0, 1):
            ctx.ref_upload(s, *refs[s])
            ctx.interp_luma(s)
            ctx.interp_chroma(s)
        ctx.cur_upload(*cur)
        # picture 1: searched from both slots (each macroblock from the slot it will NOT name in picture 2, so that the reconstruction differs
        # from the old slot 1 under every slot-1 job, the `still` macroblocks included), reconstructed
        rps = [slot_pics(name)[0], slot_pics(name)[1]]
        lam = lambda_factors(QP)
        mbs1 = two_slot_jobs(name, (1, 0))
        assert_me_equal(ctx.me_frame(me_params(pkg, name), mbs1), oracle.me_frame(oracle_params(CASES[name], None, 0), rps, cur[0], mbs1, FULL, 8, lam), mbs1, "picture 1")
        ctx.residual_frame(frame_quants(pkg), None)
        recon = ctx.recon_download()
        assert not np.array_equal(recon[0], refs[1][0])
        ctx.recon_to_ref(1)
        new = [rps[0], oracle.RefPic(*recon, yuv_format=1)]
        # picture 2: the scene as slot 3 shows it, every macroblock whose job names slot 1 now predicts from picture 1's reconstruction
        cur2 = refs[3]
        ctx.cur_upload(*cur2)
        if flush_by_search:
            on1 = mbs[mbs["ref"] == 1]
            want = oracle.me_frame(oracle_params(CASES[name], None, 0), new, cur2[0], on1, FULL, 8, lam, subpel=False)
            assert_me_equal(ctx.me_frame(me_params(pkg, name, subpel=0), on1), want, on1, "integer search between the swap and the interpolation")
        ctx.interp_luma(1)
        ctx.interp_chroma(1)
        c2 = dict(CASES[name], metric=(0, 2, 2), chroma_me=2)          # the chroma term: the new slot's eighth-pel planes take part
        want = oracle.me_frame(oracle_params(c2, None, 0), new, cur2[0], mbs, FULL, 8, lam, cur_uv=cur2[1:])
        assert changed_mbs(want, oracle.me_frame(oracle_params(c2, None, 0), rps, cur2[0], mbs, FULL, 8, lam, cur_uv=cur2[1:]))[mbs["ref"] == 1].all()
        assert_me_equal(ctx.me_frame(me_params(pkg, name, metric=(0, 2, 2), chroma_me=2), mbs), want, mbs, "picture 2")
    finally:
        ctx.close()


# ------------------------------------------------------------------ refusals

@pytest.mark.gpu
def test_jobs_naming_unusable_slots_are_refused(pkg):
    name = "union_full_rd1"
    mbs = jobs(name)
    ctx = open_context(pkg, name, luma=(0, 1))
    try:
        prm = me_params(pkg, name)
        for slot in (2, MAX_REFS):                     # never uploaded; out of range
            bad = mbs.copy()
            bad[0]["ref"] = slot
            with pytest.raises(pkg.JmhipError, match="reference slot not uploaded"):
                ctx.me_frame(prm, bad)
        with pytest.raises(pkg.JmhipError, match="jmhip_interp_luma"):
            ctx.me_frame(prm, mbs)                     # slot 3: uploaded, not interpolated
        with pytest.raises(pkg.JmhipError):
            ctx.me_frame_async(prm, None, len(mbs))    # a refused upload leaves no resident jobs behind
        ctx.interp_luma(3)
        assert_me_equal(ctx.me_frame(prm, mbs), expected(name), mbs, "after the refusals")
    finally:
        ctx.close()
