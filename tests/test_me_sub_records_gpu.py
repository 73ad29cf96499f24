"""jmhip_me_subpel on CRAFTED integer vectors: the leader records of me_sub_kernel (me_sub.hip) -- which items of a sub-block lead, which
partitions a leader serves, its origin and access method, resolved once per phase -- device against the oracle's SubPelBlockMotionSearch,
bit-exact on mv and cost of all 41 partitions.

Pictures of 64x48 and 48x48: interior macroblocks and all four picture borders. The vector patterns choose how the 112 (8x8 transform: 64)
items group into leaders; the tests without a GPU check on the oracle's side that each pattern does what its name says."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import oracle
from tests.conftest import load_pkg
from tests.test_me import lambda_factors, make_mbs, make_pair
from tests.test_slice_gpu import run_synthetic

PAD = 20                                             # IMG_PAD_SIZE
SIZES = ((64, 48), (48, 48))
FULL = (1 << 41) - 1
BT = np.array([bt for bt, _, _, _, _ in oracle.PARTS])
WP = (48, -9, 5)                                     # weight, offset, denominator
INT_MAX = 2147483647


def one_vector(mbs, mbw, mbh):
    """all 41 partitions of a macroblock on one vector (another per macroblock): 16 leaders with seven members each"""
    v = np.zeros((len(mbs), 41, 2), np.int16)
    for i in range(len(mbs)):
        v[i, :] = (i % 5 - 2, (i * 3) % 7 - 3)
    return v


def all_distinct(mbs, mbw, mbh):
    """every partition on its own vector: 112 leaders (8x8 transform: 64) with one member each"""
    v = np.zeros((len(mbs), 41, 2), np.int16)
    q = np.arange(41)
    for i in range(len(mbs)):
        v[i, :, 0], v[i, :, 1] = (q + i) % 7 - 3, q // 7 - 3
    return v


def by_type(groups):
    """the block types share `groups` vectors: every sub-block carries one item per type, so each of its leaders serves a strict subset"""
    def pattern(mbs, mbw, mbh):
        v = np.zeros((len(mbs), 41, 2), np.int16)
        for i in range(len(mbs)):
            g = np.array(groups)[BT - 1]
            v[i, :, 0], v[i, :, 1] = 2 * g - 2 + i % 2, 1 - g
        return v
    return pattern


def by_partition(n):
    """partition q on vector q % n: the items of one block type differ among themselves as well"""
    def pattern(mbs, mbw, mbh):
        v = np.zeros((len(mbs), 41, 2), np.int16)
        g = np.arange(41) % n
        v[:, :, 0], v[:, :, 1] = 3 * g - 3, g - 1
        return v
    return pattern


def across_the_edge(mbs, mbw, mbh):
    """one vector per macroblock that carries the partitions next to a picture border across the padded edge and leaves the others inside"""
    v = np.zeros((len(mbs), 41, 2), np.int16)
    for i, mb in enumerate(mbs):
        x, y = int(mb["mb_x"]), int(mb["mb_y"])
        v[i, :, 0] = -(PAD + 4) if x == 0 else PAD + 2 if x == mbw - 1 else 1
        v[i, :, 1] = -(PAD + 8) if y == 0 else PAD + 10 if y == mbh - 1 else -1
    return v


PATTERNS = {
    "one_vector": one_vector,
    "all_distinct": all_distinct,
    "two_by_type_head": by_type((0, 0, 0, 1, 1, 1, 1)),          # the second leader's members are the LAST four of its sub-block's items
    "two_by_type_alternating": by_type((0, 1, 0, 1, 0, 1, 0)),
    "three_by_type": by_type((0, 1, 2, 0, 1, 2, 1)),
    "two_by_partition": by_partition(2),
    "three_by_partition": by_partition(3),
    "across_the_edge": across_the_edge,
}
# name -> (pattern, rdopt, transform8x8_mode, weights, partition mask)
CASES = {name: (name, 1, 0, None, FULL) for name in PATTERNS}
CASES.update({
    "one_vector_rdopt0": ("one_vector", 0, 0, None, FULL),
    "one_vector_t8": ("one_vector", 1, 1, None, FULL),
    "all_distinct_t8": ("all_distinct", 1, 1, None, FULL),
    "three_by_type_t8": ("three_by_type", 1, 1, None, FULL),
    "across_the_edge_t8": ("across_the_edge", 1, 1, None, FULL),
    "three_by_partition_wp": ("three_by_partition", 1, 0, WP, FULL),
    "across_the_edge_wp_t8": ("across_the_edge", 1, 1, WP, FULL),
    "one_vector_mask": ("one_vector", 1, 0, None, 0x0AA5A5A5A5A),      # an inactive 16x16 partition: the first item of every sub-block does not lead
    "two_by_type_mask": ("two_by_type_head", 1, 0, None, 0x15555555555),
    "three_by_partition_mask_t8": ("three_by_partition", 1, 1, None, 0x1F0F0F0F0F0),
})


@functools.lru_cache(maxsize=None)
def inputs(size, pattern):
    w, h = size
    load_pkg()                                       # make_mbs takes the job layout from the package
    rng = np.random.default_rng(w + h)
    cur, ref = make_pair(rng, w, h, "shift")
    mbs = make_mbs(None, rng, w // 16, h // 16, 12)
    return cur, ref, mbs, PATTERNS[pattern](mbs, w // 16, h // 16), oracle.RefPic(ref, yuv_format=0)


@functools.lru_cache(maxsize=None)
def want(size, pattern, rdopt, t8, wp, mask, half_pel_only=False):
    """SubPelBlockMotionSearch per partition, as tests/test_dist.py::test_me_subpel_alone calls it"""
    cur, ref, mbs, mv_int, rp = inputs(size, pattern)
    L = oracle._setup_search_protos()
    p = oracle.me_params(rdopt=rdopt, transform8x8_mode=t8)
    if wp:
        p.apply_weights, p.weight_luma, p.offset_luma = 1, wp[0], wp[1]
        p.luma_log_weight_denom, p.wp_luma_round = wp[2], (1 << (wp[2] - 1)) if wp[2] else 0
    cur16 = cur.astype(np.uint16)
    lam_a = (C.c_int * 3)(*lambda_factors(28))
    mv, cost = np.zeros((len(mbs), 41, 2), np.int16), np.zeros((len(mbs), 41), np.int32)
    for i, mb in enumerate(mbs):
        ox, oy = int(mb["mb_x"]) * 16, int(mb["mb_y"]) * 16
        for q, (bt, x4, y4, w4, h4) in enumerate(oracle.PARTS):
            if not (mask >> q) & 1:
                continue
            px, py, bsx, bsy = ox + 4 * x4, oy + 4 * y4, 4 * w4, 4 * h4
            orig = np.zeros(768, np.uint16)
            orig[: bsx * bsy] = cur16[py:py + bsy, px:px + bsx].reshape(-1)
            mvq = (mv_int[i, q].astype(np.int16) * 4).copy()
            cost[i, q] = L.jmo_subpel_search(C.byref(p), C.byref(rp.ref), orig.ctypes.data, 1, px, py, bt, int(mb["pred_mv"][q][0]), int(mb["pred_mv"][q][1]),
                                             mvq.ctypes.data, mvq[1:].ctypes.data, 9, 1 if half_pel_only else 9, INT_MAX, lam_a)
            mv[i, q] = mvq
    return mv, cost


def umv_flags(size, mv4, margin):
    """the access method SubPelBlockMotionSearch picks per partition (me_fullsearch.c:412-413 with margin 1, :468-469 with margin 0)"""
    w, h = size
    mbs = inputs(size, "one_vector")[2]
    out = np.zeros(mv4.shape[:2], bool)
    for i, mb in enumerate(mbs):
        for q, (bt, x4, y4, w4, h4) in enumerate(oracle.PARTS):
            x = ((int(mb["mb_x"]) * 16 + 4 * x4 + PAD) << 2) + int(mv4[i, q, 0])
            y = ((int(mb["mb_y"]) * 16 + 4 * y4 + PAD) << 2) + int(mv4[i, q, 1])
            out[i, q] = not (margin < x < ((w - 4 * w4 + 2 * PAD) << 2) - margin and margin < y < ((h - 4 * h4 + 2 * PAD) << 2) - margin)
    return out


def leaders(mv4, umv, t8, mask=FULL):
    """per macroblock: the number of distinct (sub-block, vector, access method) among the items of the active partitions"""
    out = []
    for i in range(len(mv4)):
        keys = set()
        for q, (bt, x4, y4, w4, h4) in enumerate(oracle.PARTS):
            if not (mask >> q) & 1:
                continue
            bs = 2 if t8 and bt <= 4 else 1
            for y in range(y4, y4 + h4, bs):
                for x in range(x4, x4 + w4, bs):
                    keys.add((x, y, bs, int(mv4[i, q, 0]), int(mv4[i, q, 1]), bool(umv[i, q])))
        out.append(len(keys))
    return out


@pytest.mark.parametrize("size", SIZES)
def test_patterns_group_the_items_as_they_say(size):
    def count(pattern, t8, mask=FULL):
        mv4 = inputs(size, pattern)[3].astype(np.int32) * 4
        return leaders(mv4, umv_flags(size, mv4, 1), t8, mask)
    assert set(count("one_vector", 0)) == {16} and set(count("one_vector", 1)) == {4 + 16}
    assert set(count("all_distinct", 0)) == {112} and set(count("all_distinct", 1)) == {64}
    assert set(count("two_by_type_head", 0)) == {32} and set(count("two_by_type_alternating", 0)) == {32} and set(count("three_by_type", 0)) == {48}
    for pattern in ("two_by_partition", "three_by_partition"):
        assert all(16 < n < 112 for n in count(pattern, 0)), pattern
    # the ragged last trip: no leader count times the 9 half-pel candidates is a multiple of the 128 lanes
    assert all((n * 9) % 128 for pattern in PATTERNS for t8 in (0, 1) for n in count(pattern, t8))
    # an inactive partition leads nothing and is served by nobody: fewer leaders than with every partition on
    assert all(a <= b for a, b in zip(count("two_by_type_head", 0, CASES["two_by_type_mask"][4]), count("two_by_type_head", 0)))


@pytest.mark.parametrize("size", SIZES)
def test_the_edge_pattern_splits_partitions_with_one_vector(size):
    """the same numeric vector on both sides of the edge: the access method alone tells such partitions apart, at every border of the picture"""
    mbs, mv_int = inputs(size, "across_the_edge")[2:4]
    mv4 = mv_int.astype(np.int32) * 4
    umv = umv_flags(size, mv4, 1)
    mbw, mbh = size[0] // 16, size[1] // 16
    n = leaders(mv4, umv, 0)
    for i, mb in enumerate(mbs):
        assert len({tuple(v) for v in mv_int[i]}) == 1
        border = int(mb["mb_x"]) in (0, mbw - 1) or int(mb["mb_y"]) in (0, mbh - 1)
        assert (umv[i].any() and not umv[i].all()) == border, i
        assert (n[i] > 16) == border and n[i] <= 32, (i, n[i])


@pytest.mark.parametrize("size", SIZES)
def test_half_pel_winners_regroup_the_leaders(size):
    """one integer vector per macroblock, but the half-pel winners differ per partition: the quarter-pel phase has other leaders"""
    half = want(size, "one_vector", 1, 0, None, FULL, half_pel_only=True)[0].astype(np.int32)
    n = leaders(half, umv_flags(size, half, 0), 0)
    assert min(n) > 16, n


def device(pkg, size, pattern, rdopt, t8, wp, mask):
    from h264_amd.jmhip import ME_RESULT_DTYPE
    cur, ref, mbs, mv_int, _ = inputs(size, pattern)
    ctx = pkg.Context(size[0], size[1], yuv_format=0, max_refs=1, search_range=8)
    try:
        ctx.ref_upload(0, ref)
        ctx.interp_luma(0)
        ctx.cur_upload(cur)
        prm = pkg.MeParams()
        prm.search_mode, prm.search_range, prm.rdopt, prm.is_b_slice = -1, 8, rdopt, 0
        prm.level_mv_min, prm.level_mv_max = -511, 511
        prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lambda_factors(28)
        prm.transform8x8_mode, prm.subpel, prm.partition_mask = t8, 1, mask
        if wp:
            prm.wp_enable, prm.wp_denom, prm.wp_round = 1, wp[2], (1 << (wp[2] - 1)) if wp[2] else 0
            prm.wp_weight[0], prm.wp_offset[0] = wp[0], wp[1]
        res = np.zeros(len(mbs), dtype=ME_RESULT_DTYPE)
        res["mv_int"] = mv_int
        res["mv"], res["cost"] = -77, -777              # what an inactive partition must keep
        return ctx.me_subpel(prm, mbs, res)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_subpel_on_crafted_vectors(pkg, case, size):
    pattern, rdopt, t8, wp, mask = CASES[case]
    got = device(pkg, size, pattern, rdopt, t8, wp, mask)
    mv, cost = want(size, pattern, rdopt, t8, wp, mask)
    on = np.array([(mask >> q) & 1 for q in range(41)], bool)
    for name, g, w in (("mv", got["mv"], mv), ("cost", got["cost"], cost)):
        bad = np.argwhere(g[:, on] != w[:, on])
        assert not len(bad), "%s differs at macroblock %d, active partition %d: got %s want %s" % (
            name, bad[0][0], bad[0][1], g[:, on][bad[0][0], bad[0][1]], w[:, on][bad[0][0], bad[0][1]])
    assert np.all(got["mv"][:, ~on] == -77) and np.all(got["cost"][:, ~on] == -777), "an inactive partition was written"


@pytest.mark.gpu
def test_list_form_in_a_full_search_slice(pkg):
    """the LIST instantiation has no entry of its own: one P picture searched by FullSearch sweeps (me_xslice.hip: 16 <= range <= 40), every
    macroblock against the oracle's P-slice driver"""
    run_synthetic(pkg, -1, 96, 64, 16, 1, nframes=2)
