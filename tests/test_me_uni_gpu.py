"""The one-predictor body of the pair-lane full search (me_int_pair_kernel, work-word bit 30): macroblocks whose 41 partitions share ONE
predictor take a body that computes both mv-bit counts in place -- the vertical one per candidate row in scalar code, the horizontal one
once per lane -- instead of reading them from per-partition tables. Every case compares (mv_int, cost_int, mv, cost) of all 41 partitions
with the oracle, bit-exact, as tests/test_me.py does; JMHIP_ME_KERNEL=pair_tables sends the same items through the table body."""
import numpy as np
import pytest

from tests import oracle
from tests.test_me import lambda_factors, make_mbs, make_pair, run_case

KEYS = ("mv_int", "cost_int", "mv", "cost")
W, H = 96, 64                                        # 24 macroblocks


def inputs(pkg, kind, spread, seed, per_partition=False):
    rng = np.random.default_rng(seed)
    cur, ref = make_pair(rng, W, H, kind)
    return cur, ref, make_mbs(pkg, rng, W // 16, H // 16, spread, per_partition)


def search(pkg, cur, ref, mbs, mode, R, rdopt, qp=28, is_b=0):
    """run_case's device half with the quantiser as a parameter: the four result arrays of one jmhip_me_frame call."""
    ctx = pkg.Context(W, H, yuv_format=0, max_refs=1, search_range=R)
    ctx.ref_upload(0, ref)
    ctx.interp_luma(0)
    ctx.cur_upload(cur)
    prm = pkg.MeParams()
    prm.search_mode, prm.search_range, prm.rdopt, prm.is_b_slice = mode, R, rdopt, is_b
    prm.level_mv_min, prm.level_mv_max = -511, 511
    prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lambda_factors(qp)
    prm.transform8x8_mode, prm.subpel, prm.partition_mask = 0, 1, (1 << 41) - 1
    got = ctx.me_frame(prm, mbs)
    ctx.close()
    return got


def check(pkg, cur, ref, mbs, mode, R, rdopt, qp=28, is_b=0):
    got = search(pkg, cur, ref, mbs, mode, R, rdopt, qp, is_b)
    want = oracle.me_frame(oracle.me_params(rdopt=rdopt, is_b_slice=is_b), [oracle.RefPic(ref, yuv_format=0)], cur, mbs, mode, R, lambda_factors(qp))
    for key in KEYS:
        g, wv = got[key], want[key]
        if not np.array_equal(g, wv):
            bad = np.argwhere(g != wv)[0]
            raise AssertionError("%s differs at mb %d partition %d: got %s want %s (pred %s)" % (
                key, bad[0], bad[1], g[bad[0], bad[1]], wv[bad[0], bad[1]], mbs[bad[0]]["pred_mv"][bad[1]]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [-1, 0])
@pytest.mark.parametrize("R", [16, 32, 40])
def test_uni_ranges(pkg, R, mode):
    """R = 16: 33 columns -- one column group, four row bands, one rest column. R = 32: two groups, two bands, the 65th column.
    R = 40: 81 columns, the widest window of the path, 17 rest columns."""
    run_case(pkg, W, H, "shift", mode, R, 1, 8, per_partition=False, seed=100 + R + mode)


@pytest.mark.gpu
@pytest.mark.parametrize("is_b", [0, 1])
@pytest.mark.parametrize("spread", [0, 4])
@pytest.mark.parametrize("mode", [-1, 0])
def test_uni_ties_and_zero_vector_rules(pkg, mode, spread, is_b):
    """A flat picture: every candidate's SAD ties, so the mv cost and the spiral index alone decide -- through both spiral halves, with
    check_for_00 (FullSearch) and the position-0 tie (FastFull) at rdopt 0, and with both switched off in a B slice."""
    run_case(pkg, W, H, "flat", mode, 32, 0, spread, per_partition=False, seed=200 + spread + mode, is_b=is_b)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [-1, 0])
@pytest.mark.parametrize("rdopt", [0, 1])
@pytest.mark.parametrize("spread", [100, 200])
def test_uni_windows_outside_the_picture_and_centre_clip(pkg, spread, rdopt, mode):
    """Far predictors: windows hang over every picture edge (the border fill of the window staging), and with rdopt 0 the centre is
    clipped to +-R, so that 4 mv - p never comes near 0 and every bit count is large."""
    run_case(pkg, W, H, "noise", mode, 32, rdopt, spread, per_partition=False, seed=300 + spread + rdopt + mode)


# one predictor per macroblock, cycled over the 24 macroblocks. With rdopt 1 the window is centred on pred / 4, so 4 mv - p runs through
# -4R - r .. 4R - r in steps of 4 (r the quarter-pel remainder): through 0 and every +-2^k up to 128 for r = 0, and across every
# |d| = 2^k - 1 -> 2^k + 3 step for r = 1, 2, 3 -- the rows (and, for the horizontal count, the columns) where the bit count changes
INTEGER_PEL = [(0, 0), (4, -8), (-4, 4), (64, -64), (-128, 128), (8, 0), (0, -16), (32, 36), (-20, -12), (124, 4), (-60, 96), (16, -32)]
QUARTER_PEL = [(1, 2), (3, -1), (-2, -3), (-1, 1), (5, 6), (2, 3), (-7, 9), (63, -65), (127, -129), (-33, 34), (18, -17), (-1, -1)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,rdopt", [(-1, 1), (0, 1), (-1, 0)])
@pytest.mark.parametrize("preds", [INTEGER_PEL, QUARTER_PEL], ids=["integer_pel", "quarter_pel_low_bits_1_2_3"])
def test_uni_bit_count_boundaries(pkg, preds, mode, rdopt):
    cur, ref, mbs = inputs(pkg, "shift", 0, 400)
    for i in range(len(mbs)):
        mbs[i]["pred_mv"][:] = preds[i % len(preds)]
    check(pkg, cur, ref, mbs, mode, 32, rdopt)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [-1, 0])
@pytest.mark.parametrize("qp", [28, 51])
def test_uni_lambda(pkg, qp, mode):
    """The default lambda and the largest the encoder uses: QP 51 gives 5.5e6, near the top of the kernel's 24-bit multiply."""
    cur, ref, mbs = inputs(pkg, "shift", 8, 500 + qp)
    check(pkg, cur, ref, mbs, mode, 32, 1, qp=qp)


@pytest.mark.gpu
def test_uni_weighted_reference(pkg):
    run_case(pkg, W, H, "shift", -1, 32, 1, 2, per_partition=False, seed=600, wp=(70, -20, 6))


@pytest.mark.gpu
@pytest.mark.parametrize("rdopt", [1, 0])
def test_uni_and_table_items_in_one_launch(pkg, rdopt):
    """Half of the macroblocks have one predictor; the others 41 different ones with pred / 4 equal -- one search centre, so still one
    fast item each, but not uni: both bodies of the kernel run in one launch."""
    cur, ref, mbs = inputs(pkg, "shift", 8, 700)
    rng = np.random.default_rng(701)
    for i in range(1, len(mbs), 2):
        c = rng.integers(-2, 3, 2)                   # the common centre; the remainders keep the sign of a non-zero centre (C division)
        r = rng.integers(0, 4, (41, 2))
        r[0], r[1] = (0, 0), (1, 2)                  # never all equal
        mbs[i]["pred_mv"] = np.where(c < 0, 4 * c - r, 4 * c + r)
    check(pkg, cur, ref, mbs, -1, 32, rdopt)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,rdopt,spread", [("shift", 1, 8), ("flat", 0, 4)])
@pytest.mark.parametrize("mode", [-1, 0])
def test_uni_body_equals_table_body(pkg, kind, rdopt, spread, mode, monkeypatch):
    """A/B: the same one-predictor items through the one-predictor body and, with JMHIP_ME_KERNEL=pair_tables, through the table body."""
    cur, ref, mbs = inputs(pkg, kind, spread, 800 + spread)
    a = search(pkg, cur, ref, mbs, mode, 32, rdopt)
    monkeypatch.setenv("JMHIP_ME_KERNEL", "pair_tables")
    b = search(pkg, cur, ref, mbs, mode, 32, rdopt)
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key
