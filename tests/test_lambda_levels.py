"""Every search entry on three DIFFERENT Lagrangian factors and at the largest factor it accepts (tests/lambda_cases.py), device against
oracle, bit-exact on the fields the entry's own tests compare.

Without a GPU: for every parameter set compared below, the oracle run with each wrong triple of lambda_cases.MUTATIONS differs from the run
with the true one -- in the integer results for the mutations that change lambda[F_PEL], in the refined ones alone for those that do not --
so a device that took a factor from the wrong level cannot agree with the oracle. And on lambda_cases.saturated_pair at an entry's bound the
costs are as large as the packed keys of the kernels were sized for, while the oracle's own int products stay below 2^31."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import oracle
from tests.conftest import load_pkg
from tests.lambda_cases import BOUNDS, INTEGER_MUTATIONS, LAMBDA_SETS, MUTATIONS, lambdas, largest_mv_product, mutated, saturated_pair
from tests.test_bipred import make_jobs as make_bipred_jobs
from tests.test_bipred import oracle_bipred
from tests.test_bipred_chain import JOB_FIELDS, chain_params, make_jobs, oracle_chain
from tests.test_bipred_chain import compare as compare_chain
from tests.test_me import make_mbs, make_pair
from tests.test_slice_gpu import run_synthetic

W, H = 96, 64
INT_MAX = 2147483647
SPLITS = ("split", "split_rev")
ME_FIELDS = ("mv_int", "cost_int", "mv", "cost")
P16X16, P16X8_8X16 = [0], [1, 2, 3, 4]              # partitions of block types 1 and 2 / 3
# JmhipError carries "<call>: <jmhip_strerror(code)> (<jmhip_last_error>)": the code's own text, before the detail (which names lambda either way)
UNSUPPORTED = r"^jmhip_\w+: configuration not supported by this version \("      # JMHIP_ERR_UNSUPPORTED
BAD_ARGUMENT = r"^jmhip_\w+: bad argument \(.*lambda"                            # JMHIP_ERR_ARG


def test_sets_and_bounds_are_what_the_header_says():
    import os
    import re
    s = LAMBDA_SETS["split"]
    assert len(set(s)) == 3 and LAMBDA_SETS["split_rev"] == s[::-1]
    assert len(set(LAMBDA_SETS["jm_min"])) == 1 and len(set(LAMBDA_SETS["jm_max"])) == 1 and LAMBDA_SETS["jm_min"][0] < min(s) and max(s) < LAMBDA_SETS["jm_max"][0]
    with open(os.path.join(oracle.ROOT, "include", "jmhip.h")) as f:
        defs = dict(re.findall(r"#define JMHIP_LAMBDA_MAX_(\w+)\s+(.+)", f.read()))
    for entry, name in (("me_frame", "ME_FRAME"), ("me_subpel", "ME_SUBPEL"), ("bipred", "BIPRED"), ("slice", "SLICE")):
        assert BOUNDS[entry] == eval(defs[name], {"__builtins__": {}}), entry
    # every factor JM produces for P slices (the largest: RDOptimization off, QP2QUANT[39] << 16) passes the three P-slice entries
    assert max(LAMBDA_SETS["jm_max"][0], 91 << 16) <= min(BOUNDS["me_frame"], BOUNDS["me_subpel"], BOUNDS["slice"])
    for how in MUTATIONS:
        assert mutated(s, how) != s and set(mutated(s, how)) <= set(s)


# ------------------------------------------------------------------ jmhip_me_frame

# name -> (pair, mode, R, spread, one predictor per macroblock, metric or None (metric_set = 0), JMHIP_ME_KERNEL or None)
ME_KERNELS = {
    "union": ("shift", -1, 8, 8, False, None, None),                # me_int_kernel: the union window of 41 centres
    "pair_tables": ("shift", -1, 32, 5, False, None, None),         # me_int_pair_kernel, table body: several centres per macroblock
    "pair_uni_full": ("shift", -1, 32, 8, True, None, None),        # its one-predictor body
    "pair_uni_fastfull": ("shift", 0, 32, 8, True, None, None),     # (all 41 predictors equal: what selects that body, in FastFull too)
    "pair_tables_fastfull": ("shift", 0, 32, 8, False, None, None), # FastFull reads predictor 0 alone: one centre, but the table body
    "single": ("shift", -1, 32, 5, False, None, "single"),
    "pers": ("shift", 0, 32, 8, True, None, "pers"),
    "metric": ("shift", -1, 8, 6, False, (0, 1, 2), None),          # me_metric.hip: the levels' factors differ in the real JM too
    "wide": ("shift", -1, 45, 3, True, None, None),                 # ... and its 64-bit keys beyond the 13-bit tie field
}
RDOPT_T8 = ((0, 1), (1, 0))                                         # rdopt 0 and 1, the 4x4 and the 8x8 Hadamard in the refinement
RDOPT_T8_CROSSED = ((0, 0), (0, 1), (1, 0), (1, 1))                 # ... crossed where the oracle is cheap (R = 8)


def rdopt_t8(case):
    return RDOPT_T8_CROSSED if case[2] <= 8 else RDOPT_T8
SATURATED = {                                                       # rdopt 0: the zero-vector bonus next to the largest cost
    "full32": ("saturated", -1, 32, 5, False, None, None),
    "fastfull32": ("saturated", 0, 32, 60, False, None, None),      # far predictors: the bonus does not win everywhere
    "union8": ("saturated", -1, 8, 8, False, None, None),
    "full44": ("saturated", -1, 44, 4, True, None, None),           # the last range of the 13-bit tie field
    "fastfull44": ("saturated", 0, 44, 60, False, None, None),
}


@functools.lru_cache(maxsize=None)
def me_inputs(case):
    """case: the first six entries of a row above (the kernel choice changes nothing the oracle sees)"""
    pair, mode, R, spread, one_pred = case[:5]
    rng = np.random.default_rng(100 + R + spread)
    cur, ref = saturated_pair(rng, W, H) if pair == "saturated" else make_pair(rng, W, H, pair)
    mbs = make_mbs(None, rng, W // 16, H // 16, spread, per_partition=not one_pred)
    if R > 44:                                       # 8281 candidates per search: every other macroblock keeps the oracle's share of the CPU tests small
        mbs = mbs[::2].copy()
    return cur, ref, mbs, oracle.RefPic(ref, yuv_format=0)


@functools.lru_cache(maxsize=None)
def me_oracle(case, rdopt, t8, lam):
    cur, ref, mbs, rp = me_inputs(case[:6])
    p = oracle.me_params(rdopt=rdopt, transform8x8_mode=t8, metric=case[5] or (0, 2, 2))
    return oracle.me_frame(p, [rp], cur, mbs, case[1], case[2], list(lam))


def me_device(pkg, case, rdopt, t8, lam, monkeypatch=None):
    cur, ref, mbs, _ = me_inputs(case[:6])
    _, mode, R, _, _, metric, kernel = case
    if kernel:
        monkeypatch.setenv("JMHIP_ME_KERNEL", kernel)
    ctx = pkg.Context(W, H, yuv_format=0, max_refs=1, search_range=R)
    ctx.ref_upload(0, ref)
    ctx.interp_luma(0)
    ctx.cur_upload(cur)
    prm = pkg.MeParams()
    prm.search_mode, prm.search_range, prm.rdopt = mode, R, rdopt
    prm.level_mv_min, prm.level_mv_max = -511, 511
    prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lam
    prm.transform8x8_mode, prm.subpel, prm.partition_mask = t8, 1, (1 << 41) - 1
    if metric:
        prm.metric_set = 1
        prm.metric[0], prm.metric[1], prm.metric[2] = metric
    try:
        return ctx.me_frame(prm, mbs)
    finally:
        ctx.close()


def differs(a, b, fields):
    return any(not np.array_equal(a[f], b[f]) for f in fields)


def check_bites(true, wrong, how, integer_fields, refined_fields, where):
    """`wrong`: the oracle's results under mutation `how`. Integer mutations show in the integer fields, the others in the refined fields alone."""
    if how in INTEGER_MUTATIONS:
        assert differs(true, wrong, integer_fields), (where, how, "leaves the integer results as they are")
    else:
        assert not differs(true, wrong, integer_fields), (where, how, "must not reach the integer results")
        assert differs(true, wrong, refined_fields), (where, how, "leaves the refined results as they are")


@pytest.mark.parametrize("name", sorted(ME_KERNELS))
@pytest.mark.parametrize("lamset", SPLITS)
def test_me_frame_inputs_tell_the_levels_apart(name, lamset):
    case, lam = ME_KERNELS[name], lambdas(lamset, "me_frame")
    for rdopt, t8 in rdopt_t8(case):
        true = me_oracle(case[:6], rdopt, t8, tuple(lam))
        for how in MUTATIONS:
            check_bites(true, me_oracle(case[:6], rdopt, t8, tuple(mutated(lam, how))), how, ("mv_int", "cost_int"), ("mv", "cost"), (name, lamset, rdopt, t8))


def saturated_mbs(mbs, R):
    """macroblocks whose every candidate block stays in the saturated half (or left of the picture)"""
    half = (W // 16 // 2) * 16
    reach = [max(abs(int(v)) for v in mb["pred_mv"][:, 0]) // 4 + 1 + R + 16 for mb in mbs]
    return [i for i, mb in enumerate(mbs) if int(mb["mb_x"]) * 16 + reach[i] <= half]


@pytest.mark.parametrize("name", ["full32", "fastfull32", "union8"])
def test_me_frame_bound_inputs_fill_the_cost_fields(name):
    case = SATURATED[name][:6]
    cur, ref, mbs, _ = me_inputs(case)
    lam = lambdas("bound", "me_frame")
    R = case[2]
    # the farthest candidate: the clipped centre (within one pel of pred / 4) plus the range, in quarter-pels, against every predictor
    reach = 4 * (int(np.abs(mbs["pred_mv"]).max()) // 4 + 1 + R)
    assert largest_mv_product(lam[0], mbs["pred_mv"], reach) < 1 << 31
    assert largest_mv_product(lam[2], mbs["pred_mv"], reach + 3) < 1 << 31
    want = me_oracle(case, 0, 0, tuple(lam))
    assert want["cost_int"][:, P16X16].max() > 65535, "no 16x16 cost beyond 16 bits: the (cost + bias) << 13 key is not exercised"
    assert want["cost_int"][:, P16X8_8X16].max() >= 32640
    if name == "union8":                             # R = 8 leaves macroblocks whose whole window is saturated: SAD 65280 / 32640 for every candidate
        sat = saturated_mbs(mbs, R)
        assert len(sat) >= H // 16
        assert (want["cost_int"][sat][:, P16X8_8X16] >= 32640).all()
    for other in ("jm_min", "jm_max"):               # the same pictures at JM's own extremes decide differently: magnitude matters here
        assert differs(want, me_oracle(case, 0, 0, tuple(lambdas(other, "me_frame"))), ("mv_int",)), other


def assert_me_equal(got, want, where):
    for key in ME_FIELDS:
        if not np.array_equal(got[key], want[key]):
            bad = np.argwhere((got[key] != want[key]).reshape(len(got), 41, -1).any(axis=2))[0]
            raise AssertionError("%s: %s differs at mb %d partition %d: device %s oracle %s" % (where, key, bad[0], bad[1], got[key][bad[0], bad[1]], want[key][bad[0], bad[1]]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ME_KERNELS))
@pytest.mark.parametrize("lamset", SPLITS)
def test_me_frame_per_level_lambdas(pkg, name, lamset, monkeypatch):
    case, lam = ME_KERNELS[name], lambdas(lamset, "me_frame")
    for rdopt, t8 in rdopt_t8(case):
        assert_me_equal(me_device(pkg, case, rdopt, t8, lam, monkeypatch), me_oracle(case[:6], rdopt, t8, tuple(lam)), (name, lamset, rdopt, t8))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SATURATED))
@pytest.mark.parametrize("lamset", ["jm_min", "jm_max", "bound"])
def test_me_frame_saturated_pictures_at_the_lambda_extremes(pkg, name, lamset):
    lam = lambdas(lamset, "me_frame")
    assert_me_equal(me_device(pkg, SATURATED[name], 0, 0, lam), me_oracle(SATURATED[name][:6], 0, 0, tuple(lam)), (name, lamset))


@pytest.mark.gpu
def test_me_frame_refuses_a_lambda_above_its_bound(pkg):
    for k in range(3):
        lam = lambdas("jm_max", "me_frame")
        lam[k] = BOUNDS["me_frame"] + 1
        with pytest.raises(pkg.JmhipError, match=UNSUPPORTED):
            me_device(pkg, ME_KERNELS["union"], 1, 0, lam)


# ------------------------------------------------------------------ jmhip_me_subpel

@functools.lru_cache(maxsize=None)
def subpel_inputs(pair):
    rng = np.random.default_rng(5)
    cur, ref = saturated_pair(rng, W, H) if pair == "saturated" else make_pair(rng, W, H, pair)
    mbs = make_mbs(None, rng, W // 16, H // 16, 12)
    mv_int = rng.integers(-14, 15, (len(mbs), 41, 2)).astype(np.int16)
    return cur, ref, mbs, mv_int, oracle.RefPic(ref, yuv_format=0)


@functools.lru_cache(maxsize=None)
def subpel_oracle(pair, rdopt, t8, lam):
    """SubPelBlockMotionSearch from arbitrary integer vectors, as tests/test_dist.py::test_me_subpel_alone calls it"""
    cur, ref, mbs, mv_int, rp = subpel_inputs(pair)
    L = oracle._setup_search_protos()
    p = oracle.me_params(rdopt=rdopt, transform8x8_mode=t8)
    cur16 = cur.astype(np.uint16)
    lam_a = (C.c_int * 3)(*lam)
    out = {"mv": np.zeros((len(mbs), 41, 2), np.int16), "cost": np.zeros((len(mbs), 41), np.int32)}
    for i, mb in enumerate(mbs):
        ox, oy = int(mb["mb_x"]) * 16, int(mb["mb_y"]) * 16
        for q, (bt, x4, y4, w4, h4) in enumerate(oracle.PARTS):
            px, py, bsx, bsy = ox + 4 * x4, oy + 4 * y4, 4 * w4, 4 * h4
            orig = np.zeros(768, np.uint16)
            orig[: bsx * bsy] = cur16[py:py + bsy, px:px + bsx].reshape(-1)
            mvq = (mv_int[i, q] * 4).copy()
            out["cost"][i, q] = L.jmo_subpel_search(C.byref(p), C.byref(rp.ref), orig.ctypes.data, 1, px, py, bt, int(mb["pred_mv"][q][0]), int(mb["pred_mv"][q][1]),
                                                    mvq.ctypes.data, mvq[1:].ctypes.data, 9, 9, INT_MAX, lam_a)
            out["mv"][i, q] = mvq
    return out


def subpel_device(pkg, pair, rdopt, t8, lam):
    cur, ref, mbs, mv_int, _ = subpel_inputs(pair)
    ctx = pkg.Context(W, H, yuv_format=0, max_refs=1, search_range=8)
    ctx.ref_upload(0, ref)
    ctx.interp_luma(0)
    ctx.cur_upload(cur)
    prm = pkg.MeParams()
    prm.search_mode, prm.search_range, prm.rdopt = -1, 8, rdopt
    prm.level_mv_min, prm.level_mv_max = -511, 511
    prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lam
    prm.transform8x8_mode, prm.subpel, prm.partition_mask = t8, 1, (1 << 41) - 1
    res = np.zeros(len(mbs), dtype=pkg.ME_RESULT_DTYPE)
    res["mv_int"] = mv_int
    try:
        return ctx.me_subpel(prm, mbs, res)
    finally:
        ctx.close()


@pytest.mark.parametrize("lamset", SPLITS)
def test_me_subpel_inputs_tell_the_levels_apart(lamset):
    """the refinement reads lambda[H_PEL] and lambda[Q_PEL] alone: every mutation changes one of them, and the results"""
    lam = lambdas(lamset, "me_subpel")
    for rdopt, t8 in RDOPT_T8_CROSSED:
        true = subpel_oracle("shift", rdopt, t8, tuple(lam))
        for how in MUTATIONS:
            assert mutated(lam, how)[1:] != lam[1:]
            assert differs(true, subpel_oracle("shift", rdopt, t8, tuple(mutated(lam, how))), ("mv", "cost")), (lamset, rdopt, t8, how)


def test_me_subpel_bound_inputs_stay_inside_int():
    cur, ref, mbs, mv_int, _ = subpel_inputs("saturated")
    lam = lambdas("bound", "me_subpel")
    reach = 4 * int(np.abs(mv_int).max()) + 3
    assert largest_mv_product(lam[1], mbs["pred_mv"], reach) < 1 << 31
    want = subpel_oracle("saturated", 1, 0, tuple(lam))
    # a flat difference of 255 has Hadamard SAD 16 * 255 / 2 per 4x4 block: 32640 for the macroblock, and the motion cost on top
    assert want["cost"][:, P16X16].max() > 32640 and want["cost"].min() >= 0
    assert differs(want, subpel_oracle("saturated", 1, 0, tuple(lambdas("jm_max", "me_subpel"))), ("mv",))


@pytest.mark.gpu
@pytest.mark.parametrize("lamset,pair", [("split", "shift"), ("split_rev", "shift"), ("bound", "saturated"), ("jm_max", "saturated")])
def test_me_subpel_per_level_lambdas_and_bound(pkg, lamset, pair):
    lam = lambdas(lamset, "me_subpel")
    for rdopt, t8 in RDOPT_T8_CROSSED:
        got, want = subpel_device(pkg, pair, rdopt, t8, lam), subpel_oracle(pair, rdopt, t8, tuple(lam))
        for key in ("mv", "cost"):
            assert np.array_equal(got[key], want[key]), (lamset, rdopt, t8, key, np.argwhere((got[key] != want[key]).reshape(len(got), 41, -1).any(axis=2))[0])


@pytest.mark.gpu
def test_me_subpel_refuses_a_lambda_above_its_bound(pkg):
    for k in (1, 2):
        lam = lambdas("bound", "me_subpel")
        lam[k] += 1
        with pytest.raises(pkg.JmhipError, match=UNSUPPORTED):
            subpel_device(pkg, "shift", 1, 0, lam)


# ------------------------------------------------------------------ jmhip_bipred_search / jmhip_bipred_chain

BI_WEIGHTS = (None, (37, 29, -3, 16, 5))


@functools.lru_cache(maxsize=None)
def bipred_inputs(pair, t8):
    """the pictures and jobs of tests/test_bipred.py (integer and sub-pel calls alternate; the last eight leave the picture), and the chain's jobs"""
    rng = np.random.default_rng(7 + t8)
    if pair == "saturated":                           # both references 0 under a current picture of 255: the bi-predictive SAD is maximal too
        cur, ref1 = saturated_pair(rng, W, H)
        _, ref2 = saturated_pair(rng, W, H)
    else:
        cur, ref1 = make_pair(rng, W, H, "shift")
        _, ref2 = make_pair(rng, W, H, "shift")
        ref2 = np.roll(ref2, (1, -2), (0, 1))
    mbw, mbh = W // 16, H // 16
    jobs = make_bipred_jobs(load_pkg().BIPRED_JOB_DTYPE, rng, mbw, mbh)
    chain_jobs = make_jobs(np.dtype(JOB_FIELDS), rng, mbw, mbh, 8)
    rp = (oracle.RefPic(ref1, yuv_format=0), oracle.RefPic(ref2, yuv_format=0))
    return cur, ref1, ref2, jobs, chain_jobs, rp


@functools.lru_cache(maxsize=None)
def bipred_oracle(pair, t8, wi, lam):
    cur, _, _, jobs, _, rp = bipred_inputs(pair, t8)
    cur16 = cur.astype(np.uint16)
    return [oracle_bipred(rp[int(j["ref1"])], rp[int(j["ref2"])], cur16, j, list(lam), t8, BI_WEIGHTS[wi]) for j in jobs]


@functools.lru_cache(maxsize=None)
def chain_oracle(pair, t8, wi, lam):
    cur, _, _, _, chain_jobs, rp = bipred_inputs(pair, t8)
    cur16 = cur.astype(np.uint16)
    return [oracle_chain(list(rp), cur16, j, list(lam), t8, BI_WEIGHTS[wi], 3, 16, 2) for j in chain_jobs]


def chain_steps(chains, integer):
    return [[(s["mv_out"], s["cost"]) for s in c["steps"] if s["integer"] == integer] for c in chains]


@pytest.mark.parametrize("t8,wi", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("lamset", SPLITS)
def test_bipred_inputs_tell_the_levels_apart(lamset, t8, wi):
    lam = lambdas(lamset, "bipred")
    _, _, _, jobs, _, _ = bipred_inputs("shift", t8)
    stage = jobs["stage"]
    true, ctrue = bipred_oracle("shift", t8, wi, tuple(lam)), chain_oracle("shift", t8, wi, tuple(lam))
    for how in MUTATIONS:
        wrong, cwrong = bipred_oracle("shift", t8, wi, tuple(mutated(lam, how))), chain_oracle("shift", t8, wi, tuple(mutated(lam, how)))
        changed = np.array([a != b for a, b in zip(true, wrong)])
        if how in INTEGER_MUTATIONS:
            assert changed[stage == 0].any(), (how, "integer calls")
            assert chain_steps(ctrue, True) != chain_steps(cwrong, True), (how, "the chain's integer steps")
        else:
            assert not changed[stage == 0].any() and changed[stage == 1].any(), (how, "sub-pel calls alone")
            assert chain_steps(ctrue, True) == chain_steps(cwrong, True) and chain_steps(ctrue, False) != chain_steps(cwrong, False), (how, "the chain's sub-pel steps alone")


def test_bipred_bound_inputs_fill_the_cost_field():
    lam = lambdas("bound", "bipred")
    _, _, _, jobs, chain_jobs, _ = bipred_inputs("saturated", 0)
    # vectors within 30 + 16 pel (the chain: 40 + 2 * 16), predictors within 12 quarter-pels; two vectors are costed per candidate
    assert 2 * largest_mv_product(lam[0], np.concatenate([jobs["pred1"], jobs["pred2"], chain_jobs["pred_a"], chain_jobs["pred_b"]]), 4 * 72 + 3) < 1 << 31
    want = bipred_oracle("saturated", 0, 0, tuple(lam))
    assert max(c for (_, _, c), j in zip(want, jobs) if j["stage"] == 0) > 65535
    chains = chain_oracle("saturated", 0, 0, tuple(lam))
    assert max(s["cost"] for c in chains for s in c["steps"] if s["integer"]) > 65535
    assert want != bipred_oracle("saturated", 0, 0, tuple(lambdas("split", "bipred")))


def bipred_ctx(pkg, pair, t8):
    cur, ref1, ref2, jobs, chain_jobs, _ = bipred_inputs(pair, t8)
    ctx = pkg.Context(W, H, yuv_format=0, max_refs=2, search_range=16)
    for s, r in enumerate((ref1, ref2)):
        ctx.ref_upload(s, r)
        ctx.interp_luma(s)
    ctx.cur_upload(cur)
    return ctx, jobs, chain_jobs


def bipred_params(pkg, lam, t8, wp):
    prm = pkg.BipredParams()
    prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lam
    prm.transform8x8_mode = t8
    if wp:
        prm.apply_weights = 1
        prm.weight1, prm.weight2, prm.offset_bi, prm.wp_luma_round, prm.luma_log_weight_denom = wp
    return prm


def run_bipred(pkg, pair, t8, wi, lam):
    assert pkg.BIPRED_CHAIN_JOB_DTYPE == np.dtype(JOB_FIELDS)
    ctx, jobs, chain_jobs = bipred_ctx(pkg, pair, t8)
    try:
        got = ctx.bipred_search(bipred_params(pkg, lam, t8, BI_WEIGHTS[wi]), jobs)
        cgot = ctx.bipred_chain(chain_params(pkg, lam, t8, BI_WEIGHTS[wi], 3, 16, 2), chain_jobs)
    finally:
        ctx.close()
    for i, want in enumerate(bipred_oracle(pair, t8, wi, tuple(lam))):
        assert (int(got[i]["mv"][0]), int(got[i]["mv"][1]), int(got[i]["cost"])) == want, ("jmhip_bipred_search", i, jobs[i])
    for i, want in enumerate(chain_oracle(pair, t8, wi, tuple(lam))):
        compare_chain(cgot[i], want, ("jmhip_bipred_chain", i))


@pytest.mark.gpu
@pytest.mark.parametrize("t8,wi", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("lamset", SPLITS)
def test_bipred_per_level_lambdas(pkg, lamset, t8, wi):
    run_bipred(pkg, "shift", t8, wi, lambdas(lamset, "bipred"))


@pytest.mark.gpu
def test_bipred_saturated_pictures_at_the_bound(pkg):
    run_bipred(pkg, "saturated", 0, 0, lambdas("bound", "bipred"))


@pytest.mark.gpu
def test_bipred_refuses_a_lambda_above_its_bound(pkg):
    ctx, jobs, chain_jobs = bipred_ctx(pkg, "shift", 0)
    try:
        for k in range(3):
            lam = lambdas("bound", "bipred")
            lam[k] += 1
            with pytest.raises(pkg.JmhipError, match=UNSUPPORTED):
                ctx.bipred_search(bipred_params(pkg, lam, 0, None), jobs)
            with pytest.raises(pkg.JmhipError, match=UNSUPPORTED):
                ctx.bipred_chain(chain_params(pkg, lam, 0, None, 3, 16, 2), chain_jobs)
    finally:
        ctx.close()


# ------------------------------------------------------------------ jmhip_p_slice_search

# (search mode, transform8x8_mode, range). The exhaustive modes have two implementations: the macroblock wavefront of me_wave.hip (here R = 8) and,
# for ranges 16..40 without the 8x8 transform, the sweeps of me_xslice.hip (R = 16) -- each with its own copy of the lambda_mf[Q_PEL]-only sites
SLICE_CASES = [(-1, 0, 8), (-1, 1, 8), (0, 0, 8), (-1, 0, 16), (0, 0, 16), (1, 0, 8), (2, 0, 8), (3, 0, 8)]
SLICE_BOUND_CASES = [(-1, 8), (0, 8), (-1, 16), (0, 16)]
SLICE_NREF, SLICE_FRAMES = 2, 3                                       # two references: the reference cost (lambda_mf[Q_PEL] * refbits) takes part


@functools.lru_cache(maxsize=None)
def saturated_clip():
    rng = np.random.default_rng(9)
    cur, ref_a = saturated_pair(rng, W, H)
    _, ref_b = saturated_pair(rng, W, H)
    return (ref_b, ref_a, cur)


def slice_kwargs(mode, t8, lam, saturated):
    kw = dict(t8=t8, lambda_mf=list(lam), nframes=SLICE_FRAMES, seed=5 + mode)
    if saturated:
        kw.update(clip=list(saturated_clip()), nframes=2)
    return kw


@functools.lru_cache(maxsize=None)
def slice_oracle(mode, t8, R, lam, saturated=False):
    out = []
    run_synthetic(None, mode, W, H, R, SLICE_NREF, what_if=out, oracle_only=True, **slice_kwargs(mode, t8, lam, saturated))
    return np.concatenate(out)


@pytest.mark.parametrize("mode,t8,R", SLICE_CASES)
@pytest.mark.parametrize("lamset", SPLITS)
def test_slice_inputs_tell_the_levels_apart(lamset, mode, t8, R):
    """The sub-pel mutations also reach the sites that read lambda_mf[Q_PEL] alone -- the skip bonus, the reference cost, the UMHexagonS / EPZS
    refinements: they must move a decision (mode, sub-mode, reference; best_mode 0 is the skip flag) as well as a vector."""
    lam = lambdas(lamset, "slice")
    true = slice_oracle(mode, t8, R, tuple(lam))
    for how in MUTATIONS:
        wrong = slice_oracle(mode, t8, R, tuple(mutated(lam, how)))
        if how in INTEGER_MUTATIONS:
            assert differs(true, wrong, ("mv_int", "cost_int")), (how, "integer searches")
        else:
            assert differs(true, wrong, ("best_mode", "b8mode", "b8ref")), (how, "no decision moves")
            assert differs(true, wrong, ("mv", "final_mv")), (how, "no vector moves")


@pytest.mark.parametrize("mode,R", SLICE_BOUND_CASES)
def test_slice_bound_inputs_fill_the_cost_fields(mode, R):
    lam = lambdas("bound", "slice")
    want = slice_oracle(mode, 0, R, tuple(lam), True)
    reach = 4 * (int(np.abs(want["pred"]).max()) // 4 + 1 + R) + 3
    assert largest_mv_product(lam[0], want["pred"][:, :SLICE_NREF], reach) < 1 << 31
    assert want["cost_int"][:, :SLICE_NREF, 0].max() > 65535
    assert want["cost_int"][:, :SLICE_NREF, 1:5].max() >= 32640


@pytest.mark.gpu
@pytest.mark.parametrize("mode,t8,R", SLICE_CASES)
@pytest.mark.parametrize("lamset", SPLITS)
def test_slice_search_per_level_lambdas(pkg, lamset, mode, t8, R):
    lam = lambdas(lamset, "slice")
    run_synthetic(pkg, mode, W, H, R, SLICE_NREF, **slice_kwargs(mode, t8, lam, False))


@pytest.mark.gpu
@pytest.mark.parametrize("mode,R", SLICE_BOUND_CASES)
def test_slice_search_saturated_pictures_at_the_bound(pkg, mode, R):
    run_synthetic(pkg, mode, W, H, R, SLICE_NREF, **slice_kwargs(mode, 0, lambdas("bound", "slice"), True))


@pytest.mark.gpu
def test_slice_search_refuses_a_lambda_above_its_bound(pkg):
    """the slice search answers JMHIP_ERR_ARG (include/jmhip.h), before anything is launched"""
    for k in range(3):
        lam = lambdas("bound", "slice")
        lam[k] += 1
        with pytest.raises(pkg.JmhipError, match=BAD_ARGUMENT):
            run_synthetic(pkg, -1, W, H, 8, SLICE_NREF, **slice_kwargs(-1, 0, lam, True))
