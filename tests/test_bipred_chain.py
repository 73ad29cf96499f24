"""The bi-predictive refinement chain of BlockMotionSearch (mv-search.c:864-1034) in one launch (jmhip_bipred_chain, bipred_chain_kernel)
against a chain assembled HERE from the oracle's jmo_fullpel_bipred / jmo_subpel_bipred -- the functions tests/test_bipred.py drives, pinned
inside the real JM by tests/test_oracle_swap.py -- bit-exact: the final pair, the cost and every step of the trace.

The inputs must make the chain do something: in every parameter set with refinements >= 1 some job (a) improves the cost in an integer step
after step 0, (b) has a step that hands the carried minimum back unchanged, (c) moves mv in the second sub-pel call (sub-pel 2), (d) takes a
UMV access path. These are asserted on the ORACLE's results, without a GPU too (test_chain_inputs_exercise_the_chain)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import oracle
from tests.test_bipred import Bipred
from tests.test_me import lambda_factors, make_pair

INT_MAX = 2147483647
W, H = 96, 64
WEIGHTS = (None, (37, 29, -3, 16, 5), (20, 44, 2, 32, 6))        # weight_a != weight_b: a missed role swap shows
GEOMETRY = [(t8, wi, R) for t8 in (0, 1) for wi in range(3) for R in (16, 13)]
CHAINS = list(itertools.product((0, 1, 3, 5), (0, 1, 2)))       # refinements x sub-pel


def oracle_call(stage, rp1, rp2, cur16, mb, smv, mv, pred1, pred2, R, min_mcost, lam, t8x8, wp):
    """One FullPelBlockMotionBiPred (stage 0) / SubPelBlockSearchBiPred (stage 1) call of the oracle: (mv, cost, took a UMV path)."""
    L = oracle.lib()
    b = Bipred()
    b.ref1, b.ref2 = C.pointer(rp1.ref), C.pointer(rp2.ref)
    b.test8x8, b.max_val = t8x8, 255
    b.apply_weights = 1 if wp else 0
    if wp:
        b.weight1, b.weight2, b.offset_bi, b.wp_luma_round, b.luma_log_weight_denom = wp
    b.metric[0], b.metric[1], b.metric[2] = 0, 2, 2
    b.start_hp, b.start_qp = 0, 1
    ox, oy = mb[0] * 16, mb[1] * 16
    orig = np.zeros(768, np.uint16)
    orig[:256] = cur16[oy:oy + 16, ox:ox + 16].reshape(-1)
    v = np.array(mv, np.int16)
    s = np.array(smv, np.int16)
    vp, ip = C.c_void_p, C.c_int
    if stage == 0:
        L.jmo_fullpel_bipred.argtypes = [C.POINTER(Bipred), vp, ip, ip, ip, ip, ip, ip, ip, vp, vp, vp, vp, ip, ip, ip]
        cost = L.jmo_fullpel_bipred(C.byref(b), orig.ctypes.data, ox, oy, 1, pred1[0], pred1[1], pred2[0], pred2[1], v.ctypes.data, v[1:].ctypes.data,
                                    s.ctypes.data, s[1:].ctypes.data, R, min_mcost, lam[0])
    else:
        L.jmo_subpel_bipred.argtypes = [C.POINTER(Bipred), vp, ip, ip, ip, ip, ip, vp, vp, vp, vp, ip, ip, ip, vp]
        cost = L.jmo_subpel_bipred(C.byref(b), orig.ctypes.data, ox, oy, 1, pred2[0], pred2[1], v.ctypes.data, v[1:].ctypes.data,
                                   s.ctypes.data, s[1:].ctypes.data, 9, 9, min_mcost, (C.c_int * 3)(*lam))
    return [int(v[0]), int(v[1])], cost, bool(b.umv1 or b.umv2)


def oracle_chain(rp, cur16, job, lam, t8x8, wp, refinements, R, subpel):
    """mv-search.c:889-1022 for SearchMode -1 / 0, the bookkeeping restated; every search is the oracle's. Side "a" is `list`, "b" list ^ 1."""
    mb = (int(job["mb_x"]), int(job["mb_y"]))
    pred = {0: [int(x) for x in job["pred_a"]], 1: [int(x) for x in job["pred_b"]]}      # pred_mv, pred_mv_bi (:880)
    slot = {0: int(job["slot_a"]), 1: int(job["slot_b"])}
    steps, umv = [], False

    def search(stage, odd, smv, mv, rng, min_in):
        # iterlist = list ^ odd: pictures 1 / 2, pred_mv1 / pred_mv2 (:893-894, :903-904) and weight1 / weight2 (me_fullsearch.c:218-226) change sides
        w = None if wp is None else ((wp[1], wp[0]) + tuple(wp[2:]) if odd else wp)
        out, cost, u = oracle_call(stage, rp[slot[odd]], rp[slot[odd ^ 1]], cur16, mb, smv, mv, pred[odd], pred[odd ^ 1], rng, min_in, lam, t8x8, w)
        steps.append(dict(smv=list(smv), mv_in=list(mv), mv_out=out, min_in=min_in, cost=cost, integer=stage == 0))
        return out, cost, u

    tempmv, bimv = [int(x) for x in job["s_mv"]], [int(x) for x in job["mv"]]             # :915-926
    min_mcostbi = INT_MAX                                                                 # :867
    iterlist = 0
    for i in range(refinements + 1):                                                      # :889
        iterlist = i & 1                                                                  # :899, :929
        if i:
            tempmv, bimv = bimv, mv                                                       # :895-898, :908-911
        bimv, min_mcostbi, u = search(0, iterlist, tempmv, bimv, R >> i, min_mcostbi)     # :960-964
        umv |= u
        mv = tempmv                                                                       # :973-974
    mv, bimv = [4 * x for x in tempmv], [4 * x for x in bimv]                             # :978-981
    if subpel >= 1:                                                                       # :984
        min_mcostbi = INT_MAX                                                             # start_me_refinement_hp == 0, :986-989
        bimv, min_mcostbi, u = search(1, iterlist, mv, bimv, 0, min_mcostbi)              # :998-1000: refines bimv, mv fixed
        umv |= u
    if subpel == 2:                                                                       # :1004
        min_mcostbi = INT_MAX                                                             # :1006-1009: reset when EITHER start_me_refinement_hp or _qp is 0
        mv, min_mcostbi, u = search(1, iterlist ^ 1, bimv, mv, 0, min_mcostbi)            # :1018-1020: refines mv, bimv fixed
        umv |= u
    return dict(mv=mv, bimv=bimv, cost=min_mcostbi, iterlist=iterlist, steps=steps, umv=umv)   # :1028-1031


def conditions(chains, refinements, subpel):
    """which of (a)-(d) some job of the set meets"""
    met = set()
    for c in chains:
        later = [s for s in c["steps"][1:] if s["integer"]]
        if any(s["cost"] < s["min_in"] for s in later):
            met.add("a")
        if any(s["cost"] == s["min_in"] for s in c["steps"][1:]):
            met.add("b")
        if subpel == 2 and c["steps"][-1]["mv_out"] != c["steps"][-1]["mv_in"]:
            met.add("c")
        if c["umv"]:
            met.add("d")
    want = {"a", "b", "d"} | ({"c"} if subpel == 2 else set())
    return met, (want if refinements >= 1 else set())


def make_jobs(dtype, rng, mbw, mbh, n_far):
    """two jobs per macroblock (the lists both ways round), then n_far jobs at the picture's corners whose vectors push both blocks outside"""
    n = 2 * mbw * mbh
    jobs = np.zeros(n + n_far, dtype=dtype)
    for i in range(len(jobs)):
        j = jobs[i]
        if i < n:
            j["mb_x"], j["mb_y"] = (i // 2) % mbw, (i // 2) // mbw
            j["s_mv"], j["mv"] = rng.integers(-6, 7, 2), rng.integers(-6, 7, 2)
        else:
            cx, cy = (i >> 0) & 1, (i >> 1) & 1
            j["mb_x"], j["mb_y"] = cx * (mbw - 1), cy * (mbh - 1)
            out = np.array([1 if cx else -1, 1 if cy else -1])
            j["s_mv"], j["mv"] = out * rng.integers(24, 40, 2), out * rng.integers(24, 40, 2)
        j["slot_a"], j["slot_b"] = (0, 1) if i % 2 == 0 else (1, 0)
        j["pred_a"], j["pred_b"] = rng.integers(-12, 13, 2), rng.integers(-12, 13, 2)
    return jobs


JOB_FIELDS = [("mb_x", "<i2"), ("mb_y", "<i2"), ("slot_a", "<i2"), ("slot_b", "<i2"), ("s_mv", "<i2", (2,)), ("mv", "<i2", (2,)),
              ("pred_a", "<i2", (2,)), ("pred_b", "<i2", (2,))]     # jmhip_bipred_chain_job; the GPU tests check it against the package's dtype


@functools.lru_cache(maxsize=None)
def clip(t8x8):
    rng = np.random.default_rng(11 + t8x8)
    cur, ref1 = make_pair(rng, W, H, "shift")
    _, ref2 = make_pair(rng, W, H, "shift")
    ref2 = np.roll(ref2, (1, -2), (0, 1))
    jobs = make_jobs(np.dtype(JOB_FIELDS), rng, W // 16, H // 16, 8)
    return cur, ref1, ref2, jobs


@functools.lru_cache(maxsize=None)
def oracle_set(t8x8, wi, R, refinements, subpel):
    cur, ref1, ref2, jobs = clip(t8x8)
    rp = [oracle.RefPic(ref1, yuv_format=0), oracle.RefPic(ref2, yuv_format=0)]
    cur16 = cur.astype(np.uint16)
    return [oracle_chain(rp, cur16, j, lambda_factors(30), t8x8, WEIGHTS[wi], refinements, R, subpel) for j in jobs]


@pytest.mark.parametrize("t8x8,wi,R", GEOMETRY)
def test_chain_inputs_exercise_the_chain(t8x8, wi, R):
    """No GPU: the Python chain alone, and the conditions (a)-(d) on its results for every parameter set the device is compared on."""
    for refinements, subpel in CHAINS:
        chains = oracle_set(t8x8, wi, R, refinements, subpel)
        met, want = conditions(chains, refinements, subpel)
        assert want <= met, (refinements, subpel, sorted(want - met))
        for c in chains:
            assert len(c["steps"]) == refinements + 1 + subpel and c["iterlist"] == (refinements & 1)
            # a step never hands back more than it was given, and the chain's cost is the last step's
            assert all(s["cost"] <= s["min_in"] for s in c["steps"]) and c["cost"] == c["steps"][-1]["cost"]


def compare(got, want, where):
    n = len(want["steps"])
    assert (int(got["n_steps"]), int(got["iterlist_swapped"])) == (n, want["iterlist"]), where
    for k, s in enumerate(want["steps"]):
        g = (got["step_smv"][k].tolist(), got["step_mv_in"][k].tolist(), got["step_mv_out"][k].tolist(), int(got["step_min_in"][k]), int(got["step_cost"][k]))
        assert g == (s["smv"], s["mv_in"], s["mv_out"], s["min_in"], s["cost"]), (where, "step", k)
    assert (got["mv"].tolist(), got["bimv"].tolist(), int(got["cost"])) == (want["mv"], want["bimv"], want["cost"]), where


def chain_params(pkg, lam, t8x8, wp, refinements, R, subpel):
    prm = pkg.BipredChainParams()
    prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lam
    prm.transform8x8_mode = t8x8
    if wp:
        prm.apply_weights = 1
        prm.weight_a, prm.weight_b, prm.offset_bi, prm.wp_luma_round, prm.luma_log_weight_denom = wp
    prm.refinements, prm.search_range, prm.subpel = refinements, R, subpel
    return prm


@pytest.mark.gpu
@pytest.mark.parametrize("t8x8,wi,R", GEOMETRY)
def test_bipred_chain_matches_the_oracle(pkg, t8x8, wi, R):
    assert pkg.BIPRED_CHAIN_JOB_DTYPE == np.dtype(JOB_FIELDS)
    cur, ref1, ref2, jobs = clip(t8x8)
    ctx = pkg.Context(W, H, yuv_format=0, max_refs=2, search_range=16)
    for s, r in enumerate((ref1, ref2)):
        ctx.ref_upload(s, r)
        ctx.interp_luma(s)
    ctx.cur_upload(cur)
    for refinements, subpel in CHAINS:
        want = oracle_set(t8x8, wi, R, refinements, subpel)
        met, need = conditions(want, refinements, subpel)
        assert need <= met, (refinements, subpel, sorted(need - met))
        got = ctx.bipred_chain(chain_params(pkg, lambda_factors(30), t8x8, WEIGHTS[wi], refinements, R, subpel), jobs)
        for i in range(len(jobs)):
            compare(got[i], want[i], (refinements, subpel, i))
    ctx.close()


@pytest.mark.gpu
def test_bipred_chain_argument_checks(pkg):
    cur, ref1, ref2, jobs = clip(0)
    ctx = pkg.Context(W, H, yuv_format=0, max_refs=2, search_range=16)
    ctx.ref_upload(0, ref1)
    ctx.ref_upload(1, ref2)
    ctx.cur_upload(cur)
    lam = lambda_factors(30)
    ctx.bipred_chain(chain_params(pkg, lam, 0, None, 1, 8, 0), jobs[:4])            # integer steps alone need no sub-pel planes
    for bad in (chain_params(pkg, lam, 0, None, 1, 8, 1),                           # sub-pel planes not built
                chain_params(pkg, lam, 0, None, 6, 8, 0), chain_params(pkg, lam, 0, None, 1, 8, 3), chain_params(pkg, lam, 0, None, 1, 45, 0)):
        with pytest.raises(pkg.JmhipError):
            ctx.bipred_chain(bad, jobs[:4])
    ctx.close()


@pytest.mark.gpu
def test_bipred_chain_1080p_one_call(pkg):
    """Every 16x16 block of a 1080p picture in ONE call (8160 jobs; refinements 3, sub-pel 2, range 16), checked on every 9th macroblock."""
    w, h = 1920, 1088
    rng = np.random.default_rng(5)
    cur, ref1 = make_pair(rng, w, h, "shift")
    _, ref2 = make_pair(rng, w, h, "shift")
    ref2 = np.roll(ref2, (1, -2), (0, 1))
    mbw, mbh = w // 16, h // 16
    jobs = np.zeros(mbw * mbh, dtype=pkg.BIPRED_CHAIN_JOB_DTYPE)
    jobs["mb_x"], jobs["mb_y"] = np.arange(mbw * mbh) % mbw, np.arange(mbw * mbh) // mbw
    jobs["slot_a"], jobs["slot_b"] = np.arange(mbw * mbh) % 2, 1 - np.arange(mbw * mbh) % 2
    for f, spread in (("s_mv", 6), ("mv", 6), ("pred_a", 12), ("pred_b", 12)):
        jobs[f] = rng.integers(-spread, spread + 1, (len(jobs), 2))
    assert len(jobs) == 8160
    ctx = pkg.Context(w, h, yuv_format=0, max_refs=2, search_range=16)
    for s, r in enumerate((ref1, ref2)):
        ctx.ref_upload(s, r)
        ctx.interp_luma(s)
    ctx.cur_upload(cur)
    lam, wp = lambda_factors(30), WEIGHTS[1]
    got = ctx.bipred_chain(chain_params(pkg, lam, 0, wp, 3, 16, 2), jobs)
    ctx.close()
    rp = [oracle.RefPic(ref1, yuv_format=0), oracle.RefPic(ref2, yuv_format=0)]
    cur16 = cur.astype(np.uint16)
    for i in range(0, len(jobs), 9):
        compare(got[i], oracle_chain(rp, cur16, jobs[i], lam, 0, wp, 3, 16, 2), i)
