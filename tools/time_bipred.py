"""Times the bi-predictive refinement chain of every 16x16 block of a picture (refinements 3, sub-pel 2, range 16):
  A  jmhip_bipred_chain, the whole chain of every job in ONE call;
  B  the same searches as six batched jmhip_bipred_search calls (four integer steps, two sub-pel calls), their jobs taken from A's trace,
     so that both do exactly the same work (the results are compared);
and the n = 1 form the JM binding uses: one chain call against six per-call searches of one macroblock.
Both entries copy their jobs up, launch, copy the results back and synchronise, so the host clock round a call is the call's whole time
(job upload, kernel, result download). A and B alternate; the median of the repetitions is reported.
Usage: python tools/time_bipred.py [w h [reps]]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
pkg = ge._load_pkg()
from tests.test_me import lambda_factors, make_pair

w, h = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1920, 1088)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 15
REFINEMENTS, SUBPEL, R = 3, 2, 16
rng = np.random.default_rng(5)
cur, ref1 = make_pair(rng, w, h, "shift")
_, ref2 = make_pair(rng, w, h, "shift")
ref2 = np.roll(ref2, (1, -2), (0, 1))
mbw, mbh = w // 16, h // 16
n = mbw * mbh
jobs = np.zeros(n, dtype=pkg.BIPRED_CHAIN_JOB_DTYPE)
jobs["mb_x"], jobs["mb_y"] = np.arange(n) % mbw, np.arange(n) // mbw
jobs["slot_a"], jobs["slot_b"] = 0, 1
for f, spread in (("s_mv", 6), ("mv", 6), ("pred_a", 12), ("pred_b", 12)):
    jobs[f] = rng.integers(-spread, spread + 1, (n, 2))
ctx = pkg.Context(w, h, yuv_format=0, max_refs=2, search_range=R)
for s, r in enumerate((ref1, ref2)):
    ctx.ref_upload(s, r)
    ctx.interp_luma(s)
ctx.cur_upload(cur)
lam = lambda_factors(30)
cprm = pkg.BipredChainParams()
cprm.lambda_[0], cprm.lambda_[1], cprm.lambda_[2] = lam
cprm.refinements, cprm.search_range, cprm.subpel = REFINEMENTS, R, SUBPEL
sprm = pkg.BipredParams()
sprm.lambda_[0], sprm.lambda_[1], sprm.lambda_[2] = lam
trace = ctx.bipred_chain(cprm, jobs)


def step_jobs(tr, jb, k):
    """the jmhip_bipred_search jobs of step k, from the chain's trace"""
    odd = (k & 1) if k <= REFINEMENTS else (REFINEMENTS & 1) ^ (k - REFINEMENTS - 1)
    sj = np.zeros(len(jb), dtype=pkg.BIPRED_JOB_DTYPE)
    sj["mb_x"], sj["mb_y"] = jb["mb_x"], jb["mb_y"]
    sj["ref1"], sj["ref2"] = (jb["slot_b"], jb["slot_a"]) if odd else (jb["slot_a"], jb["slot_b"])
    sj["pred1"], sj["pred2"] = (jb["pred_b"], jb["pred_a"]) if odd else (jb["pred_a"], jb["pred_b"])
    sj["s_mv"], sj["mv"], sj["min_mcost"] = tr["step_smv"][:, k], tr["step_mv_in"][:, k], tr["step_min_in"][:, k]
    sj["search_range"], sj["stage"] = (R >> k, 0) if k <= REFINEMENTS else (0, 1)
    return sj


def run_a(jb, out):
    t0 = time.perf_counter()
    rc = ctx.lib.jmhip_bipred_chain(ctx.h, C.byref(cprm), jb.ctypes.data_as(C.c_void_p), len(jb), out.ctypes.data_as(C.c_void_p))
    t = time.perf_counter() - t0
    assert rc == 0
    return t


def run_b(steps, outs):
    t0 = time.perf_counter()
    for sj, out in zip(steps, outs):
        rc = ctx.lib.jmhip_bipred_search(ctx.h, C.byref(sprm), sj.ctypes.data_as(C.c_void_p), len(sj), out.ctypes.data_as(C.c_void_p))
        assert rc == 0
    return time.perf_counter() - t0


def measure(jb, tr, reps, label):
    nsteps = REFINEMENTS + 1 + SUBPEL
    steps = [step_jobs(tr, jb, k) for k in range(nsteps)]
    out_a = np.zeros(len(jb), dtype=pkg.BIPRED_CHAIN_RESULT_DTYPE)
    outs_b = [np.zeros(len(jb), dtype=pkg.BIPRED_RESULT_DTYPE) for _ in steps]
    for _ in range(3):                                  # warm-up: code objects, the context's arrays
        run_a(jb, out_a)
        run_b(steps, outs_b)
    for k in range(nsteps):                             # the same work: every per-call result is the trace's
        assert np.array_equal(outs_b[k]["mv"], out_a["step_mv_out"][:, k]) and np.array_equal(outs_b[k]["cost"], out_a["step_cost"][:, k]), k
    ta, tb = [], []
    for _ in range(reps):                               # alternate A and B
        ta.append(run_a(jb, out_a))
        tb.append(run_b(steps, outs_b))
    a, b = np.median(ta) * 1e3, np.median(tb) * 1e3
    print("%s: A one jmhip_bipred_chain call %.3f ms (min %.3f, max %.3f); B six jmhip_bipred_search calls %.3f ms (min %.3f, max %.3f); A / B = %.2f" % (
        label, a, min(ta) * 1e3, max(ta) * 1e3, b, min(tb) * 1e3, max(tb) * 1e3, a / b))


measure(jobs, trace, reps, "%dx%d, %d jobs, refinements %d, sub-pel %d, range %d, %d repetitions" % (w, h, n, REFINEMENTS, SUBPEL, R, reps))
one = slice(n // 2 + mbw // 2, n // 2 + mbw // 2 + 1)
measure(jobs[one].copy(), trace[one].copy(), 20 * reps, "n = 1 (one macroblock, as the JM binding calls it), %d repetitions" % (20 * reps))
ctx.close()
