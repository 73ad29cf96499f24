"""Times the frame stage on a 1080p picture whose every macroblock uses the 8x8 transform: the fused stage (frame_fused_kernel<true>)
and the separate kernels (JMHIP_FRAME_FUSED=0: mc_kernel, tq_luma8x8_kernel, tq_chroma420_kernel, finalize_kernel), alternating in one
process so that both see the same clocks. Run it under `rocprofv3 --kernel-trace --stats -- python tools/time_frame_t8.py` for per-kernel
times; it prints the host-side HIP-event time of each form too.
Usage: python tools/time_frame_t8.py [iterations [cavlc]]"""
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
pkg = ge._load_pkg()
from tests.test_frame import synth
from tests.test_me import lambda_factors, make_mbs

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
cavlc = int(sys.argv[2]) if len(sys.argv) > 2 else 0
w, h, R, qp = 1920, 1088, 8, 28
rng = np.random.default_rng(0)
cur, ref = synth(rng, w, h, 1)
ctx = pkg.Context(w, h, yuv_format=1, max_refs=1, search_range=R)
ctx.ref_upload(0, *ref)
ctx.interp_luma(0)
ctx.interp_chroma(0)
ctx.cur_upload(*cur)
mbs = make_mbs(pkg, rng, w // 16, h // 16, 24)
n = len(mbs)
prm = pkg.MeParams()
prm.search_mode, prm.search_range, prm.rdopt = -1, R, 1
prm.level_mv_min, prm.level_mv_max = -511, 511
prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lambda_factors(qp)
prm.transform8x8_mode, prm.subpel, prm.partition_mask = 1, 1, (1 << 41) - 1
ctx.me_frame(prm, mbs)
kw = dict(adaptive_rounding=1, adapt_rnd_weight=4, cavlc=cavlc)
quants = np.array([pkg.flat_quant(qp, 342, **kw), pkg.flat_quant(qp, 342, **kw), pkg.flat_quant(qp + 3, 342, **kw),
                   pkg.flat_quant(qp, 342, is8x8=True, transform8x8_flag=1, **kw)], dtype=pkg.QUANT_DTYPE)
modes = np.zeros(n, dtype=pkg.MB_MODE_DTYPE)
modes["mode"] = rng.choice([1, 2, 3, 8], n)
modes["b8mode"] = 4
modes["pad"][:, 0] = 1
ctx.frame_keep_prediction()
out = {}
for form in ("fused", "separate"):                     # warm-up, and the two forms agree
    os.environ["JMHIP_FRAME_FUSED"] = "1" if form == "fused" else "0"
    ctx.residual_frame(quants, modes)
    out[form] = (ctx.residual_download(n)["cbp_blk"], ctx.recon_download()[0])
assert all(np.array_equal(a, b) for a, b in zip(out["fused"], out["separate"])), "fused and separate frame stages differ"
tot = {"fused": 0.0, "separate": 0.0}
for it in range(iters):
    for form in (("fused", "separate") if it % 2 == 0 else ("separate", "fused")):
        os.environ["JMHIP_FRAME_FUSED"] = "1" if form == "fused" else "0"
        ctx.sync()
        t = time.perf_counter()
        ctx.residual_frame(quants, modes)
        ctx.sync()
        tot[form] += time.perf_counter() - t
print("1080p, %d macroblocks, all 8x8 transform, %s: host wall per frame stage: fused %.3f ms, separate %.3f ms (%d iterations each)"
      % (n, "CAVLC" if cavlc else "CABAC", 1e3 * tot["fused"] / iters, 1e3 * tot["separate"] / iters, iters))
ctx.close()
