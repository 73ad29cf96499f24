"""Times the 4:2:2 frame stage at 1080p (1920x1088) and at 3840x2160 (BASELINE config 5's picture), 4x4-transform only and with every macroblock
on the 8x8 transform: the fused stage (frame_fused_kernel<false, true> / <true, true>) and the separate kernels (JMHIP_FRAME_FUSED=0: mc_kernel,
tq_luma4x4_kernel, tq_luma8x8_kernel, tq_chroma_kernel, finalize_kernel), alternating in one process so that both see the same clocks. The
warm-up also asserts that the two forms agree. Run it under `rocprofv3 --kernel-trace --stats -- python tools/time_frame_422.py` for per-kernel
times; it prints the median host-side time of each form too.
Usage: python tools/time_frame_422.py [iterations [cavlc [1080|2160]]]   (no size: both)"""
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
pkg = ge._load_pkg()
from tests.test_frame import synth
from tests.test_me import lambda_factors

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
cavlc = int(sys.argv[2]) if len(sys.argv) > 2 else 0
only = sys.argv[3] if len(sys.argv) > 3 else ""
R, qp = 8, 28
for w, h in ((1920, 1088), (3840, 2160)):
    if only and not str(h).startswith(only[:3]):
        continue
    rng = np.random.default_rng(0)
    cur, ref = synth(rng, w, h, 2)
    ctx = pkg.Context(w, h, yuv_format=2, max_refs=1, search_range=R)
    ctx.ref_upload(0, *ref)
    ctx.interp_luma(0)
    ctx.interp_chroma(0)
    ctx.cur_upload(*cur)
    mbw, mbh = w // 16, h // 16
    n = mbw * mbh
    mbs = np.zeros(n, dtype=pkg.ME_MB_DTYPE)
    mbs["mb_x"], mbs["mb_y"], mbs["ref_is_0"] = np.arange(n) % mbw, np.arange(n) // mbw, 1
    mbs["pred_mv"] = rng.integers(-24, 25, (n, 41, 2))
    prm = pkg.MeParams()
    prm.search_mode, prm.search_range, prm.rdopt = 0, R, 1
    prm.level_mv_min, prm.level_mv_max = -511, 511
    prm.lambda_[0], prm.lambda_[1], prm.lambda_[2] = lambda_factors(qp)
    prm.subpel, prm.partition_mask = 1, (1 << 41) - 1
    ctx.me_frame(prm, mbs)
    kw = dict(adaptive_rounding=1, adapt_rnd_weight=4, cavlc=cavlc)
    quants = np.array([pkg.flat_quant(qp, 342, **kw), pkg.flat_quant(qp, 342, **kw), pkg.flat_quant(qp + 3, 342, **kw),
                       pkg.flat_quant(qp, 342, is8x8=True, transform8x8_flag=1, **kw)], dtype=pkg.QUANT_DTYPE)
    ctx.frame_keep_prediction()
    for t8 in (0, 1):
        modes = np.zeros(n, dtype=pkg.MB_MODE_DTYPE)
        modes["mode"] = rng.choice([1, 2, 3, 8], n)
        modes["b8mode"] = 4 if t8 else rng.integers(4, 8, (n, 4))
        modes["pad"][:, 0] = t8
        out = {}
        for form in ("fused", "separate"):                 # warm-up, and the two forms agree
            os.environ["JMHIP_FRAME_FUSED"] = "1" if form == "fused" else "0"
            ctx.residual_frame(quants, modes)
            got = ctx.residual_download(n)
            out[form] = (got["cbp"], got["cbp_blk"], got["chroma"]["ret"]) + tuple(ctx.recon_download())
        assert all(np.array_equal(a, b) for a, b in zip(out["fused"], out["separate"])), "fused and separate frame stages differ"
        ts = {"fused": [], "separate": []}
        for it in range(iters):
            for form in (("fused", "separate") if it % 2 == 0 else ("separate", "fused")):
                os.environ["JMHIP_FRAME_FUSED"] = "1" if form == "fused" else "0"
                ctx.sync()
                t = time.perf_counter()
                ctx.residual_frame(quants, modes)
                ctx.sync()
                ts[form].append(time.perf_counter() - t)
        print("%dx%d 4:2:2, %d macroblocks, %s, %s: host wall per frame stage (median of %d): fused %.3f ms, separate %.3f ms"
              % (w, h, n, "all 8x8 transform" if t8 else "4x4 transform only", "CAVLC" if cavlc else "CABAC", iters,
                 1e3 * float(np.median(ts["fused"])), 1e3 * float(np.median(ts["separate"]))), flush=True)
    ctx.close()
