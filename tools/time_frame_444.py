"""Times the 4:4:4 frame stage (frame444.hip: frame_fused444_kernel<false> / <true>) at 1080p (1920x1088) and at 3840x2160, 4x4-transform only and
with every macroblock on the 8x8 transform, and -- as context, on the same picture size and luma in the same process -- the fused 4:2:0 stage
(frame_fused_kernel<false, false> / <true, false>). There is no other 4:4:4 path to compare with. Times are the context's stream events round the
stage's one launch (jmhip_timing_read, stage "mc"); run it under `rocprofv3 --kernel-trace --stats -- python tools/time_frame_444.py` for per-kernel
times (the trace tells the picture sizes apart by grid size). The warm-up checks the 4:4:4 stage's Y plane against the 4:2:0 stage's luma.
Usage: python tools/time_frame_444.py [iterations [cavlc [1080|2160]]]   (no size: both)"""
import os
import sys

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
pkg = ge._load_pkg()
from tests.frame444_ref import synth444
from tests.test_me import lambda_factors

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
cavlc = int(sys.argv[2]) if len(sys.argv) > 2 else 0
only = sys.argv[3] if len(sys.argv) > 3 else ""
R, qp = 8, 28
REC, REC8 = pkg.MB_RESIDUAL444_DTYPE.itemsize, pkg.MB_RESIDUAL8_DTYPE.itemsize
for w, h in ((1920, 1088), (3840, 2160)):
    if only and not str(h).startswith(only[:3]):
        continue
    rng = np.random.default_rng(0)
    cur, refs = synth444(rng, w, h)
    ref = refs[0]
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
    kw = dict(adaptive_rounding=1, adapt_rnd_weight=4, cavlc=cavlc)
    q4, q8 = pkg.flat_quant(qp, 342, **kw), pkg.flat_quant(qp, 342, is8x8=True, transform8x8_flag=1, **kw)
    sub = lambda p: np.ascontiguousarray(p[::2, ::2])
    ctxs = {}
    for fmt in (3, 1):
        ctx = pkg.Context(w, h, yuv_format=fmt, max_refs=1, search_range=R)
        planes = lambda pic: pic if fmt == 3 else (pic[0], sub(pic[1]), sub(pic[2]))
        ctx.ref_upload(0, *planes(ref))
        ctx.interp_luma(0)
        ctx.interp_chroma444(0) if fmt == 3 else ctx.interp_chroma(0)
        ctx.cur_upload(*planes(cur))
        ctx.me_frame(prm, mbs)
        ctx.frame_keep_prediction()
        ctx.timing_select(["mc"])
        ctxs[fmt] = ctx
    quants = {3: np.array([q4, q4, q4, q8, q8, q8], dtype=pkg.QUANT_DTYPE), 1: np.array([q4, q4, pkg.flat_quant(qp + 3, 342, **kw), q8], dtype=pkg.QUANT_DTYPE)}
    for t8 in (0, 1):
        modes = np.zeros(n, dtype=pkg.MB_MODE_DTYPE)
        modes["mode"] = rng.choice([1, 2, 3, 8], n)
        modes["b8mode"] = 4 if t8 else rng.integers(4, 8, (n, 4))
        modes["pad"][:, 0] = t8
        luma = {}
        for fmt, ctx in ctxs.items():                      # warm-up, and the two formats agree on the luma plane
            ctx.residual_frame(quants[fmt], modes)
            got = ctx.residual_download(n, want_results=False)
            luma[fmt] = (got["cbp"] & 15 if fmt == 1 else ctx.residual_records444(n)["plane_cbp"][:, 0], got["cbp_blk"] & 0xffff, ctx.recon_download()[0])
        assert all(np.array_equal(a, b) for a, b in zip(luma[3], luma[1])), "the Y plane of the 4:4:4 stage differs from the 4:2:0 stage's luma"
        us = {}
        for fmt, ctx in ctxs.items():
            ctx.timing_enable(True)
            ctx.timing_read()
            for it in range(iters):
                ctx.residual_frame(quants[fmt], modes)
            ms, launches = ctx.timing_read()["mc"]
            ctx.timing_enable(False)
            assert launches == iters
            us[fmt] = 1e3 * ms / launches
        written = REC + (3 * REC8 if t8 else 0) + 768 + 768 + 8 + 16       # record (+ side records), recon, prediction picture, mode, coded bits
        print("%dx%d, %d macroblocks, %s, %s: per launch (mean of %d, stream events): 4:4:4 frame_fused444_kernel %.1f us, 4:2:0 frame_fused_kernel %.1f us, "
              "ratio %.2f; 4:4:4 bytes written per macroblock %d (%.1f MB per picture, %.0f GB/s)"
              % (w, h, n, "all 8x8 transform" if t8 else "4x4 transform only", "CAVLC" if cavlc else "CABAC", iters, us[3], us[1], us[3] / us[1],
                 written, written * n / 1e6, written * n / us[3] / 1e3), flush=True)
    for ctx in ctxs.values():
        ctx.close()
