#!/usr/bin/env python3
"""What the bi-predictive distortion surfaces (jmhip_bipred_surface; shim mask 0x40000) cost and serve.
  1  the n = 1 call the JM binding makes (job upload, kernel, surface download, synchronise) at R = 16 and R = 32, both kinds, plain and
     weighted, on a 1080p context: median host time round the call;
  2  the real JM bound to libjmhip.so on the 1080p bench clip, I + P + B with BiPredMotionEstimation (refinements 3, range 16, sub-pel 2),
     EPZS and UMHexagonS, under the default mask and under 0x4dfff on the same host: JM's own B-frame time, the shim's walk / computeBiPred
     rows (served, forwarded), the time inside the surface calls, and the byte comparison of the two bitstreams.
usage: tools/time_bipred_surface.py [calls|jm ...]   (default: both)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
import __graft_entry__ as ge  # noqa: E402


def time_calls(reps=200):
    pkg = ge._load_pkg()
    from tests.test_me import make_pair
    w, h = 1920, 1088
    rng = np.random.default_rng(5)
    cur, ref1 = make_pair(rng, w, h, "shift")
    _, ref2 = make_pair(rng, w, h, "shift")
    ctx = pkg.Context(w, h, yuv_format=0, max_refs=2, search_range=32)
    ctx.ref_upload(0, ref1)
    ctx.ref_upload(1, ref2)
    ctx.cur_upload(cur)
    for R in (16, 32):
        for kind, nv in ((0, 64), (1, 20)):
            for wp in (0, 1):
                job = np.zeros(1, dtype=pkg.BIPRED_SURFACE_JOB_DTYPE)
                job["mb_x"], job["mb_y"], job["ref2"], job["R"], job["s_mv"], job["cx"], job["cy"] = 60, 34, 1, R, (3, -2), 2, 1
                if wp:
                    job["wp"], job["weight1"], job["weight2"], job["offset_bi"], job["wp_round"], job["wp_denom"] = 1, 37, 24, -3, 16, 5
                out = np.zeros((2 * R + 1) ** 2 * nv, np.uint16)
                ts = []
                for k in range(reps + 10):
                    t0 = time.perf_counter()
                    rc = ctx.lib.jmhip_bipred_surface(ctx.h, kind, job.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p))
                    ts.append(time.perf_counter() - t0)
                    assert rc == 0
                ts = np.array(ts[10:]) * 1e6
                print("calls", json.dumps({"R": R, "kind": ("sad_rows", "satd_blocks")[kind], "weighted": wp, "surface_bytes": int(out.nbytes),
                                           "median_us": round(float(np.median(ts)), 1), "min_us": round(float(ts.min()), 1), "p90_us": round(float(np.percentile(ts, 90)), 1),
                                           "reps": reps}), flush=True)
    ctx.close()


def jm_b_frame(frames, search, mask):
    exe = os.path.join(bench.ROOT, "oracle", "_ref", "jm_hip")
    if not os.path.exists(exe):
        return None
    cfg = (bench.JM_CFG % (bench.QP, bench.QP, bench.R)).replace("RDOptimization = 1", "RDOptimization = 0")
    for a, b in (("ProfileIDC = 66", "ProfileIDC = 77"), ("SymbolMode = 0", "SymbolMode = 1"), ("SearchMode = -1", "SearchMode = %d" % search),
                 ("NumberBFrames = 0", "NumberBFrames = 1\nFrameSkip = 1\nQPBSlice = %d" % bench.QP), ("NumberReferenceFrames = 1", "NumberReferenceFrames = 2")):
        assert a in cfg
        cfg = cfg.replace(a, b)
    cfg += "BiPredMotionEstimation = 1\nBiPredMERefinements = 3\nBiPredMESearchRange = 16\nBiPredMESubPel = 2\n"
    out = {"search": search, "mask": mask}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "synth1080.yuv"), "wb") as f:
            for (Y, U, V) in frames[:3]:
                f.write(Y[:bench.H_SRC].tobytes()); f.write(U[:bench.H_SRC // 2].tobytes()); f.write(V[:bench.H_SRC // 2].tobytes())
        with open(os.path.join(d, "min.cfg"), "w") as f:
            f.write(cfg)
        t0 = time.perf_counter()
        r = subprocess.run([exe, "-d", "min.cfg"], cwd=d, env=dict(os.environ, JMHIP_SHIM=mask, JMHIP_SHIM_STATS="1"), capture_output=True, text=True, timeout=500)
        out["wall_s"] = round(time.perf_counter() - t0, 2)
        m = re.search(r"^\d+\(B\)\s+\d+\s+\d+\s+[\d.]+\s+[\d.]+\s+[\d.]+\s+(\d+)\s+(\d+)", r.stdout, re.M)
        if not m:
            sys.stderr.write("no B frame reported (exit %d): %s\n" % (r.returncode, (r.stderr or r.stdout)[-600:]))
            return None
        out["b_frame_ms"], out["b_frame_me_ms"] = int(m.group(1)), int(m.group(2))
        rows = {k.strip(): [int(a), int(b)] for k, a, b in re.findall(r"^  (\S[^\n]*?)\s+device\s+(\d+)\s+forwarded\s+(\d+)", r.stderr, re.M)}
        out["rows"] = {k: rows[k] for k in ("EPZS_UMHex_bipred_walks", "computeBiPred", "EPZS_UMHex_integer_walks", "computeSAD") if k in rows}
        out["hooks_ms"] = {k.strip(): float(v) for k, v in re.findall(r"^  (\S[^\n]*?)\s+device\s+\d+\s+forwarded\s+\d+\s+([\d.]+) ms inside the hook", r.stderr, re.M)}
        m = re.search(r"bi-pred surfaces: (\d+) fetched", r.stderr)
        out["surfaces_fetched"] = int(m.group(1)) if m else 0
        with open(os.path.join(d, "out.264"), "rb") as f:
            return out, f.read()


def time_jm():
    frames = bench.synth_frames(4, False)
    for search in (3, 1):
        res = [jm_b_frame(frames, search, mask) for mask in ("dfff", "4dfff")]
        if None in res:
            continue
        for r, _ in res:
            print("jm", json.dumps(r), flush=True)
        print("jm", json.dumps({"search": search, "bitstreams_identical": res[0][1] == res[1][1]}), flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["calls", "jm"]
    if "calls" in which:
        time_calls()
    if "jm" in which:
        time_jm()
