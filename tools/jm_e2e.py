#!/usr/bin/env python3
"""bench.py's end-to-end legs alone (the real JM, plain and bound to libjmhip.so, on the 1080p bench clip): wall time, JM's own P-frame
timers, the shim's per-hook wall time (JMHIP_SHIM_STATS) and the byte comparison of the bitstreams.  usage: tools/jm_e2e.py [rdopt0|config3|rdopt1 ...]

config3_mask=HEX: BASELINE config 3 (EPZS, Hadamard SAD at every level, Transform8x8Mode 1, CABAC, I + P, RDOptimization 0, DisableIntraInInter 1)
with the bound encoder under JMHIP_SHIM=HEX (e.g. config3_mask=1dfff: the default mask plus the 8x8-transform frame stage, 0x10000); prints the
P-frame times, every shim row (served / forwarded) and the hook times."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402


def config3_with_mask(frames, mask):
    exes = [os.path.join(bench.ROOT, "oracle", "_ref", e) for e in ("jm_plain", "jm_hip")]
    if not all(os.path.exists(e) for e in exes):
        return None
    cfg = (bench.JM_CFG % (bench.QP, bench.QP, bench.R)).replace("RDOptimization = 1", "RDOptimization = 0") + "DisableIntraInInter = 1\n"
    for a, b in (("ProfileIDC = 66", "ProfileIDC = 100"), ("SymbolMode = 0", "SymbolMode = 1"), ("SearchMode = -1", "SearchMode = 3"),
                 ("MEDistortionFPel = 0", "MEDistortionFPel = 2"), ("Transform8x8Mode = 0", "Transform8x8Mode = 1"), ("AdaptiveRounding = 1", "AdaptiveRounding = 0")):
        assert a in cfg
        cfg = cfg.replace(a, b)
    out = {"mask": mask}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "synth1080.yuv"), "wb") as f:
            for (Y, U, V) in frames[:2]:
                f.write(Y[:bench.H_SRC].tobytes()); f.write(U[:bench.H_SRC // 2].tobytes()); f.write(V[:bench.H_SRC // 2].tobytes())
        with open(os.path.join(d, "min.cfg"), "w") as f:
            f.write(cfg)
        digests = []
        for exe, key in zip(exes, ("jm_plain", "jm_hip")):
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-d", "min.cfg"], cwd=d, env=dict(os.environ, JMHIP_SHIM=mask, JMHIP_SHIM_STATS="1"), capture_output=True, text=True, timeout=400)
            out[key + "_s"] = round(time.perf_counter() - t0, 2)
            m = re.search(r"^0001\(P\)\s+\d+\s+\d+\s+[\d.]+\s+[\d.]+\s+[\d.]+\s+(\d+)\s+(\d+)", r.stdout, re.M)
            if not m:
                sys.stderr.write("%s did not report a P frame (exit %d): %s\n" % (key, r.returncode, (r.stderr or r.stdout)[-600:]))
                return None
            out[key + "_p_frame_ms"], out[key + "_p_frame_me_ms"] = int(m.group(1)), int(m.group(2))
            with open(os.path.join(d, "out.264"), "rb") as f:
                digests.append(f.read())
            if key == "jm_hip":
                out["rows"] = {k.strip(): [int(a), int(b)] for k, a, b in re.findall(r"^  (\S[^\n]*?)\s+device\s+(\d+)\s+forwarded\s+(\d+)", r.stderr, re.M)}
                out["hooks_ms"] = {k.strip(): float(v) for k, v in re.findall(r"^  (\S[^\n]*?)\s+device\s+\d+\s+forwarded\s+\d+\s+([\d.]+) ms inside the hook", r.stderr, re.M)}
        out["bitstreams_identical"] = digests[0] == digests[1]
    return out


def main():
    which = sys.argv[1:] or ["rdopt0", "config3", "rdopt1"]
    frames = bench.synth_frames(4, False)
    for w in which:
        if w.startswith("config3_mask="):
            print(w, json.dumps(config3_with_mask(frames, w.split("=", 1)[1])), flush=True)
            continue
        r = bench.jm_end_to_end(frames, config3=(w == "config3"), rdopt1=(w == "rdopt1"))
        print(w, json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
