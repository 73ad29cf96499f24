"""The slice-level frame stage with the 8x8 transform inside the real JM (integration/jm_shim.c, mask 0x10000 on top of the default): JM's
LumaPrediction / dct_8x8 / dct_4x4 / ChromaPrediction4x4 / dct_chroma calls of a Transform8x8Mode P slice are answered from the device's
three passes -- the 8x8-transform P8x8 candidate, the 4x4-transform P8x8 candidate, the decision -- and the bitstream and reconstruction stay
byte-identical to the unmodified encoder's. A second run under the default mask (frame stage left in JM) pins the bookkeeping: every
transform call of the P pictures moved to the records, none was lost or doubled."""
import os
import re
import time

import pytest

from tests import test_jm_shim as shim

HAVE = shim.HAVE
BOUND = "1dfff"


def shim_has_t8_binding():
    """oracle/_ref/jm_hip is a build product: one linked from an integration/jm_shim.c older than the 0x10000 binding ignores that bit (and
    has no `dct_8x8 (slice records)` row), so nothing here could be checked with it"""
    try:
        with open(os.path.join(shim.RDIR, "jm_hip"), "rb") as f:
            return b"dct_8x8 (slice records)" in f.read()
    except OSError:
        return False


STALE = HAVE and not shim_has_t8_binding()

T8_CASES = {
    "t8frame_epzs_cabac": dict(search=3, profile=100, cabac=1, t8x8=1, bframes=0, refs=2, rdopt=0, adrnd=0, yuv=1, noi=1, qp=32),
    "t8frame_umhex_cavlc": dict(search=1, profile=100, cabac=0, t8x8=1, bframes=0, refs=2, rdopt=0, adrnd=0, yuv=1, noi=1, qp=30),     # interleaved lists
    "t8frame_fastfull_t8only_adrnd": dict(search=0, profile=100, cabac=1, t8x8=2, bframes=0, refs=2, rdopt=0, adrnd=1, yuv=1, noi=1, qp=30),
    "t8frame_epzs_5ref": dict(search=3, profile=100, cabac=1, t8x8=1, bframes=0, refs=5, rdopt=0, adrnd=0, yuv=1, noi=1, frames=7, qp=32),
    "t8frame_full_slices_one_call_cavlc": dict(search=-1, profile=100, cabac=0, t8x8=1, bframes=0, refs=2, rdopt=0, adrnd=0, yuv=1, noi=1, slicemode=1, slicearg=40, qp=34),
    # (no scaling-matrix case: the test matrices give Cb and Cr lists of their own, and the frame stage takes one chroma quantiser per slice)
}
ROWS = ("frame stage of P slices", "dct_8x8 (slice records)", "dct_4x4 (slice records)", "dct_chroma (slice records)", "LumaPrediction (slice)",
        "ChromaPrediction4x4 (slice)", "dct_8x8", "dct_4x4", "BlockMotionSearch")


def rows(stats):
    out = {}
    for k in ROWS:
        m = re.search(r"^\s*%s\s+device\s+(\d+)\s+forwarded\s+(\d+)" % re.escape(k), stats, re.M)
        assert m, (k, stats)
        out[k] = (int(m.group(1)), int(m.group(2)))
    return out


def check_bound(name, tmp_path, nframes, **kw):
    shim.CASES[name] = T8_CASES.get(name, kw.get("cfg"))
    shim.prepare(tmp_path, name, frames=nframes, **kw.get("size", {}))
    t0 = time.perf_counter()
    want = shim.run("jm_plain", tmp_path)
    t_plain = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = shim.run("jm_hip", tmp_path, {"JMHIP_SHIM": BOUND, "JMHIP_SHIM_STATS": "1"})
    t_hip = time.perf_counter() - t0
    assert got[0] == want[0], "bitstream differs\n" + got[2]
    assert got[1] == want[1], "reconstruction differs\n" + got[2]
    b = rows(got[2])
    print(name, b)
    assert b["frame stage of P slices"][0] == nframes - 1, b
    for k in ("dct_8x8 (slice records)", "dct_4x4 (slice records)", "dct_chroma (slice records)", "LumaPrediction (slice)", "ChromaPrediction4x4 (slice)"):
        assert b[k][1] == 0, (k, b)
    assert b["dct_8x8 (slice records)"][0] > 0 and b["BlockMotionSearch"][1] == 0, b
    return b, got[2], t_plain, t_hip


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE, reason="oracle/_ref/jm_hip did not travel")
@pytest.mark.skipif(STALE, reason="oracle/_ref/jm_hip was linked from an integration/jm_shim.c without the 0x10000 binding: rebuild it (make -C oracle ref)")
@pytest.mark.parametrize("name", list(T8_CASES))
def test_t8_frame_stage_in_jm_is_byte_identical(tmp_path, name):
    nframes = T8_CASES[name].get("frames", 4)
    b, _, _, _ = check_bound(name, tmp_path, nframes)
    mbs = (nframes - 1) * 99
    assert b["dct_chroma (slice records)"] == (2 * mbs, 0) and b["ChromaPrediction4x4 (slice)"] == (8 * mbs, 0), b
    if T8_CASES[name]["t8x8"] == 2:
        assert b["dct_4x4 (slice records)"][0] == 0
    # the same encode under the default mask: the frame stage stays JM's, so every transform call the bound run answered from the records is a
    # per-call one there
    d = rows(shim.run("jm_hip", tmp_path, {"JMHIP_SHIM_STATS": "1"})[2])
    assert d["frame stage of P slices"][0] == 0 and d["dct_8x8 (slice records)"] == (0, 0), d
    for k in ("dct_8x8", "dct_4x4"):
        assert sum(d[k]) == sum(b[k]) + b[k + " (slice records)"][0], (k, d, b)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE, reason="oracle/_ref/jm_hip did not travel")
@pytest.mark.skipif(STALE, reason="oracle/_ref/jm_hip was linked from an integration/jm_shim.c without the 0x10000 binding: rebuild it (make -C oracle ref)")
def test_t8_frame_stage_in_jm_1080p_config3(tmp_path):
    """BASELINE config 3 through the real encoder: 1920x1080, EPZS +-32, Hadamard SAD at every level, Transform8x8Mode 1, I + P, low-complexity
    decision without intra in P: the P picture's search and all three frame-stage passes on the device."""
    cfg = dict(search=3, profile=100, cabac=1, t8x8=1, bframes=0, refs=1, rdopt=0, adrnd=0, yuv=1, noi=1, fpel=2)
    b, stats, t_plain, t_hip = check_bound("t8frame_1080p_config3", tmp_path, 2, cfg=cfg, size=dict(w=1920, h=1080, R=32))
    hook = re.search(r"^\s*frame stage of P slices\s+device\s+\d+\s+forwarded\s+\d+\s+([\d.]+) ms inside the hook", stats, re.M)
    print("1080p config 3, I+P: jm_plain %.1f s, jm_hip (mask 0x%s) %.1f s; frame stage of the P slice %s ms; %s" % (
        t_plain, BOUND, t_hip, hook.group(1) if hook else "?", b))
