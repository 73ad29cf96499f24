"""The bi-predictive refinement chain inside the real JM (integration/jm_shim.c, mask 0x20000 on top of the default): the first
FullPelBlockMotionBiPred call of a B macroblock's chain runs ONE jmhip_bipred_chain, the chain's other FullPelBlockMotionBiPred /
SubPelBlockSearchBiPred calls are answered from its trace, and the bitstream and reconstruction stay byte-identical to the unmodified
encoder's. A second run under the default mask pins the bookkeeping: every call the traces answered is a per-call one there, none was
lost or doubled. The cfg template of tests/test_jm_shim.py fixes BiPredMERefinements 3, BiPredMESearchRange 16 and BiPredMESubPel 2 (six
calls per chain); the other values are covered by tests/test_bipred_chain.py."""
import os
import re
import time

import pytest

from tests import test_jm_shim as shim

HAVE = shim.HAVE
BOUND = "2dfff"


def shim_has_chain_binding():
    """oracle/_ref/jm_hip is a build product: one linked from an integration/jm_shim.c older than the 0x20000 binding ignores that bit (and
    has no `bi-pred calls (chain)` row), so nothing here could be checked with it"""
    try:
        with open(os.path.join(shim.RDIR, "jm_hip"), "rb") as f:
            return b"bi-pred calls (chain)" in f.read()
    except OSError:
        return False


STALE = HAVE and not shim_has_chain_binding()

CHAIN_CASES = {
    "main_bipred": shim.CASES["main_bipred"],
    "high_bipred_weighted_t8": shim.CASES["high_bipred_weighted_t8"],
    # FullSearch with explicit bi-prediction weights on a fading clip: weight1 != weight2, so the chain's odd steps must swap them
    "full_bipred_explicit_weights": dict(search=-1, profile=77, cabac=1, t8x8=0, bframes=1, refs=2, rdopt=1, adrnd=0, yuv=1, bipred=1, wp=1, wbp=1, fade=1),
}
ROWS = ("bi-pred chain", "bi-pred calls (chain)", "FullPelBlockMotionBiPred", "SubPelBlockSearchBiPred")


def rows(stats):
    out = {}
    for k in ROWS:
        m = re.search(r"^\s*%s\s+device\s+(\d+)\s+forwarded\s+(\d+)" % re.escape(k), stats, re.M)
        assert m, (k, stats)
        out[k] = (int(m.group(1)), int(m.group(2)))
    return out


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE, reason="oracle/_ref/jm_hip did not travel")
@pytest.mark.skipif(STALE, reason="oracle/_ref/jm_hip was linked from an integration/jm_shim.c without the 0x20000 binding: rebuild it (make -C oracle ref)")
@pytest.mark.parametrize("name", list(CHAIN_CASES))
def test_bipred_chain_in_jm_is_byte_identical(tmp_path, name):
    shim.CASES[name] = CHAIN_CASES[name]
    shim.prepare(tmp_path, name)
    want = shim.run("jm_plain", tmp_path)
    t0 = time.perf_counter()
    got = shim.run("jm_hip", tmp_path, {"JMHIP_SHIM": BOUND, "JMHIP_SHIM_STATS": "1"})
    t_bound = time.perf_counter() - t0
    assert got[0] == want[0], "bitstream differs\n" + got[2]
    assert got[1] == want[1], "reconstruction differs\n" + got[2]
    b = rows(got[2])
    assert b["bi-pred chain"][0] > 0 and b["bi-pred chain"][1] == 0, b
    assert b["FullPelBlockMotionBiPred"] == (0, 0) and b["SubPelBlockSearchBiPred"] == (0, 0), b
    assert b["bi-pred calls (chain)"] == (6 * b["bi-pred chain"][0], 0), b          # 3 refinements + 1, sub-pel 2
    # the same encode under the default mask: every call answered from a trace is a per-call one there
    t0 = time.perf_counter()
    dflt = shim.run("jm_hip", tmp_path, {"JMHIP_SHIM_STATS": "1"})
    t_dflt = time.perf_counter() - t0
    assert dflt[0] == want[0] and dflt[1] == want[1]
    d = rows(dflt[2])
    print("%s: mask 0xdfff %.2f s %s; mask 0x%s %.2f s %s" % (name, t_dflt, d, BOUND, t_bound, b))
    assert d["bi-pred chain"] == (0, 0) and d["bi-pred calls (chain)"] == (0, 0), d
    assert d["FullPelBlockMotionBiPred"][1] == 0 and d["SubPelBlockSearchBiPred"][1] == 0, d
    assert d["FullPelBlockMotionBiPred"][0] == 4 * b["bi-pred chain"][0] and d["SubPelBlockSearchBiPred"][0] == 2 * b["bi-pred chain"][0], (d, b)
    assert d["FullPelBlockMotionBiPred"][0] + d["SubPelBlockSearchBiPred"][0] == b["bi-pred calls (chain)"][0], (d, b)
