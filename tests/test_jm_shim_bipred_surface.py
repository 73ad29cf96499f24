"""Bi-predictive distortion surfaces inside the real JM (integration/jm_shim.c, mask 0x40000 on top of the default): the bi-pred walks of EPZS,
UMHexagonS and simplified UMHexagonS stay JM's code, their computeBiPredSAD1/2 / computeBiPredSATD1 calls at integer positions are answered from
jmhip_bipred_surface, and the bitstream and reconstruction stay byte-identical to the unmodified encoder's. A second run under the default mask
pins that the bit is opt-in: same output, both new statistics rows empty. The cfg template of tests/test_jm_shim.py fixes BiPredMERefinements 3,
BiPredMESearchRange 16 and BiPredMESubPel 2, so every B macroblock runs four integer walks per searched list. QCIF, three pictures, one of them B."""
import os
import re

import pytest

from tests import test_jm_shim as shim

HAVE = shim.HAVE
BOUND = "4dfff"
ROWS = ("EPZS_UMHex_bipred_walks", "computeBiPred")


def shim_has_surface_binding():
    """oracle/_ref/jm_hip is a build product: one linked from an integration/jm_shim.c older than the 0x40000 binding ignores that bit (and has
    no `EPZS_UMHex_bipred_walks` row), so nothing here could be checked with it"""
    try:
        with open(os.path.join(shim.RDIR, "jm_hip"), "rb") as f:
            return b"EPZS_UMHex_bipred_walks" in f.read()
    except OSError:
        return False


STALE = HAVE and not shim_has_surface_binding()

B = dict(profile=77, cabac=1, t8x8=0, bframes=1, refs=2, rdopt=1, adrnd=0, yuv=1, bipred=1)
SURFACE_CASES = {
    "epzs_bipred": dict(B, search=3),
    "umhex_bipred": dict(B, search=1),
    "umhexsmp_bipred": dict(B, search=2),
    # explicit bi-prediction weights on a fading clip: computeBiPredSAD2 with weight1 != weight2
    "epzs_bipred_explicit_weights": dict(B, search=3, wp=1, wbp=1, fade=1),
    # the 8x8 transform with the Hadamard metric at integer positions: computeBiPredSATD1, the 8x8 entries of the surface
    "epzs_bipred_satd_t8": dict(B, search=3, profile=100, t8x8=1, fpel=2),
}


def rows(stats):
    out = {}
    for k in ROWS:
        m = re.search(r"^\s*%s\s+device\s+(\d+)\s+forwarded\s+(\d+)" % re.escape(k), stats, re.M)
        assert m, (k, stats)
        out[k] = (int(m.group(1)), int(m.group(2)))
    return out


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE, reason="oracle/_ref/jm_hip did not travel")
@pytest.mark.skipif(STALE, reason="oracle/_ref/jm_hip was linked from an integration/jm_shim.c without the 0x40000 binding: rebuild it (make -C oracle ref)")
@pytest.mark.parametrize("name", list(SURFACE_CASES))
def test_bipred_surfaces_in_jm_are_byte_identical(tmp_path, name):
    shim.CASES[name] = SURFACE_CASES[name]
    shim.prepare(tmp_path, name, frames=2)                  # I, P and the B picture between them
    want = shim.run("jm_plain", tmp_path)
    got = shim.run("jm_hip", tmp_path, {"JMHIP_SHIM": BOUND, "JMHIP_SHIM_STATS": "1"})
    assert got[0] == want[0], "bitstream differs\n" + got[2]
    assert got[1] == want[1], "reconstruction differs\n" + got[2]
    b = rows(got[2])
    print("%s: mask 0x%s %s" % (name, BOUND, b))
    assert b["EPZS_UMHex_bipred_walks"][0] > 0, b
    assert b["computeBiPred"][0] > 0, b
    # the same encode under the default mask: the bit is opt-in
    dflt = shim.run("jm_hip", tmp_path, {"JMHIP_SHIM_STATS": "1"})
    assert dflt[0] == want[0] and dflt[1] == want[1]
    d = rows(dflt[2])
    assert d["EPZS_UMHex_bipred_walks"] == (0, 0) and d["computeBiPred"] == (0, 0), d
