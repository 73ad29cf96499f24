"""The 4:4:4 frame stage without a device: the reference helper (tests/frame444_ref.py) pinned on the existing yardstick, the branch coverage of
the device cases (tests/test_frame_444_gpu.py runs CASES) asserted on the helper's output, and the new ABI entries."""
import ctypes

import numpy as np
import pytest

from tests import frame444_ref, oracle
from tests.quant_tables import scaled_quant
from tests.test_me import lambda_factors, make_mbs
from tests.test_tq import compare_lists

R = 8

# qp: (Y, Cb, Cr). Seeds were searched on the host (the helper alone) for the branches test_cases_cover_the_branches asserts.
CASES = {
    "qp12_cabac_ar": dict(w=64, h=48, qp=(12, 12, 12), cavlc=0, ar=1, far=6, given=True, t8="none"),
    "qp24_cavlc_ar_chosen": dict(w=64, h=48, qp=(24, 24, 24), cavlc=1, ar=1, far=6, given=False, t8="none"),
    "qp24_cabac_t8_some": dict(w=64, h=48, qp=(24, 24, 24), cavlc=0, ar=0, far=6, given=True, t8="some"),
    "qp28_cavlc_ar_t8_some": dict(w=64, h=48, qp=(28, 28, 28), cavlc=1, ar=1, far=6, given=True, t8="some"),
    "qp28_cabac_ar_t8_all": dict(w=64, h=48, qp=(28, 28, 28), cavlc=0, ar=1, far=6, given=True, t8="all"),
    "qp28_cavlc_t8_all": dict(w=64, h=48, qp=(28, 28, 28), cavlc=1, ar=0, far=6, given=True, t8="all"),
    "qp28_far": dict(w=64, h=48, qp=(28, 28, 28), cavlc=0, ar=1, far=90, given=True, t8="some"),
    "qp28_weighted": dict(w=64, h=48, qp=(28, 28, 28), cavlc=1, ar=1, far=6, given=True, t8="some", weighted=True),
    "qp40_cavlc_ar": dict(w=64, h=48, qp=(40, 40, 40), cavlc=1, ar=1, far=6, given=True, t8="none"),
    "qp40_cabac_t8_some": dict(w=64, h=48, qp=(40, 40, 40), cavlc=0, ar=0, far=6, given=True, t8="some"),
    "planes_at_their_own_qp": dict(w=64, h=48, qp=(36, 22, 30), cavlc=1, ar=1, far=6, given=True, t8="some"),
    "chroma_coarser_than_luma": dict(w=64, h=48, qp=(24, 38, 36), cavlc=0, ar=1, far=6, given=True, t8="some"),
    "tables_per_plane": dict(w=64, h=48, qp=(24, 20, 22), cavlc=1, ar=1, far=6, given=True, t8="some", tables=True),
    "two_refs_slots_0_3": dict(w=64, h=48, qp=(28, 26, 30), cavlc=0, ar=1, far=6, given=False, t8="none", slots=(0, 3)),
    "two_refs_slots_0_3_t8_weighted": dict(w=64, h=48, qp=(30, 28, 26), cavlc=1, ar=1, far=6, given=True, t8="some", slots=(0, 3), weighted=True),
    "tail_15_mbs": dict(w=80, h=48, qp=(26, 26, 26), cavlc=0, ar=1, far=6, given=True, t8="some"),       # a partly filled last workgroup
    "one_mb": dict(w=16, h=16, qp=(28, 24, 26), cavlc=1, ar=1, far=6, given=True, t8="all"),
}


def build_inputs(pkg, *, w, h, qp, cavlc, ar, far, given, t8, seed, weighted=False, tables=False, slots=(0,)):
    """Everything a case feeds the frame stage with, drawn on the host (no device involved)."""
    rng = np.random.default_rng(seed)
    cur, refs = frame444_ref.synth444(rng, w, h, len(slots))
    mbs = make_mbs(pkg, rng, w // 16, h // 16, 4 * far)
    n = len(mbs)
    if len(slots) > 1:                                     # jobs spread over the slots
        mbs["ref"] = np.array(slots)[rng.integers(0, len(slots), n)]
        mbs["ref"][:len(slots)] = slots[:n]
        mbs["ref_is_0"] = mbs["ref"] == slots[0]
    kw = dict(adaptive_rounding=ar, adapt_rnd_weight=4 if ar else 0, cavlc=cavlc)
    if tables:                                             # a scaling matrix and per-position offsets of its own for every record, none symmetric
        quants = [scaled_quant(pkg, q, rng, False, **kw) for q in qp]
        if t8 != "none":
            quants += [scaled_quant(pkg, q, rng, True, transform8x8_flag=1, **kw) for q in qp]
    else:
        quants = [pkg.flat_quant(q, 342, **kw) for q in qp]
        if t8 != "none":
            quants += [pkg.flat_quant(q, 342, is8x8=True, transform8x8_flag=1, **kw) for q in qp]
    quants = np.array(quants, dtype=pkg.QUANT_DTYPE)
    modes = None
    flags = np.zeros(n, bool)
    if given:
        modes = np.zeros(n, dtype=pkg.MB_MODE_DTYPE)
        modes["mode"] = rng.choice([1, 2, 3, 8], n)
        modes["b8mode"] = rng.integers(4, 8, (n, 4))
        if t8 != "none":
            flags = np.ones(n, bool) if t8 == "all" else rng.integers(0, 2, n).astype(bool)
            flags[0] = True
            if t8 == "some":
                flags[1] = False
            modes["b8mode"][flags] = 4
            modes["pad"][:, 0] = flags
    wp = None
    if weighted:                                           # different columns for Y, Cb and Cr, per slot
        wp = {"luma_round": 16, "luma_denom": 5, "chroma_round": 4, "chroma_denom": 3, "weight": np.zeros((16, 3), int), "offset": np.zeros((16, 3), int)}
        for k, s in enumerate(slots):
            wp["weight"][s], wp["offset"][s] = (29 + 3 * k, 9 - k, 7 + k), (4 - k, -2, 1 + 2 * k)
    return dict(w=w, h=h, qp=qp, ar=ar, cavlc=cavlc, cur=cur, refs=refs, slots=slots, mbs=mbs, quants=quants, modes=modes, t8=flags, wp=wp)


def case_inputs(pkg, name):
    kw = dict(CASES[name])
    seed = kw.pop("seed", 700 + sorted(CASES).index(name))
    return build_inputs(pkg, seed=seed, **kw)


def oracle_search(inp):
    """The motion search is luma-only: every job against the luma planes of ITS reference slot."""
    rps = [None] * (max(inp["slots"]) + 1)
    for s, ref in zip(inp["slots"], inp["refs"]):
        rps[s] = oracle.RefPic(ref[0])
    return oracle.me_frame(oracle.me_params(rdopt=1), rps, inp["cur"][0], inp["mbs"], -1, R, lambda_factors(inp["qp"][0]))


def ref_stacks(inp, refs=None):
    out = [None] * (max(inp["slots"]) + 1)
    for s, ref in zip(inp["slots"], refs if refs is not None else inp["refs"]):
        out[s] = frame444_ref.Ref444(*ref)
    return out


_expectations = {}


def host_expectation(pkg, name):
    """(inputs, oracle search, modes, expectation) of a case from the host alone, computed once per session and left unchanged."""
    if name not in _expectations:
        inp = case_inputs(pkg, name)
        me = oracle_search(inp)
        modes = inp["modes"] if inp["modes"] is not None else oracle.pick_modes(me["cost"])
        _expectations[name] = (inp, me, modes, frame444_ref.residual_frame444(pkg, ref_stacks(inp), inp["cur"], inp["mbs"], me["mv"], modes, inp["quants"], inp["wp"]))
    return _expectations[name]


def test_helper_plane0_equals_the_420_yardstick(pkg):
    """The helper's Y plane against oracle.residual_frame on a 4:2:0 picture with the same luma, motion and luma quantisers: recon, lists,
    cbp bits 0..3 and cbp_blk bits 0..15 (4x4- and 8x8-transform macroblocks, thresholds included)."""
    inp, me, modes, want = host_expectation(pkg, "qp28_cavlc_ar_t8_some")
    q = inp["quants"]
    quants420 = np.array([q[0], q[0], q[0], q[3]], dtype=pkg.QUANT_DTYPE)
    ref, cur = inp["refs"][0], inp["cur"]
    sub = lambda p: np.ascontiguousarray(p[::2, ::2])
    rp = oracle.RefPic(ref[0], sub(ref[1]), sub(ref[2]), yuv_format=1)
    yard = oracle.residual_frame(rp, (cur[0], sub(cur[1]), sub(cur[2])), inp["mbs"], me["mv"], modes, quants420, pkg.TQ_JOB_DTYPE, yuv_format=1)
    assert inp["t8"].any() and (~inp["t8"]).any()
    assert np.array_equal(want["recon"][0], yard["recon"][0])
    assert np.array_equal(want["pred"][0], yard["jobs_y"]["pred"])
    y = want["planes"][0]
    compare_lists(y["levels"], y["runs"], yard["luma"]["levels"], yard["luma"]["runs"], "Y lists")
    compare_lists(y["levels8"], y["runs8"], yard["luma"]["levels8"], yard["luma"]["runs8"], "Y 8x8 lists")
    assert np.array_equal(want["plane_cbp"][:, 0], yard["cbp"] & 15) and np.array_equal(want["cbp_blk"], yard["cbp_blk"] & 0xffff)
    assert (want["plane_cbp"][:, 0] != 0).any()


def test_helper_equal_planes_give_equal_results(pkg):
    """Cb = Cr = Y with three equal quantisers: three equal planes -- the lists too, wherever no threshold cleared them (there Y keeps its lists)."""
    inp = case_inputs(pkg, "qp28_cavlc_ar_t8_some")
    me = oracle_search(inp)
    same = lambda p: (p[0], p[0], p[0])
    q = inp["quants"]
    quants = np.array([q[0], q[0], q[0], q[3], q[3], q[3]], dtype=pkg.QUANT_DTYPE)
    want = frame444_ref.residual_frame444(pkg, [frame444_ref.Ref444(*same(inp["refs"][0]))], same(inp["cur"]), inp["mbs"], me["mv"], inp["modes"], quants)
    for pl in (1, 2):
        assert np.array_equal(want["recon"][pl], want["recon"][0]) and np.array_equal(want["pred"][pl], want["pred"][0])
        for k in ("plane_cbp", "plane_cbp_blk", "cleared8", "cleared_mb"):
            assert np.array_equal(want[k][:, pl], want[k][:, 0]), k
        for k in ("coeff_cost", "nonzero", "recon", "fadjust"):
            assert np.array_equal(want["planes"][pl][k], want["planes"][0][k]), k
    assert np.array_equal(want["planes"][1]["levels"], want["planes"][2]["levels"])
    y, cb, kept = want["planes"][0], want["planes"][1], 0
    for i in range(len(inp["mbs"])):
        for b8 in range(4):
            if want["cleared_mb"][i, 0] == 0 and not (want["cleared8"][i, 0] >> b8) & 1:
                kept += 1
                assert np.array_equal(cb["levels"][i, 4 * b8:4 * b8 + 4], y["levels"][i, 4 * b8:4 * b8 + 4]) and np.array_equal(cb["levels8"][i, b8], y["levels8"][i, b8])
    assert kept > 0
    assert np.array_equal(want["cbp"], want["plane_cbp"][:, 0])


def coverage(inp, want):
    """Which branches of the per-plane bookkeeping the helper's output shows for one case."""
    t8, cov = want["t8"], {}
    g8, gmb, pc = want["cleared8"], want["cleared_mb"], want["plane_cbp"]
    for pl, nm in enumerate("Y Cb Cr".split()):
        # one 8x8 block cleared by the block threshold although dct returned non-zero, while another block of the macroblock stays coded
        nzb = want["nonzero_before"][pl]
        nz8 = np.where(t8[:, None], nzb[:, :4] != 0, (nzb.reshape(-1, 4, 4) != 0).any(axis=2))
        hit = np.array([[(g8[i, pl] >> b) & 1 for b in range(4)] for i in range(len(t8))], bool) & nz8
        cov["block_threshold_%s" % nm] = bool((hit.any(axis=1) & (pc[:, pl] != 0)).any())
        cov["dct_8x8_nonzero_%s_%s" % (nm, "cavlc" if inp["cavlc"] else "cabac")] = bool((nz8[t8]).any())
        if pl:                                             # a cleared Cb / Cr block whose lists were non-empty before the zeroing (dct returned non-zero)
            coded = np.array([[(pc[i, pl] >> b) & 1 for b in range(4)] for i in range(len(t8))], bool)
            cov["chroma_lists_zeroed"] = cov.get("chroma_lists_zeroed", False) or bool((nz8 & ~coded).any())
    chroma_mb = ((gmb[:, 1] == 1) & (g8[:, 1] != 15)) | ((gmb[:, 2] == 1) & (g8[:, 2] != 15))     # the macroblock threshold decided, not the block one
    cov["mb_threshold_chroma_while_Y_coded"] = bool((chroma_mb & (pc[:, 0] != 0)).any())
    cov["mb_threshold_Y_while_chroma_coded"] = bool(((gmb[:, 0] == 1) & (g8[:, 0] != 15) & ((pc[:, 1] | pc[:, 2]) != 0)).any())
    cov["cbp_differs_from_Y_cbp"] = bool((want["cbp"] != pc[:, 0]).any())
    return cov


def test_cases_cover_the_branches(pkg):
    """No GPU: over the device cases, every branch of LumaResidualCoding's 4:4:4 bookkeeping occurs IN THE HELPER'S OUTPUT."""
    seen = {}
    for name in sorted(CASES):
        inp, me, modes, want = host_expectation(pkg, name)
        for k, v in coverage(inp, want).items():
            seen[k] = seen.get(k, False) or v
        for pl in (1, 2):                                  # zeroed means zeroed: a Cb / Cr block outside the plane's cbp has empty lists
            r = want["planes"][pl]
            for i in range(len(inp["mbs"])):
                for b8 in range(4):
                    if not (want["plane_cbp"][i, pl] >> b8) & 1:
                        assert not r["levels"][i, 4 * b8:4 * b8 + 4].any() and not r["levels8"][i, b8].any() and not r["runs"][i, 4 * b8:4 * b8 + 4].any()
    for nm in ("Y", "Cb", "Cr"):
        assert seen.get("dct_8x8_nonzero_%s_cavlc" % nm) and seen.get("dct_8x8_nonzero_%s_cabac" % nm), nm
    assert all(seen.values()), "branches the cases do not reach: %s" % [k for k, v in seen.items() if not v]


def test_abi_of_the_444_entries(pkg):
    """The three new symbols, the record's size, and no silent success without a device (as tests/test_abi.py shows for the others)."""
    pkg.build_library()
    lib = pkg.load_library()
    for name in ("jmhip_interp_chroma444", "jmhip_residual_records444_download", "jmhip_residual_records8_444_download"):
        assert hasattr(lib, name), name
        assert name in pkg.declared_symbols()
    assert lib.jmhip_sizeof(26) == pkg.MB_RESIDUAL444_DTYPE.itemsize == 4896 and pkg.MB_RESIDUAL444_DTYPE.itemsize % 16 == 0
    assert lib.jmhip_sizeof(25) == -1 and lib.jmhip_sizeof(27) == -1      # 25 stays unassigned, as before
    # a NULL context is refused by every entry (JMHIP_ERR_ARG = 1), before any device work
    rec = np.zeros(1, pkg.MB_RESIDUAL444_DTYPE)
    assert lib.jmhip_interp_chroma444(None, 0) == 1
    assert lib.jmhip_residual_records444_download(None, rec.ctypes.data_as(ctypes.c_void_p), 1) == 1
    assert lib.jmhip_residual_records8_444_download(None, rec.ctypes.data_as(ctypes.c_void_p), 1) == 1
    # without a GPU a 4:4:4 context cannot be made, so the calls raise (never fall back to the CPU); with one, they work on it
    try:
        ctx = pkg.Context(64, 48, yuv_format=3)
    except pkg.JmhipError as e:
        assert "HIP" in str(e) or "device" in str(e)
        return
    try:
        for call in (lambda: ctx.interp_chroma444(0), lambda: ctx.residual_records444(1), lambda: ctx.residual_records8_444(1)):
            with pytest.raises(pkg.JmhipError):            # no reference picture / no frame stage yet
                call()
    finally:
        ctx.close()
