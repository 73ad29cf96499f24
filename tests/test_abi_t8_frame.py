"""The 8x8-transform P8x8 candidate hand-over (jmhip_slice_to_frame_candidates8) and the per-block references of that pass
(jmhip_slice_ref8ts_download): declared in include/jmhip.h, exported by libjmhip.so, bound in Python; additive, ABI version 1 (no GPU)."""
import ctypes

NEW = ("jmhip_slice_to_frame_candidates8", "jmhip_slice_ref8ts_download")


def test_t8_candidate_entry_points_are_declared_and_exported(pkg):
    lib = pkg.load_library()
    declared = pkg.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert lib.jmhip_abi_version() == 1
    assert hasattr(pkg.Context, "slice_to_frame_candidates8") and hasattr(pkg.Context, "slice_ref8ts")


def test_t8_candidate_entry_points_reject_a_null_context(pkg):
    lib = pkg.load_library()
    slots = (ctypes.c_int32 * 2)(0, 1)
    out = (ctypes.c_int32 * 4)()
    assert lib.jmhip_slice_to_frame_candidates8(None, slots, 2, 0, 1) != 0
    assert lib.jmhip_slice_ref8ts_download(None, out, 0, 1) != 0
