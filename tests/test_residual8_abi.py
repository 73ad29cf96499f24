"""jmhip_mb_residual8 (the 8x8-transform side record of the fused frame stage): the C struct and the binding's dtype agree (no GPU)."""


def test_residual8_record_layout(pkg):
    lib = pkg.load_library()
    assert lib.jmhip_sizeof(23) == pkg.MB_RESIDUAL8_DTYPE.itemsize == 832
    assert hasattr(lib, "jmhip_residual_records8_download")
