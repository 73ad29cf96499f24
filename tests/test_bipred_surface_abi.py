"""jmhip_bipred_surface_job in the ABI: the C struct (jmhip_sizeof index 33) and the binding's dtype agree, the entry point is exported (no GPU)."""


def test_bipred_surface_job_layout(pkg):
    lib = pkg.load_library()
    dt = pkg.BIPRED_SURFACE_JOB_DTYPE
    assert lib.jmhip_sizeof(33) == dt.itemsize == 32
    assert [dt.fields[k][1] for k in ("mb_x", "ref1", "s_mv", "R", "cx", "wp", "weight1", "offset_bi", "wp_denom", "pad")] == [0, 4, 8, 12, 14, 18, 20, 24, 28, 30]
    assert hasattr(lib, "jmhip_bipred_surface") and "jmhip_bipred_surface" in pkg.declared_symbols()
    assert lib.jmhip_sizeof(9) == pkg.SURFACE_JOB_DTYPE.itemsize          # the uni-directional job keeps its index and size
