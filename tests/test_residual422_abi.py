"""The 4:2:2 record of the fused frame stage in the ABI: jmhip_mb_residual422 (jmhip_sizeof index 24), its numpy mirror, the new entry point.
No GPU needed: the library loads without one."""
import re
import os

import numpy as np


def test_residual422_record_layout(pkg):
    lib = pkg.load_library()
    dt = pkg.MB_RESIDUAL422_DTYPE
    assert lib.jmhip_sizeof(24) == dt.itemsize
    assert dt.itemsize % 16 == 0                       # copied out of LDS as 16-byte pieces
    # the existing records keep their indices and sizes
    assert lib.jmhip_sizeof(22) == pkg.MB_RESIDUAL_DTYPE.itemsize
    assert lib.jmhip_sizeof(23) == pkg.MB_RESIDUAL8_DTYPE.itemsize == 832
    assert lib.jmhip_sizeof(25) == -1
    # luma fields as in jmhip_mb_residual, chroma for two 8 x 16 components
    assert dt["lev"].shape == (32, 16) and dt["run"].shape == (32, 16) and dt["cnt"].shape == (32,)
    assert dt["dc_lev"].shape == (2, 8) and dt["dc_run"].shape == (2, 8)
    assert dt["fadj_c"].shape == (2, 16, 8) and dt["recon_c"].shape == (2, 16, 8)
    for f in ("coeff_cost", "nonzero", "fadj_y", "recon_y", "ret", "cbp_blk", "cbp_clear", "ac_zeroed", "dc_cnt"):
        assert pkg.MB_RESIDUAL_DTYPE[f].shape == dt[f].shape and pkg.MB_RESIDUAL_DTYPE[f].base == dt[f].base, f
    assert dt.fields["cbp_blk"][1] % 8 == 0 and dt.fields["coeff_cost"][1] % 4 == 0 and dt.fields["fadj_y"][1] % 2 == 0


def test_residual422_entry_point_and_abi_version(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "jmhip_residual_records422_download")
    assert "jmhip_residual_records422_download" in pkg.declared_symbols()
    assert hasattr(pkg.Context, "residual_records422")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "jmhip.h")) as f:
        assert re.search(r"#define\s+JMHIP_ABI_VERSION\s+1\b", f.read())
    assert isinstance(np.zeros(1, pkg.MB_RESIDUAL422_DTYPE)["lev"], np.ndarray)
