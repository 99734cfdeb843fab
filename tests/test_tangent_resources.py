"""The UV-tangent kernels (zdr_amd/csrc/zdr_tangent.hip) read from the metadata of the BUILT libraries, like
tests/test_aniso_resources.py.  They are a translation unit of their own, linked into libzdr_tangent.so, which libzdr_hip.so names as a
dependency and finds beside itself: the kernels must exist there and in none of the other nine libraries, none with scratch or static
LDS and none above 128 VGPRs.  No GPU needed."""
import re
import subprocess

import pytest

from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

KERNELS = ("k_tan_resolve", "k_tan_footprint")
OTHERS = ("LIB_PATH", "TEXEL_LIB_PATH", "BAKE_LIB_PATH", "PUSHPULL_LIB_PATH", "PROJECT_LIB_PATH", "MIP_LIB_PATH", "ANISO_LIB_PATH", "PLAN_LIB_PATH",
          "VIEWGRAD_LIB_PATH")


def test_the_tangent_kernels_exist_in_their_own_library_and_nowhere_else():
    names = kernels_of(_native.TANGENT_LIB_PATH)
    assert all("k_tan_" in n for n in names), names
    for kernel in KERNELS:
        assert len([n for n in names if re.fullmatch(r"_Z\d+%s[^_].*" % kernel, n)]) == 1, (kernel, names)
    assert len(names) == len(KERNELS), names
    assert len(OTHERS) == 9
    for attr in OTHERS:
        assert not any("k_tan_" in n for n in kernels_of(getattr(_native, attr))), attr


def test_the_tangent_kernels_use_no_scratch_no_lds_and_at_most_128_vgprs():
    sel = kernels_of(_native.TANGENT_LIB_PATH)
    assert len(sel) == len(KERNELS), sel
    for name, r in sorted(sel.items()):
        print(f"[tangent resources] {name}: scratch {r['private_segment_fixed_size']} B, LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["private_segment_fixed_size"] == 0, (name, r)        # the rows cross the wave in registers, float by float
        assert r["group_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= 128, (name, r)                     # 256 threads a block: never what limits the waves of a CU


def test_the_main_library_names_the_tangent_library_and_finds_it_beside_itself():
    if not __import__("os").path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_tangent.so" in dyn and "libzdr_texel.so" in dyn and "libzdr_aniso.so" in dyn and "$ORIGIN" in dyn


def test_the_texel_and_aniso_libraries_hold_the_three_kernels_each_that_they_held():
    assert len(kernels_of(_native.TEXEL_LIB_PATH)) == 3 and all("k_texel_" in n for n in kernels_of(_native.TEXEL_LIB_PATH))
    assert len(kernels_of(_native.ANISO_LIB_PATH)) == 3 and all("k_aniso_" in n for n in kernels_of(_native.ANISO_LIB_PATH))
