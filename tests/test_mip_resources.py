"""The prefiltering kernels (zdr_amd/csrc/zdr_mip.hip) read from the metadata of the BUILT libraries, like
tests/test_project_resources.py.  They are a translation unit of their own, linked into libzdr_mip.so, which libzdr_hip.so names as a
dependency and finds beside itself: the kernels must exist there and in none of the other five libraries, none with scratch, the gather
and the scatter without static LDS and the fused tails with their levels in LDS; the other five libraries hold the kernels they held
(their own tests' assertions, called from here).  No GPU needed."""
import re
import subprocess

import pytest

import test_bake_resources
import test_envmap_sampling_resources
import test_project_resources
import test_push_pull_resources
import test_texel_resources
from test_denoise_resources import LDS_PER_WORKGROUP
from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

KERNELS = ("k_mip_down1", "k_mip_down2", "k_mip_up1", "k_mip_up2", "k_mip_tail_fwd", "k_mip_tail_bwd", "k_mip_gather", "k_mip_scatter")
TAIL_TEXELS = 1368                                                 # ZDR_MIP_TAIL_TEXELS (csrc/mip.h)
OTHERS = ("LIB_PATH", "TEXEL_LIB_PATH", "BAKE_LIB_PATH", "PUSHPULL_LIB_PATH", "PROJECT_LIB_PATH")


def test_the_mip_kernels_exist_in_their_own_library_and_nowhere_else():
    names = kernels_of(_native.MIP_LIB_PATH)
    assert all("k_mip_" in n for n in names), names
    for kernel in KERNELS:
        assert len([n for n in names if re.fullmatch(r"_Z\d+%s[^_].*" % kernel, n)]) == 1, (kernel, names)
    assert len(names) == len(KERNELS), names
    for attr in OTHERS:
        assert not any("k_mip_" in n for n in kernels_of(getattr(_native, attr))), attr


def test_the_mip_kernels_use_no_scratch_and_the_gather_and_the_scatter_no_lds():
    sel = kernels_of(_native.MIP_LIB_PATH)
    assert len(sel) == len(KERNELS), sel
    for name, r in sorted(sel.items()):
        print(f"[mip resources] {name}: scratch {r['private_segment_fixed_size']} B, LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["private_segment_fixed_size"] == 0, (name, r)
        lds = TAIL_TEXELS * 16 if "k_mip_tail" in name else 0        # a float4 per pixel of the tail's levels
        assert r["group_segment_fixed_size"] == lds and lds <= LDS_PER_WORKGROUP, (name, r)
        assert r["vgpr_count"] <= 128, (name, r)                     # 256 threads a block: never what limits the waves of a CU


def test_the_main_library_names_the_mip_library_and_finds_it_beside_itself():
    if not __import__("os").path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_mip.so" in dyn and "libzdr_project.so" in dyn and "$ORIGIN" in dyn


def test_the_other_five_libraries_hold_the_kernels_they_held():
    test_texel_resources.test_the_texel_kernels_exist_in_the_built_library()
    test_bake_resources.test_the_bake_kernels_exist_in_their_own_library_and_nowhere_else()
    test_push_pull_resources.test_the_push_pull_kernels_exist_in_their_own_library_and_nowhere_else()
    test_project_resources.test_the_view_kernels_exist_in_their_own_library_and_nowhere_else()
    test_envmap_sampling_resources.test_the_code_objects_in_front_hold_what_they_held(test_envmap_sampling_resources.code_objects())
