"""The gather-plan kernels (zdr_amd/csrc/zdr_plan.hip) read from the metadata of the BUILT libraries, like tests/test_aniso_resources.py.
They are a translation unit of their own, linked into libzdr_plan.so, which libzdr_hip.so names as a dependency and finds beside
itself: the k_plan_* kernels must exist there and in none of the other seven libraries (the library also holds the kernels of the radix
sort it instantiates, which are not the project's own and are not counted), the apply — the hot path, two instantiations — without
scratch and with at most 128 VGPRs; the other seven libraries hold the kernels they held (their own tests' assertions, called from
here).  No GPU needed."""
import re
import subprocess

import pytest

import test_aniso_resources
from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

BUILD_KERNELS = ("k_plan_count", "k_plan_scan", "k_plan_fill", "k_plan_rows")
OTHERS = test_aniso_resources.OTHERS + ("ANISO_LIB_PATH",)


def plan_kernels():
    return {n: r for n, r in kernels_of(_native.PLAN_LIB_PATH).items() if "k_plan_" in n}


def test_the_plan_kernels_exist_in_their_own_library_and_nowhere_else():
    names = plan_kernels()
    for kernel in BUILD_KERNELS:
        assert len([n for n in names if re.fullmatch(r"_Z\d+%s[^_].*" % kernel, n)]) == 1, (kernel, sorted(names))
    assert len([n for n in names if re.fullmatch(r"_Z\d+k_plan_applyILb[01]EE.*", n)]) == 2, sorted(names)      # short rows, long rows
    assert len(names) == len(BUILD_KERNELS) + 2, sorted(names)
    assert len(OTHERS) == 7
    for attr in OTHERS:
        assert not any("k_plan_" in n for n in kernels_of(getattr(_native, attr))), attr


def test_the_apply_uses_no_scratch_and_at_most_128_vgprs():
    sel = plan_kernels()
    for name, r in sorted(sel.items()):
        print(f"[plan resources] {name}: scratch {r['private_segment_fixed_size']} B, LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
    apply = {n: r for n, r in sel.items() if "k_plan_apply" in n}
    assert len(apply) == 2, sorted(sel)
    for name, r in apply.items():
        assert r["private_segment_fixed_size"] == 0, (name, r)        # the unrolled products stay in registers
        assert r["group_segment_fixed_size"] == 0, (name, r)          # the tree is shuffles
        assert r["vgpr_count"] <= 128, (name, r)
    for name, r in sel.items():                                       # the build's own kernels keep nothing per entry either
        assert r["private_segment_fixed_size"] == 0, (name, r)


def test_the_main_library_names_the_plan_library_and_finds_it_beside_itself():
    if not __import__("os").path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_plan.so" in dyn and "libzdr_aniso.so" in dyn and "$ORIGIN" in dyn


def test_the_other_seven_libraries_hold_the_kernels_they_held():
    test_aniso_resources.test_the_aniso_kernels_exist_in_their_own_library_and_nowhere_else()
    test_aniso_resources.test_the_other_six_libraries_hold_the_kernels_they_held()
