"""The kernels of the light baker's adjoint (zdr_amd/csrc/zdr_bakegrad.hip) read from the metadata of the BUILT libraries, like
tests/test_bake_resources.py.  They are a translation unit of their own, linked into libzdr_bakegrad.so, which libzdr_hip.so names as a
dependency and finds beside itself: the library holds only k_lgrad_* kernels, the shading adjoint in every instantiation (sampler x
accelerator x environment), no other library holds one, and none uses more scratch than the any-hit ray query k_trace<A, true> of the
same accelerator in libzdr_hip.so.  No GPU needed."""
import re
import subprocess

import pytest

from test_bake_resources import ACCELS, accel_of
from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

OTHERS = ("LIB_PATH", "TEXEL_LIB_PATH", "BAKE_LIB_PATH", "PUSHPULL_LIB_PATH", "PROJECT_LIB_PATH", "MIP_LIB_PATH", "ANISO_LIB_PATH", "PLAN_LIB_PATH",
          "VIEWGRAD_LIB_PATH", "TANGENT_LIB_PATH")


def test_the_lgrad_kernels_exist_in_their_own_library_and_nowhere_else():
    names = kernels_of(_native.BAKEGRAD_LIB_PATH)
    assert all("k_lgrad_" in n for n in names), names
    for kernel in ("k_lgrad_clear", "k_lgrad_compact", "k_lgrad_gather"):
        assert len([n for n in names if re.fullmatch(r"_Z\d+%s.*" % kernel, n)]) == 1, (kernel, names)
    shade = [n for n in names if "k_lgrad_shade" in n]
    assert len(shade) == 8 and len(names) == 11, names               # 2 samplers x 2 accelerators x with / without environment
    for accel in ACCELS:
        assert len([n for n in shade if accel in n]) == 4, (accel, shade)
    assert len(OTHERS) == 10
    for attr in OTHERS:
        assert not any("k_lgrad_" in n for n in kernels_of(getattr(_native, attr))), attr


def test_the_lgrad_kernels_use_no_more_scratch_than_the_any_hit_query_of_their_accelerator():
    trace = {accel_of(n): r for n, r in kernels_of(_native.LIB_PATH).items() if re.match(r"_Z\d+k_traceI\d+\w+AccelLb1EE", n)}   # k_trace<A, true>
    assert sorted(trace) == sorted(ACCELS), trace
    for name, r in sorted(kernels_of(_native.BAKEGRAD_LIB_PATH).items()):
        bound = trace[accel_of(name)]["private_segment_fixed_size"] if "k_lgrad_shade" in name else 0
        print(f"[bakegrad resources] {name}: scratch {r['private_segment_fixed_size']} B (bound {bound}), LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["private_segment_fixed_size"] <= bound, (name, r, bound)
        # static LDS: the emission table, the merged cells and their keys; the BVH stacks are dynamic LDS on top, sized at launch
        assert r["group_segment_fixed_size"] <= 1024, (name, r)


def test_the_main_library_names_the_bakegrad_library_and_finds_it_beside_itself():
    if not __import__("os").path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_bakegrad.so" in dyn and "libzdr_bake.so" in dyn and "$ORIGIN" in dyn
