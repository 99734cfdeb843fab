"""The texture-space lighting kernels (zdr_amd/csrc/zdr_bake.hip) read from the metadata of the BUILT libraries, like
tests/test_texel_resources.py.  They are a translation unit of their own, linked into libzdr_bake.so, which libzdr_hip.so names as a
dependency and finds beside itself: the kernels must exist there and nowhere else, the shading kernel in every instantiation (sampler x
accelerator x environment), and none may use more scratch than the any-hit ray query k_trace<A, true> of the same accelerator in
libzdr_hip.so — the per-lane BVH stack beyond its LDS part is all either may hold there.  No GPU needed."""
import re
import subprocess

import pytest

from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

ACCELS = ("BruteAccel", "BvhAccel")


def accel_of(name):
    found = [a for a in ACCELS if a in name]
    assert len(found) == 1, name
    return found[0]


def test_the_bake_kernels_exist_in_their_own_library_and_nowhere_else():
    names = kernels_of(_native.BAKE_LIB_PATH)
    assert all("k_bake_" in n for n in names), names
    for kernel in ("k_bake_clear", "k_bake_compact"):
        assert [n for n in names if re.fullmatch(r"_Z\d+%s.*" % kernel, n)], (kernel, names)
    shade = [n for n in names if "k_bake_shade" in n]
    assert len(shade) == 8 and len(names) == 10, names               # 2 samplers x 2 accelerators x with / without environment
    for accel in ACCELS:
        assert len([n for n in shade if accel in n]) == 4, (accel, shade)
    for path in (_native.LIB_PATH, _native.TEXEL_LIB_PATH):
        assert not any("k_bake_" in n for n in kernels_of(path)), path


def test_the_bake_kernels_use_no_more_scratch_than_the_any_hit_query_of_their_accelerator():
    trace = {accel_of(n): r for n, r in kernels_of(_native.LIB_PATH).items() if re.match(r"_Z\d+k_traceI\d+\w+AccelLb1EE", n)}   # k_trace<A, true>
    assert sorted(trace) == sorted(ACCELS), trace
    for name, r in sorted(kernels_of(_native.BAKE_LIB_PATH).items()):
        bound = trace[accel_of(name)]["private_segment_fixed_size"] if "k_bake_shade" in name else 0
        print(f"[bake resources] {name}: scratch {r['private_segment_fixed_size']} B (bound {bound}), LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["private_segment_fixed_size"] <= bound, (name, r, bound)
        assert r["group_segment_fixed_size"] == 0, (name, r)         # the stacks are dynamic LDS, sized at launch


def test_the_main_library_names_the_bake_library_and_finds_it_beside_itself():
    if not __import__("os").path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_bake.so" in dyn and "libzdr_texel.so" in dyn and "$ORIGIN" in dyn
