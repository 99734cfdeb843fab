"""The bounced-light kernels (zdr_amd/csrc/zdr_bounce.hip) read from the metadata of the BUILT libraries, like
tests/test_bake_resources.py.  They are a translation unit of their own, linked into libzdr_bounce.so, which libzdr_hip.so names as a
dependency and finds beside itself: the kernels must exist there and nowhere else, the shade and the dump kernel in every instantiation
(sampler x accelerator x environment), none may hold static LDS, and a shade kernel may use no more scratch than the closest-hit ray
query k_trace<A, false> of the same accelerator in libzdr_hip.so — the per-lane BVH stack beyond its LDS part is all either may hold
there.  VGPRs and scratch are printed.  No GPU needed."""
import os
import re
import subprocess

import pytest

from test_bake_resources import ACCELS, accel_of
from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

OTHER_LIBS = ("LIB_PATH", "TEXEL_LIB_PATH", "BAKE_LIB_PATH", "PUSHPULL_LIB_PATH", "PROJECT_LIB_PATH", "MIP_LIB_PATH", "ANISO_LIB_PATH", "PLAN_LIB_PATH",
              "VIEWGRAD_LIB_PATH", "TANGENT_LIB_PATH", "BAKEGRAD_LIB_PATH")


def test_the_bounce_kernels_exist_in_their_own_library_and_nowhere_else():
    names = kernels_of(_native.BOUNCE_LIB_PATH)
    assert all("k_bounce_" in n for n in names), names
    for kernel in ("k_bounce_clear", "k_bounce_compact"):
        assert [n for n in names if re.fullmatch(r"_Z\d+%s.*" % kernel, n)], (kernel, names)
    shade, dump = [n for n in names if "k_bounce_shade" in n], [n for n in names if "k_bounce_dump" in n]
    assert len(shade) == 8 and len(dump) == 8 and len(names) == 18, names    # 2 samplers x 2 accelerators x with / without environment, twice, + 2
    for accel in ACCELS:
        assert len([n for n in shade if accel in n]) == 4 and len([n for n in dump if accel in n]) == 4, (accel, names)
    for lib in OTHER_LIBS:
        assert not any("k_bounce_" in n for n in kernels_of(getattr(_native, lib))), lib


def test_the_bake_library_keeps_its_ten_kernels():
    assert len(kernels_of(_native.BAKE_LIB_PATH)) == 10


def test_no_static_lds_and_no_more_scratch_than_the_closest_hit_query_of_the_accelerator():
    trace = {accel_of(n): r for n, r in kernels_of(_native.LIB_PATH).items() if re.match(r"_Z\d+k_traceI\d+\w+AccelLb0EE", n)}   # k_trace<A, false>
    assert sorted(trace) == sorted(ACCELS), trace
    for name, r in sorted(kernels_of(_native.BOUNCE_LIB_PATH).items()):
        bound = trace[accel_of(name)]["private_segment_fixed_size"] if "k_bounce_shade" in name else None
        print(f"[bounce resources] {name}: scratch {r['private_segment_fixed_size']} B (bound {bound}), LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["group_segment_fixed_size"] == 0, (name, r)          # the stacks and the compaction's counts are dynamic LDS, sized at launch
        if bound is not None:
            assert r["private_segment_fixed_size"] <= bound, (name, r, bound)


def test_the_main_library_names_the_bounce_library_and_finds_it_beside_itself():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_bounce.so" in dyn and "libzdr_bake.so" in dyn and "$ORIGIN" in dyn
