"""The texture-space view kernels (zdr_amd/csrc/zdr_project.hip) read from the metadata of the BUILT libraries, like
tests/test_bake_resources.py.  They are a translation unit of their own, linked into libzdr_project.so, which libzdr_hip.so names as a
dependency and finds beside itself: the kernels must exist there and in none of the other four libraries, the walk once per
accelerator with no more scratch than the any-hit ray query k_trace<A, true> of the same accelerator in libzdr_hip.so, and the gather
and its adjoint without scratch or static LDS.  No GPU needed."""
import re
import subprocess

import pytest

from test_bake_resources import ACCELS, accel_of
from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

PLAIN = ("k_proj_clear", "k_proj_compact", "k_proj_gather", "k_proj_scatter")


def test_the_view_kernels_exist_in_their_own_library_and_nowhere_else():
    names = kernels_of(_native.PROJECT_LIB_PATH)
    assert all("k_proj_" in n for n in names), names
    for kernel in PLAIN:
        assert len([n for n in names if re.fullmatch(r"_Z\d+%s[^_].*" % kernel, n)]) == 1, (kernel, names)
    walk = [n for n in names if "k_proj_view" in n]
    assert len(walk) == 2 and len(names) == len(PLAIN) + 2, names
    for accel in ACCELS:
        assert len([n for n in walk if accel in n]) == 1, (accel, walk)
    for path in (_native.LIB_PATH, _native.TEXEL_LIB_PATH, _native.BAKE_LIB_PATH, _native.PUSHPULL_LIB_PATH):
        assert not any("k_proj_" in n for n in kernels_of(path)), path


def test_the_walk_uses_no_more_scratch_than_the_any_hit_query_and_the_gathers_none():
    trace = {accel_of(n): r for n, r in kernels_of(_native.LIB_PATH).items() if re.match(r"_Z\d+k_traceI\d+\w+AccelLb1EE", n)}   # k_trace<A, true>
    assert sorted(trace) == sorted(ACCELS), trace
    for name, r in sorted(kernels_of(_native.PROJECT_LIB_PATH).items()):
        bound = trace[accel_of(name)]["private_segment_fixed_size"] if "k_proj_view" in name else 0
        print(f"[project resources] {name}: scratch {r['private_segment_fixed_size']} B (bound {bound}), LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["private_segment_fixed_size"] <= bound, (name, r, bound)
        lds = 20 if "k_proj_compact" in name else 0                  # the four waves' counts and the workgroup's base; the walk's stacks are dynamic LDS, sized at launch
        assert r["group_segment_fixed_size"] == lds, (name, r)


def test_the_main_library_names_the_project_library_and_finds_it_beside_itself():
    if not __import__("os").path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_project.so" in dyn and "libzdr_pushpull.so" in dyn and "$ORIGIN" in dyn
