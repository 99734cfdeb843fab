"""The kernels of the bounced light's adjoint (zdr_amd/csrc/zdr_bouncegrad.hip) read from the metadata of the BUILT libraries, like
tests/test_bounce_resources.py.  They are a translation unit of their own, linked into libzdr_bouncegrad.so, which libzdr_hip.so names as
a dependency and finds beside itself: the k_bgrad_* kernels must exist there and nowhere else, the shade kernel in every instantiation
(sampler x accelerator x environment), and a shade kernel may use no more scratch than the closest-hit ray query k_trace<A, false> of the
same accelerator in libzdr_hip.so — the vertex records are indexed by a run-time vertex number and live in dynamic LDS, sized by
``bounces`` at launch, not in scratch.  VGPRs, scratch and static LDS (the scatter queue and the emission table) are printed.  Resource
metadata only, never instructions.  No GPU needed."""
import os
import re
import subprocess

import pytest

from test_bake_resources import ACCELS, accel_of
from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

OTHER_LIBS = ("LIB_PATH", "TEXEL_LIB_PATH", "BAKE_LIB_PATH", "PUSHPULL_LIB_PATH", "PROJECT_LIB_PATH", "MIP_LIB_PATH", "ANISO_LIB_PATH", "PLAN_LIB_PATH",
              "VIEWGRAD_LIB_PATH", "TANGENT_LIB_PATH", "BAKEGRAD_LIB_PATH", "BOUNCE_LIB_PATH")
SCATTER_QUEUE_BYTES = 4 * 7 * 64            # ZDR_SCATTER_LDS_FLOATS (csrc/scene.h)
EMISSION_TABLE_BYTES = 4 * 3 * 32           # ZDR_BGRAD_LDS_LIGHTS x 3 floats (csrc/bouncegrad.h)


def test_the_bgrad_kernels_exist_in_their_own_library_and_nowhere_else():
    names = kernels_of(_native.BOUNCEGRAD_LIB_PATH)
    assert all("k_bgrad_" in n for n in names), names
    assert not any("k_bounce_" in n for n in names), names
    for kernel in ("k_bgrad_clear", "k_bgrad_compact", "k_bgrad_gather_mat", "k_bgrad_gather_emit"):
        assert [n for n in names if re.fullmatch(r"_Z\d+%s.*" % kernel, n)], (kernel, names)
    shade = [n for n in names if "k_bgrad_shade" in n]
    assert len(shade) == 8 and len(names) == 12, names                # 2 samplers x 2 accelerators x with / without environment, + 4
    for accel in ACCELS:
        assert len([n for n in shade if accel in n]) == 4, (accel, names)
    for lib in OTHER_LIBS:
        assert not any("k_bgrad_" in n for n in kernels_of(getattr(_native, lib))), lib


def test_the_bounce_library_keeps_its_eighteen_kernels():
    assert len(kernels_of(_native.BOUNCE_LIB_PATH)) == 18


def test_the_records_are_not_in_scratch():
    trace = {accel_of(n): r for n, r in kernels_of(_native.LIB_PATH).items() if re.match(r"_Z\d+k_traceI\d+\w+AccelLb0EE", n)}   # k_trace<A, false>
    assert sorted(trace) == sorted(ACCELS), trace
    for name, r in sorted(kernels_of(_native.BOUNCEGRAD_LIB_PATH).items()):
        bound = trace[accel_of(name)]["private_segment_fixed_size"] if "k_bgrad_shade" in name else None
        print(f"[bouncegrad resources] {name}: scratch {r['private_segment_fixed_size']} B (bound {bound}), static LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        if bound is not None:
            assert r["private_segment_fixed_size"] <= bound, (name, r, bound)
            # static LDS: the queue and the table, nothing that grows with the number of bounces
            assert r["group_segment_fixed_size"] <= SCATTER_QUEUE_BYTES + EMISSION_TABLE_BYTES, (name, r)
        else:
            assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (name, r)


def test_the_main_library_names_the_bouncegrad_library_and_finds_it_beside_itself():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_bouncegrad.so" in dyn and "libzdr_bounce.so" in dyn and "$ORIGIN" in dyn
