"""The kernels of the bounced light's adjoint in the environment map (zdr_amd/csrc/zdr_bounceenv.hip) read from the metadata of the BUILT
libraries, like tests/test_bounce_resources.py.  They are a translation unit of their own, linked into libzdr_bounceenv.so, which
libzdr_hip.so names as a dependency and finds beside itself: the k_benv_* kernels must exist there and nowhere else, the shade kernel in
every instantiation (sampler x accelerator), with no scratch at all and no more static LDS than the merge's slots and their keys.  The
VGPR counts are printed beside those of the forward's k_bounce_shade with an environment map — the expectation is the forward's waves per
SIMD; it is reported, not asserted.  Resource metadata only, never instructions.  No GPU needed."""
import os
import re
import subprocess

import pytest

from test_bake_resources import ACCELS, accel_of
from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

OTHER_LIBS = ("LIB_PATH", "TEXEL_LIB_PATH", "BAKE_LIB_PATH", "PUSHPULL_LIB_PATH", "PROJECT_LIB_PATH", "MIP_LIB_PATH", "ANISO_LIB_PATH", "PLAN_LIB_PATH",
              "VIEWGRAD_LIB_PATH", "TANGENT_LIB_PATH", "BAKEGRAD_LIB_PATH", "BOUNCE_LIB_PATH", "BOUNCEGRAD_LIB_PATH")
MERGE_ROUNDS = 4                                # ZDR_LGRAD_MERGE_ROUNDS (csrc/bakegrad.h)
MERGE_LDS_BYTES = 4 * 16 * MERGE_ROUNDS + 4 * MERGE_ROUNDS      # the slots [round][tap][rgb, unused] and one key per round


def waves_per_simd(vgprs):
    """the occupancy 512 VGPRs per SIMD lane allow a kernel of one wave per workgroup (allocation granule 8, at most 8 waves)"""
    return min(8, 512 // (8 * ((vgprs + 7) // 8)))


def test_the_benv_kernels_exist_in_their_own_library_and_nowhere_else():
    names = kernels_of(_native.BOUNCEENV_LIB_PATH)
    assert all("k_benv_" in n for n in names), names
    for kernel in ("k_benv_clear", "k_benv_compact"):
        assert [n for n in names if re.fullmatch(r"_Z\d+%s.*" % kernel, n)], (kernel, names)
    shade = [n for n in names if "k_benv_shade" in n]
    assert len(shade) == 4 and len(names) == 6, names                 # 2 samplers x 2 accelerators, + 2
    for accel in ACCELS:
        assert len([n for n in shade if accel in n]) == 2, (accel, names)
    for lib in OTHER_LIBS:
        assert not any("k_benv_" in n for n in kernels_of(getattr(_native, lib))), lib


def test_the_neighbouring_libraries_keep_their_kernels():
    assert len(kernels_of(_native.BOUNCE_LIB_PATH)) == 18
    assert len(kernels_of(_native.BOUNCEGRAD_LIB_PATH)) == 12


def test_the_shade_kernels_use_no_scratch_and_only_the_merge_slots_of_static_lds():
    forward = {}
    for n, r in kernels_of(_native.BOUNCE_LIB_PATH).items():
        if "k_bounce_shade" in n:
            forward.setdefault(accel_of(n), []).append(r["vgpr_count"])
    for name, r in sorted(kernels_of(_native.BOUNCEENV_LIB_PATH).items()):
        line = (f"[bounceenv resources] {name}: scratch {r['private_segment_fixed_size']} B, static LDS {r['group_segment_fixed_size']} B, "
                f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        if "k_benv_shade" in name:
            fwd = sorted(forward[accel_of(name)])
            line += (f", {waves_per_simd(r['vgpr_count'])} waves per SIMD by VGPRs; k_bounce_shade of this accelerator: {fwd} VGPRs, "
                     f"{sorted(waves_per_simd(v) for v in fwd)} waves per SIMD")
        print(line)
        assert r["private_segment_fixed_size"] == 0, (name, r)
        if "k_benv_shade" in name:
            assert r["group_segment_fixed_size"] == MERGE_LDS_BYTES, (name, r)
        else:
            assert r["group_segment_fixed_size"] == 0, (name, r)


def test_the_main_library_names_the_bounceenv_library_and_finds_it_beside_itself():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_bounceenv.so" in dyn and "libzdr_bouncegrad.so" in dyn and "$ORIGIN" in dyn
