"""The push-pull kernels (zdr_amd/csrc/zdr_pushpull.hip) read from the metadata of the BUILT libraries, like tests/test_bake_resources.py.
They are a translation unit of their own, linked into libzdr_pushpull.so, which libzdr_hip.so names as a dependency and finds beside
itself: the kernels must exist there and in none of the other three libraries, use no scratch, and the fused tails must hold their
levels in LDS within what one workgroup may have.  No GPU needed."""
import re
import subprocess

import pytest

from test_denoise_resources import LDS_PER_WORKGROUP
from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

# kernel -> its instantiations (L0: the finer level is the caller's own texture and weight)
KERNELS = {"k_pp_push": 2, "k_pp_pull": 2, "k_pp_gather": 2, "k_pp_spread": 2, "k_pp_tail_fwd": 2, "k_pp_tail_bwd": 2, "k_pp_top": 1}
TAIL_TEXELS = 1368                                                 # ZDR_PUSHPULL_TAIL_TEXELS (csrc/pushpull.h)


def test_the_push_pull_kernels_exist_in_their_own_library_and_nowhere_else():
    names = kernels_of(_native.PUSHPULL_LIB_PATH)
    assert all("k_pp_" in n for n in names), names
    for kernel, count in KERNELS.items():
        assert len([n for n in names if re.fullmatch(r"_Z\d+%s(ILb[01]EEv)?[^_].*" % kernel, n)]) == count, (kernel, names)
    assert len(names) == sum(KERNELS.values()), names
    for path in (_native.LIB_PATH, _native.TEXEL_LIB_PATH, _native.BAKE_LIB_PATH):
        assert not any("k_pp_" in n for n in kernels_of(path)), path


def test_the_push_pull_kernels_use_no_scratch_and_the_tails_keep_their_levels_in_lds():
    sel = kernels_of(_native.PUSHPULL_LIB_PATH)
    assert len(sel) == sum(KERNELS.values()), sel
    for name, r in sorted(sel.items()):
        print(f"[push-pull resources] {name}: scratch {r['private_segment_fixed_size']} B, LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["private_segment_fixed_size"] == 0, (name, r)
        lds = TAIL_TEXELS * 20 if "k_pp_tail_fwd" in name else TAIL_TEXELS * 24 if "k_pp_tail_bwd" in name else 0   # float4 + a (+ r) per texel
        assert r["group_segment_fixed_size"] == lds and lds <= LDS_PER_WORKGROUP, (name, r)
        assert r["vgpr_count"] <= 128, (name, r)                     # 256 threads a block: never what limits the waves of a CU


def test_the_main_library_names_the_push_pull_library_and_finds_it_beside_itself():
    if not __import__("os").path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_pushpull.so" in dyn and "libzdr_bake.so" in dyn and "libzdr_texel.so" in dyn and "$ORIGIN" in dyn
