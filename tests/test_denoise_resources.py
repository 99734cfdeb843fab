"""The denoiser's kernels (zdr_amd/csrc/zdr_denoise.hip) read from the metadata of the BUILT library, like tests/test_aov_resources.py.
They are a translation unit of their own, so the library carries a second code object behind the path kernels': every code object in
it is read here.  The kernels must exist, use no scratch, and stay within the LDS one workgroup may have.  No GPU needed."""
import os
import re
import struct
import subprocess

import pytest

from test_kernel_resources import READELF
from zdr_amd import _native

LDS_PER_WORKGROUP = 160 * 1024        # gfx950: a single workgroup may declare all of a CU's LDS
KEYS = ("group_segment_fixed_size", "vgpr_count", "sgpr_count", "private_segment_fixed_size")


def all_kernels():
    """{kernel name: resources} over EVERY gfx code object embedded in the library."""
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()                                                  # builds libzdr_hip.so if it is missing or stale
    blob = open(_native.LIB_PATH, "rb").read()
    found, off = {}, 0
    path = os.path.join(os.path.dirname(_native.LIB_PATH), "_gfx950_code_object_denoise.tmp")
    while True:
        off = blob.find(b"\x7fELF\x02\x01\x01\x40", off + 1)       # ELF64, little endian, OS ABI 64 = AMDGPU HSA
        if off < 0:
            break
        e_shoff, = struct.unpack_from("<Q", blob, off + 0x28)
        e_shentsize, e_shnum = struct.unpack_from("<HH", blob, off + 0x3A)
        try:
            with open(path, "wb") as f:
                f.write(blob[off:off + e_shoff + e_shentsize * e_shnum])
            out = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
        finally:
            if os.path.exists(path):
                os.remove(path)
        for m in re.finditer(r"- \.agpr_count.*?(?=\n  - \.agpr_count|\Z)", out, re.S):
            blk = m.group(0)
            found[re.search(r"\.name:\s*(\S+)", blk).group(1)] = {k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1)) for k in KEYS}
    return found


def denoise_kernels():
    return {n: r for n, r in all_kernels().items() if "k_denoise" in n}


def test_the_denoiser_kernels_exist_in_the_built_library():
    names = denoise_kernels()
    assert [n for n in names if re.fullmatch(r"_Z16k_denoise_guides.*", n)], names
    for mode in (0, 1, 2):                                         # filter, divide, gather (csrc/denoise.h)
        assert [n for n in names if re.fullmatch(r"_Z15k_denoise_levelILi%dEEv.*" % mode, n)], (mode, names)


def test_the_denoiser_kernels_use_no_scratch_and_fit_the_lds_of_one_workgroup():
    sel = denoise_kernels()
    assert len(sel) == 4, sel
    for name, r in sorted(sel.items()):
        print(f"[denoise resources] {name}: scratch {r['private_segment_fixed_size']} B, LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] <= LDS_PER_WORKGROUP, (name, r)


def test_the_path_kernels_are_still_the_first_code_object():
    """tests/test_kernel_resources.py reads the FIRST code object of the library: the denoiser's must come after it."""
    from test_kernel_resources import kernels
    first = kernels()
    assert any("k_path" in n for n in first) and not any("k_denoise" in n for n in first)
