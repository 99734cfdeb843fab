"""The texture-space kernels (zdr_amd/csrc/zdr_texel.hip) read from the metadata of the BUILT libraries, like
tests/test_denoise_resources.py.  They are a translation unit of their own, linked into libzdr_texel.so, which libzdr_hip.so names as a
dependency and finds beside itself: the three kernels must exist there and use no scratch, and libzdr_hip.so must hold the code objects
it held, the path kernels' first and none of the new kernels in any.  No GPU needed."""
import os
import re
import struct
import subprocess

import pytest

from test_denoise_resources import KEYS, LDS_PER_WORKGROUP
from test_kernel_resources import READELF
from zdr_amd import _native


def kernels_of(lib_path):
    """{kernel name: resources} over every gfx code object embedded in ``lib_path``"""
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()                                                  # builds the libraries if they are missing or stale
    blob = open(lib_path, "rb").read()
    found, off = {}, 0
    path = os.path.join(os.path.dirname(lib_path), "_gfx950_code_object_texel.tmp")
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


def test_the_texel_kernels_exist_in_the_built_library():
    names = kernels_of(_native.TEXEL_LIB_PATH)
    for kernel in ("k_texel_clear", "k_texel_raster", "k_texel_resolve"):
        assert [n for n in names if re.fullmatch(r"_Z\d+%s.*" % kernel, n)], (kernel, names)
    assert len(names) == 3, names


def test_the_texel_kernels_use_no_scratch_and_no_lds():
    sel = kernels_of(_native.TEXEL_LIB_PATH)
    assert len(sel) == 3, sel
    for name, r in sorted(sel.items()):
        print(f"[texel resources] {name}: scratch {r['private_segment_fixed_size']} B, LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] <= LDS_PER_WORKGROUP, (name, r)


def test_the_main_library_holds_what_it_held_and_names_the_texel_library():
    """tests/test_kernel_resources.py reads the FIRST code object of libzdr_hip.so: still the path kernels', and no texel kernel is in
    that library at all; it finds libzdr_texel.so as a dependency beside itself"""
    from test_kernel_resources import kernels
    first = kernels()
    assert any("k_path" in n for n in first) and not any("k_texel" in n for n in first)
    assert not any("k_texel" in n for n in kernels_of(_native.LIB_PATH))
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_texel.so" in dyn and "$ORIGIN" in dyn
