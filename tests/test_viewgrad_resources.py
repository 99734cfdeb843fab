"""The camera-gradient kernels (zdr_amd/csrc/zdr_viewgrad.hip) read from the metadata and the disassembly of the BUILT libraries, like
tests/test_gather_plan_resources.py.  They are a translation unit of their own, linked into libzdr_viewgrad.so, which libzdr_hip.so
names as a dependency and finds beside itself: the four k_vg_* kernels must exist there and in none of the other eight libraries,
without scratch, with only the LDS they declare (none for the d_view kernels; the cross-wave step of stage 1 and the sub-sums of
stage 2), and no atomic instruction appears in the library.  No GPU needed."""
import os
import re
import struct
import subprocess

import pytest

from test_kernel_resources import READELF
from test_texel_resources import kernels_of
from zdr_amd import _native

OBJDUMP = os.path.join(os.path.dirname(READELF), "llvm-objdump")
OTHERS = ("LIB_PATH", "TEXEL_LIB_PATH", "BAKE_LIB_PATH", "PUSHPULL_LIB_PATH", "PROJECT_LIB_PATH", "MIP_LIB_PATH", "ANISO_LIB_PATH", "PLAN_LIB_PATH")
LDS = {"k_vg_dview": 0, "k_vg_partial": 4 * 15 * 8, "k_vg_camera": 16 * 13 * 8}     # bytes, as zdr_viewgrad.hip declares them


def viewgrad_kernels():
    return {n: r for n, r in kernels_of(_native.VIEWGRAD_LIB_PATH).items() if "k_vg_" in n}


def test_the_kernels_exist_in_their_own_library_and_nowhere_else():
    names = viewgrad_kernels()
    assert len([n for n in names if re.fullmatch(r"_Z\d+k_vg_dviewILi[01]EE.*", n)]) == 2, sorted(names)      # bilinear, mip
    for kernel in ("k_vg_partial", "k_vg_camera"):
        assert len([n for n in names if re.fullmatch(r"_Z\d+%s[^_].*" % kernel, n)]) == 1, (kernel, sorted(names))
    assert len(names) == 4 and len(kernels_of(_native.VIEWGRAD_LIB_PATH)) == 4, sorted(names)
    assert len(OTHERS) == 8
    for attr in OTHERS:
        assert not any("k_vg_" in n for n in kernels_of(getattr(_native, attr))), attr


def test_the_kernels_use_no_scratch_and_only_the_lds_they_declare():
    sel = viewgrad_kernels()
    assert len(sel) == 4, sorted(sel)
    for name, r in sorted(sel.items()):
        print(f"[viewgrad resources] {name}: scratch {r['private_segment_fixed_size']} B, LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == [v for k, v in LDS.items() if k in name][0], (name, r)
        assert r["vgpr_count"] <= 128, (name, r)


def test_no_atomic_instruction_appears_in_the_library():
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not found")
    _native.lib()
    blob = open(_native.VIEWGRAD_LIB_PATH, "rb").read()
    path = os.path.join(os.path.dirname(_native.VIEWGRAD_LIB_PATH), "_gfx950_code_object_viewgrad.tmp")
    off, objects, instructions = 0, 0, 0
    while True:
        off = blob.find(b"\x7fELF\x02\x01\x01\x40", off + 1)       # ELF64, little endian, OS ABI 64 = AMDGPU HSA
        if off < 0:
            break
        e_shoff, = struct.unpack_from("<Q", blob, off + 0x28)
        e_shentsize, e_shnum = struct.unpack_from("<HH", blob, off + 0x3A)
        try:
            with open(path, "wb") as f:
                f.write(blob[off:off + e_shoff + e_shentsize * e_shnum])
            asm = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
        finally:
            if os.path.exists(path):
                os.remove(path)
        objects += 1
        for line in asm.splitlines():
            m = re.match(r"\s+([a-z][a-z0-9_]+)\b", line)
            if m:
                instructions += 1
                assert "atomic" not in m.group(1) and not re.match(r"ds_\w*(add|cmpst|max|min)", m.group(1)), line
    assert objects == 1 and instructions > 500, (objects, instructions)


def test_the_main_library_names_the_viewgrad_library_and_finds_it_beside_itself():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()
    dyn = subprocess.run([READELF, "-d", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libzdr_viewgrad.so" in dyn and "libzdr_plan.so" in dyn and "$ORIGIN" in dyn
