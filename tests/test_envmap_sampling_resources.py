"""The environment-table kernels (zdr_amd/csrc/zdr_envmap.hip) read from the metadata of the BUILT library, like
tests/test_denoise_resources.py.  They are a translation unit of their own, so the library carries a third code object behind the
path kernels' and the denoiser's.  The kernels must exist, use no scratch and stay below one 64 KiB allocation of LDS, and the two
code objects in front of them must hold what they held: nothing of the new file reaches them.  No GPU needed."""
import os
import re
import struct
import subprocess

import pytest

from test_denoise_resources import KEYS
from test_kernel_resources import READELF
from zdr_amd import _native

LDS_ALLOCATION = 64 * 1024
ENV_KERNELS = ("k_env_weight", "k_env_rows", "k_env_marginal", "k_env_pdf")


def code_objects():
    """[{kernel name: resources}] of every gfx code object embedded in the library, in file order."""
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    _native.lib()                                                  # builds libzdr_hip.so if it is missing or stale
    blob = open(_native.LIB_PATH, "rb").read()
    objects, off = [], 0
    path = os.path.join(os.path.dirname(_native.LIB_PATH), "_gfx950_code_object_envmap.tmp")
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
        found = {}
        for m in re.finditer(r"- \.agpr_count.*?(?=\n  - \.agpr_count|\Z)", out, re.S):
            blk = m.group(0)
            found[re.search(r"\.name:\s*(\S+)", blk).group(1)] = {k: int(re.search(r"\.%s:\s*(\d+)" % k, blk).group(1)) for k in KEYS}
        objects.append(found)
    return objects


@pytest.fixture(scope="module")
def objects():
    return code_objects()


def env_kernels(objects):
    return {n: r for obj in objects for n, r in obj.items() if "k_env_" in n}


def test_the_table_kernels_exist_in_the_built_library(objects):
    names = env_kernels(objects)
    for k in ENV_KERNELS:
        assert [n for n in names if re.fullmatch(r"_Z\d+%s.*" % k, n)], (k, sorted(names))
    assert len(names) == len(ENV_KERNELS), sorted(names)


def test_the_table_kernels_use_no_scratch_and_less_lds_than_one_allocation(objects):
    sel = env_kernels(objects)
    assert sel
    for name, r in sorted(sel.items()):
        print(f"[envmap sampling resources] {name}: scratch {r['private_segment_fixed_size']} B, LDS {r['group_segment_fixed_size']} B, "
              f"{r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] < LDS_ALLOCATION, (name, r)
    rows = [r for n, r in sel.items() if "k_env_rows" in n][0]
    assert rows["group_segment_fixed_size"] >= 512 * (4 + 8 + 4 + 4 + 4)      # the row's weights, prob, alias and two work lists live in LDS


def test_the_code_objects_in_front_hold_what_they_held(objects):
    """The path kernels' code object is the first and the denoiser's the second, as before; the new kernels are a third, and no
    kernel of theirs is in the other two (tests/test_kernel_resources.py and tests/test_denoise_resources.py read those)."""
    assert len(objects) == 3, [sorted(o)[:3] for o in objects]
    first, second, third = objects
    assert any("k_path" in n for n in first) and not any("k_denoise" in n or "k_env_" in n for n in first)
    assert len(second) == 4 and all("k_denoise" in n for n in second), sorted(second)
    assert len(third) == len(ENV_KERNELS) and all("k_env_" in n for n in third), sorted(third)


def test_the_new_translation_unit_is_seen_by_no_other_kernel_file():
    csrc = os.path.dirname(_native.LIB_PATH)
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")) and name not in ("zdr_envmap.hip", "envsample.h"):
            assert "envsample.h" not in open(os.path.join(csrc, name)).read(), name
    api = open(os.path.join(csrc, "zdr_api.cpp")).read()
    assert re.search(r"#define ZDR_ENVMAP_LAUNCHER_REF __attribute__\(\(weak\)\)[^\n]*\n#include \"envsample.h\"", api)
