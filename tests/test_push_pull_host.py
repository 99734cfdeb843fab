"""Host side of zdr_push_pull / zdr_push_pull_backward (include/zdr.h): every argument check comes before the first HIP call, so they run
without a GPU, like tests/test_denoise_host.py — the pointers given here are never dereferenced — and the argument checks of the Python
layer (zdr_amd/pushpull.py), which come before the library is asked anything."""
import ctypes as C

import pytest
import torch

from zdr_amd import _native as N
from zdr_amd import TexelAovs, push_pull
from zdr_amd.pushpull import PushPullOperator, push_pull_backward, push_pull_forward, workspace_bytes

OK_PTR = 1 << 20       # non-null, 16-byte aligned, never dereferenced
INVALID, UNSUPPORTED = -1, -3


def params(width=8, height=8, levels=0):
    p = N.PushPullParams()
    p.struct_size = C.sizeof(N.PushPullParams)
    p.width, p.height, p.levels = width, height, levels
    return p


def calls(L):
    return (L.zdr_push_pull, L.zdr_push_pull_backward)


def refused(L, rc, needle, code=INVALID):
    return rc == code and needle in L.zdr_last_error()


def test_struct_layout_matches_the_header():
    assert C.sizeof(N.PushPullParams) == 16 and N.PushPullParams.levels.offset == 12


def test_a_wrong_struct_size_is_refused():
    L = N.lib()
    p = params()
    p.struct_size += 4
    for f in calls(L):
        assert refused(L, f(C.byref(p), OK_PTR, 2 * OK_PTR, 3 * OK_PTR, 4 * OK_PTR, None), b"struct_size")
    assert L.zdr_push_pull_workspace_bytes(C.byref(p)) == 0


@pytest.mark.parametrize("width,height", [(0, 8), (8, 0), (-3, 8), (8, -1)])
def test_non_positive_sizes_are_refused(width, height):
    L = N.lib()
    p = params(width, height)
    for f in calls(L):
        assert refused(L, f(C.byref(p), OK_PTR, 2 * OK_PTR, 3 * OK_PTR, 4 * OK_PTR, None), b"positive")
    assert L.zdr_push_pull_workspace_bytes(C.byref(p)) == 0


def test_negative_levels_are_refused():
    L = N.lib()
    p = params(levels=-1)
    for f in calls(L):
        assert refused(L, f(C.byref(p), OK_PTR, 2 * OK_PTR, 3 * OK_PTR, 4 * OK_PTR, None), b"levels")
    assert L.zdr_push_pull_workspace_bytes(C.byref(p)) == 0


@pytest.mark.parametrize("which", range(4))
def test_a_null_or_misaligned_pointer_is_refused(which):
    L = N.lib()
    p = params()
    for f in calls(L):
        for bad, needle in ((None, b"null"), (OK_PTR + 4, b"aligned"), (OK_PTR + 8, b"aligned")):
            ptrs = [OK_PTR, 2 * OK_PTR, 3 * OK_PTR, 4 * OK_PTR]
            ptrs[which] = bad
            assert refused(L, f(C.byref(p), *ptrs, None), needle), (which, bad)
        assert refused(L, f(None, OK_PTR, 2 * OK_PTR, 3 * OK_PTR, 4 * OK_PTR, None), b"null")


def test_overlapping_buffers_are_refused():
    """8 x 8: the texture and the output are 1 KiB, the weight 256 bytes, the workspace as the library sizes it"""
    L = N.lib()
    p = params()
    ws = L.zdr_push_pull_workspace_bytes(C.byref(p))
    assert ws >= (16 + 4 + 1) * 24
    Wt, X, OUT, WS = 0x100000, 0x200000, 0x300000, 0x400000
    for f in calls(L):
        for ptrs in ((Wt, X, X, WS), (Wt, X, X + 512, WS), (Wt, X, X - 1024 + 16, WS), (Wt, X, Wt + 256 - 16, WS), (Wt, X, Wt - 1024 + 16, WS),
                     (Wt, X, WS + ws - 16, WS), (Wt, X, WS - 1024 + 16, WS), (Wt, X, OUT, X + 1024 - 16), (Wt, X, OUT, Wt - ws + 16)):
            assert refused(L, f(C.byref(p), *ptrs, None), b"overlap"), ptrs


def test_more_than_2_to_the_26_texels_are_unsupported():
    L = N.lib()
    for w, h in ((8193, 8192), (1 << 26, 2), (1 << 30, 1 << 30)):
        p = params(w, h)
        for f in calls(L):
            assert refused(L, f(C.byref(p), OK_PTR, 2 * OK_PTR, 3 * OK_PTR, 4 * OK_PTR, None), b"2^26", UNSUPPORTED)
        assert L.zdr_push_pull_workspace_bytes(C.byref(p)) == 0
    assert L.zdr_push_pull_workspace_bytes(C.byref(params(8192, 8192))) > 0 and L.zdr_push_pull_workspace_bytes(C.byref(params(1 << 26, 1))) > 0


def test_workspace_bytes_are_positive_and_monotone_in_the_size():
    sizes = [(1, 1), (2, 1), (2, 2), (5, 3), (7, 7), (37, 29), (64, 64), (257, 131), (1024, 1024), (2048, 2048)]       # each holds the one before
    for levels in (None, 1, 2, 5):
        b = [workspace_bytes(s, levels) for s in sizes]
        assert b[0] > 0 and b == sorted(b) and all(v % 16 == 0 for v in b), b
        assert b[3] < b[5] < b[7] < b[9]
    by_levels = [workspace_bytes((257, 131), lv) for lv in (1, 2, 3, 9, None)]
    assert by_levels == sorted(by_levels) and by_levels[-1] == by_levels[-2] == workspace_bytes((257, 131), 40)
    # the levels >= 1: a float4 and two floats per texel
    assert workspace_bytes((64, 64)) >= 24 * (32 * 32 + 16 * 16 + 8 * 8 + 4 * 4 + 2 * 2 + 1)
    with pytest.raises(N.ZdrError, match="positive"):
        workspace_bytes((0, 4))


def test_the_python_layer_checks_its_arguments():
    x, w = torch.zeros(6, 5, 4), torch.ones(6, 5)
    for f in (push_pull, push_pull_forward, push_pull_backward):
        with pytest.raises(ValueError, match="texture"):
            f(x[..., :3], w)
        with pytest.raises(ValueError, match="texture"):
            f(x.double(), w)
        with pytest.raises(ValueError, match="texture"):
            f(x[0], w)
        with pytest.raises(ValueError, match="weight"):
            f(x, w[:-1])
        with pytest.raises(ValueError, match="weight"):
            f(x, w.double())
        with pytest.raises(ValueError, match="weight"):
            f(x, w[..., None])
        with pytest.raises(ValueError, match="levels"):
            f(x, w, levels=0)
        with pytest.raises(ValueError, match="levels"):
            f(x, w.bool(), levels=-2)
        with pytest.raises(ValueError, match="GPU"):            # float32 and bool weights of the right shape pass up to here
            f(x, w)
        with pytest.raises(ValueError, match="GPU"):
            f(x, w.bool())
    assert issubclass(PushPullOperator, torch.autograd.Function)
    aovs = TexelAovs(torch.zeros(6, 5, 16))
    with pytest.raises(ValueError, match="by"):
        aovs.fill(x, by="slot")
    with pytest.raises(ValueError, match="GPU"):
        aovs.fill(x)
