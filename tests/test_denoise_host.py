"""Host side of zdr_denoise / zdr_denoise_backward (include/zdr.h): every argument check comes before the first HIP call, so they run
without a GPU, like tests/test_host.py — the pointers given here are never dereferenced."""
import ctypes as C

import pytest

from zdr_amd import _native as N

OK_PTR = 4096          # non-null, 16-byte aligned, never dereferenced


def params(width=8, height=8, levels=4):
    p = N.DenoiseParams()
    p.struct_size = C.sizeof(N.DenoiseParams)
    p.width, p.height, p.levels = width, height, levels
    p.sigma_normal, p.sigma_depth, p.sigma_albedo = 0.25, 0.1, 0.0
    return p


def calls(L):
    return (("zdr_denoise", L.zdr_denoise), ("zdr_denoise_backward", L.zdr_denoise_backward))


def test_struct_layout_matches_the_header():
    assert C.sizeof(N.DenoiseParams) == 28 and N.DenoiseParams.sigma_normal.offset == 16


def refused(L, rc, needle):
    return rc == -1 and needle in L.zdr_last_error()


def test_a_wrong_struct_size_is_refused():
    L = N.lib()
    p = params()
    p.struct_size -= 4
    for _, f in calls(L):
        assert refused(L, f(C.byref(p), OK_PTR, OK_PTR, 2 * OK_PTR, 3 * OK_PTR, None), b"struct_size")
    assert L.zdr_denoise_workspace_bytes(C.byref(p)) == 0


@pytest.mark.parametrize("levels", [0, -1, 7])
def test_levels_outside_one_to_six_are_refused(levels):
    L = N.lib()
    p = params(levels=levels)
    for _, f in calls(L):
        assert refused(L, f(C.byref(p), OK_PTR, OK_PTR, 2 * OK_PTR, 3 * OK_PTR, None), b"levels")
    assert L.zdr_denoise_workspace_bytes(C.byref(p)) == 0


@pytest.mark.parametrize("width,height", [(0, 8), (8, 0), (-3, 8), (8, -1)])
def test_non_positive_sizes_are_refused(width, height):
    L = N.lib()
    p = params(width, height)
    for _, f in calls(L):
        assert refused(L, f(C.byref(p), OK_PTR, OK_PTR, 2 * OK_PTR, 3 * OK_PTR, None), b"positive")
    assert L.zdr_denoise_workspace_bytes(C.byref(p)) == 0


@pytest.mark.parametrize("which", range(4))
def test_a_null_or_misaligned_pointer_is_refused(which):
    L = N.lib()
    p = params()
    for _, f in calls(L):
        for bad, needle in ((None, b"null"), (OK_PTR + 4, b"aligned"), (OK_PTR + 8, b"aligned")):
            ptrs = [OK_PTR, 2 * OK_PTR, 3 * OK_PTR, 4 * OK_PTR]
            ptrs[which] = bad
            assert refused(L, f(C.byref(p), *ptrs, None), needle), (which, bad)
    for _, f in calls(L):
        assert refused(L, f(None, OK_PTR, 2 * OK_PTR, 3 * OK_PTR, 4 * OK_PTR, None), b"null")


def test_the_output_may_not_be_an_input():
    L = N.lib()
    p = params()
    for _, f in calls(L):
        assert refused(L, f(C.byref(p), OK_PTR, 2 * OK_PTR, 2 * OK_PTR, 4 * OK_PTR, None), b"alias")


def test_overlapping_buffers_are_refused():
    """The sizes follow from the parameters (8 x 8: image and out 1 KiB, feature buffers 4 KiB, workspace 4 KiB), so partial overlap of the
    output with an input or the workspace, and of the workspace with an input, is refused too."""
    L = N.lib()
    p = params()
    assert L.zdr_denoise_workspace_bytes(C.byref(p)) == 4096
    A, X, OUT, WS = 0x10000, 0x20000, 0x30000, 0x40000
    for _, f in calls(L):
        for ptrs in ((A, X, X + 512, WS), (A, X, A + 4096 - 16, WS), (A, X, WS + 4096 - 16, WS), (A, X, WS - 1024 + 16, WS), (A, X, OUT, X - 4096 + 16),
                     (A, X, OUT, A + 2048)):
            assert refused(L, f(C.byref(p), *ptrs, None), b"overlap"), ptrs


def test_workspace_bytes_grow_with_the_size_and_never_shrink_with_the_levels():
    L = N.lib()
    size = lambda w, h, lv: L.zdr_denoise_workspace_bytes(C.byref(params(w, h, lv)))   # noqa: E731
    assert size(1, 1, 1) > 0
    for lv in range(1, 7):
        by_size = [size(w, h, lv) for w, h in ((1, 1), (5, 64), (37, 29), (64, 64), (1024, 1024))]
        assert by_size == sorted(by_size) and len(set(by_size)) == len(by_size)
        assert all(b % 16 == 0 for b in by_size)
    by_levels = [size(37, 29, lv) for lv in range(1, 7)]
    assert by_levels == sorted(by_levels)
    assert size(37, 29, 6) >= 37 * 29 * 16 * 3                     # the packed guides and one level, at the very least
