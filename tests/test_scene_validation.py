"""CPU: a caller's bad mesh is named as such before anything reaches a GPU.  zdr_scene_create and zdr_debug_build_accel refuse a
world-space position that is not finite or beyond ZDR_MAX_COORD = 2^30 (include/zdr.h; the derivation is at position_ok in
csrc/zdr_api.cpp) with ZDR_E_INVALID and a message that names the vertex; a scene exactly at the limit builds with finite records; a
triangle without area stays legal."""
import ctypes as C

import numpy as np
import pytest

import geometry_cases as gc
from zdr_amd import _native

LIMIT = np.float32(_native.MAX_COORD)
BEYOND = np.nextafter(LIMIT, np.float32(np.inf))
ACCELS = [_native.ACCEL_BRUTE, _native.ACCEL_BVH]


def soup():
    return gc.soup_tris(80, 5, 0.1, 1.0).astype(np.float32)


def build(tris, accel):
    """zdr_debug_build_accel -> (rc, message, nodes, isect)"""
    tri = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    n = tri.shape[0]
    nodes = np.zeros((max(n, 8), 16), np.float32); order = np.zeros(n, np.int32); isect = np.zeros((n, 12), np.float32)
    nn, se = C.c_uint32(), C.c_uint32()
    L = _native.lib()
    rc = L.zdr_debug_build_accel(tri.ctypes.data, n, accel, nodes.ctypes.data, nodes.shape[0], C.byref(nn), C.byref(se), order.ctypes.data, isect.ctypes.data)
    return rc, L.zdr_last_error().decode(), nodes[:nn.value] if accel == _native.ACCEL_BVH else nodes[:0], isect


def create(A, accel):
    """zdr_scene_create -> (rc, message); a scene that comes into being is destroyed again"""
    L = _native.lib()
    h = C.c_void_p()
    rc = L.zdr_scene_create(A.verts.ctypes.data, A.verts.shape[0], A.tris.ctypes.data, A.tris.shape[0], A.inst_tri_begin.ctypes.data,
                            A.inst_xform.ctypes.data, A.inst_emission.ctypes.data, A.ninst, 0, accel, C.byref(h))
    msg = L.zdr_last_error().decode()
    if rc == 0:
        L.zdr_scene_destroy(h)
    return rc, msg


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("bad, what", [(np.nan, "not finite"), (np.inf, "not finite"), (-np.inf, "not finite"), (BEYOND, "exceeds"), (-BEYOND, "exceeds"),
                                       (np.float32(1e30), "exceeds")])
def test_the_host_builder_names_the_bad_corner(bad, what, accel):
    t = soup()
    t[41, 2, 1] = bad
    rc, msg, _, _ = build(t, accel)
    assert rc == -1 and what in msg and "triangle 41, vertex 2" in msg, (rc, msg)       # ZDR_E_INVALID
    t[7, 0, 2] = bad                                      # the FIRST offender is the one named
    rc, msg, _, _ = build(t, accel)
    assert rc == -1 and "triangle 7, vertex 0" in msg, (rc, msg)


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("bad, what", [(np.nan, "not finite"), (np.inf, "not finite"), (BEYOND, "exceeds")])
def test_scene_create_names_the_instance_and_the_vertex_without_a_device(bad, what, accel):
    """The refusal comes before the first HIP call: this test runs where there is no GPU (and on one as well)."""
    A = gc.arrays_of(soup(), 4)                           # instance 0: triangles 0 .. 75, instance 1: 76 .. 79; vertex 3 t + k
    A.verts[3 * 78 + 1, 0] = bad
    rc, msg = create(A, accel)
    assert rc == -1 and what in msg and "instance 1, vertex 235" in msg and "triangle 2 of the instance" in msg, (rc, msg)
    A.verts[3 * 5 + 2, 2] = bad
    rc, msg = create(A, accel)
    assert rc == -1 and "instance 0, vertex 17" in msg, (rc, msg)


@pytest.mark.parametrize("accel", ACCELS)
def test_it_is_the_world_space_position_that_counts(accel):
    A = gc.arrays_of(soup(), 4)
    A.inst_xform[1, 3] = 2.0 ** 31                        # the translation of instance 1 carries its vertices beyond the limit
    rc, msg = create(A, accel)
    assert rc == -1 and "exceeds" in msg and "instance 1, vertex 228" in msg, (rc, msg)
    A.inst_xform[1, 3] = 0.0; A.inst_xform[0, 5] = np.nan # a NaN in a transform: every position of the instance
    rc, msg = create(A, accel)
    assert rc == -1 and "not finite" in msg and "instance 0, vertex 0" in msg, (rc, msg)
    A = gc.arrays_of(soup(), 4)
    A.verts[0, 0] = np.nan
    A.tris[0] = A.tris[1]                                 # a bad vertex that no triangle uses is nobody's position
    rc, msg = create(A, accel)
    assert not (rc == -1 and "position" in msg), (rc, msg)


def at_the_limit():
    """a soup blown up so that its largest coordinate is exactly 2^30, and a triangle as large as the whole allowed range"""
    t = soup().astype(np.float64)
    t *= float(LIMIT) / np.abs(t).max()
    t = t.astype(np.float32)
    t[0] = [[-LIMIT, -LIMIT, -LIMIT], [LIMIT, LIMIT, -LIMIT], [-LIMIT, LIMIT, LIMIT]]
    assert np.abs(t).max() == LIMIT
    return t


@pytest.mark.parametrize("accel", ACCELS)
def test_a_scene_exactly_at_the_limit_builds_with_finite_records(accel):
    t = at_the_limit()
    rc, msg, nodes, isect = build(t, accel)
    assert rc == 0, msg
    assert np.isfinite(isect).all() and np.isfinite(nodes[:, :6]).all()
    assert np.abs(isect[:, 3]).max() > 1e27               # N.w ~ L^3: what the limit is about
    # what world_records computes in float32 (the bound that binds): the squared length of the float32 cross product of two edges
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    with np.errstate(over="raise"):
        c = np.cross(e1, e2).astype(np.float32)
        cc = (c * c).sum(1, dtype=np.float32)
    assert np.isfinite(cc).all() and cc.max() > 2.0 ** 125
    rc, msg = create(gc.arrays_of(t, 4), accel)           # with a GPU it builds; without one it fails at the first HIP call — not at the positions
    assert not (rc == -1 and "position" in msg), (rc, msg)
    with np.errstate(over="ignore"):                      # ... and twice the limit would not do: the same number overflows
        e = np.float32(4.0) * LIMIT
        assert not np.isfinite(np.float32(3) * (np.float32(2) * e * e) * (np.float32(2) * e * e))


@pytest.mark.parametrize("accel", ACCELS)
def test_triangles_without_area_stay_legal(accel):
    t = gc.degenerate_tris().astype(np.float32)
    rc, msg, _, isect = build(t, accel)
    assert rc == 0, msg
    rc, msg = create(gc.arrays_of(t, 4), accel)
    assert not (rc == -1 and "position" in msg), (rc, msg)
