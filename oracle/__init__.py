"""ctypes front end of the CPU oracle (oracle/zdr_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and the
``cpu_baseline`` leg of bench.py — never by anything under zdr_amd/.
PARITY UNPINNED at the LuisaCompute boundary (see zdr_oracle.h).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBS = {}

COLLOCATED, DIRECT, PATH, UVGRAD = 0, 1, 2, 3
SAMPLER_CMJ, SAMPLER_PMJ02BN = 0, 1
PRB_CORRECT, PRB_LITERAL, PRB_DETACHED = 0, 1, 2
INTEGRATORS = {"collocated": COLLOCATED, "direct": DIRECT, "path": PATH, "uvgrad": UVGRAD}
COUNTER_NAMES = ("samples", "closest_rays", "closest_hits", "shadow_rays", "shaded_vertices",
                 "emitter_hits_bsdf", "nan_samples", "grad_scatters")


class Params(C.Structure):
    _fields_ = [
        ("integrator", C.c_int32), ("sampler", C.c_int32),
        ("width", C.c_int32), ("height", C.c_int32),
        ("spp", C.c_uint32), ("seed", C.c_uint32),
        ("use_tent", C.c_int32),
        ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
        ("sample_begin", C.c_uint32), ("sample_end", C.c_uint32),
        ("max_depth", C.c_int32), ("rr_depth", C.c_int32), ("prb_mode", C.c_int32),
        ("cam_fov", C.c_float), ("cam_origin", C.c_float * 3), ("cam_target", C.c_float * 3), ("cam_up", C.c_float * 3),
        ("tex_h", C.c_int32), ("tex_w", C.c_int32), ("nthreads", C.c_int32),
    ]


VARIANTS = {"ieee": "libzdr_oracle.so", "fma": "libzdr_oracle_fma.so"}


def build(force: bool = False, variant: str = "ieee") -> str:
    """'ieee' is THE oracle (no contraction).  'fma' is the same source compiled with FMA contraction:
    it differs from 'ieee' only by last-ulp roundings and is used to MEASURE the fp32 noise floor of
    the reference's formulas (how far two correct float32 evaluations drift apart), never as a reference."""
    so = os.path.join(_HERE, VARIANTS[variant])
    src = os.path.join(_HERE, "zdr_oracle.c")
    hdr = os.path.join(_HERE, "zdr_oracle.h")
    if force or not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["make", "-C", _HERE, "-B", VARIANTS[variant]], check=True, capture_output=True)
    return so


def lib(variant: str = "ieee"):
    if variant not in _LIBS:
        L = C.CDLL(build(variant=variant))
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.zdro_scene_create.restype = C.c_void_p
        L.zdro_scene_create.argtypes = [fp, C.c_int, ip, C.c_int, ip, fp, fp, C.c_int]
        L.zdro_scene_destroy.argtypes = [C.c_void_p]
        L.zdro_scene_set_emissions.argtypes = [C.c_void_p, fp]
        L.zdro_scene_set_envmap.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, fp, ip, C.c_int, fp, C.c_int, C.c_int]
        L.zdro_render_forward.argtypes = [C.c_void_p, C.POINTER(Params), fp, fp, C.POINTER(C.c_uint64)]
        L.zdro_render_backward.argtypes = [C.c_void_p, C.POINTER(Params), fp, fp, fp, C.POINTER(C.c_uint64)]
        L.zdro_scene_set_material_slots.argtypes = [C.c_void_p, ip]
        L.zdro_render_forward_materials.argtypes = [C.c_void_p, C.POINTER(Params), fp, ip, C.c_int, fp, C.POINTER(C.c_uint64)]
        L.zdro_render_backward_materials.argtypes = [C.c_void_p, C.POINTER(Params), fp, fp, ip, C.c_int, fp, C.POINTER(C.c_uint64)]
        L.zdro_path_dump.argtypes = [C.c_void_p, C.POINTER(Params), fp, fp, ip, C.c_int, C.c_int, fp]
        L.zdro_trace_closest.argtypes = [C.c_void_p, fp, C.c_int, ip, fp]
        L.zdro_trace_any.argtypes = [C.c_void_p, fp, C.c_int, ip]
        L.zdro_xxhash32_4.restype = C.c_uint32
        L.zdro_xxhash32_4.argtypes = [C.c_uint32] * 4
        L.zdro_permutation_element.restype = C.c_uint32
        L.zdro_permutation_element.argtypes = [C.c_uint32] * 4
        L.zdro_sampler_dump.restype = C.c_int
        L.zdro_sampler_dump.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, fp]
        L.zdro_ggx_brdf.argtypes = [fp, fp, fp, C.c_float, fp]
        L.zdro_ggx_sample_pdf.restype = C.c_float
        L.zdro_ggx_sample_pdf.argtypes = [fp, fp, C.c_float]
        L.zdro_ggx_sample.argtypes = [fp, C.c_float, C.c_float, fp, fp]
        L.zdro_ggx_brdf_grad.argtypes = [fp, fp, fp, C.c_float, fp, fp]
        L.zdro_ggx_dlnpdf_dr.restype = C.c_float
        L.zdro_ggx_dlnpdf_dr.argtypes = [fp, fp, C.c_float]
        L.zdro_ggx_eval_batch.argtypes = [fp, C.c_int, fp]
        L.zdro_ggx_sample_batch.argtypes = [fp, C.c_int, fp]
        L.zdro_generate_ray.argtypes = [C.POINTER(Params), C.c_float, C.c_float, fp, fp]
        L.zdro_offset_ray_origin.argtypes = [fp, fp, fp]
        L.zdro_read_bsdf.argtypes = [fp, C.c_int, C.c_int, C.c_float, C.c_float, fp]
        L.zdro_write_bsdf_grad.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int, fp, C.c_int]
        for name in ("zdro_sample_light", "zdro_sample_light_pdf", "zdro_env_dir_uv", "zdro_surface_interact"):
            getattr(L, name).argtypes = [C.c_void_p, fp, C.c_int, fp]
        L.zdro_light_misc.argtypes = [fp, C.c_int, fp]
        L.zdro_debug_force_brute.argtypes = [C.c_int]
        L.zdro_set_pmj02bn_tables.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.c_int, C.POINTER(C.c_uint16), C.c_int, C.c_int]
        _LIBS[variant] = L
    return _LIBS[variant]


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def f3(v):
    return (C.c_float * 3)(*[float(c) for c in v])


def make_params(integrator, width, height, spp, seed, camera, tex_hw, *, sampler=SAMPLER_CMJ, use_tent=True,
                rect=None, samples=None, max_depth=16, rr_depth=2, prb_mode=PRB_CORRECT, nthreads=0) -> Params:
    """camera = (fov, origin, target, up) or an object with those attributes."""
    if not isinstance(camera, (tuple, list)):
        camera = (camera.fov, tuple(camera.origin), tuple(camera.target), tuple(camera.up))
    p = Params()
    p.integrator = INTEGRATORS[integrator] if isinstance(integrator, str) else int(integrator)
    p.sampler = sampler
    p.width, p.height, p.spp, p.seed = width, height, spp, seed & 0xFFFFFFFF
    p.use_tent = int(bool(use_tent))
    p.x0, p.y0, p.x1, p.y1 = rect if rect is not None else (0, 0, width, height)
    p.sample_begin, p.sample_end = samples if samples is not None else (0, spp)
    p.max_depth, p.rr_depth, p.prb_mode = max_depth, rr_depth, prb_mode
    p.cam_fov = camera[0]
    p.cam_origin, p.cam_target, p.cam_up = f3(camera[1]), f3(camera[2]), f3(camera[3])
    p.tex_h, p.tex_w = tex_hw
    p.nthreads = nthreads
    return p


class OracleScene:
    """CPU twin of zdr_amd.Scene's native handle, built from zdr_amd.geometry.SceneArrays-like arrays."""

    def __init__(self, verts, tris, inst_tri_begin, inst_xform, inst_emission, variant="ieee"):
        self._L = lib(variant)
        self._keep = [np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.int32),
                      np.ascontiguousarray(inst_tri_begin, np.int32), np.ascontiguousarray(inst_xform, np.float32),
                      np.ascontiguousarray(inst_emission, np.float32)]
        v, t, b, x, e = self._keep
        self.ninst = e.reshape(-1, 3).shape[0]
        self.h = self._L.zdro_scene_create(_f(v), v.reshape(-1, 8).shape[0], _i(t), t.reshape(-1, 3).shape[0], _i(b), _f(x), _f(e), self.ninst)

    @classmethod
    def from_arrays(cls, A, variant="ieee"):
        return cls(A.verts, A.tris, A.inst_tri_begin, A.inst_xform, A.inst_emission, variant=variant)

    def __del__(self):
        if getattr(self, "h", None):
            self._L.zdro_scene_destroy(self.h)
            self.h = None

    def set_emissions(self, e):
        e = np.ascontiguousarray(e, np.float32).reshape(self.ninst, 3)
        self._L.zdro_scene_set_emissions(self.h, _f(e))

    def set_envmap(self, tex, alias_prob, alias_idx, pdf, map_w=512, map_h=256):
        tex = np.ascontiguousarray(tex, np.float32); ap = np.ascontiguousarray(alias_prob, np.float32)
        ai = np.ascontiguousarray(alias_idx, np.int32); pd = np.ascontiguousarray(pdf, np.float32)
        self._L.zdro_scene_set_envmap(self.h, _f(tex), tex.shape[0], tex.shape[1], _f(ap), _i(ai), ap.shape[0], _f(pd), map_w, map_h)

    def render_forward(self, params: Params, material: np.ndarray, counters: bool = False):
        material = np.ascontiguousarray(material, np.float32)
        assert material.ndim == 3 and material.shape[2] == 4
        img = np.zeros((params.height, params.width, 4), np.float32)
        cnt = (C.c_uint64 * 8)()
        rc = self._L.zdro_render_forward(self.h, C.byref(params), _f(material), _f(img), cnt)
        if rc:
            raise RuntimeError(f"oracle forward failed rc={rc}")
        return (img, dict(zip(COUNTER_NAMES, list(cnt)))) if counters else img

    def render_backward(self, params: Params, d_image: np.ndarray, material: np.ndarray, counters: bool = False):
        material = np.ascontiguousarray(material, np.float32)
        d_image = np.ascontiguousarray(d_image, np.float32)
        assert d_image.shape == (params.height, params.width, 4)
        dm = np.zeros_like(material)
        cnt = (C.c_uint64 * 8)()
        rc = self._L.zdro_render_backward(self.h, C.byref(params), _f(d_image), _f(material), _f(dm), cnt)
        if rc:
            raise RuntimeError(f"oracle backward failed rc={rc}")
        return (dm, dict(zip(COUNTER_NAMES, list(cnt)))) if counters else dm

    def set_material_slots(self, slots):
        """One entry per instance: its material's index in the lists given to render_*_materials, or None / -1; None = no material
        anywhere (zdr_amd.Scene.material_slots)."""
        if slots is None:
            self._L.zdro_scene_set_material_slots(self.h, None)
            return
        t = np.array([-1 if k is None else int(k) for k in slots], np.int32)
        assert t.shape == (self.ninst,), (t.shape, self.ninst)
        self._L.zdro_scene_set_material_slots(self.h, _i(t))

    @staticmethod
    def _pack(materials):
        mats = [np.ascontiguousarray(m, np.float32) for m in materials]
        for m in mats:
            assert m.ndim == 3 and m.shape[2] == 4, m.shape
        dims = np.array([m.shape[:2] for m in mats], np.int32).reshape(-1, 2)
        return mats, np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in mats])), dims

    def render_forward_materials(self, params: Params, materials, counters: bool = False):
        """render_forward with one material per slot (set_material_slots); ``materials``: a list of (h_k, w_k, 4) arrays."""
        _, packed, dims = self._pack(materials)
        img = np.zeros((params.height, params.width, 4), np.float32)
        cnt = (C.c_uint64 * 8)()
        rc = self._L.zdro_render_forward_materials(self.h, C.byref(params), _f(packed), _i(dims), dims.shape[0], _f(img), cnt)
        if rc:
            raise RuntimeError(f"oracle forward (materials) failed rc={rc}")
        return (img, dict(zip(COUNTER_NAMES, list(cnt)))) if counters else img

    def render_backward_materials(self, params: Params, d_image: np.ndarray, materials, counters: bool = False):
        """render_backward with one material per slot: returns one gradient per material, shaped like it."""
        mats, packed, dims = self._pack(materials)
        d_image = np.ascontiguousarray(d_image, np.float32)
        assert d_image.shape == (params.height, params.width, 4)
        dm = np.zeros_like(packed)
        cnt = (C.c_uint64 * 8)()
        rc = self._L.zdro_render_backward_materials(self.h, C.byref(params), _f(d_image), _f(packed), _i(dims), dims.shape[0], _f(dm), cnt)
        if rc:
            raise RuntimeError(f"oracle backward (materials) failed rc={rc}")
        out, off = [], 0
        for m in mats:
            out.append(dm[off:off + m.size].reshape(m.shape))
            off += m.size
        return (out, dict(zip(COUNTER_NAMES, list(cnt)))) if counters else out

    def path_dump(self, params: Params, material: np.ndarray, queries: np.ndarray, d_image=None, maxv: int = 16) -> np.ndarray:
        """queries (n, 3) int32 {px, py, sample_index} -> (n, 8 + 24 maxv) float32 per-path trace (layout: zdr_oracle.c)."""
        material = np.ascontiguousarray(material, np.float32)
        q = np.ascontiguousarray(queries, np.int32).reshape(-1, 3)
        out = np.zeros((q.shape[0], 8 + 24 * maxv), np.float32)
        cot = None if d_image is None else np.ascontiguousarray(d_image, np.float32)
        rc = self._L.zdro_path_dump(self.h, C.byref(params), _f(material), None if cot is None else _f(cot), _i(q), q.shape[0], maxv, _f(out))
        if rc:
            raise RuntimeError(f"oracle path_dump failed rc={rc}")
        return out

    def trace_closest(self, rays: np.ndarray):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = rays.shape[0]
        ip = np.zeros((n, 2), np.int32)
        bt = np.zeros((n, 3), np.float32)
        self._L.zdro_trace_closest(self.h, _f(rays), n, _i(ip), _f(bt))
        return ip, bt

    LIGHT_ROWS = {"sample": "zdro_sample_light", "pdf": "zdro_sample_light_pdf", "env": "zdro_env_dir_uv", "interact": "zdro_surface_interact"}

    def light_rows(self, what: str, rows: np.ndarray) -> np.ndarray:
        """The oracle's copies of the light-side functions row by row (zdr_oracle.c, zdro_sample_light ...): (n, 16) float32 in the
        layout of the kernels' zdr_light_dump -> (n, 16) float32; "misc" needs no scene; "interact" takes {bits(inst), bits(prim), u, v}
        and returns {p[3], uv[2], ns[3], ng[3]}."""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 16)
        out = np.zeros_like(rows)
        if what == "misc":
            self._L.zdro_light_misc(_f(rows), rows.shape[0], _f(out))
        else:
            getattr(self._L, self.LIGHT_ROWS[what])(self.h, _f(rows), rows.shape[0], _f(out))
        return out

    def trace_any(self, rays: np.ndarray):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        occ = np.zeros(rays.shape[0], np.int32)
        self._L.zdro_trace_any(self.h, _f(rays), rays.shape[0], _i(occ))
        return occ


def sampler_dump(kind, px, py, seed, spp, sample_index, nvert=3, rr_depth=2) -> np.ndarray:
    out = np.zeros(2 + 8 * nvert, np.float32)
    n = lib().zdro_sampler_dump(kind, px, py, seed & 0xFFFFFFFF, spp, sample_index, nvert, rr_depth, _f(out))
    return out[:n].copy()
