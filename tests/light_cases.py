"""The light side of a path vertex point by point: seeded families of rows for zdr_light_dump (include/zdr.h), a float64 reference of
light.py:16-111, envmap.py:85-106,206-248, interaction.py:9-30, the origin offset (Waechter & Binder) and camera.py:20-31 on the float32
inputs, and one bound per output per row (tests/test_light_cases_host.py on the CPU, tests/test_gpu_light_cases.py on the GPU).

One arithmetic, two number types.  Every formula below is written once, on `Num` values:
  * float64 (`ref`): the reference.  A Num carries its value v and a bound e on what a float32 evaluation of the same expression may be
    off by — a first-order forward error model: every rounded operation adds K 2^-24 |v|, a transcendental (sin, cos, atan2, acos)
    KT 2^-24 |v|; operands hand their e on through the operation's derivative, so a difference that cancels (p - origin next to the light,
    1 - u - v, 1 - prob) keeps the ABSOLUTE error of what fed it; division, rcp, rsq, sqrt and acos are NOT linearised: their e is
    the width of the image of the operand's interval, infinite once the interval reaches the pole.
  * e = 0 means exact: the operands were exact and the float64 result is a float32 number (rcp: of a power of two; sqrt: of 0 or 1;
    sin, cos: of 0).  IEEE addition, multiplication and FMA then return it whatever the contraction, so wherever a row's output has
    e = 0 the kernel must return it BIT FOR BIT: dyadic u against power-of-two counts, the 8 x 4 map's dyadic texels on the
    quarter-texel lattice, offset_ray_origin, sample_uniform_triangle and tent_warp1 at dyadic points.  Integers are always exact.
  * float32 (`f32`): the IEEE transcription (NumPy rounds every operation once); `mut` switches one deliberate mistake on in it
    (MUTATIONS), so that the judge can be shown to bite.
Decisions that may legitimately flip are OPEN only while the operand's own e reaches the threshold — u.x < u.y, ur < prob, cos_light >
1e-4, |p| < 1/32, sin(pi v) > 0, a > 0 at the seam, the truncations and floors, and the domain of acos at the poles — and there a row
is accepted under the natural branches or under any combination of its own open decisions flipped.  Rows with an open
decision or an infinite bound are counted, and capped at OPEN_CAP per family by the reference alone.

K, KT are measured on the CPU, never on a GPU (measure_k, profiles/light_cases_margins.txt): the smallest integers at which the oracle's
copies (zdro_sample_light, zdro_sample_light_pdf, zdro_env_dir_uv, zdro_light_misc, zdro_surface_interact; IEEE and FMA build) and the
float32 transcription pass on every row of every family, times 4 for the device's uncorrected v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 and
its transcendental routines.

The scene's per-triangle constants (world corners, transformed normals, geometric normal, area) are float32 results of the host's IEEE
code (csrc/zdr_api.cpp, world_records, compiled without contraction): Tables repeats those operations in NumPy float32, the
reference takes them as inputs, and the host test pins the corners against the oracle's bit for bit.

Scenes (scene_arrays): cbox (one light: light0_T), stage (three lights of 2, 8 and 6 triangles: light_range), chandelier (15 lights),
quad (no light: the n <= 0 branch), cbox_env and quad_env (the same with the 8 x 4 map: n counts the environment), normals (a quad
whose vertex normals oppose across its diagonal: the interpolated normal vanishes at its centre), terrain (a BVH scene).
Families (family(name, scene), PLAN): sample (origins generic, 1e-3 / 1e-5 / 0 above the light's plane, behind it, 1e4 away, at a vertex;
u_pick, u_prim at k / n and either side, 0, 1 - 2^-24; u_pt on the diagonal, either side, the square's edges, a 1/16 lattice), pdf (the same
origins against points on every light triangle, origin = p), env (a grid over both halves of the sphere, the seam and its opposite, the
poles, the map's borders and either side, v in {0, 2^-24, 1/2, 1 - 2^-24, 1}, the round trip), alias (u at k / n and (k + prob) / n and either
side, through the sample mode on the environment-only scene), misc (balanced_heuristic, offset_ray_origin, sample_uniform_triangle,
tent_warp1), interact (the features and axis rays of tests/ray_cases.py; the vanishing normal).
"""
import functools
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:       # (run as a script: python tests/light_cases.py prints the table of profiles/light_cases_margins.txt)
    sys.path.insert(0, ROOT)

from zdr_amd import geometry  # noqa: E402
from zdr_amd.scenes import cbox_models, multi_light_arrays, terrain_arrays  # noqa: E402

U = 2.0 ** -24
K_MEASURED, K = 1, 4           # measure_k() -> K_MEASURED; K = 4 x (profiles/light_cases_margins.txt; test_light_cases_host.py holds them to it)
KT_MEASURED, KT = 2, 8         # the same for sin, cos, atan2, acos
OPEN_CAP = 0.01
F32, F64 = np.float32, np.float64
PI32 = float(F32(3.14159265358979323846))
INV_PI32 = float(F32(0.31830988618379067154))
TWO_PI32 = float(F32(2.0) * F32(PI32))
INV_TWO_PI32 = float(F32(1.0) / (F32(2.0) * F32(PI32)))
TWO_PI_SQ32 = float(F32(2.0) * F32(PI32) * F32(PI32))
C4, C9999 = float(F32(1e-4)), float(F32(0.9999))
ONE_M = 1.0 - 2.0 ** -24       # the largest float32 below 1
FLT_MAX, TINY = float(np.finfo(np.float32).max), 2.0 ** -126          # TINY: where float32 goes subnormal, a rounding is absolute
FAMILIES = ("sample", "pdf", "env", "alias", "misc", "interact")
MUTATIONS = {                  # mutation -> the families that exercise the term (each of them must reject it)
    "tri_swapped": ("sample", "misc"), "dist_without_9999": ("sample",), "cos_without_sign": ("sample", "pdf"),
    "n_without_env": ("sample", "pdf", "env"), "offset_floor": ("misc",), "offset_not_negated": ("misc",),
    "u_not_wrapped": ("env",), "pdf_index_x_for_y": ("env",), "alias_uu_unscaled": ("alias",), "ns_unnormalised": ("interact",),
}


# ------------------------------------------------------------------------------------------------------------ numbers
class Ctx:
    """One evaluation: the number type, the margins, the mutation, which open decisions to flip — and what was open."""

    def __init__(self, f32=False, k=None, kt=None, mut=None, flips=(), computed_tables=False):
        self.f32, self.mut, self.flips, self.computed_tables = f32, mut, flips, computed_tables
        self.eps, self.eps_t = (K if k is None else k) * U, (KT if kt is None else kt) * U
        self.open = {}

    def num(self, x):
        """an exact input"""
        v = np.asarray(x, F32)
        return Num(self, v if self.f32 else v.astype(F64), None)

    def table(self, x):
        """a per-triangle constant the host derived (geometric normal, area): exact for the kernels, which read the host's float32
        number; computed_tables: the oracle forms it afresh in its own build's arithmetic (six operations and a square root)"""
        r = self.num(x)
        return Num(self, r.v, 8 * self.eps * np.maximum(np.abs(r.v), 1.0)) if self.computed_tables and not self.f32 else r

    def const(self, x, like):
        return Num(self, np.full(like.v.shape, x, like.v.dtype), None)

    def decide(self, site, cond, open_):
        if self.f32:
            return cond
        self.open[site] = self.open.get(site, False) | open_
        return cond ^ (open_ & (site in self.flips or "*" in self.flips))


def _rep(v):
    with np.errstate(all="ignore"):
        return v.astype(F32).astype(F64) == v


class Num:
    __slots__ = ("c", "v", "e")

    def __init__(self, c, v, e):
        self.c, self.v = c, v
        self.e = None if c.f32 else (np.zeros(v.shape) if e is None else e)

    def _o(self, b):
        return b if isinstance(b, Num) else self.c.const(b, self)

    def _r(self, v, e, exact_ok=True, t=False):
        """the result of one rounded operation: e = what the operands hand on"""
        if self.c.f32:
            return Num(self.c, v, None)
        with np.errstate(all="ignore"):
            exact = (e == 0) & _rep(v) & exact_ok
            e = np.where(exact, 0.0, e + (self.c.eps_t if t else self.c.eps) * np.abs(v) + TINY)
            e = np.where((np.isnan(e) & ~np.isnan(v)) | (~exact & (np.abs(v) + e > FLT_MAX)), np.inf, e)          # float32 may have overflowed
        return Num(self.c, v, e)

    def __neg__(self):
        return Num(self.c, -self.v, self.e)

    def __abs__(self):
        return Num(self.c, np.abs(self.v), self.e)

    def __add__(self, b):
        b = self._o(b)
        with np.errstate(all="ignore"):
            return self._r(self.v + b.v, None if self.c.f32 else self.e + b.e)

    def __sub__(self, b):
        b = self._o(b)
        with np.errstate(all="ignore"):
            return self._r(self.v - b.v, None if self.c.f32 else self.e + b.e)

    def __mul__(self, b):
        b = self._o(b)
        with np.errstate(all="ignore"):
            e = None if self.c.f32 else np.where((self.e == 0) & (b.e == 0), 0.0, np.abs(self.v) * b.e + np.abs(b.v) * self.e + self.e * b.e)
            return self._r(self.v * b.v, e)
    __radd__, __rmul__ = __add__, __mul__

    def mul_rn(self, b):
        """a product that goes straight into a conversion (nothing to contract it with): of exact operands it is THE float32 product"""
        r = self * b
        if self.c.f32:
            return r
        b = self._o(b)
        with np.errstate(all="ignore"):
            det = (self.e == 0) & (b.e == 0)
            return Num(self.c, np.where(det, r.v.astype(F32).astype(F64), r.v), np.where(det, 0.0, r.e))

    def __rsub__(self, b):
        return self._o(b) - self

    def _image(self, f, lo_clip=None, hi_clip=None):
        """|f(v +- e) - f(v)| at its largest, f monotone on the interval; inf where the interval leaves f's domain"""
        with np.errstate(all="ignore"):
            lo, hi = self.v - self.e, self.v + self.e
            out = np.zeros(self.v.shape, bool)
            if lo_clip is not None:
                out |= lo < lo_clip; lo = np.maximum(lo, lo_clip)
            if hi_clip is not None:
                out |= hi > hi_clip; hi = np.minimum(hi, hi_clip)
            f0 = f(self.v)
            w = np.maximum(np.abs(f(lo) - f0), np.abs(f(hi) - f0))
            return np.where(self.e == 0, 0.0, np.where(np.isfinite(w), w, np.inf)), out

    def rcp(self):
        with np.errstate(all="ignore"):
            one = self.v.dtype.type(1)
            v = one / self.v
            if self.c.f32:
                return Num(self.c, v, None)
            w, _ = self._image(lambda x: 1.0 / x)
            w = np.where((np.abs(self.v) <= self.e) & (self.e > 0), np.inf, w)          # the interval holds 0
            m, _ = np.frexp(self.v)
            return self._r(v, w, exact_ok=np.abs(m) == 0.5)

    def sqrt(self):
        with np.errstate(all="ignore"):
            v = np.sqrt(self.v)
            if self.c.f32:
                return Num(self.c, v, None)
            w, _ = self._image(np.sqrt, lo_clip=0.0)
            return self._r(v, w, exact_ok=(self.v == 0) | (self.v == 1))

    def rsq(self):
        with np.errstate(all="ignore"):
            v = self.v.dtype.type(1) / np.sqrt(self.v)
            if self.c.f32:
                return Num(self.c, v, None)
            w, _ = self._image(lambda x: 1.0 / np.sqrt(x), lo_clip=0.0)
            w = np.where((self.v <= self.e) & (self.e > 0), np.inf, w)
            return self._r(v, w, exact_ok=False)

    def _trig(self, f):
        with np.errstate(all="ignore"):
            v = f(self.v)
            return Num(self.c, v, None) if self.c.f32 else self._r(v, self.e, exact_ok=self.v == 0, t=True)

    def sin(self):
        return self._trig(np.sin)

    def cos(self):
        return self._trig(np.cos)

    def acos(self, site):
        """acosf: NaN outside [-1, 1]; OPEN where the operand's interval crosses +-1 (the other answer is NaN)"""
        with np.errstate(all="ignore"):
            v = np.arccos(self.v)
            if self.c.f32:
                return Num(self.c, v, None)
            w, out = self._image(np.arccos, lo_clip=-1.0, hi_clip=1.0)
            inside = np.abs(self.v) <= 1
            flip = self.c.decide(site, inside, out & inside & (self.e > 0)) != inside
            r = self._r(v, w, exact_ok=np.abs(self.v) == 1, t=True)
            return Num(self.c, np.where(flip, np.nan, r.v), r.e)

    def lt(self, b, site):
        """self < b, OPEN while the two intervals touch"""
        b = self._o(b)
        with np.errstate(all="ignore"):
            cond = self.v < b.v
            return cond if self.c.f32 else self.c.decide(site, cond, (np.abs(self.v - b.v) <= self.e + b.e) & ((self.e > 0) | (b.e > 0)))

    def gt(self, b, site):
        return self._o(b).lt(self, site)

    def _to_int(self, f, site):
        with np.errstate(all="ignore"):
            safe = lambda x: np.where(np.isfinite(x), np.clip(x, -2.0 ** 31, 2.0 ** 31 - 1), 0.0)      # v_cvt_i32_f32 saturates, NaN -> 0
            nat = f(safe(self.v.astype(F64))).astype(np.int64)
            if self.c.f32:
                return nat
            lo, hi = f(safe(self.v - self.e)).astype(np.int64), f(safe(self.v + self.e)).astype(np.int64)
            flip = self.c.decide(site, np.zeros(nat.shape, bool), lo != hi)
            return np.where(flip, np.where(nat == lo, hi, lo), nat)

    def trunc(self, site):
        return self._to_int(np.trunc, site)

    def floor_int(self, site):
        return self._to_int(np.floor, site)

    def floor(self):
        """floorf as a number (the decision is taken where the integer is formed from it)"""
        return Num(self.c, np.floor(self.v), None if self.c.f32 else np.zeros(self.v.shape))


def where(cond, a, b):
    return Num(a.c, np.where(cond, a.v, b.v), None if a.c.f32 else np.where(cond, a.e, b.e))


def atan2(y, x, site="cut"):
    with np.errstate(all="ignore"):
        v = np.arctan2(y.v, x.v)
        if y.c.f32:
            return Num(y.c, v, None)
        r2 = x.v * x.v + y.v * y.v
        e = np.where((x.e == 0) & (y.e == 0), 0.0, (np.abs(x.v) * y.e + np.abs(y.v) * x.e) / np.maximum(r2 - (x.e + y.e) * np.sqrt(r2), 0.0))
        # the cut: with y within its own error of 0 behind x < 0 the answer may be near +pi or near -pi (the same direction): OPEN
        e = np.where((np.abs(x.v) <= x.e) & (np.abs(y.v) <= y.e), np.inf, e)          # the origin, exact zeros included: any angle (the signs of the zeros decide)
        other = y.c.decide(site, np.zeros(v.shape, bool), (x.v < 0) & (np.abs(y.v) <= y.e) & (y.e > 0))
        v = np.where(other, np.where(v > 0, v - 2 * np.pi, v + 2 * np.pi), v)
        return y._r(v, e, exact_ok=(y.v == 0) & (x.v > 0), t=True)


def from_int(c, i, like):
    return Num(c, np.asarray(i).astype(like.v.dtype), None)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def normalize(a):
    r = dot(a, a).rsq()
    return [a[0] * r, a[1] * r, a[2] * r]


def vec(c, x):
    return [c.num(x[:, k]) for k in range(3)]


def clampi(i, lo, hi):
    return np.minimum(np.maximum(i, lo), hi)


# ------------------------------------------------------------------------------------------------------------- scenes
def normals_arrays():
    """A quad in the plane y = 0 whose vertex normals oppose at the two ends of its diagonal ((0, 1, 0) and (0, -1, 0); the other two are
    tilted): the interpolated normal of either triangle is exactly 0 at the quad's centre.  A small light above, so that the scene has one."""
    v = np.array([[-1, 0, -1, 0, 0, 0, 1, 0], [1, 0, -1, 1, 0, 0.6, 0.8, 0], [1, 0, 1, 1, 1, 0, -1, 0], [-1, 0, 1, 0, 1, 0, 0.8, 0.6],
                  [-0.25, 3, -0.25, 0, 0, 0, -1, 0], [0.25, 3, -0.25, 1, 0, 0, -1, 0], [0.25, 3, 0.25, 1, 1, 0, -1, 0]], np.float32)
    t = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6]], np.int32)
    return geometry.from_arrays(v, t, [0, 2, 3], None, [[0, 0, 0], [5, 5, 5]])


def quad_arrays():
    v = np.array([[-1, 0, -1, 0, 0, 0, 1, 0], [-1, 0, 1, 0, 1, 0, 1, 0], [1, 0, 1, 1, 1, 0, 1, 0], [1, 0, -1, 1, 0, 0, 1, 0]], np.float32)
    return geometry.from_arrays(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32))


MAP_W, MAP_H = 8, 4


@functools.lru_cache(None)
def env_tables():
    """(tex (8, 8, 4), alias_prob, alias_idx, pdf) by hand.  Texels are multiples of 1/8 (each of the 8 x 4 rows repeated: the map made
    square), different in every column and row.  The alias tables (4 marginal entries, then 4 rows of 8) hold probability exactly 0,
    exactly 1 and 1/2 with an alias five entries away, besides 1/4, 3/4 and two values that are no float32 fraction of a power of
    two; the pdf is different in every texel, so that a wrong column or row is a wrong number."""
    y, x = np.meshgrid(np.arange(MAP_H), np.arange(MAP_W), indexing="ij")
    t4 = np.stack([(1 + x + 8 * y) / 8.0, (2 + 3 * x + y) / 8.0, (40 - x - 8 * y) / 8.0, np.ones_like(x, float)], -1)
    tex = np.repeat(t4, 2, axis=0).astype(F32)
    cyc = np.array([0.0, 1.0, 0.5, 0.25, 0.75, 0.3, 0.5, 0.9], F32)
    prob = np.concatenate([np.array([0.5, 0.0, 1.0, 0.7], F32)] + [np.roll(cyc, r) for r in range(MAP_H)]).astype(F32)
    alias = np.concatenate([(np.arange(MAP_H) + 2) % MAP_H] + [(np.arange(MAP_W) + 5) % MAP_W] * MAP_H).astype(np.int32)
    pdf = (0.25 + (x + 8 * y) / 32.0 + ((x * y) % 3) / 3.0).astype(F32).reshape(-1)
    assert len(set(pdf.tolist())) == MAP_W * MAP_H
    return np.ascontiguousarray(tex), prob, alias, pdf


@functools.lru_cache(None)
def scene_arrays(name):
    from many_lights import chandelier_arrays
    base = name[:-4] if name.endswith("_env") else name
    if base == "cbox":
        return geometry.assemble(cbox_models())
    return {"stage": multi_light_arrays, "chandelier": chandelier_arrays, "quad": quad_arrays, "normals": normals_arrays,
            "terrain": lambda: terrain_arrays(n=14)}[base]()


class Tables:
    """What the kernels read of a scene, as float32 (the host's IEEE operations repeated one by one: csrc/zdr_api.cpp, world_records)."""

    def __init__(self, name):
        A = scene_arrays(name)
        self.name, self.A = name, A
        self.env = env_tables() if name.endswith("_env") else None
        self.env_count = 1 if self.env else 0
        nt = A.tris.shape[0]
        self.begin = np.asarray(A.inst_tri_begin, np.int64)
        self.tri_inst = np.repeat(np.arange(A.ninst), np.diff(self.begin))
        X = np.asarray(A.inst_xform, F32).reshape(-1, 16)[self.tri_inst]                      # (nt, 16)
        V = np.asarray(A.verts, F32)[A.tris]                                                  # (nt, 3, 8)
        with np.errstate(all="ignore"):
            m = lambda k: X[:, k][:, None]
            x, y, z = V[..., 0], V[..., 1], V[..., 2]
            self.P = np.stack([m(0) * x + m(1) * y + m(2) * z + m(3), m(4) * x + m(5) * y + m(6) * z + m(7), m(8) * x + m(9) * y + m(10) * z + m(11)], -1)
            a, b, c, d, e, f, g, h, i = (X[:, k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
            co = [e * i - f * h, f * g - d * i, d * h - e * g, c * h - b * i, a * i - c * g, b * g - a * h, b * f - c * e, c * d - a * f, a * e - b * d]
            inv = F32(1.0) / (a * co[0] + b * co[1] + c * co[2])
            nm = [(q * inv)[:, None] for q in co]
            nx, ny, nz = V[..., 5], V[..., 6], V[..., 7]
            self.N = np.stack([nm[0] * nx + nm[1] * ny + nm[2] * nz, nm[3] * nx + nm[4] * ny + nm[5] * nz, nm[6] * nx + nm[7] * ny + nm[8] * nz], -1)
            e1, e2 = self.P[:, 1] - self.P[:, 0], self.P[:, 2] - self.P[:, 0]
            cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
            d2 = cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1] + cr[:, 2] * cr[:, 2]
            self.ng = cr * (F32(1.0) / np.sqrt(d2))[:, None]
            self.area = np.sqrt(d2) / F32(2.0)
        self.UV = V[..., 3:5]
        for q in (self.P, self.N, self.ng, self.area):
            assert q.dtype == F32
        E = np.asarray(A.inst_emission, F32).reshape(-1, 3)
        self.emission = E
        self.lights = np.flatnonzero((E > 0).any(1))                                          # instances, in list order
        self.light_count = len(self.lights)
        self.n = self.env_count + self.light_count
        assert nt == self.begin[-1]

    def light_tris(self, l):
        i = self.lights[l]
        return np.arange(self.begin[i], self.begin[i + 1])


@functools.lru_cache(None)
def tables(name):
    return Tables(name)


# --------------------------------------------------------------------------------------------------- the formulas
def sample_uniform_triangle(c, ux, uy):                          # light.py:16-20
    # (mut "tri_le", u.x <= u.y, is NOT a mistake: on the diagonal both branches return (u / 2, u / 2, 1 - u) in the same operations.
    #  The host test holds it to bit-equality; the mistake that is rejected is the two branches swapped.)
    lt = ~(uy.lt(ux, "tri")) if c.mut == "tri_le" else ux.lt(uy, "tri")
    if c.mut == "tri_swapped":
        lt = ~lt
    ax, ay = ux * 0.5, ux * -0.5 + uy
    bx, by = uy * -0.5 + ux, uy * 0.5
    x, y = where(lt, ax, bx), where(lt, ay, by)
    return [x, y, (1.0 - x) - y]


def light_pdf(c, origin, p, ln, area, nT):                       # light.py:69-73, 105-110
    dp = [p[k] - origin[k] for k in range(3)]
    wi = normalize(dp)
    cos = dot(ln, wi) if c.mut == "cos_without_sign" else -dot(ln, wi)
    sqr = dot(dp, dp)
    return sqr * ((nT * area) * cos).rcp(), wi, cos, sqr


def uv_to_direction(c, u, v):                                    # envmap.py:206-214
    phi, theta = (1.0 - u) * TWO_PI32, v * PI32
    st = theta.sin()
    return normalize([phi.sin() * st, theta.cos(), phi.cos() * st])


def direction_to_uv(c, d, at=""):                                # envmap.py:216-220, u wrapped into [0, 1)
    a = atan2(d[0], d[2], at + "cut") * INV_TWO_PI32
    wrapped = 1.0 - a
    u = wrapped if c.mut == "u_not_wrapped" else where(a.gt(0.0, at + "seam"), wrapped, -a)
    return u, d[1].acos(at + "pole") * INV_PI32


def env_pdf_scale(c, v, n):                                      # 1 / (sin(pi v) 2 pi^2 n)
    sn = (v * PI32).sin()
    inv = where(sn.gt(0.0, "sin"), sn.rcp(), c.const(0.0, sn))
    return inv * (from_int(c, n, v) * TWO_PI_SQ32).rcp()


def env_lookup(c, T, u, v):                                      # bilinear between texel centres, clamp to edge
    tex = T.env[0]
    H, W = tex.shape[:2]
    x, y = u * float(W) - 0.5, v * float(H) - 0.5
    x0f, y0f = x.floor(), y.floor()
    fx, fy = x - x0f, y - y0f
    ix, iy = x.floor_int("tex_x"), y.floor_int("tex_y")
    if not c.f32:       # an open floor: the fraction belongs to the cell that was chosen
        fx, fy = where(ix == x0f.v, fx, x - from_int(c, ix, x)), where(iy == y0f.v, fy, y - from_int(c, iy, y))
    x0, x1, y0, y1 = clampi(ix, 0, W - 1), clampi(ix + 1, 0, W - 1), clampi(iy, 0, H - 1), clampi(iy + 1, 0, H - 1)
    out = []
    for k in range(3):
        c00, c10, c01, c11 = (c.num(tex[yy, xx, k]) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
        top, bot = c00 + (c10 - c00) * fx, c01 + (c11 - c01) * fx
        out.append(top + (bot - top) * fy)
    return out


def sample_alias_table(c, T, n, u_in, offset, site):             # envmap.py:85-106
    prob_t, alias_t = T.env[1], T.env[2]
    u = u_in * float(n)
    i = clampi(u.trunc(site + "_i"), 0, n - 1)
    ur = u - u.floor()
    prob = c.num(prob_t[i + offset])
    own = ur.lt(prob, site + "_p")
    one_m = 1.0 - prob
    uu_alias = (ur - prob) if c.mut == "alias_uu_unscaled" else (ur - prob) * one_m.rcp()
    with np.errstate(all="ignore"):
        uu = where(own, ur * prob.rcp(), uu_alias)
    return np.where(own, i, alias_t[i + offset]), uu


def env_sampled_light_pdf(c, T, d, n):                           # envmap.py:240-248
    u, v = direction_to_uv(c, d)
    if c.mut == "pdf_index_x_for_y":
        iy, ix = clampi((u * float(MAP_H)).trunc("pdf_y"), 0, MAP_H - 1), clampi((v * float(MAP_W)).trunc("pdf_x"), 0, MAP_W - 1)
    else:
        iy, ix = clampi((v * float(MAP_H)).trunc("pdf_y"), 0, MAP_H - 1), clampi((u * float(MAP_W)).trunc("pdf_x"), 0, MAP_W - 1)
    return c.num(T.env[3][iy * MAP_W + ix]) * env_pdf_scale(c, v, n), iy * MAP_W + ix


def eval_sample(c, T, rows):
    """ZDR_LIGHT_SAMPLE -> {name: Num or int array}"""
    m = len(rows)
    origin = vec(c, rows)
    u_pick, u_prim, ux, uy = (c.num(rows[:, k]) for k in (3, 4, 5, 6))
    n = T.light_count if c.mut == "n_without_env" else T.n
    z = c.const(0.0, u_pick)
    out = {"wi": [z, z, c.const(1.0, z)], "dist": z, "pdf": c.const(1.0, z), "eval": [z, z, z], "env_uv": [c.const(-1.0, z)] * 2,
           "mesh_light": np.full(m, -1), "env": np.zeros(m, bool)}
    if T.n <= 0:
        return out
    idx = clampi(u_pick.mul_rn(float(n)).trunc("pick"), 0, max(n, 1) - 1)
    is_env = idx < T.env_count
    sel = lambda a, b, cond: [where(cond, p, q) for p, q in zip(a, b)]
    if T.env_count:
        iy, uy_ = sample_alias_table(c, T, MAP_H, uy, 0, "ay")
        ix, ux_ = sample_alias_table(c, T, MAP_W, ux, MAP_H + iy * MAP_W, "ax")
        eu, ev = (from_int(c, ix, ux_) + ux_) * (1.0 / MAP_W), (from_int(c, iy, uy_) + uy_) * (1.0 / MAP_H)
        e_wi = uv_to_direction(c, eu, ev)
        e_pdf = c.num(T.env[3][iy * MAP_W + ix]) * env_pdf_scale(c, ev, n)
        e_eval = env_lookup(c, T, eu, ev)
        out["alias"] = iy * MAP_W + ix
    if T.light_count:
        l = clampi(idx - T.env_count, 0, T.light_count - 1)
        inst = T.lights[l]
        Tn = (T.begin[inst + 1] - T.begin[inst])
        prim = clampi(u_prim.mul_rn(from_int(c, Tn, u_prim)).trunc("prim"), 0, Tn - 1)
        tri = T.begin[inst] + prim
        abc = sample_uniform_triangle(c, ux, uy)
        P = [[c.num(T.P[tri, j, k]) for k in range(3)] for j in range(3)]
        p = [(P[0][k] * abc[0] + P[1][k] * abc[1]) + P[2][k] * abc[2] for k in range(3)]
        ln, area = [c.table(T.ng[tri, k]) for k in range(3)], c.table(T.area[tri])
        pdf, wi, cos, sqr = light_pdf(c, origin, p, ln, area, from_int(c, n * Tn, u_prim))
        dist = sqr.sqrt() if c.mut == "dist_without_9999" else sqr.sqrt() * C9999
        front = cos.gt(C4, "front")
        m_eval = [where(front, c.num(T.emission[inst, k]), z) for k in range(3)]
        out["tri"] = np.where(is_env, -1, tri)
        out["p"] = p
    if T.env_count and T.light_count:
        out.update(wi=sel(e_wi, wi, is_env), dist=where(is_env, c.const(1e30, z), dist), pdf=where(is_env, e_pdf, pdf), eval=sel(e_eval, m_eval, is_env),
                   env_uv=sel([eu, ev], out["env_uv"], is_env), mesh_light=np.where(~is_env & front, l, -1), env=is_env)
    elif T.env_count:
        out.update(wi=e_wi, dist=c.const(1e30, z), pdf=e_pdf, eval=e_eval, env_uv=[eu, ev], env=np.ones(m, bool))
    else:
        out.update(wi=wi, dist=dist, pdf=pdf, eval=m_eval, mesh_light=np.where(front, l, -1))
    return out


def eval_pdf(c, T, rows, p=None):
    """ZDR_LIGHT_PDF -> pdf (both forms of the kernel compute it); p: the point as numbers with a bound, in place of the row's"""
    inst, tri = rows[:, 6].view(np.int32).astype(np.int64), rows[:, 7].view(np.int32).astype(np.int64)
    n = T.light_count if c.mut == "n_without_env" else T.n
    Tn = T.begin[inst + 1] - T.begin[inst]
    pdf, _, _, _ = light_pdf(c, vec(c, rows), vec(c, rows[:, 3:6]) if p is None else p, [c.table(T.ng[tri, k]) for k in range(3)], c.table(T.area[tri]), from_int(c, n * Tn, c.num(rows[:, 0])))
    return {"pdf": pdf}


def eval_env(c, T, rows, d=None):
    d = vec(c, rows) if d is None else d                         # d: the direction as numbers with a bound, in place of the row's
    u, v = c.num(rows[:, 3]), c.num(rows[:, 4])
    n = T.light_count if c.mut == "n_without_env" else T.n
    du, dv = direction_to_uv(c, d)
    pdf, index = env_sampled_light_pdf(c, T, d, n)
    w = uv_to_direction(c, u, v)
    bu, bv = direction_to_uv(c, w, "back_")
    return {"duv": [du, dv], "pdf": pdf, "lookup": env_lookup(c, T, du, dv), "w": w, "back": [bu, bv], "scale": env_pdf_scale(c, v, n), "index": index}


def offset1(c, p, n):                                            # Waechter & Binder, as LuisaCompute's offset_ray_origin
    s = n * 256.0
    of_i = s.floor_int("of_i") if c.mut == "offset_floor" else s.trunc("of_i")
    pb = p.v.astype(F32).view(np.int32).astype(np.int64)
    neg = np.zeros(p.v.shape, bool) if c.mut == "offset_not_negated" else (p.v < 0)
    with np.errstate(all="ignore"):
        pi = ((pb + np.where(neg, -of_i, of_i) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32).view(F32)
    return where(abs(p).lt(1.0 / 32.0, "near"), p + n * (1.0 / 65536.0), c.num(pi))


def tent_warp1(c, u):                                            # camera.py:20-31, radius 1
    return where(u.lt(0.5, "tent"), (u * 2.0).sqrt() - 1.0, 1.0 - (2.0 - u * 2.0).sqrt())


def eval_misc(c, T, rows):
    a, b = c.num(rows[:, 0]), c.num(rows[:, 1])
    s = a + b
    with np.errstate(all="ignore"):
        mx = where(s.v >= C4, s, c.const(C4, s)) if c.f32 else where(c.decide("bh", s.v >= C4, (np.abs(s.v - C4) <= s.e) & (s.e > 0)), s, c.const(C4, s))
    mx = where(np.isnan(s.v), c.const(C4, s), mx)                # fmaxf returns the number
    p, n = vec(c, rows[:, 2:5]), vec(c, rows[:, 5:8])
    return {"bh": a * mx.rcp(), "offset": [offset1(c, p[k], n[k]) for k in range(3)],
            "tri": sample_uniform_triangle(c, c.num(rows[:, 8]), c.num(rows[:, 9])), "tent": tent_warp1(c, c.num(rows[:, 10]))}


def eval_interact(c, T, inst, prim, u, v):
    """surface_interact at the hit (inst, prim, u, v) — the barycentrics of input corners 1 and 2 — of input triangle begin[inst] + prim"""
    tri = T.begin[inst] + prim
    w1, w2 = c.num(u), c.num(v)
    w0 = (1.0 - w1) - w2
    if not c.f32:       # the kernel interpolates at the SLOT's barycentrics, of which the reported pair may be a rotation: the weight that
        w0 = Num(c, w0.v, w0.e + c.eps)      # was 1 - u' - v' there was rounded at magnitude 1 whatever is left of it — an absolute term
    P, N = [vec(c, T.P[tri, j]) for j in range(3)], [vec(c, T.N[tri, j]) for j in range(3)]
    p = [(P[0][k] * w0 + P[1][k] * w1) + P[2][k] * w2 for k in range(3)]
    uv = [(w0 * c.num(T.UV[tri, 0, k]) + w1 * c.num(T.UV[tri, 1, k])) + w2 * c.num(T.UV[tri, 2, k]) for k in range(2)]
    ns = [(N[0][k] * w0 + N[1][k] * w1) + N[2][k] * w2 for k in range(3)]
    return {"p": p, "uv": uv, "ns": ns if c.mut == "ns_unnormalised" else normalize(ns), "ng": [c.table(T.ng[tri, k]) for k in range(3)]}


# ----------------------------------------------------------------------------------------------------------- families
def _f32(x):
    return np.asarray(x, F32)


def near(x):
    """x and the float32 numbers on either side of it"""
    x = _f32(x).reshape(-1)
    lo, hi = np.nextafter(x, F32(-np.inf)), np.nextafter(x, F32(np.inf))
    return np.concatenate([np.where(x == 0, F32(-2.0 ** -24), lo), x, np.where(x == 0, F32(2.0 ** -24), hi)])      # (0: 2^-24, not a subnormal)


def unit_interval(vals):
    v = _f32(vals)
    return np.unique(v[(v >= 0) & (v < 1)])


def _rows(m):
    return np.zeros((m, 16), F32)


def _origins(T, rng, tris, count):
    """origins against light triangles `tris`: generic, 1e-3 / 1e-5 / 0 above the plane, behind it, far away, at a vertex"""
    tri = tris[rng.integers(len(tris), size=count)]
    P, ng = T.P[tri].astype(F64), T.ng[tri].astype(F64)
    w = rng.dirichlet((1, 1, 1), count)
    foot = (P * w[:, :, None]).sum(1)
    side = rng.standard_normal((count, 3))
    side -= (side * ng).sum(1, keepdims=True) * ng
    kind = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 7, 4, 5, 0, 7])[np.arange(count) % 16]       # in the plane and at a vertex: one row in sixteen each
    h = np.choose(kind, [0, 1e-3, 1e-5, 0.0, -0.5, 1e4, 0, 0])[:, None]
    o = foot + h * ng + np.where(kind[:, None] >= 1, 0.7 * side, 0)
    gen = kind == 0
    o[gen] = foot[gen] + rng.uniform(0.2, 3.0, (gen.sum(), 1)) * (ng[gen] + 0.8 * side[gen])
    o[kind == 6] = P[kind == 6, 0]                                # exactly a vertex of the light
    o[kind == 7] = foot[kind == 7] + rng.uniform(0.5, 2.0, ((kind == 7).sum(), 1)) * ng[kind == 7]      # straight above
    return _f32(o), tri


@functools.lru_cache(None)
def family(name, scene):
    """-> (mode, rows (n, 16) float32, read-only)"""
    T = tables(scene)
    rng = np.random.default_rng(sum(map(ord, name + scene)))
    if name == "sample":
        n = max(T.n, 1)
        grid = [k / n for k in range(n + 1)]
        picks = unit_interval(np.concatenate([near(grid), [0.0, ONE_M], rng.uniform(0, 1, 8)]))
        counts = sorted({len(T.light_tris(l)) for l in range(T.light_count)} | {1})
        prims = unit_interval(np.concatenate([near([k / t for t in counts for k in range(t + 1)]), [0.0, ONE_M, 0.5, 0.25], rng.uniform(0, 1, 6)]))
        d = unit_interval(np.concatenate([[0.0, 0.25, 0.5, 0.75, ONE_M], rng.uniform(0, 1, 4)]))
        pts = [(a, b) for a in d for b in np.concatenate([near([a]), [0.0, ONE_M]]) if 0 <= b < 1]
        pts += [(0.0, b) for b in d] + [(a, 0.0) for a in d] + [(ONE_M, b) for b in d] + [(float(a), float(b)) for a, b in rng.uniform(0, 1, (24, 2))]
        pts += [(k / 16.0, j / 16.0) for k in range(16) for j in range(0, 16, 3)]                     # the lattice the 8 x 4 map is exact on
        combos = list(itertools.product(picks, prims[:: max(1, len(prims) // 12)], range(0, len(pts), 7)))
        combos += [(picks[i % len(picks)], prims[i % len(prims)], i % len(pts)) for i in range(len(prims) * 3 + len(pts))]
        sel = rng.permutation(len(combos))[:4000] if len(combos) > 4000 else np.arange(len(combos))
        rows = _rows(len(sel))
        tris = np.concatenate([T.light_tris(l) for l in range(T.light_count)]) if T.light_count else np.arange(T.P.shape[0])
        rows[:, 0:3], _ = _origins(T, rng, tris, len(sel))
        for r, k in enumerate(sel):
            rows[r, 3], rows[r, 4] = combos[k][0], combos[k][1]
            rows[r, 5:7] = pts[combos[k][2]]
        mode = "sample"
    elif name == "pdf":
        tris = np.concatenate([T.light_tris(l) for l in range(T.light_count)])
        m = max(400, 40 * len(tris))
        rows = _rows(m)
        rows[:, 0:3], tri = _origins(T, rng, tris, m)
        w = rng.dirichlet((1, 1, 1), m)
        w[::5] = np.eye(3)[rng.integers(3, size=len(w[::5]))]                                         # at a corner
        rows[:, 3:6] = _f32((T.P[tri].astype(F64) * w[:, :, None]).sum(1))
        same = np.arange(m) % 17 == 3
        rows[same, 0:3] = rows[same, 3:6]                                                             # origin = p
        rows[:, 6] = T.tri_inst[tri].astype(np.int32).view(F32)
        rows[:, 7] = tri.astype(np.int32).view(F32)
        mode = "pdf"
    elif name == "env":
        th = np.linspace(0.02, np.pi - 0.02, 91) + 0.003
        ph = np.linspace(-np.pi, np.pi, 96, endpoint=False) + 0.013
        g = np.array([[np.sin(t) * np.sin(p), np.cos(t), np.sin(t) * np.cos(p)] for t in th for p in ph]
                     + [[np.sin(t) * np.sin(p), np.cos(t), np.sin(t) * np.cos(p)] for t in near([np.pi / 2]).astype(F64) for p in (-2.0, 1.1)])
        tiny = [0.0, -0.0, 1e-30, -1e-30, 1e-8, -1e-8, 2.0 ** -24, -2.0 ** -24]
        seam = [[x, 0.3, z] for x in tiny for z in (1.0, 0.5, -1.0)] + [[x, -0.8, 1.0] for x in tiny]
        one_up = float(np.nextafter(F32(1), F32(2)))
        poles = [[0, 1, 0], [0, -1, 0], [0, one_up, 0], [0, -one_up, 0], [1e-4, 1, 0], [-1e-4, 1, 1e-4], [1e-4, -1, -1e-4], [2e-4, ONE_M, 0], [-2e-4, -ONE_M, 1e-4]]
        cols = near(np.arange(0, MAP_W + 1) / MAP_W).astype(F64)                                      # the sample map's column borders, and the texture's (8 wide too)
        rows_b = near(np.arange(0, MAP_H + 1) / MAP_H).astype(F64)
        border = [[np.sin(np.pi * v) * np.sin(2 * np.pi * (1 - u)), np.cos(np.pi * v), np.sin(np.pi * v) * np.cos(2 * np.pi * (1 - u))] for u in cols for v in (0.3,)]
        border += [[np.sin(np.pi * v) * np.sin(2 * np.pi * (1 - u)), np.cos(np.pi * v), np.sin(np.pi * v) * np.cos(2 * np.pi * (1 - u))] for v in rows_b for u in (0.7,)]
        d = _f32(np.concatenate([g, seam, poles, border]))
        us = np.concatenate([[0.3, 0.9], (np.arange(64) + 0.37) / 64])
        uvs = _f32([(u, v) for u in us for v in (0.5, 0.25, 0.125, 0.3, 0.77, 0.91)] + [(u, v) for u in np.concatenate([cols, [0.0, ONE_M]]) for v in (0.5, 0.3, 0.77) if 0 <= u <= 1]
                   + [(u, v) for u in (0.3, 0.625, 0.9) for v in (0.0, 2.0 ** -24, ONE_M, 1.0)])
        rows = _rows(max(len(d), len(uvs)))
        rows[:, 0:3] = d[:len(rows)]
        rows[:, 3:5] = _f32(np.stack([rng.uniform(0.01, 0.99, len(rows)), rng.uniform(0.03, 0.97, len(rows))], 1))
        rows[:len(uvs), 3:5] = uvs
        mode = "env"
    elif name == "alias":
        prob = T.env[1]
        uy = [k / MAP_H for k in range(MAP_H + 1)] + [(k + float(prob[k])) / MAP_H for k in range(MAP_H)]
        ux = [k / MAP_W for k in range(MAP_W + 1)] + [(k + float(prob[MAP_H + r * MAP_W + k])) / MAP_W for r in range(MAP_H) for k in range(MAP_W)]
        ux = unit_interval(np.concatenate([near(ux), [ONE_M, 0.0], (np.arange(32) + 0.5) / 32]))
        uy = unit_interval(np.concatenate([near(uy), [ONE_M, 0.0], (np.arange(16) + 0.5) / 16]))
        combos = [(a, b) for a in ux for b in (0.15625, 0.28125, 0.40625, 0.53125, 0.65625, 0.78125, 0.90625, 0.03125, 0.33, 0.71)]
        combos += [(a, b) for b in uy for a in (0.046875, 0.34375, 0.578125, 0.890625, 0.21, 0.77)]
        combos += [((i + 0.37) / 60, (j + 0.41) / 60) for i in range(60) for j in range(60)]
        rows = _rows(len(combos))
        rows[:, 5:7] = _f32(combos)
        rows[:, 0:3] = (0.1, 0.5, -0.2)
        rows[:, 3] = 0.0                                                                              # u_pick = 0: the environment is light 0
        mode = "sample"
    elif name == "misc":
        ab = [(a, b) for a in (0.0, 1e-5, 4e-5, 6e-5, 1e-4, 0.3, 7.0, np.inf, 1e30) for b in (0.0, 2e-5, 5e-5, 6e-5, 1e-4, 0.4, 1e30)]
        ab += [tuple(x) for x in rng.uniform(0, 2, (40, 2))] + [tuple(x) for x in rng.uniform(0, 1e-4, (40, 2))]
        ps = np.concatenate([near([1 / 32, -1 / 32, 1.0, -1.0, 2.0, 0.5, -4.0, 1 / 64, 1024.0]), [0.0, -0.0, 0.3, -0.3, 0.03, -0.03, 100.0, -7.5], rng.uniform(-3, 3, 12)])
        ns = np.concatenate([[0.0, -0.0, 1.0, -1.0, 1 / 512, -1 / 512, 1 / 256, -1 / 256, 0.5, -0.5, 0.0039, -0.0039, 0.7071, -0.7071], rng.uniform(-1, 1, 8)])
        pn = list(itertools.product(ps, ns))
        d = unit_interval(np.concatenate([[0.0, 0.25, 0.5, 0.75, ONE_M, 0.125], rng.uniform(0, 1, 6)]))
        uu = [(a, b) for a in d for b in np.concatenate([near([a]), [0.0, ONE_M]]) if 0 <= b < 1] + [tuple(x) for x in rng.uniform(0, 1, (60, 2))]
        ts = unit_interval(np.concatenate([near([0.5, 0.125, 0.25, 0.75]), [0.0, ONE_M, 2.0 ** -24], rng.uniform(0, 1, 30)]))
        m = len(pn)
        rows = _rows(m)
        rows[:, 0:2] = _f32(ab)[np.arange(m) % len(ab)]
        P, Nn = _f32([x[0] for x in pn]), _f32([x[1] for x in pn])
        rows[:, 2], rows[:, 5] = P, Nn
        rows[:, 3], rows[:, 6] = np.roll(P, 7), np.roll(Nn, 3)
        rows[:, 4], rows[:, 7] = np.roll(P, 31), np.roll(Nn, 11)
        rows[:, 8:10] = _f32(uu)[np.arange(m) % len(uu)]
        rows[:, 10] = ts[np.arange(m) % len(ts)]
        mode = "misc"
    elif name == "interact":
        rows = interact_rays(scene)
        mode = "interact"
    else:
        raise KeyError(name)
    rows.setflags(write=False)
    return mode, rows


def interact_rays(scene):
    """{o[3], d[3], tmin, tmax}: the `features` and `axis` rays of tests/ray_cases.py on the Cornell box and the terrain — hits at corners,
    on edges and on the diagonals of merged quads among them — and, on `normals`, rays at the point where the interpolated normal vanishes."""
    import ray_cases as rc
    if scene in ("cbox", "terrain"):
        c = rc.case(scene)
        r = np.concatenate([rc.features_rays(c, 5)[0], rc.axis_rays(c, 6)])
        if scene == "terrain":
            r = r[:: max(1, len(r) // 3000)]
    else:
        tg = [(0.0, 0.0), (2.0 ** -10, 0.0), (0.5, 0.5), (-0.5, -0.5), (0.25, -0.125), (-0.75, 0.125), (2.0 ** -12, -(2.0 ** -12)), (0.0, 2.0 ** -20)]
        o = [(x, 2.0, z) for x, z in tg] + [(x * 0.5 + 0.25, 1.0, z * 0.5 - 0.25) for x, z in tg]      # straight down, then slanted
        t = [(x, 0.0, z) for x, z in tg] * 2
        r = rc.mk(o, np.array(t) - np.array(o))
    rows = _rows(len(r))
    rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7] = r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7]
    return rows


PLAN = (("sample", ("cbox", "stage", "chandelier", "quad", "cbox_env", "quad_env")), ("pdf", ("cbox", "stage", "chandelier", "cbox_env")),
        ("env", ("cbox_env", "quad_env")), ("alias", ("quad_env",)), ("misc", ("quad",)), ("interact", ("cbox", "terrain", "normals")))
ACCEL = {"terrain": "bvh"}


# -------------------------------------------------------------------------------------------------------------- judge
SAMPLE_OUT = (("wi", 0, 3), ("dist", 3, 1), ("pdf", 4, 1), ("eval", 5, 3), ("env_uv", 8, 2))
ENV_OUT = (("duv", 0, 2), ("pdf", 2, 1), ("lookup", 3, 3), ("w", 6, 3), ("back", 9, 2), ("scale", 11, 1))
MISC_OUT = (("bh", 0, 1), ("offset", 1, 3), ("tri", 4, 3), ("tent", 7, 1))
INTERACT_OUT = (("p", 5, 3), ("uv", 8, 2), ("ns", 10, 3), ("ng", 13, 3))


def _cols(x):
    return x if isinstance(x, list) else [x]


def _within(got, ref):
    """(ok, error / bound, exact): one column of float32 answers against a Num"""
    got64 = got.astype(F64)
    with np.errstate(all="ignore"):
        exact = ref.e == 0
        same_bits = got.view(np.uint32) == ref.v.astype(F32).view(np.uint32)
        both_nan = np.isnan(got64) & np.isnan(ref.v)
        err = np.abs(got64 - ref.v)
        err = np.where(got64 == ref.v, 0.0, err)                  # inf against inf
        ok = np.where(exact, same_bits | both_nan | ((got64 == 0) & (ref.v == 0)), both_nan | (err <= ref.e))      # (a zero's sign: x * 0 takes it from an x that may be rounded)
        ratio = np.where(exact | both_nan | np.isinf(ref.e), 0.0, err / np.where(ref.e > 0, ref.e, 1.0))
    return ok, np.where(np.isfinite(ratio), ratio, np.inf), exact, np.isinf(ref.e) & ~both_nan


def compare(layout, got, ref, ints=()):
    """-> {output: (ok (n,), worst error / bound (n,), exact (n,), bound infinite (n,))}"""
    res = {}
    for name, at, w in layout:
        cols = [_within(np.ascontiguousarray(got[:, at + k]), r) for k, r in enumerate(_cols(ref[name]))]
        res[name] = (np.all([c[0] for c in cols], 0), np.max([c[1] for c in cols], 0), np.all([c[2] for c in cols], 0), np.any([c[3] for c in cols], 0))
    for name, at in ints:
        g = np.ascontiguousarray(got[:, at]).view(np.int32)
        ok = g == ref[name]
        res[name] = (ok, np.zeros(len(g)), np.ones(len(g), bool), np.zeros(len(g), bool))
    return res


class Verdict:
    def __init__(self, res, open_rows, unbounded, used):
        self.res, self.open_rows, self.unbounded, self.used = res, open_rows, unbounded, used
        self.ok = np.all([r[0] for r in res.values()], 0)

    def report(self, what):
        for name, (ok, ratio, exact, _) in self.res.items():
            print(f"[light] {what:22s} {name:10s} worst error / bound {ratio.max():.3f}   exact rows {int(exact.sum()):5d}   outside {int((~ok).sum())} of {len(ok)}")
        print(f"[light] {what:22s} open by the reference {int(self.open_rows.sum())} ({self.open_rows.mean():.4f}), bound infinite {int(self.unbounded.sum())}, accepted under a flipped decision {int(self.used.sum())}")

    def assert_all_inside(self, what):
        self.report(what)
        for name, (ok, _, _, _) in self.res.items():
            bad = np.flatnonzero(~ok)
            assert not len(bad), (what, name, f"{len(bad)} rows outside their bound", bad[:8].tolist())


def judge(name, scene, got, hit=None, **ctx_kw):
    """Every output of every row of family `name` on `scene` against the float64 reference.  A row that fails the natural branches is
    tried with each open decision flipped, then with all of them; `hit` (interact): the (inst, prim, u, v) the answers themselves report."""
    T = tables(scene)
    mode, rows = family(name, scene)

    def run(flips):
        c = Ctx(flips=flips, **ctx_kw)
        if mode == "sample":
            ref = eval_sample(c, T, rows)
            return c, compare(SAMPLE_OUT, got, ref, ints=(("mesh_light", 10),))
        if mode == "pdf":
            ref = eval_pdf(c, T, rows)
            ref["pdf_wide"] = ref["pdf"]
            return c, compare((("pdf", 0, 1), ("pdf_wide", 1, 1)), got, ref)
        if mode == "env":
            return c, compare(ENV_OUT, got, eval_env(c, T, rows))
        if mode == "misc":
            return c, compare(MISC_OUT, got, eval_misc(c, T, rows))
        inst, prim, u, v = hit
        h = inst >= 0
        ref = eval_interact(c, T, np.where(h, inst, 0), np.where(h, prim, 0), np.where(h, u, 0).astype(F32), np.where(h, v, 0).astype(F32))
        res = compare(INTERACT_OUT, got, ref)
        zero = ~got[:, 5:].any(1)
        return c, {k: (np.where(h, r[0], zero), np.where(h, r[1], 0.0), r[2] & h, r[3] & h) for k, r in res.items()}

    c0, res = run(())
    open_rows = np.zeros(len(rows), bool)
    for m in c0.open.values():
        open_rows |= np.broadcast_to(m, open_rows.shape)
    ok = np.all([r[0] for r in res.values()], 0)
    used = np.zeros(len(rows), bool)
    masks = {s: np.broadcast_to(m, ok.shape) for s, m in c0.open.items()}
    tried = set()
    for row in np.flatnonzero(~ok & open_rows):                 # every combination of the decisions that are open on a failing row, smallest first
        if ok[row]:
            continue
        sites = sorted(s for s, m in masks.items() if m[row])
        for size in range(1, len(sites) + 1):
            for flips in itertools.combinations(sites, size):
                if flips in tried or ok[row] or len(tried) >= 256:
                    continue
                tried.add(flips)
                _, alt = run(flips)
                alt_ok = np.all([r[0] for r in alt.values()], 0) & open_rows & ~ok
                for k in res:
                    res[k] = tuple(np.where(alt_ok, a, b) for a, b in zip(alt[k], res[k]))
                used |= alt_ok
                ok |= alt_ok
    unbounded = np.any([r[3] for r in res.values()], 0)
    return Verdict(res, open_rows, unbounded, used)


def reference(name, scene, **ctx_kw):
    """(context, outputs) of the natural branches — what the host test counts open rows and hollow families on"""
    T = tables(scene)
    mode, rows = family(name, scene)
    c = Ctx(**ctx_kw)
    return c, {"sample": eval_sample, "pdf": eval_pdf, "env": eval_env, "misc": eval_misc}[mode](c, T, rows)


def transcription(name, scene, hit=None, mut=None):
    """The float32 transcription's answers in the layout of zdr_light_dump"""
    mode, rows = family(name, scene)
    return transcription_rows(mode, scene, rows, hit=hit, mut=mut)


def transcription_rows(mode, scene, rows, hit=None, mut=None):
    T = tables(scene)
    c = Ctx(f32=True, mut=mut)
    out = np.zeros((len(rows), 16), F32)

    def put(layout, ref):
        for nm, at, w in layout:
            for k, r in enumerate(_cols(ref[nm])):
                out[:, at + k] = r.v
    with np.errstate(all="ignore"):
        if mode == "sample":
            ref = eval_sample(c, T, rows)
            put(SAMPLE_OUT, ref)
            out[:, 10] = ref["mesh_light"].astype(np.int32).view(F32)
        elif mode == "pdf":
            out[:, 0] = out[:, 1] = eval_pdf(c, T, rows)["pdf"].v
        elif mode == "env":
            put(ENV_OUT, eval_env(c, T, rows))
        elif mode == "misc":
            put(MISC_OUT, eval_misc(c, T, rows))
        else:
            inst, prim, u, v = hit
            h = inst >= 0
            put(INTERACT_OUT, eval_interact(c, T, np.where(h, inst, 0), np.where(h, prim, 0), np.where(h, u, 0).astype(F32), np.where(h, v, 0).astype(F32)))
            out[~h, 5:] = 0
    return out


# ---------------------------------------------------------------------------------------- the oracle's copies, as rows
def oracle_scene(scene, variant="ieee"):
    import oracle
    S = oracle.OracleScene.from_arrays(scene_arrays(scene), variant=variant)
    if scene.endswith("_env"):
        tex, prob, alias, pdf = env_tables()
        S.set_envmap(tex, prob, alias, pdf, map_w=MAP_W, map_h=MAP_H)
    return S


def oracle_hits(scene, rows):
    """the oracle's closest hits of the interact rays -> (inst, prim, u, v)"""
    S = oracle_scene(scene)
    rays = np.zeros((len(rows), 8), F32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = rows[:, 0:3], rows[:, 6], rows[:, 3:6], rows[:, 7]
    ip, bt = S.trace_closest(rays)
    return ip[:, 0].astype(np.int64), ip[:, 1].astype(np.int64), bt[:, 0].copy(), bt[:, 1].copy()


def oracle_answers(name, scene, variant="ieee", hit=None):
    """The oracle's answers in the layout of zdr_light_dump (interact: at `hit`)"""
    mode, rows = family(name, scene)
    S = oracle_scene(scene, variant)
    if mode != "interact":
        return S.light_rows(mode, rows)
    inst, prim, u, v = hit
    h = inst >= 0
    q = np.zeros((len(rows), 16), F32)
    q[:, 0], q[:, 1] = np.where(h, inst, 0).astype(np.int32).view(F32), np.where(h, prim, 0).astype(np.int32).view(F32)
    q[:, 2], q[:, 3] = np.where(h, u, 0), np.where(h, v, 0)
    o = S.light_rows("interact", q)
    out = np.zeros((len(rows), 16), F32)
    out[:, 5:16] = o[:, 0:11]
    out[~h, 5:] = 0
    return out


def measure_k():
    """-> (K_MEASURED, KT_MEASURED, table): the smallest integers at which both oracle builds and the transcription pass everywhere"""
    answers = []
    for name, scenes in PLAN:
        for scene in scenes:
            hit = oracle_hits(scene, family(name, scene)[1]) if name == "interact" else None
            for who in ("ieee", "fma", "f32"):
                got = transcription(name, scene, hit=hit) if who == "f32" else oracle_answers(name, scene, who, hit=hit)
                answers.append((name, scene, who, got, hit))

    def passes(k, kt, only=None):
        return all(judge(name, scene, got, hit=hit, k=k, kt=kt, computed_tables=who != "f32").ok.all() for name, scene, who, got, hit in answers if only is None or name in only)
    plain = ("sample", "pdf", "misc", "interact")
    k = next(k for k in range(1, 65) if passes(k, 64, only=plain) and passes(k, 64))
    kt = next(kt for kt in range(1, 65) if passes(k, kt))
    lines = [f"K_MEASURED {k}  KT_MEASURED {kt}   (K = 4 x {k} = {4 * k}, KT = 4 x {kt} = {4 * kt})"]
    for name, scene, who, got, hit in answers:
        v = judge(name, scene, got, hit=hit, k=k, kt=kt, computed_tables=who != "f32")
        worst = max(float(r[1].max()) for r in v.res.values())
        lines.append(f"{name:9s} {scene:11s} {who:5s} rows {len(got):5d}  worst error / bound at the measured margins {worst:.3f}  open {int(v.open_rows.sum()):4d}  flipped {int(v.used.sum()):3d}")
    return k, kt, lines


if __name__ == "__main__":
    print("\n".join(measure_k()[2]))
