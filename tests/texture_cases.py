"""The bilinear texture lookup and its adjoint row by row: seeded rows of (u, v, g, material), the ballots that deal them to the waves, a
float64 reference of both directions, and one bound per row (lookup) or per texel (scatter).  tests/test_texture_cases_host.py judges the
reference and the bound on the CPU, tests/test_gpu_texture_cases.py the kernels through zdr_texture_lookup / zdr_texture_scatter.

Reference (footprint, ref_lookup, ref_scatter): the float32 inputs as they are, px = u (W - 1), py = (1 - v) (H - 1) formed in float64,
ix = trunc(px) — truncation, as interaction.py:47-60 and the oracle have it —, weights and sums in float64, CLAMP of the four corners.
The environment map: texel centres (x = u W - 0.5), floor, clamp, as env_lookup / env_cell.  The adjoint is stated from the rows' side
(every corner adds to its clamped texel), never through cells: the kernels' staging cells, copies and fold are what is under test.

Restatement (restate32): the cells and the fold in float32 NumPy, every operation rounded once in the order of csrc/scene.h, with the
summation order, the contracted offset (px - ix as one FMA) and one deliberate fault (FAULTS) as switches.  It measures K and shows that
the judge bites; it is never a reference.

Exact family (exact_case): sizes with H - 1, W - 1 zero or a power of two, uvs on the quarter-texel lattice from two texels outside on one
side to two texels outside on the other (px = -1, 0, W - 1, W among them), v = 1 - j / (4 (H - 1)) so that 1 - v is exact, g, texels and
the gradient's pre-fill integers in [-8, 8]: every term is a multiple of 2^-4 and every partial sum stays below 2^20 (exact_precondition),
so float32 gives the float64 answer in ANY order and the kernels must return it bit for bit, whatever the regime or the copies.

General families (general_case; GENERAL_SIZES x UV_FAMILIES) are judged under a bound computed in float64 from the rows alone:
  offsets    px is rounded once (or not at all where px - ix is contracted): |d ox| <= 2^-24 |px|; py carries the rounding of 1 - v as
             well: |d oy| <= 2 * 2^-24 |py| (the map: the product and the - 0.5).  Propagated through d w / d ox, d w / d oy and |g|; a
             contracted offset next to an integer px leaves the reference's footprint by that much, so the texel beyond receives it too.
  products   (wx * wy) * g: 1 - ox, 1 - oy, the two products: 4 roundings; the lookup: three lerpf of three roundings, two deep: 6.
             That count times 2^-24 times sum |w| |value|.
  summation  order-free: (m + 1) 2^-24 (sum |term| + |pre-fill|) over the m terms that reach the texel through all cells and copies — float
             atomics arrive in any order; the two extra roundings are the fold's += and its conversion of the copies' float64 sum.
             sum |term|, not |sum term|: the cancellation family is judged fairly.
  floor      m * 2^-126: a float32 pipeline may flush subnormals (float atomics do), each term loses at most the smallest normal.
The first three are multiplied by K = 4 x K_MEASURED; K_MEASURED (measure_k, profiles/texture_cases_margins.txt) is the smallest integer
at which the restatement (five orders, with and without the contracted offset) and the oracle (IEEE and FMA build) are inside: the GPU's
contraction and order are a fourth float32 evaluation, not a fifth kind of error.

Conditions on the inputs (input_conditions): the lookup is continuous in uv except at px = -1 and py = -1, where ix goes from -1 to 0 while
both clamped corners move; no row of a general family is within 4 ulp32 of it (the exact family holds -1 itself, exactly), and no row has
|px| or |py| >= 2^24 (deviations).
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:       # (run as a script: python tests/texture_cases.py writes profiles/texture_cases_margins.txt)
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
K_MEASURED, K = 1, 4           # measure_k() -> K_MEASURED; K = 4 x (profiles/texture_cases_margins.txt; test_texture_cases_host.py holds them to it)
TINY = 2.0 ** -126
ROUNDS = 6
WAVES = 150
LDS_CELLS, MAX_COPIES, ENV_ENTRY, ENV_BUDGET = 28, 1024, 15, 1 << 22   # DESIGN.md §2, the staging cells
ENV_SIZE = (32, 32)            # a 16 x 32 map as Scene.add_envmap prepares it: rows repeated, square
EXACT_SIZES = [(1, 1), (2, 2), (3, 2), (2, 3), (3, 5), (5, 5), (1, 9), (9, 1), (17, 33), (129, 129), (257, 257)]
GENERAL_SIZES = [(4, 4), (3, 6), (4, 5), (5, 3), (7, 1), (1, 6), (37, 91), (254, 255), (255, 255)]
UV_FAMILIES = ("uniform", "borders", "outside", "hot_spot", "cancellation")
TABLES = {                     # tests/test_gpu_materials_oracle.py, CELL_MODES and sixteen(); `idle`: material 1 receives no row
    "lds": [(1, 1), (2, 2), (1, 3)], "copies": [(37, 91), (5, 3), (1, 1)], "one_copy": [(256, 256), (1, 1), (2, 2)],
    "sixteen": [(37, 91), (128, 64), (5, 3), (1, 1), (3, 5), (2, 2), (64, 32), (9, 17), (7, 1), (1, 6), (33, 20), (4, 4), (11, 13), (2, 9), (16, 3), (3, 5)],
    "idle": [(5, 3), (9, 17), (2, 2)],
}
PATTERNS = ("full", "one_lane", "empty_round", "40+40", "63+1", "64+3", "empty_wave", "full")   # wave b deals by PATTERNS[b % 8]
FAULTS = ("corner_index", "base_clamp_0", "fold_last_column", "floor_for_trunc", "queue_drops_65th", "copy_stride")


# ------------------------------------------------------------------------------ the regimes, from DESIGN.md's text
def cells_of(size):
    return (size[0] + 1) * (size[1] + 1)


def expected_copies_single(size):
    """One material: copies = min(1024, 2^20 / cells) below 2^16 cells, else one; the cells live in LDS iff cells <= 28."""
    c = cells_of(size)
    return min(MAX_COPIES, (1 << 20) // c) if c < (1 << 16) else 1


def expected_copies_table(sizes):
    """A table: at most 28 cells in all -> LDS, every material copied like the whole array; otherwise each material has copies of its own,
    min(1024, max(1, (2^20 / nmat) / cells)) below 2^16 cells of its own, else one."""
    total = sum(cells_of(s) for s in sizes)
    if total <= LDS_CELLS:
        return [min(MAX_COPIES, (1 << 20) // total)] * len(sizes)
    return [min(MAX_COPIES, max(1, ((1 << 20) // len(sizes)) // cells_of(s))) if cells_of(s) < (1 << 16) else 1 for s in sizes]


def expected_copies_env(size):
    return min(MAX_COPIES, max(1, ENV_BUDGET // cells_of(size)))


def in_lds(sizes, env=False):
    return not env and sum(cells_of(s) for s in sizes) <= LDS_CELLS


# ------------------------------------------------------------------------------ the float64 reference
def footprint(u, v, size, env=False):
    """-> px, py, ix, iy (int64), ox, oy of float32 u, v in float64"""
    h, w = size
    u, v = np.asarray(u, F32).astype(F64), np.asarray(v, F32).astype(F64)
    if env:
        px, py = u * w - 0.5, v * h - 0.5
        ix, iy = np.floor(px), np.floor(py)
    else:
        px, py = u * (w - 1), (1.0 - v) * (h - 1)
        ix, iy = np.trunc(px), np.trunc(py)
    return px, py, ix.astype(np.int64), iy.astype(np.int64), px - ix, py - iy


def _corners(ix, iy, size):
    h, w = size
    return (np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)), (np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1))


def offset_error(u, v, size, env=False):
    """|d ox|, |d oy| of a float32 evaluation (module docstring, offsets)"""
    h, w = size
    px, py = footprint(u, v, size, env)[:2]
    if env:
        u, v = np.asarray(u, F32).astype(F64), np.asarray(v, F32).astype(F64)
        return U * (np.abs(u * w) + np.abs(px)), U * (np.abs(v * h) + np.abs(py))
    return U * np.abs(px), 2.0 * U * np.abs(py)


def ref_lookup(tex, u, v, env=False, k=K):
    """float64 lookup of tex (h, w, 4) float32 at float32 (u, v) -> (value (n, 4), bound (n, 4))"""
    tex = np.asarray(tex, F32).astype(F64)
    size = tex.shape[:2]
    px, py, ix, iy, ox, oy = footprint(u, v, size, env)
    dpx, dpy = offset_error(u, v, size, env)
    ox_, oy_, dpx_, dpy_ = ox[:, None], oy[:, None], dpx[:, None], dpy[:, None]

    def at(sx, sy):
        (x0, x1), (y0, y1) = _corners(ix + sx, iy + sy, size)
        return tex[y0, x0], tex[y1, x0], tex[y0, x1], tex[y1, x1]
    c00, c01, c10, c11 = at(0, 0)
    val = (1 - ox_) * ((1 - oy_) * c00 + oy_ * c01) + ox_ * ((1 - oy_) * c10 + oy_ * c11)
    slope_x = np.zeros_like(val); slope_y = np.zeros_like(val); cross = np.zeros_like(val)
    for sx in (-1, 0, 1):                    # a rounded px next to an integer may sit in the neighbouring cell: the steeper slope counts
        for sy in (-1, 0, 1):
            a00, a01, a10, a11 = at(sx, sy)
            near = ((sx == 0) | (np.abs(px - np.rint(px)) <= 4 * dpx + 1e-300)) & ((sy == 0) | (np.abs(py - np.rint(py)) <= 4 * dpy + 1e-300))
            n_ = near[:, None]
            wy = np.abs(1 - oy_) + np.abs(oy_) + 1; wx = np.abs(1 - ox_) + np.abs(ox_) + 1
            slope_x = np.maximum(slope_x, n_ * np.maximum(np.abs(a10 - a00), np.abs(a11 - a01)) * wy)
            slope_y = np.maximum(slope_y, n_ * np.maximum(np.abs(a01 - a00), np.abs(a11 - a10)) * wx)
            cross = np.maximum(cross, n_ * np.abs(a00 - a01 - a10 + a11))
    env_ = (np.abs(c00) * (1 + np.abs(oy_)) + np.abs(c01) * np.abs(oy_)) * (1 + np.abs(ox_)) + (np.abs(c10) * (1 + np.abs(oy_)) + np.abs(c11) * np.abs(oy_)) * np.abs(ox_)
    bound = k * (dpx_ * slope_x + dpy_ * slope_y + dpx_ * dpy_ * cross + 6 * U * env_) + 4 * TINY
    return val, bound


def ref_scatter(size, u, v, g, prefill, env=False, k=K, parts=False):
    """float64 adjoint: prefill (h, w, 4) + every row's four corner terms -> (gradient (h, w, 4), bound (h, w, 4))"""
    h, w = size
    px, py, ix, iy, ox, oy = footprint(u, v, size, env)
    dpx, dpy = offset_error(u, v, size, env)
    g = np.asarray(g, F32).astype(F64).reshape(-1, 4)
    ag = np.abs(g)
    xs, ys = _corners(ix, iy, size)
    wxs, wys = (1 - ox, ox), (1 - oy, oy)
    n = h * w
    acc = {name: np.zeros((n, 4)) for name in ("sum", "abs", "off")}
    cnt = np.zeros(n)

    def add(name, t, val):
        for c in range(4):
            acc[name][:, c] += np.bincount(t, weights=val[:, c], minlength=n)
    near_x = np.abs(px - np.rint(px)) <= 4 * dpx + 1e-300
    near_y = np.abs(py - np.rint(py)) <= 4 * dpy + 1e-300
    for dx in (0, 1):
        for dy in (0, 1):
            t = ys[dy] * w + xs[dx]
            term = (wxs[dx] * wys[dy])[:, None] * g
            add("sum", t, term); add("abs", t, np.abs(term))
            cnt += np.bincount(t, minlength=n)
            add("off", t, ag * (dpx * np.abs(wys[dy]) + dpy * np.abs(wxs[dx]) + dpx * dpy)[:, None])
    for s in (-1, 2):                        # the texels beyond the footprint (module docstring, offsets)
        xb, yb = np.clip(ix + s, 0, w - 1), np.clip(iy + s, 0, h - 1)
        for d in (0, 1):
            add("off", ys[d] * w + xb, ag * (near_x * 2 * dpx * (np.abs(wys[d]) + dpy))[:, None])
            add("off", yb * w + xs[d], ag * (near_y * 2 * dpy * (np.abs(wxs[d]) + dpx))[:, None])
    pre = np.asarray(prefill, F32).astype(F64).reshape(n, 4)
    ref = pre + acc["sum"]
    summation = (cnt[:, None] + 1) * U * (acc["abs"] + np.abs(pre))
    bound = k * (acc["off"] + 4 * U * acc["abs"] + summation) + cnt[:, None] * TINY
    if parts:
        return ref.reshape(h, w, 4), bound.reshape(h, w, 4), acc["abs"].reshape(h, w, 4), cnt.reshape(h, w)
    return ref.reshape(h, w, 4), bound.reshape(h, w, 4)


# ------------------------------------------------------------------------------ the ballots
def deal(nwaves, rng, thin=1.0):
    """-> active (nwaves, ROUNDS, 64) bool: wave b deals by PATTERNS[b % 8]; `thin`: share of the active rows kept (general families)"""
    a = np.zeros((nwaves, ROUNDS, 64), bool)
    lanes = np.arange(64)
    for b in range(nwaves):
        p = PATTERNS[b % len(PATTERNS)]
        spread = (lanes * 37 + 11 * b) % 64                  # a permutation of the lanes, another one per wave
        if p == "full":
            a[b] = True
        elif p == "one_lane":                                # one active lane per round, moving
            for r in range(ROUNDS):
                a[b, r, (7 * b + 11 * r) % 64] = True
        elif p == "empty_round":                             # rounds without an active lane: the early return
            a[b, [0, 2, 5]] = True
        elif p == "40+40":                                   # 40 + 40 > 64: the flush before the push
            a[b] = (spread < 40)[None, :]
        elif p == "63+1":                                    # fills to exactly 64: the flush after the push
            a[b, 0::2] = (spread < 63)[None, :]
            a[b, 1::2] = (spread == 63)[None, :]
        elif p == "64+3":                                    # 64, then 3 rows left for scatter_finish
            a[b, 0] = True
            a[b, ROUNDS - 1] = spread < 3
        # "empty_wave": no active row at all
    if thin < 1.0:
        a &= rng.random(a.shape) < thin
    return a


def queue_drops(active):
    """-> rows that a queue without the flush before the push would drop: the entries from the 65th on (FAULTS, queue_drops_65th)"""
    drop = np.zeros_like(active)
    for b in range(active.shape[0]):
        count = 0
        for r in range(active.shape[1]):
            n = int(active[b, r].sum())
            if n == 0:
                continue
            slot = count + np.cumsum(active[b, r]) - 1
            drop[b, r] = active[b, r] & (slot >= 64)
            count = min(count + n, 64)
            if count >= 64:
                count = 0
    return drop


# ------------------------------------------------------------------------------ cases
class Case:
    """Rows for one launch of zdr_texture_scatter / zdr_texture_lookup.  sizes: the table; env: rows of material ENV_ENTRY go to a map of
    ENV_SIZE.  u, v, g, mat: per row SLOT (nwaves * ROUNDS * 64, inactive slots included, mat < 0 there); n: rows passed (a partial last wave)."""

    def __init__(self, name, sizes, active, u, v, g, mat, n, seed, exact, env=False):
        self.name, self.sizes, self.active, self.n, self.exact, self.env = name, list(sizes), active, n, exact, env
        self.u, self.v, self.g, self.mat = u.astype(F32), v.astype(F32), g.astype(F32), mat.astype(np.int32)
        self.mat[n:] = -1
        rng = np.random.default_rng(seed + 77)
        ival = (lambda s: rng.integers(-8, 9, s).astype(F32)) if exact else (lambda s: rng.uniform(0.05, 1.0, s).astype(F32))
        self.textures = [ival((h, w, 4)) for h, w in self.sizes]
        self.prefill = [ival((h, w, 4)) if exact else rng.uniform(-1e-3, 1e-3, (h, w, 4)).astype(F32) for h, w in self.sizes]
        self.env_texture, self.env_prefill = ival(ENV_SIZE + (4,)), (ival(ENV_SIZE + (4,)) if exact else np.zeros(ENV_SIZE + (4,), F32))
        self.wave = np.repeat(np.arange(active.shape[0]), ROUNDS * 64)
        for a in (self.u, self.v, self.g, self.mat, self.wave):
            a.setflags(write=False)

    def rows(self):
        """-> (n, 7) float32 as zdr_texture_scatter takes them (the material's bits in column 6)"""
        r = np.zeros((self.n, 7), F32)
        r[:, 0], r[:, 1], r[:, 2:6] = self.u[:self.n], self.v[:self.n], self.g[:self.n]
        r[:, 6] = self.mat[:self.n].view(F32)
        return r

    def entries(self):
        """-> [(k, size, env?)] of the table entries that can receive rows"""
        return [(k, s, False) for k, s in enumerate(self.sizes)] + ([(ENV_ENTRY, ENV_SIZE, True)] if self.env else [])

    def of(self, k):
        return np.flatnonzero(self.mat == k)

    def tex(self, k):
        return self.env_texture if k == ENV_ENTRY and self.env else self.textures[k]

    def pre(self, k):
        return self.env_prefill if k == ENV_ENTRY and self.env else self.prefill[k]

    def copies(self, single=False):
        c = [expected_copies_single(self.sizes[0])] if single else expected_copies_table(self.sizes)
        d = dict(enumerate(c))
        if self.env:
            d[ENV_ENTRY] = expected_copies_env(ENV_SIZE)
        return d

    @functools.lru_cache(maxsize=None)
    def reference(self, k):
        """float64 gradient and bound of entry k, computed once"""
        i = self.of(k)
        size = ENV_SIZE if (k == ENV_ENTRY and self.env) else self.sizes[k]
        ref, bound = ref_scatter(size, self.u[i], self.v[i], self.g[i], self.pre(k), env=(k == ENV_ENTRY and self.env))
        ref.setflags(write=False); bound.setflags(write=False)
        return ref, bound


def _lattice(d, n, rng):
    """n positions on the quarter-texel lattice of a dimension of d texels, as u (x) — two texels outside on either side"""
    if d == 1:
        return rng.choice(np.array([-1.0, 0.0, 0.25, 1.0, 2.0]), n)
    j = rng.integers(-8, 4 * (d - 1) + 9, n)
    edge = np.array([-8, -5, -4, -3, -1, 0, 1, 4 * (d - 1) - 1, 4 * (d - 1), 4 * (d - 1) + 1, 4 * (d - 1) + 3, 4 * d, 4 * (d - 1) + 8])
    pick = rng.random(n) < 0.3               # px = -2, -1, 0, W - 1, W exactly, and their neighbours, often
    j[pick] = rng.choice(edge, int(pick.sum()))
    return j / (4.0 * (d - 1))


def _assign(sizes, slots, rng, env, idle=()):
    """material of each slot: material 0 most often in small tables, all alike in large ones; the map's entry for a fifth when env"""
    live = [k for k in range(len(sizes)) if k not in idle]
    mat = rng.choice(np.array(live), slots)
    if env:
        mat[rng.random(slots) < 0.2] = ENV_ENTRY
    return mat


@functools.lru_cache(maxsize=None)
def exact_case(sizes, env=False, seed=0):
    """sizes: a tuple of sizes with H - 1, W - 1 zero or a power of two"""
    rng = np.random.default_rng([seed, len(sizes), env] + [x for s in sizes for x in s])
    active = deal(WAVES, rng)
    slots = active.size
    mat = _assign(sizes, slots, rng, env)
    u, v = np.zeros(slots), np.zeros(slots)
    for k, (h, w) in enumerate(sizes):
        i = np.flatnonzero(mat == k)
        u[i], v[i] = _lattice(w, i.size, rng), 1.0 - _lattice(h, i.size, rng)
    if env:
        i = np.flatnonzero(mat == ENV_ENTRY)
        eh, ew = ENV_SIZE
        u[i], v[i] = rng.integers(-8, 4 * ew + 9, i.size) / (4.0 * ew), rng.integers(-8, 4 * eh + 9, i.size) / (4.0 * eh)
    g = rng.integers(-8, 9, (slots, 4))
    mat[~active.reshape(-1)] = -1
    n = slots - ROUNDS * 64 + 2 * 64 + 37    # a partial last wave
    return Case("exact " + "+".join("%dx%d" % s for s in sizes) + (" env" if env else ""), sizes, active, u, v, g, mat, n, seed, True, env)


def _general_uv(family, size, n, rng, env):
    h, w = size
    if family == "uniform":
        return rng.random(n), rng.random(n)
    if family == "outside":
        return rng.uniform(-1.5, 2.5, n), rng.uniform(-1.5, 2.5, n)
    if family == "borders":
        one, zero = F32(1), F32(0)
        pts = np.array([0.0, 1.0, np.nextafter(zero, one), np.nextafter(zero, -one), np.nextafter(one, zero), np.nextafter(one, F32(2))], F64)
        def draw(inner):                        # one coordinate on a border (a third of the rows: both), the other anywhere
            x = rng.choice(pts, n)
            k = rng.random(n) < 0.5
            x[k] = rng.choice(np.array([0.0, 1.0]), int(k.sum())) + rng.uniform(-1e-3, 1e-3, int(k.sum()))
            x[inner] = rng.random(int(inner.sum()))
            return x
        which = rng.integers(0, 3, n)
        return draw(which == 0), draw(which == 1)
    if family == "hot_spot":                 # every row the same uv, and four uvs that share one cell: several requests to one address per instruction
        if env:
            cx, cy = (w // 2 + 0.5) / w, (h // 2 + 0.5) / h
            du, dv = 0.4 / w, 0.4 / h
        else:
            cx, cy = ((w - 1) // 2 + 0.25) / max(w - 1, 1), 1.0 - ((h - 1) // 2 + 0.25) / max(h - 1, 1)
            du, dv = 0.5 / max(w - 1, 1), -0.5 / max(h - 1, 1)
        q = rng.integers(0, 8, n)            # half the rows the very same uv, the others one of four in its cell
        return cx + du * ((q == 5) | (q == 7)) + 0.3 * du * (q == 4), cy + dv * ((q == 6) | (q == 7))
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def general_case(family, sizes, env=False, seed=1, idle=()):
    """Rows of one UV family for a table of `sizes` (a tuple; one size = the single-material cases).  About 12 rows per texel reached, so that a
    texel's bound stays a small multiple of 2^-24 of its value (profiles/texture_cases_margins.txt), in as many waves as that takes."""
    rng = np.random.default_rng([seed, UV_FAMILIES.index(family), len(sizes), env] + [x for s in sizes for x in s])
    reach = {"borders": lambda h, w: 2 * (h + w), "hot_spot": lambda h, w: 4}.get(family, lambda h, w: h * w)   # texels the family's rows land on
    texels = sum(reach(h, w) for h, w in sizes) + (reach(*ENV_SIZE) if env else 0)
    want = max(96, min(12 * texels, WAVES * ROUNDS * 64 // 2))
    nwaves = int(min(WAVES, max(2 * len(PATTERNS), -(-want * 2 // (ROUNDS * 64)))))
    base = deal(nwaves, np.random.default_rng(0))
    active = deal(nwaves, rng, thin=min(1.0, want / max(1, base.sum())))
    slots = active.size
    mat = _assign(sizes, slots, rng, env, idle)
    u, v = np.zeros(slots), np.zeros(slots)
    fam = "uniform" if family == "cancellation" else family
    for k, size, is_env in [(k, s, False) for k, s in enumerate(sizes)] + ([(ENV_ENTRY, ENV_SIZE, True)] if env else []):
        i = np.flatnonzero(mat == k)
        u[i], v[i] = _general_uv(fam, size, i.size, rng, is_env)
    g = rng.uniform(0.0, 1.0, (slots, 4))
    g[rng.random(slots) < 0.05] = 0.0        # rows that are pushed with a zero gradient
    if family == "cancellation":             # pairs of +-1e6 at one uv beside values near 1, and denormal g
        p = np.flatnonzero(rng.random(slots // 2) < 0.25) * 2
        g[p] = 1e6 * rng.uniform(0.5, 1.0, (p.size, 4)); g[p + 1] = -g[p].astype(F32)
        u[p + 1], v[p + 1], mat[p + 1] = u[p], v[p], mat[p]
        d = np.flatnonzero(rng.random(slots) < 0.1)
        d = d[~np.isin(d, np.concatenate([p, p + 1]))]
        g[d] = rng.uniform(-1.0, 1.0, (d.size, 4)) * 1e-40
    mat[~active.reshape(-1)] = -1
    n = slots - 64 + 37 if nwaves > 2 else slots
    u, v = u.astype(F32), v.astype(F32)
    # the one zone where the lookup is discontinuous: rows within 4 ulp32 of px = -1 or py = -1 are moved inside (input_conditions asserts it)
    for k, size, is_env in [(k, s, False) for k, s in enumerate(sizes)]:
        i = np.flatnonzero(mat == k)
        px, py = footprint(u[i], v[i], size)[:2]
        bad = i[(np.abs(px + 1) < 1e-5) | (np.abs(py + 1) < 1e-5)]
        u[bad], v[bad] = F32(0.25), F32(0.75)
    return Case("%s %s%s" % (family, "+".join("%dx%d" % s for s in sizes), " env" if env else ""), sizes, active, u, v, g, mat, n, seed, False, env)


def input_conditions(case):
    """-> None, or what is wrong with the rows (module docstring, conditions on the inputs)"""
    for k, size, is_env in case.entries():
        i = case.of(k)
        px, py = footprint(case.u[i], case.v[i], size, is_env)[:2]
        if i.size and max(np.abs(px).max(), np.abs(py).max()) >= 2.0 ** 24:
            return "entry %d: |px| or |py| >= 2^24" % k
        if not is_env and not case.exact:
            ulp = 4 * 2.0 ** -23             # 4 ulp32 at 1
            if i.size and (np.abs(px + 1).min() <= ulp or np.abs(py + 1).min() <= ulp):
                return "entry %d: a row within 4 ulp32 of px = -1 or py = -1" % k
    return None


def exact_precondition(case):
    """-> (largest sum of |term| into one texel incl. the pre-fill, every term a multiple of 2^-4?) over all entries of an exact case"""
    worst, dyadic = 0.0, True
    for k, size, is_env in case.entries():
        i = case.of(k)
        _, _, _, _, ox, oy = footprint(case.u[i], case.v[i], size, is_env)
        _, _, sabs, _ = ref_scatter(size, case.u[i], case.v[i], case.g[i], case.pre(k), env=is_env, parts=True)
        worst = max(worst, float((sabs + np.abs(case.pre(k))).max()))
        for wx in (1 - ox, ox):
            for wy in (1 - oy, oy):
                t = (wx * wy)[:, None] * case.g[i].astype(F64) * 16
                dyadic &= bool((t == np.rint(t)).all())
        t = case.tex(k).astype(F64)
        dyadic &= bool((t == np.rint(t)).all()) and bool((case.pre(k) == np.rint(case.pre(k))).all())
    return worst, dyadic


# ------------------------------------------------------------------------------ the float32 restatement
def restate32(case, k, copies, *, lds=False, contract=False, order="forward", fault=None, seed=0):
    """Entry k's gradient as csrc/scene.h computes it, in float32 NumPy: scatter_cell / env_cell, the flush's (wx * wy) * g into 16-float
    cells of copy wave % copies, the fold (float64 over the copies, float32 in order otherwise), += pre-fill.  order: forward | backward |
    a seed's random order, of the rows into the cells and of the cells into the texel."""
    is_env = case.env and k == ENV_ENTRY
    h, w = ENV_SIZE if is_env else case.sizes[k]
    i = case.of(k)
    if fault == "queue_drops_65th" and not lds:
        i = i[~queue_drops(case.active).reshape(-1)[i]]
    u, v, g, wave = case.u[i], case.v[i], case.g[i], case.wave[i]
    if is_env:
        a, b = u * F32(w), v * F32(h)
        px, py = a - F32(0.5), b - F32(0.5)
        ix, iy = np.floor(px), np.floor(py)
        ox, oy = px - ix, py - iy
        if contract:
            ox = (u.astype(F64) * w - 0.5 - ix).astype(F32); oy = (v.astype(F64) * h - 0.5 - iy).astype(F32)
    else:
        one_v = F32(1) - v
        px, py = u * F32(w - 1), one_v * F32(h - 1)
        trunc = np.floor if fault == "floor_for_trunc" else np.trunc
        ix, iy = trunc(px), trunc(py)
        ox, oy = px - ix, py - iy
        if contract:                         # px * 1 - ix as one FMA: the product is not rounded
            ox = (u.astype(F64) * (w - 1) - ix).astype(F32); oy = (one_v.astype(F64) * (h - 1) - iy).astype(F32)
    lo = 0 if fault == "base_clamp_0" else -1
    ix, iy = np.clip(ix, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64), np.clip(iy, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)   # the conversion saturates
    cell = (np.clip(ix, lo, w - 1) + 1) + (w + 1) * (np.clip(iy, lo, h - 1) + 1)
    ncells = (h + 1) * (w + 1)
    terms = np.zeros((i.size, 16), F32)
    wxs, wys = (F32(1) - ox, ox), (F32(1) - oy, oy)
    for dx in (0, 1):
        for dy in (0, 1):
            m = dx + 2 * dy if fault == "corner_index" else 2 * dx + dy
            terms[:, 4 * m:4 * m + 4] = (wxs[dx] * wys[dy])[:, None] * g
    rng = np.random.default_rng([seed, 5]) if isinstance(order, int) else None
    perm = np.arange(i.size)
    if order == "backward":
        perm = perm[::-1]
    elif rng is not None:
        perm = rng.permutation(i.size)
    cells = np.zeros((copies * ncells, 16), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        np.add.at(cells, ((wave % copies) * ncells + cell)[perm], terms[perm])
        # the fold, from the cells' side: corner (dx, dy) of cell (cx - 1, cy - 1) belongs to texel clamp(ix + dx), clamp(iy + dy)
        cy, cx = np.divmod(np.arange(ncells), w + 1)
        stride = ncells - 1 if fault == "copy_stride" else ncells
        out = np.zeros((h * w, 4), F64 if copies > 1 else F32)
        src, dst, corner = [], [], []
        for dx in (0, 1):
            for dy in (0, 1):
                keep = np.ones(ncells, bool)
                if fault == "fold_last_column":
                    keep = ~((cx - 1 == w - 1) & (dx == 1))
                t = np.clip(cy - 1 + dy, 0, h - 1) * w + np.clip(cx - 1 + dx, 0, w - 1)
                src.append(np.arange(ncells)[keep]); dst.append(t[keep]); corner.append(np.full(int(keep.sum()), 2 * dx + dy))
        src, dst, corner = np.concatenate(src), np.concatenate(dst), np.concatenate(corner)
        src = (src[None, :] + (np.arange(copies) * stride)[:, None]).reshape(-1)              # copy kc at kc * stride
        dst, corner = np.tile(dst, copies), np.tile(corner, copies)
        fp = np.arange(src.size)
        if order == "backward":
            fp = fp[::-1]
        elif rng is not None:
            fp = rng.permutation(src.size)
        vals = cells.reshape(-1, 4, 4)[src[fp], corner[fp]]
        np.add.at(out, dst[fp], vals.astype(out.dtype))
        return (case.pre(k).reshape(-1, 4) + out.astype(F32)).reshape(h, w, 4)


def lookup32(tex, u, v, env=False, contract=False):
    """read_bsdf / env_lookup in float32 NumPy, in the order of csrc/scene.h"""
    tex = np.asarray(tex, F32)
    h, w = tex.shape[:2]
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    if env:
        px, py = u * F32(w) - F32(0.5), v * F32(h) - F32(0.5)
        ix, iy = np.floor(px), np.floor(py)
        ox, oy = px - ix, py - iy
        if contract:
            ox = (u.astype(F64) * w - 0.5 - ix).astype(F32); oy = (v.astype(F64) * h - 0.5 - iy).astype(F32)
    else:
        one_v = F32(1) - v
        px, py = u * F32(w - 1), one_v * F32(h - 1)
        ix, iy = np.trunc(px), np.trunc(py)
        ox, oy = px - ix, py - iy
        if contract:
            ox = (u.astype(F64) * (w - 1) - ix).astype(F32); oy = (one_v.astype(F64) * (h - 1) - iy).astype(F32)
    (x0, x1), (y0, y1) = _corners(ix.astype(np.int64), iy.astype(np.int64), (h, w))
    c00, c01, c10, c11 = tex[y0, x0], tex[y1, x0], tex[y0, x1], tex[y1, x1]
    ox, oy = ox[:, None], oy[:, None]
    lerp = lambda a, b, t: a + t * (b - a)
    if env:
        return lerp(lerp(c00, c10, ox), lerp(c01, c11, ox), oy)
    return lerp(lerp(c00, c01, oy), lerp(c10, c11, oy), ox)


# ------------------------------------------------------------------------------ judging
def ratio(err, bound):
    """worst error / bound (0 / 0 = 0: a texel that nothing reaches and whose pre-fill came back)"""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def scatter_ratio(case, k, got):
    ref, bound = case.reference(k)
    return ratio(np.abs(np.asarray(got, F64) - ref), bound)


def median_relative_bound(case):
    """median over the texels that receive rows of bound / |reference| (all entries)"""
    r = []
    for k, size, is_env in case.entries():
        ref, bound = case.reference(k)
        m = np.abs(ref - case.pre(k)) > 0
        r.append((bound[m] / np.abs(ref[m])).ravel())
    r = np.concatenate(r)
    return float(np.median(r)) if r.size else 0.0


def all_general_cases():
    """every general case the GPU test runs: (label, case, single?)"""
    out = []
    for fam in UV_FAMILIES:
        for s in GENERAL_SIZES:
            out.append((fam, general_case(fam, (s,)), True))
        for t in ("lds", "copies", "one_copy", "sixteen"):
            out.append((fam, general_case(fam, tuple(TABLES[t])), False))
        out.append((fam, general_case(fam, tuple(TABLES["idle"]), idle=(1,)), False))
        out.append((fam, general_case(fam, tuple(TABLES["copies"]), env=True), False))
    return out


def oracle_scatter(case, k, variant):
    """entry k through the oracle's write_bsdf_grad (float32 weights and products, float64 sums) + pre-fill, rounded to float32"""
    import ctypes as C
    import oracle
    L = oracle.lib(variant)
    h, w = case.sizes[k]
    i = case.of(k)
    rows = np.ascontiguousarray(np.concatenate([case.u[i, None], case.v[i, None], case.g[i]], 1), F32)
    dm = np.zeros((h, w, 4), F64)
    L.zdro_write_bsdf_grad(dm.ctypes.data_as(C.POINTER(C.c_double)), h, w, rows.ctypes.data_as(C.POINTER(C.c_float)), i.size)
    return (case.pre(k).astype(F64) + dm).astype(F32)


def oracle_lookup(tex, u, v, variant):
    import ctypes as C
    import oracle
    L = oracle.lib(variant)
    tex = np.ascontiguousarray(tex, F32)
    out = np.zeros((len(u), 4), F32)
    fp = C.POINTER(C.c_float)
    t = tex.ctypes.data_as(fp)
    for j in range(len(u)):
        L.zdro_read_bsdf(t, tex.shape[0], tex.shape[1], float(u[j]), float(v[j]), out[j].ctypes.data_as(fp))
    return out


ORDERS = ("forward", "backward", 1, 2, 3)


def measure_case(case, single, oracle_too=True, lookup_cap=4000):
    """worst error / bound at K = 1 of every float32 evaluation of the case -> {evaluation: ratio}"""
    worst = {}

    def note(name, r):
        worst[name] = max(worst.get(name, 0.0), r)
    copies = case.copies(single)
    for k, size, is_env in case.entries():
        if not case.of(k).size:
            continue
        ref, bound = case.reference(k)
        b1 = bound / K                                   # the bound at K = 1 (the floor rides along, scaled down: stricter)
        for contract in (False, True):
            for order in ORDERS:
                got = restate32(case, k, copies[k], lds=in_lds(case.sizes, case.env), contract=contract, order=order)
                note("restatement" + (" fma" if contract else ""), ratio(np.abs(got.astype(F64) - ref), b1))
        i = case.of(k)[:lookup_cap]
        val, lb = ref_lookup(case.tex(k), case.u[i], case.v[i], env=is_env)
        for contract in (False, True):
            note("lookup restatement" + (" fma" if contract else ""), ratio(np.abs(lookup32(case.tex(k), case.u[i], case.v[i], is_env, contract).astype(F64) - val), lb / K))
        if oracle_too and not is_env:
            for variant in ("ieee", "fma"):
                note("oracle " + variant, ratio(np.abs(oracle_scatter(case, k, variant).astype(F64) - ref), b1))
                note("lookup oracle " + variant, ratio(np.abs(oracle_lookup(case.tex(k), case.u[i], case.v[i], variant).astype(F64) - val), lb / K))
    return worst


def measure_k(cases=None, oracle_too=True):
    """-> (K_MEASURED, table lines): the smallest integer K at which every float32 evaluation is inside K x the bound, over all general cases"""
    per_family, med = {}, {}
    for fam, case, single in (cases or all_general_cases()):
        w = measure_case(case, single, oracle_too)
        d = per_family.setdefault(fam, {})
        for name, r in w.items():
            d[name] = max(d.get(name, 0.0), r)
        med.setdefault(fam, []).append(median_relative_bound(case))
    worst = max(r for d in per_family.values() for r in d.values())
    lines = []
    for fam, d in per_family.items():
        lines.append("%-13s %s" % (fam, "  ".join("%s %.3f" % (n, r) for n, r in sorted(d.items()))))
        lines.append("%-13s median bound / |reference| at K = %d: %.2e (largest case %.2e)" % ("", K, float(np.median(med[fam])), max(med[fam])))
    return int(np.ceil(worst)), lines, per_family, med


if __name__ == "__main__":      # the table of profiles/texture_cases_margins.txt (the [texture] lines of a GPU run are appended by hand)
    k, lines, _, _ = measure_k()
    path = os.path.join(ROOT, "profiles", "texture_cases_margins.txt")
    keep = []
    if os.path.exists(path):
        keep = [l.rstrip("\n") for l in open(path) if l.startswith("[texture]") or l.startswith("# GPU")]
    text = ["# python tests/texture_cases.py — worst error / bound at K = 1 of every float32 evaluation, per general family (no GPU)",
            "# evaluations: the float32 NumPy restatement (5 orders; `fma`: px - ix contracted), the oracle built ieee and fma",
            "# (zdro_read_bsdf, zdro_write_bsdf_grad).  K_MEASURED = the smallest integer above all of them; the tests use K = 4 x that."] + lines + \
           ["K_MEASURED = %d  (tests/texture_cases.py has %d, K = %d)" % (k, K_MEASURED, K)] + keep
    open(path, "w").write("\n".join(text) + "\n")
    print("\n".join(text))
