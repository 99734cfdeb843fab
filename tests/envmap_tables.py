"""Importance-sampling tables of the environment map (zdr_amd/envmap.py, build_tables; zdr_scene_update_envmap_sampling): the map families
the tests build them from, a checker that works on the tables alone, and a float64 restatement of the weights they are built from.
A helper, not a test; no GPU involved anywhere in this file.

The checker (check_tables) takes (alias_prob, alias_idx, pdf) in the layout of zdr_scene_set_envmap, in float64 NumPy, and for each of the
257 tables (the marginal p(y), then 256 conditionals p(x|y)) holds:
  1. alias in range, prob finite and within [0, 1];
  2. the mass the table assigns, q_j = (prob_j + sum over i with alias_i = j of (1 - prob_i)) / n, agrees with the pmf the pdf implies
     (conditional: pdf[y, :] / sum_x pdf[y, :]; marginal: sum_x pdf[y, :] / sum pdf): |q_j - pmf_j| <= bar max(pmf_j, 1 / n) — relative
     for the heavy entries (a sun holds most of a row), in units of the uniform mass for the light ones.  A row whose pdf is 0 throughout
     implies no pmf and is not compared; it must never be drawn, which 3. asks of the marginal table;
  3. exact zeros: in a table with a positive total every entry whose pdf is 0 has q_j = 0 exactly — prob_j = 0, and no entry with
     prob_i < 1 has it as its alias;
  4. mean(pdf) = 1 to 1e-5 and pdf >= 0.

The bars are MEASURED, never taken from a GPU (``python tests/envmap_tables.py`` prints profiles/envmap_sampling_margins.txt, about four
minutes; tests/test_envmap_tables_host.py holds the constants below to what it measures on the maps it builds):
  Q_MEASURED      the largest residual of 2. over the host's tables (float64 pairing, float32 storage) of every family and shape below,
                  compensate_mis on and off; Q_BAR = max(4 x that, 2^-20) is the bar for tables paired and stored on the device;
  AGREE_MEASURED  max |pdf_host - pdf_64| / max(pdf_host) over the same maps without the constant one, pdf_64 from weights64 below: what
                  the host's float32 weight map and compensation cost.  AGREE_BAR = 4 x that bounds |pdf_device - pdf_host| / max(pdf_host).
                  The constant map is left out of this comparison alone: under compensation its weights are scale - mean row / row_mean
                  = 0 +- rounding, so the host's own answer is rounding noise.
"""
import math
import os
import sys
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:       # (run as a script)
    sys.path.insert(0, ROOT)

from zdr_amd import envmap as E  # noqa: E402

W, H = E.SAMPLE_MAP_W, E.SAMPLE_MAP_H
FAMILIES = ("random_hdr", "sun_sky", "black", "black_rows", "constant")
SHAPES = ((16, 32), (24, 48), (64, 128), (32, 32))
BIG_SHAPE = (256, 512)

Q_MEASURED = 1.72e-7           # measure() -> 1.712e-07, rounded up (profiles/envmap_sampling_margins.txt)
Q_BAR = max(4.0 * Q_MEASURED, 2.0 ** -20)      # = 2^-20
AGREE_MEASURED = 1.42e-6       # measure() -> 1.414e-06, rounded up
AGREE_BAR = 4.0 * AGREE_MEASURED


def make_map(family, shape, seed=0):
    """(h, w, 3) float32, seeded"""
    h, w = shape
    rng = np.random.default_rng(seed + 1000 * FAMILIES.index(family) + h)
    if family == "random_hdr":
        return (rng.random((h, w, 3)) ** 4 * 5.0).astype(np.float32)
    if family == "sun_sky":                                       # a sun of a few texels: compensation zeroes most of the map
        img = rng.uniform(0.05, 0.6, (h, w, 3)).astype(np.float32)
        y, x, n = h * 5 // 32, w * 40 // 64, max(2, h // 16)
        img[y:y + n, x:x + n + 1] = (300.0, 260.0, 200.0)
        return img
    if family == "black":
        return np.zeros((h, w, 3), np.float32)
    if family == "black_rows":                                    # the top 200 of 256 rows zero
        img = (rng.random((h, w, 3)) ** 4 * 5.0).astype(np.float32)
        img[:h * 200 // 256] = 0.0
        return img
    if family == "constant":
        return np.full((h, w, 3), 2.0, np.float32)
    raise ValueError(family)


def sun_map(shape, at, seed=0):
    """a dim sky and a sun of 2 x 3 texels whose corner is texel `at` = (row, column): the maps A and B of the stale-table test"""
    h, w = shape
    img = np.random.default_rng(seed).uniform(0.02, 0.05, (h, w, 3)).astype(np.float32)
    img[at[0]:at[0] + 2, at[1]:at[1] + 3] = (600.0, 520.0, 400.0)
    return img


_WEIGHT_MAPS = {}


def host_tables(img, compensate_mis=True):
    """E.build_tables(E.prepare_image(img), compensate_mis), with its weight map (seven seconds, the same for both values of
    compensate_mis) computed once per image and handed back to build_tables itself"""
    I = E.prepare_image(img)
    key = (I.shape, I.tobytes())
    if key not in _WEIGHT_MAPS:
        _WEIGHT_MAPS[key] = E.weight_map(I)
    with mock.patch.object(E, "weight_map", lambda _img: _WEIGHT_MAPS[key].copy()):
        return E.build_tables(I, compensate_mis=compensate_mis)


def _bilinear_matrix(coord, n):
    """(len(coord), n) float64: row k holds the two clamp-to-edge bilinear weights of texture coordinate coord[k] in [0, 1] units"""
    t = coord * n - 0.5
    t0 = np.floor(t)
    f = t - t0
    i0 = np.clip(t0.astype(np.int64), 0, n - 1); i1 = np.clip(t0.astype(np.int64) + 1, 0, n - 1)
    M = np.zeros((coord.shape[0], n))
    np.add.at(M, (np.arange(coord.shape[0]), i0), 1.0 - f)
    np.add.at(M, (np.arange(coord.shape[0]), i1), f)
    return M


def weights64(img, compensate_mis=True):
    """The weights the tables are built from, (H, W) float64: E.weight_map and the compensation of E.build_tables restated in float64.
    Luminance and the bilinear lookup are linear and no tap comes near the clamp of 1e8 (asserted), so the 289 taps factor into one
    matrix per axis: sum_dy w(dy) sin(pi v) R_y(dy)  .  L  .  (sum_dx w(dx) R_x(dx))^T."""
    I = E.prepare_image(img).astype(np.float64)
    L = 0.212671 * I[..., 0] + 0.715160 * I[..., 1] + 0.072169 * I[..., 2]
    assert np.abs(L).max() < 1e8
    h, w = L.shape
    n = int(math.ceil(1.0 / 0.125))
    Ay, Ax, sw = np.zeros((H, h)), np.zeros((W, w)), 0.0
    for d in range(-n, n + 1):
        o = d * 0.125
        g = math.exp(-4.0 * o * o)
        v = (np.arange(H) + 0.5 + o) / H
        Ay += (g * np.sin(v * math.pi))[:, None] * _bilinear_matrix(v, h)
        Ax += g * _bilinear_matrix((np.arange(W) + 0.5 + o) / W, w)
        sw += g
    s = Ay @ L @ Ax.T / (sw * sw)
    if compensate_mis:
        rw = np.sin((np.arange(H) + 0.5) / H * math.pi)
        s = np.maximum(s - s.mean() * (rw / rw.mean())[:, None], 0.0)
    return s


def pdf64(img, compensate_mis=True):
    """the pdf of exact tables over weights64: p(x|y) p(y) W H = |w| / mean |w|, 1 everywhere for a map without weight"""
    a = np.abs(weights64(img, compensate_mis))
    rows = a.sum(axis=1, keepdims=True)
    cond = np.where(rows > 0, a / np.where(rows > 0, rows, 1.0), 1.0 / W)
    marg = rows / rows.sum() if rows.sum() > 0 else np.full_like(rows, 1.0 / H)
    return cond * marg * (W * H)


def agreement(pdf_a, pdf_b):
    """max |a - b| / max(b): absolute, relative to the largest density — near-zero texels may clamp differently on two sides"""
    a, b = np.asarray(pdf_a, np.float64).reshape(-1), np.asarray(pdf_b, np.float64).reshape(-1)
    return float(np.abs(a - b).max() / b.max())


def table_mass(prob, alias):
    """q of the docstring for a stack of tables: prob, alias (T, n) -> (T, n) float64"""
    T, n = prob.shape
    q = prob.astype(np.float64).copy()
    np.add.at(q, (np.repeat(np.arange(T), n), alias.reshape(-1)), (1.0 - prob.astype(np.float64)).reshape(-1))
    return q / n


def _check_stack(name, prob, alias, mass, bar):
    """one stack of tables against the (unnormalised) mass its pdf implies; returns the residual of 2."""
    T, n = prob.shape
    assert alias.min() >= 0 and alias.max() < n, (name, "alias out of range", int(alias.min()), int(alias.max()))
    assert np.isfinite(prob).all() and prob.min() >= 0.0 and prob.max() <= 1.0, (name, "prob outside [0, 1]", float(prob.min()), float(prob.max()))
    q = table_mass(prob, alias)
    total = mass.sum(axis=1, keepdims=True)
    live = total[:, 0] > 0
    zero = (mass == 0) & live[:, None]
    if zero.any():
        t, j = np.nonzero(zero & (q != 0))
        assert t.size == 0, (name, "entries with pdf 0 that can be drawn", t.size, "first", int(t[0]), int(j[0]), float(q[t[0], j[0]]))
        assert (prob[zero] == 0).all(), (name, "an entry with pdf 0 whose prob is not 0")
    pmf = mass[live] / total[live]
    res = np.abs(q[live] - pmf) / np.maximum(pmf, 1.0 / n)
    worst = float(res.max()) if res.size else 0.0
    if bar is not None:
        t, j = np.unravel_index(int(res.argmax()), res.shape) if res.size else (0, 0)
        assert worst <= bar, (name, "table mass and pdf disagree", worst, "bar", bar, "table", int(np.nonzero(live)[0][t]), "entry", int(j))
    return worst


def check_tables(alias_prob, alias_idx, pdf, bar=None):
    """Holds the four properties of the module docstring; returns the largest residual of 2. (bar None: measured, not asserted)."""
    prob = np.asarray(alias_prob, np.float64); alias = np.asarray(alias_idx, np.int64); pdf = np.asarray(pdf, np.float64).reshape(H, W)
    assert prob.shape == (H + H * W,) and alias.shape == prob.shape
    assert np.isfinite(pdf).all() and pdf.min() >= 0.0, ("pdf", float(pdf.min()))
    assert abs(pdf.mean() - 1.0) <= 1e-5, ("mean(pdf)", float(pdf.mean()))
    r_marg = _check_stack("marginal", prob[None, :H], alias[None, :H], pdf.sum(axis=1)[None, :], bar)
    r_cond = _check_stack("conditional", prob[H:].reshape(H, W), alias[H:].reshape(H, W), pdf, bar)
    return max(r_marg, r_cond)


def uniform_tables():
    """valid tables of the wrong density: every entry keeps itself, pdf 1"""
    return (np.ones(H + H * W, np.float32), np.concatenate([np.arange(H), np.tile(np.arange(W), H)]).astype(np.int32), np.ones(H * W, np.float32))


def set_map_with_uniform_tables(scene, img):
    """What Scene.add_envmap does, with uniform_tables() in place of the seven seconds of build_tables: the scene gets the map's texture,
    and tables that a rebuild on the device has to replace."""
    from zdr_amd import _native as N
    I = E.prepare_image(img)
    prob, alias, pdf = uniform_tables()
    N.check(N.lib().zdr_scene_set_envmap(scene._handle, I.ctypes.data, I.shape[0], I.shape[1], prob.ctypes.data, alias.ctypes.data, pdf.ctypes.data, W, H))
    scene.env_count = 1
    scene._envmap = (I, prob, alias, pdf)
    return scene


def env_only_scene(integrator="path", **kw):
    """the Cornell box without its light: every light sample goes to the environment"""
    from zdr_amd.scenes import cbox_models, make_scene
    return make_scene(integrator, models=[(cbox_models()[0][0], None, 0.0)], **kw)


SUN_A, SUN_B = (12, 5), (11, 56)      # the stale-table case: the sun of a 32 x 64 map in front of the box's opening, upper left, then upper right


def all_maps():
    """(family, shape) of every map of the tests: the four small shapes of every family, and the random map at the large shape"""
    return [(f, s) for f in FAMILIES for s in SHAPES] + [("random_hdr", BIG_SHAPE)]


def measure(maps=None, out=None):
    """-> (largest residual of the host's tables, largest host-vs-float64 disagreement) over `maps`, both values of compensate_mis"""
    q_worst = a_worst = 0.0
    for family, shape in (all_maps() if maps is None else maps):
        img = make_map(family, shape)
        for comp in (True, False):
            prob, alias, pdf = host_tables(img, comp)
            q = check_tables(prob, alias, pdf)
            a = agreement(pdf64(img, comp), pdf) if family != "constant" else float("nan")
            q_worst = max(q_worst, q); a_worst = max(a_worst, a) if a == a else a_worst
            if out is not None:
                print(f"  {family:10s} {shape[0]:3d} x {shape[1]:3d}  compensate_mis {int(comp)}  table residual {q:.3e}  host float32 vs float64 pdf {a:.3e}"
                      f"  pdf == 0: {float((pdf == 0).mean()):.3f}  max pdf {float(pdf.max()):.4g}", file=out, flush=True)
        _WEIGHT_MAPS.clear()
    return q_worst, a_worst


if __name__ == "__main__":      # the table of profiles/envmap_sampling_margins.txt
    print("host tables (zdr_amd/envmap.py, build_tables: float64 pairing, float32 storage) of every map of the tests; no GPU involved")
    q, a = measure(out=sys.stdout)
    print(f"Q_MEASURED = {q:.3e}  x 4 = {4 * q:.3e}, never below 2^-20 = {2.0 ** -20:.3e}   (module: Q_MEASURED = {Q_MEASURED:.3e}, Q_BAR = {Q_BAR:.3e})")
    print(f"AGREE_MEASURED = {a:.3e}  x 4 = {4 * a:.3e}   (module: AGREE_MEASURED = {AGREE_MEASURED:.3e}, AGREE_BAR = {AGREE_BAR:.3e})")
