"""The shading math point by point: seeded families of (wo, wi, roughness, ...) rows, a float64 reference of microfacet.py's formulas, and
one bound per output per point (tests/test_brdf_cases_host.py on the CPU, tests/test_gpu_brdf_cases.py through zdr_shading_dump).

Reference (ggx_eval / ggx_sample_np with dt = float64): microfacet.py:7-92 and the closed-form d/dr of SURVEY App. A.6 on the float32
inputs, with the same clamps (the float32 values of 1e-5, 1e-6, 0.99999, as the kernels compare against them).  The SAME functions with
dt = float32 are the IEEE float32 transcription (NumPy rounds every operation to float32 once, in the order of csrc/microfacet.h);
`mut` switches one deliberate mistake on in it (MUTATIONS), so that the bound can be shown not to be vacuous.

Bound (eval_bounds): a first-order forward error model in float64, eps = K * 2^-24.
  * every rounded intermediate carries a relative error eps per operation (the counts are written next to each line);
  * the three differences that cancel carry an ABSOLUTE error eps, whatever fed them:  t = nh2 (a2 - 1) + 1,  the numerator
    1 - nh2 (1 + a2) of dD,  and 1 - nv^2 in ki / ko;  t itself is checked directly, |t - t64| <= eps;
  * c = clamp(wo.h) is a dot product of terms of either sign: absolute error through sum |wo_i h_i|;
  * sums of terms of opposite sign (dS, dglossy, the two halves of pdf when wi.z < 0) are bounded through the terms' absolute values;
  * powers of 1 / t are NOT linearised: with rel = eps / t64 the factor is (1 - rel)^-n - 1, infinite from rel >= 1 on.  In exact
    arithmetic t >= a2 = r^4, so this is where roughness meets its floor: a point with t64 <= eps may have t = 0, D = inf in float32
    and its bound says so (inf); every output must be FINITE wherever t64 > 2 eps (finite_required).
K is measured, never taken from a GPU (measure_k; profiles/brdf_points_margins.txt): the smallest integer at which the oracle's float32
functions (zdro_ggx_brdf, zdro_ggx_sample_pdf, zdro_ggx_brdf_grad, zdro_ggx_dlnpdf_dr, zdro_ggx_sample; IEEE and FMA build) and the
float32 transcription pass at every point of every family, times 4: v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 are uncorrected at about 1 ulp
each, the kernels chain several and contract differently.  The sampled direction has a bound of its own kind (wi_bound, K_S measured
the same way): absolute, and aware of the two square roots of the VNDF warp that cancel (h = sqrt(1 - px^2), pz = sqrt(1 - px^2 - py^2)).
The frame's bound is FRAME_K * 2^-24 * max(1, |d|), measured on the transcription alone (the oracle exports no frame function).

Families (family(name) -> rows as zdr_shading_dump takes them; no point is exempt):
  generic     wo.z, wi.z in [1e-4, 1], r in [0.03, 1], diffuse in [0, 1] with exact 0 and 1
  peak        wi = reflection of wo about a normal tilted by atan(x alpha), x in {0, 2^-12, 2^-8, 2^-4, 1, 4}, random azimuth;
              r in {0.03, 0.05, 0.1, 0.15, 0.3, 0.6, 1}; wo = wi = (0, 0, 1) for every r (r = 1: a2 - 1 = 0)
  collocated  wi = wo, wo.z in [1e-4, 1]
  grazing     wo.z in {1e-4, 1e-3, 1e-2} x wi.z in {1e-4, 1e-3, 1e-2, 2e-5, 1e-5, 5e-6, 0, -1e-3, -0.5}: the 1e-5 clamps from both sides.
              wi = -wo is left out (h = 0 / 0, also in the reference): azimuths are random, so no row has it.
  floor       r in [1e-3, 0.03), generic and peak directions
  sampling    wo as generic plus normal incidence; u_lobe in {0, 0.5-, 0.5, 1-}; u_dir.x in {0, 2^-24, ..., 1-}; u_dir.y in
              {0, .25, .5, .75, 1-} and random.  pdf, f / pdf, dfdr, dlnpdf_dr are judged at the wi_local under test.  Two decisions may
              flip: wh.z < 0.99999 in sample_wm_disk (both branches accepted when wh.z64 is within eps of it) and the flag
              wi_local.z < 1e-4 (open within wi_bound); the share of such rows is capped at FLIP_CAP.
  frame       the six axes, |n.x| = |n.z| ties, nearly-axis and random normals
"""
import functools
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:       # (run as a script: python tests/brdf_cases.py prints the table of profiles/brdf_points_margins.txt)
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
K_MEASURED, K = 6, 24          # measure_k() -> K_MEASURED; K = 4 x (profiles/brdf_points_margins.txt; test_brdf_cases_host.py holds them to it)
KS_MEASURED, K_S = 2, 8        # the same for wi_bound
FRAME_MEASURED, FRAME_K = 6, 24
FLIP_CAP = 0.01
F32 = np.float32
C5, C6, C4, CT1 = float(F32(1e-5)), float(F32(1e-6)), float(F32(1e-4)), float(F32(0.99999))
EVAL_FAMILIES = ("generic", "peak", "collocated", "grazing", "floor")
FAMILIES = EVAL_FAMILIES + ("sampling", "frame")
PEAK_R = (0.03, 0.05, 0.1, 0.15, 0.3, 0.6, 1.0)
PEAK_TILT = (0.0, 2.0 ** -12, 2.0 ** -8, 2.0 ** -4, 1.0, 4.0)
EVAL_OUT = ("f", "pdf", "dfdr", "dlnpdf_dr", "t", "D", "grad")
# mutation -> the families that exercise the term (every one of them must reject it)
MUTATIONS = {
    "g1_without_sqrt": EVAL_FAMILIES,
    "dD_one_minus_a2": ("generic", "peak", "collocated", "grazing"),   # floor: the variants differ by 2 nh2 a2 < 2 r^4 < 1.7e-6, inside the numerator's absolute eps
    "fresnel_fourth_power": ("generic", "peak", "grazing", "floor"),   # collocated: wo.h = 1, Fresnel is 0.04 whatever the power
    "pdf_without_half": EVAL_FAMILIES, "dlnpdf_without_4r3": EVAL_FAMILIES, "dglossy_without_dG1o": EVAL_FAMILIES,
    "inv4_without_clamp": ("grazing",), "wi_z_sign_dropped": ("grazing",),
    "vndf_without_lerp": ("sampling",), "t2_cross_swapped": ("sampling",),
}


# ---------------------------------------------------------------------------------- the formulas, float64 or float32
def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _normalize(a):
    return a * (a.dtype.type(1) / np.sqrt(_dot(a, a)))[:, None]


def ggx_eval(wo, wi, r, diffuse, ct, dt=np.float64, mut=None):
    """ggx_terms / ggx_brdf_from / ggx_pdf_from / ggx_dfdr_from / brdf_grad, every intermediate kept (eval_bounds reads them)."""
    one, PI = dt(1), dt(np.pi)
    INV_PI = dt(1 / np.pi)
    wo, wi, diffuse, ct = (np.asarray(x, dt).reshape(-1, 3) for x in (wo, wi, diffuse, ct))
    r = np.asarray(r, dt).reshape(-1)
    g = NS(wo=wo, wi=wi, r=r, diffuse=diffuse, ct=ct)
    with np.errstate(all="ignore"):
        alpha = r * r
        g.a2 = alpha * alpha
        g.h = _normalize(wi + wo)
        nh = np.maximum(dt(C5), g.h[:, 2])
        g.nh2 = nh * nh
        g.t = g.nh2 * (g.a2 - one) + one
        g.D = g.a2 / (PI * (g.t * g.t))
        g.wdh = _dot(wo, g.h)
        g.c = np.clip(g.wdh, dt(C5), one)
        x = one - g.c
        x2 = x * x
        g.p5 = x2 * x2 if mut == "fresnel_fourth_power" else x2 * x2 * x
        g.F = dt(0.04) + dt(0.96) * g.p5
        g.nvi, g.nvo = np.maximum(dt(C5), wi[:, 2]), np.maximum(dt(C5), wo[:, 2])
        g.omi, g.omo = one - g.nvi * g.nvi, one - g.nvo * g.nvo
        g.ki, g.ko = g.omi / (g.nvi * g.nvi), g.omo / (g.nvo * g.nvo)
        g.yi, g.yo = one + g.a2 * g.ki, one + g.a2 * g.ko
        g.si, g.so = (g.yi, g.yo) if mut == "g1_without_sqrt" else (np.sqrt(g.yi), np.sqrt(g.yo))
        g.opi, g.opo = one + g.si, one + g.so
        g.G1i, g.G1o = dt(2) / g.opi, dt(2) / g.opo
        g.inv4 = one / (dt(4) * wi[:, 2] * wo[:, 2]) if mut == "inv4_without_clamp" else one / (dt(4) * g.nvi * g.nvo)
        g.wiz = np.abs(wi[:, 2]) if mut == "wi_z_sign_dropped" else wi[:, 2]
        g.spec = (g.D * g.F * (g.G1i * g.G1o)) * g.inv4
        g.dpi = diffuse * INV_PI
        g.f = (g.spec[:, None] + g.dpi) * g.wiz[:, None]
        a = np.abs(g.wdh)
        g.glossy = (g.G1o / np.abs(wo[:, 2]) * g.D * a) / (dt(4) * a)
        g.cz = g.wiz * INV_PI
        g.pdf = dt(0.5) * g.cz + (one if mut == "pdf_without_half" else dt(0.5)) * g.glossy
        g.numD = one - g.nh2 * ((one - g.a2) if mut == "dD_one_minus_a2" else (one + g.a2))
        g.dD = g.numD / (PI * (g.t * g.t * g.t))
        g.dG1i, g.dG1o = -g.ki / (g.si * (g.opi * g.opi)), -g.ko / (g.so * (g.opo * g.opo))
        g.T1 = g.dD * (g.G1i * g.G1o)
        g.A, g.B = g.dG1i * g.G1o, g.G1i * g.dG1o
        g.T2 = g.D * (g.A + g.B)
        g.dS = g.T1 + g.T2
        g.r3 = r * r * r
        g.U1, g.U2 = (dt(0) * g.D if mut == "dglossy_without_dG1o" else g.dG1o * g.D), g.G1o * g.dD
        g.dgl = (g.U1 + g.U2) / (dt(4) * np.abs(wo[:, 2]))
        g.num = dt(0.5) * g.dgl if mut == "dlnpdf_without_4r3" else dt(0.5) * g.dgl * dt(4) * g.r3
        g.dlnpdf_dr = g.num / g.pdf
        g.pref = dt(4) * g.r3 * (g.F * g.wiz * g.inv4)
        g.dfdr = g.pref * g.dS
        g.csum = ct[:, 0] + ct[:, 1] + ct[:, 2]
        g.grad = np.concatenate([ct * g.cz[:, None], (g.csum * g.dfdr)[:, None]], 1)
        g.thr = g.f / g.pdf[:, None]
    return g


def ggx_sample_np(wo, r, u_lobe, u2, dt=np.float64, mut=None, axis_branch=None):
    """ggx_sample (microfacet.h:78-103).  axis_branch: None = decide wh.z < 0.99999 as computed; a bool (array) = T1 = (1, 0, 0) where True, the
    cross product where False (the float64 answer under the other decision).  -> (wi_local, whz, parts for wi_bound)"""
    one = dt(1)
    wo = np.asarray(wo, dt).reshape(-1, 3)
    r, u_lobe, u2 = np.asarray(r, dt).reshape(-1), np.asarray(u_lobe, dt).reshape(-1), np.asarray(u2, dt).reshape(-1, 2)
    with np.errstate(all="ignore"):
        rad, phi = np.sqrt(u2[:, 0]), dt(2) * dt(np.pi) * u2[:, 1]
        px, py = rad * np.cos(phi), rad * np.sin(phi)
        cosine = np.stack([px, py, np.sqrt(one - u2[:, 0])], 1)
        alpha = r * r
        wh = _normalize(np.stack([alpha * wo[:, 0], alpha * wo[:, 1], wo[:, 2]], 1))
        wh = np.where((wh[:, 2] < 0)[:, None], -wh, wh)
        generic = (wh[:, 2] < dt(CT1)) if axis_branch is None else ~np.broadcast_to(np.asarray(axis_branch, bool), r.shape)
        ez = np.zeros_like(wh); ez[:, 2] = 1
        ex = np.zeros_like(wh); ex[:, 0] = 1
        T1 = np.where(generic[:, None], _normalize(_cross(ez, wh)), ex)
        T2 = _cross(T1, wh) if mut == "t2_cross_swapped" else _cross(wh, T1)
        h = np.sqrt(one - px * px)
        py2 = py if mut == "vndf_without_lerp" else h + ((one + wh[:, 2]) * dt(0.5)) * (py - h)
        q = one - (px * px + py2 * py2)
        pz = np.sqrt(np.maximum(dt(0), q))
        nh = px[:, None] * T1 + py2[:, None] * T2 + pz[:, None] * wh
        v = np.stack([alpha * nh[:, 0], alpha * nh[:, 1], np.maximum(dt(C6), nh[:, 2])], 1)
        wm = _normalize(v)
        i = -wo
        glossy = i - wm * (dt(2) * _dot(wm, i))[:, None]
        wi = np.where((u_lobe < dt(0.5))[:, None], cosine, glossy)
    return wi, wh[:, 2], NS(px=px, py2=py2, h=h, s=(one + wh[:, 2]) * dt(0.5), pz=pz, vlen=np.sqrt(_dot(v, v)), is_cos=u_lobe < dt(0.5), wolen=np.sqrt(_dot(wo, wo)))


def onb_np(n, d, dt=np.float64):
    """make_onb, to_local, to_world(to_local) (scene.h:547-556) -> (n, 15): tangent, binormal, normal, local, world"""
    n, d = np.asarray(n, dt).reshape(-1, 3), np.asarray(d, dt).reshape(-1, 3)
    z = np.zeros(len(n), dt)
    first = np.abs(n[:, 0]) > np.abs(n[:, 2])
    b = _normalize(np.where(first[:, None], np.stack([-n[:, 1], n[:, 0], z], 1), np.stack([z, -n[:, 2], n[:, 1]], 1)))
    t = _normalize(_cross(b, n))
    loc = np.stack([_dot(d, t), _dot(d, b), _dot(d, n)], 1)
    w = loc[:, 0:1] * t + loc[:, 1:2] * b + loc[:, 2:3] * n
    return np.concatenate([t, b, n, loc, w], 1)


# ---------------------------------------------------------------------------------------------------- bounds
def _inv_pow(rel, n):
    """relative error of x^-n when x carries the relative error rel, not linearised; inf from rel >= 1 on"""
    with np.errstate(all="ignore"):
        return np.where(rel < 1, (1 - np.minimum(rel, 0.999999999)) ** -n - 1, np.inf)


def eval_bounds(g, k=K):
    """g = ggx_eval(..., float64) -> NS of ABSOLUTE bounds for f (n, 3), pdf, dfdr, dlnpdf_dr, t, D, grad (n, 4), thr (n, 3), and
    finite_required (t64 > 2 eps).  Counts in units of eps = k 2^-24, one per rounded operation."""
    e = k * U
    ab = np.abs
    with np.errstate(all="ignore"):
        relT = e / g.t                                                       # t: absolute eps, flat
        rel_D = 3 * e + _inv_pow(relT, 2) + 3 * e                            # a2 (r*r, alpha*alpha: 3), 1/t^2, t*t, pi*, divide
        abs_c = 8 * e * (ab(g.wo * g.h).sum(1))                              # h (normalise: 5), product, two additions
        abs_x = abs_c + e * ab(1 - g.c)
        abs_F = 0.96 * (5 * g.p5 / np.maximum(ab(1 - g.c), 1e-300) * abs_x + g.p5 * 4 * e) + g.F * e
        rel_F = abs_F / g.F

        def g1(om, nv, k_, y, s, op):
            abs_k = (e + ab(om) * 3 * e) / (nv * nv)                         # 1 - nv^2: absolute eps, flat; nv*nv, divide
            abs_y = g.a2 * abs_k + g.a2 * k_ * 4 * e + y * e
            rel_s = 0.5 * abs_y / y + e
            abs_op = s * rel_s + op * e
            rel_op = abs_op / op
            abs_dG1 = (abs_k + k_ * (rel_s + 2 * rel_op + 3 * e)) / (s * op * op)
            return rel_op + e, abs_dG1
        rel_G1i, abs_dG1i = g1(g.omi, g.nvi, g.ki, g.yi, g.si, g.opi)
        rel_G1o, abs_dG1o = g1(g.omo, g.nvo, g.ko, g.yo, g.so, g.opo)
        rel_spec = rel_D + rel_F + rel_G1i + rel_G1o + (2 + 4) * e           # inv4: 2
        abs_f = ab(g.wi[:, 2:3]) * ((g.spec * rel_spec)[:, None] + g.dpi * e + (g.spec[:, None] + g.dpi) * 2 * e)
        rel_gl = rel_G1o + rel_D + 6 * e                                     # |wo.h| enters and leaves: only its roundings stay
        abs_pdf = 0.5 * ab(g.cz) * 2 * e + 0.5 * g.glossy * (rel_gl + e) + 0.5 * (ab(g.cz) + g.glossy) * e
        abs_dD = (e + ab(g.numD) * (_inv_pow(relT, 3) + 4 * e)) * (1 + _inv_pow(relT, 3)) / (np.pi * g.t ** 3)   # numerator: absolute eps, flat
        GG = g.G1i * g.G1o
        abs_T1 = abs_dD * GG + ab(g.T1) * (rel_G1i + rel_G1o + 2 * e)
        abs_A = abs_dG1i * g.G1o + ab(g.A) * (rel_G1o + e)
        abs_B = abs_dG1o * g.G1i + ab(g.B) * (rel_G1i + e)
        abs_AB = abs_A + abs_B + ab(g.A + g.B) * e
        abs_T2 = ab(g.T2) * (rel_D + e) + g.D * (1 + rel_D) * abs_AB
        abs_dS = abs_T1 + abs_T2 + (ab(g.T1) + ab(g.T2)) * e
        rel_pref = rel_F + 7 * e                                             # r^3: 2, inv4: 2, three products
        abs_dfdr = ab(g.pref) * (1 + rel_pref) * abs_dS + ab(g.dfdr) * (rel_pref + e)
        abs_U1 = abs_dG1o * g.D * (1 + rel_D) + ab(g.U1) * (rel_D + e)
        abs_U2 = g.G1o * abs_dD + ab(g.U2) * (rel_G1o + e)
        abs_dgl = (abs_U1 + abs_U2 + (ab(g.U1) + ab(g.U2)) * e + ab(g.U1 + g.U2) * 2 * e) / (4 * ab(g.wo[:, 2]))
        abs_num = 2 * g.r3 * (abs_dgl + ab(g.dgl) * 3 * e)
        rel_ip = _inv_pow(abs_pdf / ab(g.pdf), 1)
        abs_dln = abs_num * (1 + rel_ip) / ab(g.pdf) + ab(g.dlnpdf_dr) * (rel_ip + 2 * e)
        abs_grad = np.concatenate([ab(g.grad[:, :3]) * 2 * e,
                                   (ab(g.ct).sum(1) * 2 * e * (ab(g.dfdr) + abs_dfdr) + ab(g.csum) * abs_dfdr + ab(g.grad[:, 3]) * e)[:, None]], 1)
        abs_thr = abs_f * (1 + rel_ip)[:, None] / ab(g.pdf)[:, None] + ab(g.thr) * (rel_ip + 2 * e)[:, None]
    B = NS(f=abs_f, pdf=abs_pdf, dfdr=abs_dfdr, dlnpdf_dr=abs_dln, t=np.full(len(g.t), e), D=g.D * rel_D, grad=abs_grad, thr=abs_thr,
           finite_required=g.t > 2 * e)
    for name in ("f", "pdf", "dfdr", "dlnpdf_dr", "D", "grad", "thr"):       # a NaN bound (0 x inf) bounds nothing
        v = getattr(B, name)
        v[np.isnan(v)] = np.inf
    return B


def judge(got, ref, bound, finite_required):
    """-> (ok per row, error / bound per row): inside the bound — a non-finite answer only where the bound is infinite and finiteness is
    not required; a NaN reference (0 / 0 in float64 as well) leaves the row open."""
    got, ref, bound = (np.asarray(x, np.float64) for x in (got, ref, bound))
    if got.ndim == 1:
        got, ref, bound = got[:, None], ref[:, None], bound[:, None]
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        fr = finite_required[:, None]
        inside = np.where(fr, np.isfinite(got) & (err <= bound), (err <= bound) | np.isinf(bound)) | np.isnan(ref)
        ratio = np.where(err == 0, 0.0, err / bound)                              # err / inf = 0, err / 0 = inf
        ratio = np.where(np.isnan(ratio), np.where(inside, 0.0, np.inf), ratio)    # a non-finite answer: admissible or not, nothing in between
    return inside.all(1), ratio.max(1)


def judge_eval(out, g, k=K, names=EVAL_OUT):
    """out: {name: array} of the answers under test, g the float64 reference at the same inputs -> {name: (ok, ratio)}"""
    B = eval_bounds(g, k)
    return {n: judge(out[n], getattr(g, n), getattr(B, n), B.finite_required) for n in names if n in out}


def wi_bound(p, ks=K_S):
    """absolute bound of every component of the sampled wi_local; p = the parts ggx_sample_np returns in float64"""
    e = ks * U
    with np.errstate(all="ignore"):
        abs_h = np.minimum(np.sqrt(3 * e), 3 * e / (2 * np.maximum(p.h, 1e-300)))          # h = sqrt(1 - px^2) cancels at |px| -> 1
        abs_py = (1 - p.s) * abs_h + e
        abs_q = 2 * np.abs(p.px) * e + 2 * np.abs(p.py2) * abs_py + e
        abs_pz = np.minimum(np.sqrt(abs_q), abs_q / (2 * np.maximum(p.pz, 1e-300)))        # pz = sqrt(1 - px^2 - py^2) likewise
        abs_nh = abs_py + abs_pz + 2 * e                                                   # px T1 + py T2 + pz wh, unit axes
        glossy = 4 * e + 2 * p.wolen * abs_nh / p.vlen                                     # normalising (alpha nh.x, alpha nh.y, nh.z): 1 / |v|; reflecting: 2 |wo|
    return np.where(p.is_cos, 4 * e, glossy)


# -------------------------------------------------------------------------------------------------- families
def _dirs(rng, n, zlo=1.0001e-4):
    """unit vectors with z in [zlo, 1]: half log-uniform, half uniform in z"""
    z = np.where(rng.random(n) < 0.5, np.exp(rng.uniform(np.log(zlo), 0.0, n)), rng.uniform(zlo, 1.0, n))
    return _with_z(rng, z)


def _with_z(rng, z):
    phi = rng.uniform(0, 2 * np.pi, len(z))
    s = np.sqrt(np.maximum(0.0, 1 - z * z))
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)


def _rough(rng, n, lo=0.03, hi=1.0):
    return np.where(rng.random(n) < 0.5, np.exp(rng.uniform(np.log(lo), np.log(hi), n)), rng.uniform(lo, hi, n))


def _diffuse(rng, n):
    d = rng.uniform(0, 1, (n, 3))
    pick = rng.random(n)
    d[pick < 0.125] = 0.0
    d[pick > 0.875] = 1.0
    return d


def _peak_dirs(rng, r, per):
    """for every roughness of r (m,) and tilt: `per` rows (wo, wi = reflection of wo about a normal at polar angle atan(tilt alpha))"""
    wo_l, wi_l, r_l = [], [], []
    for tilt in PEAK_TILT:
        rr = np.repeat(r, per)
        wo = _dirs(rng, len(rr))
        m = _with_z(rng, np.cos(np.arctan(tilt * rr * rr)))
        wi = 2 * (wo * m).sum(1)[:, None] * m - wo
        wo_l.append(wo); wi_l.append(wi); r_l.append(rr)
    wo, wi, r = np.concatenate(wo_l), np.concatenate(wi_l), np.concatenate(r_l)
    keep = wi[:, 2] >= 1.0001e-4
    return wo[keep], wi[keep], r[keep]


def _eval_rows(rng, wo, wi, r):
    n = len(r)
    rows = np.zeros((n, 16), np.float32)
    rows[:, 0:3], rows[:, 3:6], rows[:, 6] = wo, wi, r
    rows[:, 7:10], rows[:, 10:13] = _diffuse(rng, n), rng.uniform(-1, 1, (n, 3))
    return rows[:-1] if n % 64 == 0 else rows


@functools.lru_cache(None)
def family(name):
    """-> (n, 16) float32 rows in the layout of zdr_shading_dump (eval, sample or frame), read-only"""
    rng = np.random.default_rng(7000 + FAMILIES.index(name))
    up = np.array([[0.0, 0.0, 1.0]])
    if name == "generic":
        n = 60001
        rows = _eval_rows(rng, _dirs(rng, n), _dirs(rng, n), _rough(rng, n))
    elif name == "peak":
        wo, wi, r = _peak_dirs(rng, np.array(PEAK_R), 500)
        k = len(PEAK_R)
        wo, wi, r = np.concatenate([np.repeat(up, k, 0), wo]), np.concatenate([np.repeat(up, k, 0), wi]), np.concatenate([np.array(PEAK_R), r])
        rows = _eval_rows(rng, wo, wi, r)
    elif name == "collocated":
        n = 20001
        wo = np.concatenate([up, _dirs(rng, n - 1)])
        rows = _eval_rows(rng, wo, wo, _rough(rng, n))
    elif name == "grazing":
        zo = np.array([1e-4, 1e-3, 1e-2])
        zi = np.array([1e-4, 1e-3, 1e-2, 2e-5, 1e-5, 5e-6, 0.0, -1e-3, -0.5])
        Z = np.stack(np.meshgrid(zo, zi, np.array(PEAK_R), np.arange(40), indexing="ij"), -1).reshape(-1, 4)
        Z = np.concatenate([Z, Z[:1]])
        rows = _eval_rows(rng, _with_z(rng, Z[:, 0]), _with_z(rng, Z[:, 1]), Z[:, 2])
    elif name == "floor":
        n = 15001
        r = np.exp(rng.uniform(np.log(1e-3), np.log(0.03), n))
        r = np.minimum(r, 0.0299)
        pwo, pwi, pr = _peak_dirs(rng, np.minimum(np.exp(rng.uniform(np.log(1e-3), np.log(0.03), 2500)), 0.0299), 1)
        rows = _eval_rows(rng, np.concatenate([_dirs(rng, n), pwo]), np.concatenate([_dirs(rng, n), pwi]), np.concatenate([r, pr]))
    elif name == "sampling":
        one_m = 1 - 2.0 ** -24
        ul = np.array([0.0, 0.5 - 2.0 ** -25, 0.5, one_m])
        ux = np.array([0.0, 2.0 ** -24, 2.0 ** -12, 0.01, 0.25, 0.5, 0.9, one_m])
        uy = np.array([0.0, 0.25, 0.5, 0.75, one_m, -1.0])                       # -1: a random one per row
        rs = np.array(PEAK_R + (-1.0,))                                          # -1: a random one per row
        G = np.stack(np.meshgrid(ul, ux, uy, rs, np.arange(28), indexing="ij"), -1).reshape(-1, 5)
        G = G[(G[:, 1] < one_m) | (G[:, 4] < 2)]                                 # u_dir.x just under 1: both square roots of the warp cancel, wi.z is open — few such rows (FLIP_CAP)
        n = len(G)
        wo = _dirs(rng, n)
        wo[G[:, 4] == 0] = up                                                    # normal incidence
        G[:, 2] = np.where(G[:, 2] < 0, rng.uniform(0, one_m, n), G[:, 2])
        G[:, 3] = np.where(G[:, 3] < 0, _rough(rng, n), G[:, 3])
        rows = np.zeros((n + 1, 16), np.float32)
        rows[:n, 0:3], rows[:n, 3], rows[:n, 4:7] = wo, G[:, 3], _diffuse(rng, n)
        rows[:n, 7], rows[:n, 8], rows[:n, 9] = G[:, 0], G[:, 1], G[:, 2]
        rows[n] = rows[0]
        assert rows[:, 7:10].max() < 1.0
    elif name == "frame":
        ax = np.concatenate([np.eye(3), -np.eye(3)])
        a, b = rng.uniform(-1, 1, 500), rng.uniform(-1, 1, 500)
        ties = np.stack([a, b, a * rng.choice([-1.0, 1.0], 500)], 1)
        near = np.repeat(ax, 200, 0) + rng.normal(size=(1200, 3)) * (10.0 ** rng.uniform(-7, -2, (1200, 1)))
        nr = np.concatenate([ax, ties, near, rng.normal(size=(6000, 3))])
        nr = nr / np.linalg.norm(nr, axis=1, keepdims=True)
        d = rng.uniform(-2, 2, (len(nr), 3))
        d[::3] /= np.linalg.norm(d[::3], axis=1, keepdims=True)
        rows = np.zeros((len(nr), 16), np.float32)
        rows[:, 0:3], rows[:, 3:6] = nr, d
        t = slice(6, 506)
        rows[t, 2] = np.copysign(rows[t, 0], rows[t, 2])                         # the tie exact in float32 as well
        rows = rows[:-1] if len(rows) % 64 == 0 else rows
    else:
        raise KeyError(name)
    assert len(rows) % 64 != 0
    rows.setflags(write=False)
    return rows


def eval_inputs(rows):
    return rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7:10], rows[:, 10:13]


@functools.lru_cache(None)
def eval_ref(name):
    """the float64 reference of an eval family, computed once and shared"""
    return ggx_eval(*eval_inputs(family(name)))


def eval_out_of(g):
    return {n: getattr(g, n) for n in EVAL_OUT}


# ------------------------------------------------------------------------------------------ judging a sampler
def judge_sample(rows, wi, out, k=K, ks=K_S):
    """rows: the sampling family; wi (n, 3) float32 the directions under test; out: {pdf, thr, dfdr, dlnpdf_dr, flag?, t?, D?} evaluated at wi
    -> ({name: (ok, ratio)}, used): `used` marks the rows that needed one of the two allowances."""
    wo, r, d, ul, u2 = rows[:, 0:3], rows[:, 3], rows[:, 4:7], rows[:, 7], rows[:, 8:10]
    w64, whz, p = ggx_sample_np(wo, r, ul, u2)
    bound = wi_bound(p, ks)
    near_t1 = (np.abs(whz - CT1) <= k * U) & ~p.is_cos
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(wi, np.float64) - w64).max(1)
        primary = err <= bound
        w_alt, _, p_alt = ggx_sample_np(wo, r, ul, u2, axis_branch=whz < CT1) if near_t1.any() else (w64, None, p)
        alt = near_t1 & (np.abs(np.asarray(wi, np.float64) - w_alt).max(1) <= wi_bound(p_alt, ks))
    res = {"wi": (primary | alt, np.where(alt & ~primary, 0.0, err / bound))}
    used = alt & ~primary
    g = ggx_eval(wo, wi, r, d, np.zeros_like(wo))
    res.update(judge_eval(out, g, k, names=("pdf", "thr", "dfdr", "dlnpdf_dr", "t", "D")))
    if "flag" in out:
        flag64 = w64[:, 2] < C4
        open_ = np.abs(w64[:, 2] - C4) <= bound
        got = np.asarray(out["flag"]) != 0
        res["flag"] = ((got == flag64) | open_, np.zeros(len(r)))
        used = used | ((got != flag64) & open_)
    return res, used


def sample_open_share(k=K, ks=K_S):
    """share of the sampling family inside either allowance's zone, from the reference alone"""
    rows = family("sampling")
    w64, whz, p = ggx_sample_np(rows[:, 0:3], rows[:, 3], rows[:, 7], rows[:, 8:10])
    near_t1 = (np.abs(whz - CT1) <= k * U) & ~p.is_cos
    open_flag = np.abs(w64[:, 2] - C4) <= wi_bound(p, ks)
    return float((near_t1 | open_flag).mean()), float(near_t1.mean()), float(open_flag.mean())


# ------------------------------------------------------------------------------------------- sources under test on the CPU
def oracle_eval(rows, variant):
    import oracle
    inp = np.ascontiguousarray(rows[:, :13])
    out = np.zeros((len(rows), 10), np.float32)
    oracle.lib(variant).zdro_ggx_eval_batch(oracle._f(inp), len(rows), oracle._f(out))
    return {"f": out[:, 0:3], "pdf": out[:, 3], "grad": out[:, 4:8], "dfdr": out[:, 8], "dlnpdf_dr": out[:, 9]}


def oracle_sample(rows, variant):
    import oracle
    inp = np.ascontiguousarray(np.concatenate([rows[:, 0:4], rows[:, 7:10]], 1))
    wi = np.zeros((len(rows), 3), np.float32)
    oracle.lib(variant).zdro_ggx_sample_batch(oracle._f(inp), len(rows), oracle._f(wi))
    e = np.zeros((len(rows), 16), np.float32)
    e[:, 0:3], e[:, 3:6], e[:, 6], e[:, 7:10] = rows[:, 0:3], wi, rows[:, 3], rows[:, 4:7]
    o = oracle_eval(e, variant)
    with np.errstate(all="ignore"):
        thr = o["f"] / o["pdf"][:, None]
    return wi, {"pdf": o["pdf"], "thr": thr, "dfdr": o["dfdr"], "dlnpdf_dr": o["dlnpdf_dr"]}


def np32_eval(rows, mut=None):
    return eval_out_of(ggx_eval(*eval_inputs(rows), dt=np.float32, mut=mut))


def np32_sample(rows, mut=None):
    wi, _, _ = ggx_sample_np(rows[:, 0:3], rows[:, 3], rows[:, 7], rows[:, 8:10], dt=np.float32, mut=mut)
    wi = wi.astype(np.float32)
    g = ggx_eval(rows[:, 0:3], wi, rows[:, 3], rows[:, 4:7], np.zeros_like(wi), dt=np.float32)
    return wi, {"pdf": g.pdf, "thr": g.thr, "dfdr": g.dfdr, "dlnpdf_dr": g.dlnpdf_dr, "t": g.t, "D": g.D, "flag": (wi[:, 2] < F32(1e-4)).astype(np.float32)}


SOURCES = ("oracle ieee", "oracle fma", "numpy float32")


def source_eval(src, rows):
    return np32_eval(rows) if src == "numpy float32" else oracle_eval(rows, src.split()[1])


def source_sample(src, rows):
    return np32_sample(rows) if src == "numpy float32" else oracle_sample(rows, src.split()[1])


def frame_bound(rows, fk=FRAME_K):
    return fk * U * np.maximum(1.0, np.linalg.norm(rows[:, 3:6].astype(np.float64), axis=1))


def _smallest(passes, hi=64):
    """smallest integer k in [1, hi] with passes(k) (monotone), hi + 1 if none"""
    if not passes(hi):
        return hi + 1
    lo = 1
    while lo < hi:
        mid = (lo + hi) // 2
        if passes(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def measure_k():
    """-> ({(family, source): smallest k}, {source: smallest ks}, smallest frame k): the smallest integers at which the CPU sources pass"""
    ke = {}
    for fam in EVAL_FAMILIES:
        g = eval_ref(fam)
        for src in SOURCES:
            out = source_eval(src, family(fam))
            ke[fam, src] = _smallest(lambda k: all(ok.all() for ok, _ in judge_eval(out, g, k).values()))
    rows = family("sampling")
    ks = {}
    for src in SOURCES:
        wi, out = source_sample(src, rows)
        ks[src] = _smallest(lambda s: judge_sample(rows, wi, {}, K, s)[0]["wi"][0].all())
        ke["sampling", src] = _smallest(lambda k: all(ok.all() for n, (ok, _) in judge_sample(rows, wi, out, k, K_S)[0].items() if n != "wi"))
    fr = family("frame")
    e = np.abs(onb_np(fr[:, 0:3], fr[:, 3:6], np.float32).astype(np.float64) - onb_np(fr[:, 0:3], fr[:, 3:6])).max(1)
    kf = int(np.ceil((e / frame_bound(fr, 1)).max()))
    return ke, ks, max(kf, 1)


def unbounded_counts(name, k=K):
    """{roughness range: (rows, rows with t64 <= 2 eps — finiteness not required —, rows with t64 <= eps — bound infinite —, rows whose
    float32 transcription has t <= 0, i.e. D = inf)}"""
    g = eval_ref(name)
    t32 = ggx_eval(*eval_inputs(family(name)), dt=np.float32).t
    out = {}
    edges = [1e-3, 2e-3, 5e-3, 1e-2, 0.0131, 2e-2, 0.0299, 0.0301, 5e-2, 0.1, 1.0001]
    for lo, hi in zip(edges[:-1], edges[1:]):
        m = (g.r >= lo) & (g.r < hi)
        if m.any():
            out[f"[{lo:g}, {hi:g})"] = (int(m.sum()), int((g.t[m] <= 2 * k * U).sum()), int((g.t[m] <= k * U).sum()), int((t32[m] <= 0).sum()))
    return out


if __name__ == "__main__":      # the table of profiles/brdf_points_margins.txt
    import time
    t0 = time.time()
    ke, ks, kf = measure_k()
    print("smallest integer k at which every point of the family is inside its bound (float64 reference, eps = k 2^-24; no GPU involved)")
    for fam in EVAL_FAMILIES + ("sampling",):
        print(f"  {fam:11s} rows {len(family(fam)):6d}  " + "  ".join(f"{src}: {ke[fam, src]:3d}" for src in SOURCES))
    km = max(ke.values())
    print(f"K_MEASURED = {km}  x 4 = {4 * km}   (module: K_MEASURED = {K_MEASURED}, K = {K})")
    print("  sampled direction, smallest ks of wi_bound: " + "  ".join(f"{src}: {v}" for src, v in ks.items()))
    print(f"KS_MEASURED = {max(ks.values())}  x 4 = {4 * max(ks.values())}   (module: KS_MEASURED = {KS_MEASURED}, K_S = {K_S})")
    print(f"  frame rows {len(family('frame'))}, numpy float32 against float64: max error / (2^-24 max(1, |d|)) -> FRAME_MEASURED = {kf}  x 4 = {4 * kf}   (module: {FRAME_MEASURED}, {FRAME_K})")
    for fam in EVAL_FAMILIES:
        g = eval_ref(fam)
        B = eval_bounds(g)
        with np.errstate(all="ignore"):
            med = {n: float(np.nanmedian((np.asarray(getattr(B, n)).reshape(len(g.t), -1)[:, -1] / np.abs(np.asarray(getattr(g, n)).reshape(len(g.t), -1)[:, -1]))[np.isfinite(B.D)])) for n in ("f", "pdf", "dfdr", "dlnpdf_dr")}
        print(f"  {fam:11s} median bound / |reference| at K = {K}: " + "  ".join(f"{n} {v:.1e}" for n, v in med.items()))
    sh = sample_open_share()
    print(f"sampling rows inside an allowance's zone: {sh[0]:.5f} (wh.z within K 2^-24 of 0.99999: {sh[1]:.5f}; wi.z within wi_bound of 1e-4: {sh[2]:.5f}); cap {FLIP_CAP}")
    for fam in EVAL_FAMILIES:
        for dec, (n, nf, ni, nz) in unbounded_counts(fam).items():
            if nf or fam == "floor":
                print(f"  {fam:11s} r in {dec:16s} rows {n:6d}  t64 <= 2 K 2^-24 (may be non-finite): {nf:5d}  t64 <= K 2^-24 (bound infinite): {ni:5d}  float32 t <= 0 in NumPy: {nz:5d}")
    print(f"{time.time() - t0:.1f} s")
