"""CPU: the reference and the bound of tests/brdf_cases.py, checked without any kernel.  The float64 reference against itself (analytic
derivatives against central differences, the pdf against the numerical Jacobian of the warp); the oracle's float32 functions (IEEE and FMA
build) and the NumPy float32 transcription inside the bound at the measured K; deliberately wrong variants of the transcription rejected
by the same judgement in every family that exercises the term; the share of sampling rows that may use an allowance; and the committed
constants held to what the measurement yields."""
import functools

import numpy as np
import pytest

import brdf_cases as bc


@functools.lru_cache(None)
def measured():
    return bc.measure_k()


# ------------------------------------------------------------------------------------------- the families
def test_families_are_what_the_docstring_says():
    total = 0
    for name in bc.FAMILIES:
        rows = bc.family(name)
        assert rows.dtype == np.float32 and rows.shape[1] == 16 and len(rows) % 64 != 0 and np.isfinite(rows).all(), name
        assert 2000 <= len(rows) <= 70000, (name, len(rows))
        total += len(rows)
    assert 1.5e5 <= total <= 2.5e5, total
    for name in bc.EVAL_FAMILIES:                                                    # the reference is finite at every row: judge()'s NaN clause exempts none
        ref = bc.eval_ref(name)
        assert all(np.isfinite(getattr(ref, out)).all() for out in bc.EVAL_OUT + ("thr",)), name
    g = bc.family("generic")
    assert g[:, 2].min() >= 1e-4 and g[:, 5].min() >= 1e-4 and g[:, 6].min() >= 0.03 - 1e-9 and g[:, 6].max() <= 1.0
    assert (g[:, 7:10] == 0).all(1).any() and (g[:, 7:10] == 1).all(1).any()
    p = bc.family("peak")
    assert sorted(set(p[:, 6].tolist())) == sorted(float(np.float32(r)) for r in bc.PEAK_R)
    up = (p[:, 0:6] == [0, 0, 1, 0, 0, 1]).all(1)
    assert up.sum() >= len(bc.PEAK_R) and (p[up, 6] == 1.0).any()                     # wo = wi = normal, and a2 - 1 = 0 among them
    c = bc.family("collocated")
    assert np.array_equal(c[:, 0:3], c[:, 3:6]) and c[:, 2].min() >= 1e-4 and c[:, 2].min() < 2e-4
    z = bc.family("grazing")
    assert set(np.unique(z[:, 2]).tolist()) == {float(np.float32(v)) for v in (1e-4, 1e-3, 1e-2)}
    assert {float(np.float32(v)) for v in (2e-5, 1e-5, 5e-6, 0.0, -1e-3, -0.5)} <= set(np.unique(z[:, 5]).tolist())
    assert np.abs(z[:, 0:3] + z[:, 3:6]).max(1).min() > 1e-4                          # no row has wi = -wo (h = 0 / 0)
    fl = bc.family("floor")
    assert fl[:, 6].min() >= 1e-3 and fl[:, 6].max() < 0.03
    s = bc.family("sampling")
    assert {0.0, 0.5, float(np.float32(1 - 2.0 ** -24))} <= set(np.unique(s[:, 7]).tolist()) and (s[:, 7] < 0.5).any() and s[:, 7:10].max() < 1.0
    assert {0.0, float(np.float32(2.0 ** -24)), float(np.float32(1 - 2.0 ** -24))} <= set(np.unique(s[:, 8]).tolist())
    assert (s[:, 0:3] == [0, 0, 1]).all(1).sum() > 500
    f = bc.family("frame")
    assert all((f[:, 0:3] == a).all(1).any() for a in np.concatenate([np.eye(3), -np.eye(3)]))
    assert (np.abs(f[:, 0]) == np.abs(f[:, 2])).sum() >= 400
    assert np.abs(np.linalg.norm(f[:, 0:3].astype(np.float64), axis=1) - 1).max() < 2e-7


# ---------------------------------------------------------------- the reference against itself, float64 only
def _scale_dfdr(g):
    return np.abs(g.pref) * (np.abs(g.T1) + np.abs(g.T2))


def test_analytic_derivatives_match_central_differences_in_float64():
    """d f / d r and d ln pdf / d r of the reference against central differences of its own f and pdf, step h = 1e-5 r, on rows with
    t >= 1e-3.  Tolerance: 1e-6 of the magnitude of the terms that make up the derivative (|pref| (|T1| + |T2|); for ln pdf the two terms
    of dglossy over pdf) — the truncation h^2 f(3) / 6 with f(3) ~ (4 / r)^3 f is 1e-9 of it, a lost factor or a wrong sign is O(1) of
    it — plus the rounding of the difference quotient itself, |f| 2^-52 (2 / t + 8) / h (t = 1 - nh2 (1 - a2) cancels in float64 too):
    that part matters where the derivative vanishes, at tilt = alpha, where 1 - nh2 (1 + a2) = 0."""
    rows = np.concatenate([bc.family("generic")[:6000], bc.family("peak")[::3], bc.family("collocated")[:3000]])
    wo, wi, r, d, ct = (x.astype(np.float64) for x in bc.eval_inputs(rows))
    g = bc.ggx_eval(wo, wi, r, d, ct)
    h = 1e-5 * r
    gp, gm = bc.ggx_eval(wo, wi, r + h, d, ct), bc.ggx_eval(wo, wi, r - h, d, ct)
    keep = (g.t >= 1e-3) & (r + h <= 1.0)
    assert keep.sum() > 8000
    quot = 2.0 ** -52 * (2 / g.t + 8) / h
    fd = (gp.f - gm.f) / (2 * h)[:, None]
    e = np.abs(fd - g.dfdr[:, None]).max(1)
    tol = 1e-6 * _scale_dfdr(g) + np.abs(g.f).max(1) * quot
    print(f"[brdf host] d f/d r analytic against central differences: worst error / tolerance {(e / tol)[keep].max():.3f} over {keep.sum()} rows")
    assert (e <= tol)[keep].all()
    fdl = (np.log(gp.pdf) - np.log(gm.pdf)) / (2 * h)
    el = np.abs(fdl - g.dlnpdf_dr)
    tol_l = 1e-6 * 2 * g.r3 * (np.abs(g.U1) + np.abs(g.U2)) / (4 * np.abs(wo[:, 2])) / g.pdf + quot
    print(f"[brdf host] d ln pdf/d r analytic against central differences: worst error / tolerance {(el / tol_l)[keep].max():.3f}")
    assert (el <= tol_l)[keep].all()
    gd = bc.ggx_eval(wo, wi, r, d + 1.0, ct)                                           # f is linear in diffuse: one difference, exact to the rounding of f
    assert (np.abs((gd.f - g.f) - g.cz[:, None]) <= 2.0 ** -50 * (np.abs(g.f) + np.abs(gd.f) + 1)).all()
    np.testing.assert_allclose(g.grad[:, :3], ct * g.cz[:, None], rtol=0, atol=0)
    np.testing.assert_allclose(g.grad[:, 3], ct.sum(1) * g.dfdr, rtol=1e-15)


def _jacobian_pdf(wo, r, ul, u, h=1e-5):
    def w(du):
        return bc.ggx_sample_np(wo, r, ul, u + du)[0]
    d1 = (w(np.array([h, 0.0])) - w(np.array([-h, 0.0]))) / (2 * h)
    d2 = (w(np.array([0.0, h])) - w(np.array([0.0, -h]))) / (2 * h)
    return 1.0 / np.linalg.norm(np.cross(d1, d2), axis=1)


def test_pdf_is_the_density_of_the_warp_in_float64():
    """u_dir uniform on the unit square -> wi has density 1 / |d wi/d u.x x d wi/d u.y| on the sphere.  The glossy half of the pdf
    (G1(wo) D(h) / (4 |wo.z|), the visible-normal density through the reflection) and the cosine half (wi.z / pi) against that Jacobian by
    central differences, h = 1e-5, away from the clamps (u in [0.05, 0.95], wo.z >= 0.1, r >= 0.1).  Tolerance 1e-5 relative: truncation
    h^2 x (third derivatives over first, up to ~1e4 at r = 0.1) = 1e-6, rounding 1e-16 / h = 1e-11.  Rows with wh.z >= 0.99999 are left out
    of the glossy half: there the warp takes T1 = (1, 0, 0), which is not orthogonal to wh unless wh is the axis itself — the reference's
    own approximation (microfacet.py:76), off by up to 1 % of the density, and the kernels reproduce it."""
    rng = np.random.default_rng(11)
    n = 4000
    wo = bc._dirs(rng, n, 0.1)
    r = rng.uniform(0.1, 1.0, n)
    u = rng.uniform(0.05, 0.95, (n, 2))
    zero3 = np.zeros((n, 3))
    for ul, name in ((0.75, "glossy"), (0.25, "cosine")):
        wi = bc.ggx_sample_np(wo, r, np.full(n, ul), u)[0]
        np.testing.assert_allclose(np.linalg.norm(wi, axis=1), 1.0, atol=1e-12)
        jac = _jacobian_pdf(wo, r, np.full(n, ul), u)
        g = bc.ggx_eval(wo, wi, r, zero3, zero3)
        half = g.glossy if name == "glossy" else wi[:, 2] / np.pi
        whz = bc.ggx_sample_np(wo, r, np.full(n, ul), u)[1]
        keep = (wi[:, 2] > 1e-3) & (whz < bc.CT1) if name == "glossy" else np.ones(n, bool)
        e = np.abs(jac / half - 1)[keep]
        print(f"[brdf host] {name} half of the pdf against the warp's Jacobian: worst relative difference {e.max():.2e} over {keep.sum()} rows")
        assert e.max() < 1e-5, name
        np.testing.assert_allclose(g.pdf, 0.5 * wi[:, 2] / np.pi + 0.5 * g.glossy, rtol=1e-14)


# ------------------------------------------------------------------- float32 sources under the bound
def test_committed_constants_are_what_the_measurement_yields():
    ke, ks, kf = measured()
    print("[brdf host] smallest k per (family, source):", {f"{a} / {b}": v for (a, b), v in ke.items()})
    assert max(ke.values()) == bc.K_MEASURED and bc.K == 4 * bc.K_MEASURED
    assert max(ks.values()) == bc.KS_MEASURED and bc.K_S == 4 * bc.KS_MEASURED
    assert kf == bc.FRAME_MEASURED and bc.FRAME_K == 4 * bc.FRAME_MEASURED


@pytest.mark.parametrize("family", bc.EVAL_FAMILIES)
def test_oracle_and_transcription_are_inside_the_bound_at_the_measured_k(family):
    g = bc.eval_ref(family)
    for src in bc.SOURCES:
        res = bc.judge_eval(bc.source_eval(src, bc.family(family)), g, bc.K_MEASURED)
        for name, (ok, ratio) in res.items():
            print(f"[brdf host] {family:10s} {src:13s} {name:9s} worst error / bound(k = {bc.K_MEASURED}) {ratio.max():.3f}")
            assert ok.all(), (family, src, name, int((~ok).sum()), np.flatnonzero(~ok)[:4])


def test_oracle_and_transcription_sample_inside_the_bound_at_the_measured_k():
    rows = bc.family("sampling")
    for src in bc.SOURCES:
        wi, out = bc.source_sample(src, rows)
        res, used = bc.judge_sample(rows, wi, out, bc.K_MEASURED, bc.KS_MEASURED)
        for name, (ok, ratio) in res.items():
            print(f"[brdf host] sampling   {src:13s} {name:9s} worst error / bound {ratio.max():.3f}")
            assert ok.all(), (src, name, int((~ok).sum()), np.flatnonzero(~ok)[:4])
        assert used.mean() <= bc.FLIP_CAP, (src, used.mean())


def test_frame_transcription_is_inside_its_bound_and_orthonormal():
    fr = bc.family("frame")
    ref = bc.onb_np(fr[:, 0:3], fr[:, 3:6])
    got = bc.onb_np(fr[:, 0:3], fr[:, 3:6], np.float32)
    assert (np.abs(got - ref).max(1) <= bc.frame_bound(fr, bc.FRAME_MEASURED)).all()
    t, b, n = ref[:, 0:3], ref[:, 3:6], ref[:, 6:9]
    for a, c, want in ((t, t, 1), (b, b, 1), (t, b, 0), (t, n, 0), (b, n, 0)):
        assert np.abs((a * c).sum(1) - want).max() < 1e-12                           # the float64 frame is orthonormal whatever the normal
    np.testing.assert_allclose(np.cross(t, b), n, atol=3e-7)                           # right-handed; n is unit to float32 only
    np.testing.assert_allclose(ref[:, 12:15], fr[:, 3:6], atol=1e-6)                   # the round trip returns d (to |n|^2 - 1)


# ---------------------------------------------------------------------------- the bound is not vacuous
@pytest.mark.parametrize("mutation", sorted(bc.MUTATIONS))
def test_the_judgement_rejects_a_wrong_formula(mutation):
    """One term wrong in the float32 transcription: rejected at the committed K (the bound the kernels are held to) in every family that
    exercises the term — while the unmutated transcription passes there (the tests above)."""
    for family in bc.MUTATIONS[mutation]:
        rows = bc.family(family)
        if family == "sampling":
            wi, out = bc.np32_sample(rows, mutation)
            res, _ = bc.judge_sample(rows, wi, out, bc.K, bc.K_S)
        else:
            res = bc.judge_eval(bc.np32_eval(rows, mutation), bc.eval_ref(family), bc.K)
        bad = {name: int((~ok).sum()) for name, (ok, _) in res.items() if not ok.all()}
        print(f"[brdf host] {mutation:22s} {family:10s} rows rejected per output: {bad}")
        assert bad, (mutation, family)


def test_the_allowances_stay_under_their_cap_by_the_reference_alone():
    share, t1, flag = bc.sample_open_share()
    print(f"[brdf host] sampling rows inside an allowance's zone: {share:.5f} (T1 branch {t1:.5f}, stop flag {flag:.5f})")
    assert share <= bc.FLIP_CAP


def test_where_the_bound_is_infinite():
    """Only where float32 t can vanish: t64 <= eps needs r^4 <= eps, i.e. r <= (K 2^-24)^(1/4) = 0.0346; every other family row has a
    finite bound for t, D, f and pdf."""
    e = bc.K * bc.U
    for family in bc.EVAL_FAMILIES:
        g = bc.eval_ref(family)
        B = bc.eval_bounds(g)
        inf = ~np.isfinite(B.D) | ~np.isfinite(B.f).all(1)
        assert (g.t[inf] <= e).all() and (g.r[inf] ** 4 <= e).all(), family
        assert (B.finite_required == (g.t > 2 * e)).all()
        if family == "generic":
            assert inf.mean() < 0.001
        print(f"[brdf host] {family:10s} rows with an infinite bound {int(inf.sum())} of {len(inf)}; finiteness not required on {int((~B.finite_required).sum())}")
