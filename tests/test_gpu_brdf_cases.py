"""-m gpu: the shading math point by point.  Every row of every family of tests/brdf_cases.py through zdr_shading_dump — lane i calls
ggx_terms, ggx_brdf_from, ggx_pdf_from, ggx_dfdr_from, ggx_sample / sample_wm_disk, brdf_grad, make_onb, to_local and to_world as the path
kernels do — and every output of every row judged by the float64 reference under the bound of its own conditioning (eps = K 2^-24, K from
CPU measurements only).  No row is exempt; a row's bound is infinite only where float32 t may vanish (t64 <= eps, roughness below 0.035)."""
import functools

import numpy as np
import pytest
import torch

import brdf_cases as bc
from gpu_util import make_scene
from zdr_amd import _native

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def scene():
    return make_scene("path")                # the hook reads no geometry: the scene names the device


def dump(mode, rows):
    out = scene().shading_dump(mode, torch.from_numpy(np.array(rows, np.float32)))
    scene().check()
    return out.cpu().numpy()


def eval_out(o):
    return {"f": o[:, 0:3], "pdf": o[:, 3], "dfdr": o[:, 4], "dlnpdf_dr": o[:, 5], "t": o[:, 6], "D": o[:, 7], "grad": o[:, 8:12]}


def all_inside(res, what):
    for name, (ok, ratio) in res.items():
        print(f"[brdf] {what:10s} {name:9s} worst error / bound {ratio.max():.3f}   rows outside {int((~ok).sum())} of {len(ok)}")
    for name, (ok, ratio) in res.items():
        bad = np.flatnonzero(~ok)
        assert not len(bad), (what, name, f"{len(bad)} rows outside their bound", bad[:6].tolist())


# ----------------------------------------------------------------------------- a. every family, every row
@pytest.mark.parametrize("family", bc.EVAL_FAMILIES)
def test_every_point_of_the_eval_family_is_inside_its_bound(family):
    rows = bc.family(family)
    o = dump("eval", rows)
    g = bc.eval_ref(family)
    assert not o[:, 12:].any()
    all_inside(bc.judge_eval(eval_out(o), g), family)
    B = bc.eval_bounds(g)
    nonfinite = ~np.isfinite(o[:, :12]).all(1)
    assert not (nonfinite & B.finite_required).any()
    for dec, (n, nf, ni, nz) in bc.unbounded_counts(family).items():
        m = (g.r >= float(dec[1:].split(",")[0])) & (g.r < float(dec.split(",")[1][:-1]))
        if nf or family == "floor":
            print(f"[brdf] {family:10s} r in {dec:16s} rows {n:6d}  finiteness not required (t64 <= 2 K 2^-24) {nf:5d}  bound infinite {ni:5d}  "
                  f"non-finite answers {int((nonfinite & m).sum()):5d}  t <= 0 on the GPU {int(((o[:, 6] <= 0) & m).sum()):5d}")


def test_brdf_grad_is_the_cotangent_times_the_reference_derivatives():
    """brdf_grad(wi.z / pi, dfdr, ct) against ct . d f / d (diffuse, roughness) of the reference: d f_c / d diffuse_c = wi.z / pi,
    d f_c / d r = dfdr for every channel."""
    rows = bc.family("generic")
    o = dump("eval", rows)
    g = bc.eval_ref("generic")
    ct = rows[:, 10:13].astype(np.float64)
    want = np.concatenate([ct * (g.wi[:, 2] / np.pi)[:, None], (ct.sum(1) * g.dfdr)[:, None]], 1)
    np.testing.assert_allclose(want, g.grad, rtol=1e-15, atol=0)
    B = bc.eval_bounds(g)
    ok, ratio = bc.judge(o[:, 8:12], want, B.grad, B.finite_required)
    print(f"[brdf] brdf_grad against ct . df/d(diffuse, r): worst error / bound {ratio.max():.3f}")
    assert ok.all()
    assert (np.abs(o[:, 8:11] - want[:, :3]) <= 2 * bc.K * bc.U * np.abs(want[:, :3])).all()          # the diffuse part: two roundings


def test_every_point_of_the_sampling_family_is_inside_its_bound():
    rows = bc.family("sampling")
    o = dump("sample", rows)
    assert not o[:, 12:].any()
    out = {"pdf": o[:, 3], "thr": o[:, 4:7], "dfdr": o[:, 7], "dlnpdf_dr": o[:, 8], "flag": o[:, 9], "t": o[:, 10], "D": o[:, 11]}
    assert np.isin(o[:, 9], (0.0, 1.0)).all() and np.array_equal(o[:, 9] != 0, o[:, 2] < np.float32(1e-4))   # the flag is the kernel's own wi_local.z < 1e-4
    at = bc.ggx_eval(rows[:, 0:3], o[:, 0:3], rows[:, 3], rows[:, 4:7], np.zeros((len(rows), 3)))
    open_ref = np.isnan(np.concatenate([np.asarray(getattr(at, name)).reshape(len(rows), -1) for name in ("pdf", "thr", "dfdr", "dlnpdf_dr", "t", "D")], 1)).any(1)
    print(f"[brdf] sampling: rows whose float64 pdf at the sampled direction is 0 / 0 (wo.h = 0: normal incidence reflected about a grazing normal, wi = -wo) {int(open_ref.sum())}")
    assert (o[open_ref, 9] == 1).all() and open_ref.mean() < 1e-3                    # judge() leaves only these open, and the path stops at every one (wi_local.z < 1e-4)
    res, used = bc.judge_sample(rows, o[:, 0:3], out)
    all_inside(res, "sampling")
    print(f"[brdf] sampling: rows that needed an allowance (T1 branch or stop flag) {int(used.sum())} of {len(used)} = {used.mean():.5f}; cap {bc.FLIP_CAP}")
    assert used.mean() <= bc.FLIP_CAP
    cos = rows[:, 7] < 0.5
    assert np.array_equal(o[cos & (rows[:, 8] == 0), 0:3], np.repeat([[0, 0, 1]], (cos & (rows[:, 8] == 0)).sum(), 0).astype(np.float32))


def test_every_frame_is_orthonormal_and_matches_float64():
    fr = bc.family("frame")
    o = dump("frame", fr).astype(np.float64)
    ref = bc.onb_np(fr[:, 0:3], fr[:, 3:6])
    bound = bc.frame_bound(fr)
    assert not o[:, 15].any() and np.array_equal(o[:, 6:9], fr[:, 0:3].astype(np.float64))      # the normal is handed through
    err = np.abs(o[:, :15] - ref)
    names = ("tangent", "binormal", "normal", "to_local", "round trip")
    for k, name in enumerate(names):
        print(f"[brdf] frame {name:10s} worst error / bound {(err[:, 3 * k:3 * k + 3].max(1) / bound).max():.3f}")
    assert (err.max(1) <= bound).all()
    t, b, n = o[:, 0:3], o[:, 3:6], o[:, 6:9]
    e = bc.FRAME_K * bc.U
    for a, c, want, what in ((t, t, 1, "|t|"), (b, b, 1, "|b|"), (t, b, 0, "t.b"), (t, n, 0, "t.n"), (b, n, 0, "b.n")):
        d = np.abs((a * c).sum(1) - want)
        print(f"[brdf] frame {what}: worst deviation / (4 FRAME_K 2^-24) {(d / (4 * e)).max():.3f}")
        assert (d <= 4 * e).all(), what                                                # each vector within e per component of an orthonormal triple: |da| + |dc| <= 2 sqrt(3) e


# ------------------------------------------------------------------------------------- b. the hook itself
@pytest.mark.parametrize("n", [1, 63, 65])
def test_rows_beyond_n_are_untouched(n):
    L = _native.lib()
    s = scene()
    for mode, fam in ((0, "peak"), (1, "sampling"), (2, "frame")):
        rows = torch.from_numpy(np.array(bc.family(fam)[:128])).to(s.device)
        out = torch.full((128, 16), -777.0, device=s.device)
        assert L.zdr_shading_dump(s._handle, mode, rows.data_ptr(), n, out.data_ptr(), None) == 0
        s.check()
        o = out.cpu().numpy()
        assert (o[n:] == -777.0).all(), (mode, n)
        assert (o[:n] != -777.0).all(), (mode, n)
        full = dump(("eval", "sample", "frame")[mode], bc.family(fam)[:128])
        assert np.array_equal(o[:n].view(np.uint32), full[:n].view(np.uint32))       # a row's answer does not depend on n


def test_two_calls_agree_bit_for_bit():
    for mode, fam in (("eval", "floor"), ("eval", "grazing"), ("sample", "sampling"), ("frame", "frame")):
        a, b = dump(mode, bc.family(fam)), dump(mode, bc.family(fam))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (mode, fam)


def test_shading_dump_arguments():
    L = _native.lib()
    s = scene()
    rows = torch.zeros((64, 16), device=s.device); rows[:, 2] = 1; rows[:, 5] = 1; rows[:, 6] = 0.5
    out = torch.zeros((64, 16), device=s.device)
    good = [s._handle, 0, rows.data_ptr(), 64, out.data_ptr(), None]
    for mode in (0, 1, 2):
        args = list(good); args[1] = mode
        assert L.zdr_shading_dump(*args) == 0
    torch.cuda.synchronize()
    for k in (0, 2, 4):
        args = list(good); args[k] = None
        assert L.zdr_shading_dump(*args) == -1 and b"null" in L.zdr_last_error(), k                 # ZDR_E_INVALID
    for mode in (-1, 3, 99):
        args = list(good); args[1] = mode
        assert L.zdr_shading_dump(*args) == -1 and b"mode" in L.zdr_last_error(), mode
    args = list(good); args[3] = 0; args[2] = None; args[4] = None
    assert L.zdr_shading_dump(*args) == 0                                                            # n = 0: nothing to read or write
    args[1] = 7
    assert L.zdr_shading_dump(*args) == -1                                                           # ... but the mode is still checked
    assert s.shading_dump("eval", torch.empty((0, 16))).shape == (0, 16)
    with pytest.raises(KeyError):
        s.shading_dump("nonsense", rows)
    s.check()
