"""-m gpu: the gather plan (zdr_amd/plan.py; include/zdr.h, zdr_gather_plan_*) against the NumPy reference of tests/gather_plan_ref.py,
for the three filters: the CSR structure and the weights bit for bit, the apply bit for bit against the float32 reference in the
header's summation order, the atomic adjoints' own products bit for bit on the rows of one or two entries, run-to-run equality,
accuracy against float64 within the existing bars, the transpose, the buffer rules
(added into, untouched, written), autograd through ``plan=``, and the argument checks.

Views: the kernels' own view and footprint buffers of cbox_16x16 and cbox_64x64 through the standard camera, for images of 96 x 64
(short rows), 4 x 3 (rows of several hundred entries) and 1 x 1 (ONE row that holds every entry); and views made by hand.

One operation of the enumeration is not IEEE: f = log2f(mantissa).  The reference takes the GPU's (``device_log2``: zdr_texel_gather_mip
of a 2 x 2 image of zeros over a pyramid of ones, through a view whose scale is the mantissa, returns f itself), so the weights are held
to the bits of the scatter kernels' own f.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import gather_plan_ref as GR
import test_gpu_texel_project as TP
import texel_aniso_cases as AC
import texel_aniso_ref as AR
import texel_mip_ref as MR
import texel_project_cases as PC
import texel_project_ref as PR
from zdr_amd import (GatherPlan, TexelView, gather_plan, image_pyramid_backward, texel_footprint_forward, texel_gather, texel_gather_aniso_backward,
                     texel_gather_backward, texel_gather_mip_backward, texel_gather_mip_forward)
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID = -1
FILTERS = {"bilinear": {}, "mip": {"footprint": 2.0}, "aniso": {"footprint": 1.5, "max_aniso": 8}}
SCENE_VIEWS = [("cbox_16x16_standard", (96, 64)), ("cbox_64x64_standard", (96, 64)), ("cbox_64x64_standard", (4, 3)), ("cbox_64x64_standard", (1, 1))]


def device_log2(m):
    m = np.asarray(m, F)
    view = np.zeros((1, m.size, 8), F)
    view[0, :, 0] = 1.0; view[0, :, 2:4] = 0.5; view[0, :, 6] = m
    image, pyramid = torch.zeros(2, 2, 4, device="cuda"), torch.ones(1, 4, device="cuda")
    return texel_gather_mip_forward(image, pyramid, torch.from_numpy(view).cuda(), 1.0)[0, :, 0].cpu().numpy()


_views = {}


def scene_view(name, res):
    if (name, res) not in _views:
        cam, pts = TP.camera(PC.CASES[name][1]), TP.case_points(name)
        data = TP.case_scene(name, "bvh").texel_view_forward(pts, res, camera=cam)
        _views[(name, res)] = TexelView(data, res, texel_footprint_forward(pts, res, cam))
    return _views[(name, res)]


def hand_view(kind, res):
    """(view (H, W, 8), footprint (H, W, 4)) float32, made by hand for an image of ``res``"""
    w, h = res
    rng = np.random.default_rng(11)
    view, fp = np.zeros((5, 13, 8), F), np.zeros((5, 13, 4), F)
    v, f = view.reshape(-1, 8), fp.reshape(-1, 4)
    if kind == "empty":
        v[:, 2:4] = np.nan; v[:, 6] = 7.0; f[:] = 3.0                 # (nothing of an invisible texel is read)
    elif kind == "single":
        v[17] = (1.0, 0.3, 2.25, 1.75, 1.0, 1.0, 2.9, 0.0); f[17] = (2.0, 1.0, 1.2, 2.3)
    elif kind in ("nan_visible", "half", "random"):
        v[:, 0] = {"nan_visible": 1.0, "half": 0.5, "random": 1.0}[kind]
        v[:, 2], v[:, 3] = rng.uniform(-2, w + 2, 65), rng.uniform(-2, h + 2, 65)
        v[:, 6] = np.exp2(rng.uniform(-1, 6, 65))
        ang, major = rng.uniform(0, 2 * np.pi, 65), np.exp2(rng.uniform(-1, 5, 65))
        f[:, 0], f[:, 1], f[:, 3], f[:, 2] = major * np.cos(ang), major * np.sin(ang), major, major * rng.uniform(0.05, 1, 65)
        if kind == "nan_visible":
            v[::3, 0] = np.nan
        if kind == "random":
            v[:, 0] = rng.choice(np.array([0.0, 1.0, 0.5, -2.0, np.nan], F), 65)
            v[5, 6] = np.inf; v[6, 6] = np.nan; v[7, 6] = 2.0; v[8, 6] = 4.0; f[9, 2:] = np.nan; f[10, 3] = np.inf
    elif kind == "outside":
        v[:, 0] = 1.0; v[:, 6] = 2.5; f[:] = (1.5, 0.5, 1.0, 1.6)
        far = [(-1e9, 3.0), (1e9, 3.0), (2.0, -1e9), (2.0, 1e9), (-1e30, 1e30), (np.inf, 1.0), (1.0, -np.inf), (np.nan, 1.0), (1.0, np.nan), (-0.75, -0.25),
               (w + 0.75, h + 0.25), (-1.0, h + 1.0), (3e9, -3e9)]
        for k in range(65):
            v[k, 2:4] = far[k % len(far)]
    else:                                                            # "rows_<n>": n texels on the centre of one pixel of an otherwise empty view
        n = int(kind.split("_")[1])
        v[:n, 0] = 1.0; v[:n, 2], v[:n, 3] = (w // 2) + 0.5, (h // 2) + 0.5; v[:n, 6] = 1.0
    return view, fp


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def same_bits(got, want):
    """equal bit for bit, NaNs compared as NaNs (their payload is unspecified)"""
    got, want = np.asarray(got, F), np.asarray(want, F)
    nan = np.isnan(want)
    return got.shape == want.shape and bool((np.isnan(got) == nan).all()) and bool((bits(got)[~nan] == bits(want)[~nan]).all())


def to_view(view, fp, res):
    return TexelView(torch.from_numpy(view).cuda(), res, torch.from_numpy(fp).cuda())


def adjoint_bar(filter, g, view, fp, res):
    """(bar, float64 result) of the full adjoint of ``filter`` by the existing rule: 4 x the float32 reference's own error against the
    float64 one, floor 4 float32 ulps of the largest value (texel_project_cases.linear_bar, texel_mip_ref.linear_bar)"""
    kw = FILTERS[filter]
    if filter == "bilinear":
        return PC.linear_bar(view, g, res, True)
    if filter == "mip":
        r64 = MR.gather_mip_adjoint_ref(g, view, res, kw["footprint"])
        return MR.linear_bar(MR.gather_mip_adjoint_ref(g, view, res, kw["footprint"], 0, F), r64), r64
    r64 = AR.gather_aniso_adjoint_ref(g, view, fp, res, kw["footprint"], kw["max_aniso"])
    return AC.gather_bar(AR.gather_aniso_adjoint_ref(g, view, fp, res, kw["footprint"], kw["max_aniso"], 0, F), r64), r64


def check_structure_and_apply(tv, res, filter, label, kw=None):
    kw = FILTERS[filter] if kw is None else kw
    view, fp = tv.data.cpu().numpy(), tv.footprint_data.cpu().numpy()
    ref = GR.plan_ref(view, fp, res, filter, log2=device_log2, **kw)
    plan, again = gather_plan(tv, res, filter, **kw), tv.gather_plan(res, filter, **kw)
    torch.cuda.synchronize()
    counts = GR.counts(ref)
    print(f"[gather plan] {label} {filter}: nnz {plan.nnz} (reference {ref['nnz']}), rows {plan.rows}, longest row {int(counts.max())}, "
          f"rows of 64 entries or more {int((counts >= 64).sum())}, plan {plan.nbytes} bytes")
    # structure
    assert isinstance(plan, GatherPlan) and plan.nnz == ref["nnz"] and plan.rows == ref["rows"] and plan.res == tuple(res) and plan.filter == filter
    assert plan.row_start.dtype == torch.int32 and tuple(plan.entries.shape) == (plan.nnz, 2)
    assert (plan.row_start.cpu().numpy().astype(np.int64) == ref["row_start"]).all()
    assert (plan.texels.cpu().numpy().astype(np.int64) == ref["texel"]).all()
    assert same_bits(plan.weights.cpu().numpy(), ref["weight"])
    assert torch.equal(plan.row_start, again.row_start) and torch.equal(plan.entries, again.entries)
    # apply: exact, added into / untouched / written, twice the same bits; then with an infinity and a NaN in known texels
    rng = np.random.default_rng(1)
    h, w, p0 = res[1], res[0], ref["p0"]
    g = rng.standard_normal(view.shape[:2] + (4,)).astype(F)
    g_bad = g.copy()
    g_bad.reshape(-1, 4)[3, 1] = np.inf; g_bad.reshape(-1, 4)[20] = np.nan
    pattern = rng.standard_normal((p0, 4)).astype(F)
    empty = np.nonzero(counts[:p0] == 0)[0]
    pattern[empty[0::2]] = np.nan; pattern[empty[1::2]] = F(-0.0)
    for what, gg in (("normal", g), ("inf and NaN", g_bad)):
        rows = GR.apply_ref(ref, gg)
        with np.errstate(invalid="ignore", over="ignore"):
            want_image = np.where((counts[:p0] > 0)[:, None], (pattern + rows[:p0]).astype(F), pattern)
        outs = []
        for _ in range(2):
            d_image = torch.from_numpy(pattern.reshape(h, w, 4).copy()).cuda()
            d_pyr = None if filter == "bilinear" else torch.full((plan.rows - p0, 4), float("nan"), device="cuda")
            plan.apply(torch.from_numpy(gg).cuda(), d_image, d_pyr)
            outs.append((d_image.cpu().numpy().reshape(-1, 4), None if d_pyr is None else d_pyr.cpu().numpy()))
        assert same_bits(outs[0][0], want_image), (label, filter, what)
        if what == "normal":
            assert (bits(outs[0][0])[empty] == bits(pattern)[empty]).all()          # an empty row keeps its NaN (payload and all) and its -0
        assert same_bits(outs[1][0], outs[0][0]) and (what != "normal" or (bits(outs[1][0]) == bits(outs[0][0])).all())
        if filter != "bilinear":
            assert same_bits(outs[0][1], rows[p0:]), (label, filter, what)
            assert same_bits(outs[1][1], outs[0][1])
            if what == "normal":
                # fully written: no prefilled NaN is left but where the sum itself is one (a weight of an X at infinity); +0 on empty rows
                assert (np.isnan(outs[0][1]) == np.isnan(rows[p0:])).all() and (bits(outs[0][1])[counts[p0:] == 0] == 0).all()
    return plan, ref, g


@pytest.mark.parametrize("filter", list(FILTERS))
@pytest.mark.parametrize("name,res", SCENE_VIEWS)
def test_structure_apply_accuracy_and_transpose_on_the_kernels_own_views(name, res, filter):
    tv, kw = scene_view(name, res), FILTERS[filter]
    plan, ref, g = check_structure_and_apply(tv, res, filter, f"{name} {res[0]}x{res[1]}")
    if res == (1, 1):
        assert GR.counts(ref)[0] == plan.nnz >= 2000                 # the one pixel holds every tap of every visible texel: thousands of entries
    view, fp = tv.data.cpu().numpy(), tv.footprint_data.cpu().numpy()
    if filter == "aniso":                                            # texels within NEAR of a switch of N send nothing back (tests/test_gpu_texel_aniso.py)
        g = np.where(AR.exempt(fp, kw["footprint"], kw["max_aniso"])[..., None], F(0.0), g).astype(F)
    gt = torch.from_numpy(g).cuda()
    got = plan.adjoint(gt).cpu().numpy().astype(np.float64)
    bar, r64 = adjoint_bar(filter, g, view, fp, res)
    if filter == "bilinear":
        atomic = texel_gather_backward(gt, tv.data, res)
        bar_fwd = lambda x: PC.linear_bar(view, x, res, False)[0]
    elif filter == "mip":
        d_image, d_pyr = texel_gather_mip_backward(gt, tv.data, res, kw["footprint"])
        atomic = image_pyramid_backward(d_pyr, res, d_image=d_image)
        bar_fwd = lambda x: MR.linear_bar(MR.gather_mip_ref(x, view, kw["footprint"], 0, F), MR.gather_mip_ref(x, view, kw["footprint"]))
    else:
        d_image, d_pyr = texel_gather_aniso_backward(gt, tv.data, tv.footprint_data, res, kw["footprint"], kw["max_aniso"])
        atomic = image_pyramid_backward(d_pyr, res, d_image=d_image)
        bar_fwd = lambda x: AC.gather_bar(AR.gather_aniso_ref(x, view, fp, kw["footprint"], kw["max_aniso"], 0, F),
                                          AR.gather_aniso_ref(x, view, fp, kw["footprint"], kw["max_aniso"]))
    err, err_atomic = float(np.abs(got - r64).max()), float(np.abs(atomic.cpu().numpy().astype(np.float64) - r64).max())
    print(f"[gather plan] {name} {res[0]}x{res[1]} {filter}: full adjoint vs float64, plan {err:.3e}, atomic adjoint {err_atomic:.3e}; bar {bar:.3e} "
          f"(largest |value| {float(np.abs(r64).max()):.3e})")
    assert err <= bar and np.abs(r64).max() > 0
    # <K x, y> = <x, K^T y>: each side is off its exact value by at most its own bar per element
    x = np.random.default_rng(2).random((res[1], res[0], 4)).astype(F)
    color = texel_gather(torch.from_numpy(x).cuda(), tv, filter=filter, **kw).cpu().numpy().astype(np.float64)
    lhs, rhs = float((color * g).sum()), float((x.astype(np.float64) * got).sum())
    bound = bar * float(np.abs(x).sum()) + bar_fwd(x) * float(np.abs(g).sum())
    print(f"[gather plan] {name} {res[0]}x{res[1]} {filter}: <Kx, y> {lhs:.9e}, <x, K^T y> {rhs:.9e}, difference {abs(lhs - rhs):.3e}; bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("filter", list(FILTERS))
@pytest.mark.parametrize("kind", ["empty", "single", "nan_visible", "outside", "half", "random", "rows_1", "rows_15", "rows_16", "rows_17", "rows_64", "rows_65"])
def test_structure_and_apply_on_views_made_by_hand(kind, filter):
    res = (7, 5)
    view, fp = hand_view(kind, res)
    plan, ref, _ = check_structure_and_apply(to_view(view, fp, res), res, filter, kind)
    counts = GR.counts(ref)
    if kind == "empty":
        assert plan.nnz == 0 and not plan.row_start.any()
    if kind == "single":
        assert plan.nnz in (4, 8) or filter == "aniso"
    if kind.startswith("rows_"):
        n = int(kind.split("_")[1])
        assert plan.nnz == 4 * n and int((counts == n).sum()) == 4 and int((counts == 0).sum()) == plan.rows - 4


@pytest.mark.parametrize("filter", list(FILTERS))
@pytest.mark.parametrize("kind", ["single", "half", "random"])
def test_the_atomic_adjoints_add_the_plans_own_products(kind, filter):
    """The tie between the two families: on a row of one or two entries the atomic adjoint, run onto zeros, leaves fl(w0 g0) or
    fl(fl(w0 g0) + fl(w1 g1)) with the plan's weights — two addends onto a zero commute, so the order of the atomics cannot show — and
    that is compared bit for bit, all four channels.  Rows of three or more entries are left out; an empty row holds +0.  Every
    (kind, filter) pair must compare at least 60 % of its non-empty rows and at least two of them: asserted before the comparison."""
    res, kw = (96, 64), FILTERS[filter]
    view, fp = hand_view(kind, res)
    ref = GR.plan_ref(view, fp, res, filter, log2=device_log2, **kw)
    p0, rows, counts = ref["p0"], ref["rows"], GR.counts(ref)
    g = np.random.default_rng(5).standard_normal(view.shape[:2] + (4,)).astype(F)
    gt, vt, ft = torch.from_numpy(g).cuda(), torch.from_numpy(view).cuda(), torch.from_numpy(fp).cuda()
    d_image = torch.zeros(res[1], res[0], 4, device="cuda")
    d_pyr = torch.zeros(max(rows - p0, 1), 4, device="cuda")
    if filter == "bilinear":
        texel_gather_backward(gt, vt, res, d_image=d_image)
    elif filter == "mip":
        texel_gather_mip_backward(gt, vt, res, kw["footprint"], d_image=d_image, d_pyramid=d_pyr)
    else:
        texel_gather_aniso_backward(gt, vt, ft, res, kw["footprint"], kw["max_aniso"], d_image=d_image, d_pyramid=d_pyr)
    got = np.concatenate([d_image.cpu().numpy().reshape(-1, 4), d_pyr.cpu().numpy()])[:rows]
    nonempty, short = int((counts > 0).sum()), np.nonzero((counts == 1) | (counts == 2))[0]
    print(f"[gather plan] atomic adjoint against the plan's products, {kind} {filter}: {short.size} rows compared of {nonempty} non-empty ones")
    assert short.size >= 2 and short.size >= 0.6 * nonempty
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (ref["weight"][:, None] * g.reshape(-1, 4)[ref["texel"]]).astype(F)
        first, second = ref["row_start"][short], ref["row_start"][short] + 1
        want = (np.zeros((short.size, 4), F) + prod[first]).astype(F)
        two = counts[short] == 2
        want[two] = (want[two] + prod[second[two]]).astype(F)
    assert same_bits(got[short], want), (kind, filter)
    assert (bits(got[counts == 0]) == 0).all()


@pytest.mark.parametrize("filter", list(FILTERS))
def test_autograd_goes_through_the_plan_and_keeps_the_forward(filter):
    name, res = "cbox_16x16_standard", (96, 64)
    kw = FILTERS[filter]
    tv = TexelView(scene_view(name, res).data, res, scene_view(name, res).footprint_data)      # (a view of its own: nothing cached yet)
    gen = torch.Generator().manual_seed(4)
    photo = torch.rand(res[1], res[0], 4, generator=gen).cuda().requires_grad_()
    g = torch.randn(tv.data.shape[0], tv.data.shape[1], 4, generator=gen).cuda()
    plain = texel_gather(photo, tv, filter=filter, **kw)
    assert "_gather_plans" not in tv.__dict__
    color = texel_gather(photo, tv, filter=filter, plan=True, **kw)
    assert torch.equal(color.view(torch.int32), plain.view(torch.int32)) and float(color.detach().abs().sum()) > 0
    color.backward(g)
    cached = list(tv._gather_plans.values())
    assert len(cached) == 1
    assert torch.equal(photo.grad.view(torch.int32), cached[0].adjoint(g).view(torch.int32)) and float(photo.grad.abs().sum()) > 0
    first = photo.grad.clone()
    photo.grad = None
    tv.gather(photo, filter=filter, plan=True, **kw).backward(g)
    assert list(tv._gather_plans.values())[0] is cached[0] and list(tv._gather_plans.values())[0].entries is cached[0].entries
    assert torch.equal(photo.grad.view(torch.int32), first.view(torch.int32))                  # the same bits from run to run
    photo.grad = None
    texel_gather(photo, tv, filter=filter, plan=gather_plan(tv, res, filter, **kw), **kw).backward(g)
    assert torch.equal(photo.grad.view(torch.int32), first.view(torch.int32))


@pytest.mark.parametrize("filter", ["mip", "aniso"])
def test_a_truncated_pyramid(filter):
    """levels=2 under a footprint of 8: three levels only, and the texels whose level lies beyond are clamped onto level 2"""
    res, kw = (96, 64), dict(FILTERS[filter], footprint=8.0, levels=2)
    plan, ref, _ = check_structure_and_apply(scene_view("cbox_64x64_standard", res), res, filter, "cbox_64x64_standard 96x64 levels=2", kw)
    assert plan.levels == 2 and plan.rows == 96 * 64 + 48 * 32 + 24 * 16
    assert GR.counts(ref)[96 * 64 + 48 * 32:].sum() > 0                # (under this footprint no texel is left on level 0)


def test_an_nnz_above_the_count_still_gives_the_plan():
    """zdr_gather_plan_build with more room than entries: the same row_start, the same entries, no row reaches the tail"""
    res = (96, 64)
    tv = scene_view("cbox_16x16_standard", res)
    plan = gather_plan(tv, res, "mip", footprint=2.0)
    L, p, nnz = N.lib(), plan._params, plan.nnz + 37
    ws = torch.empty(int(L.zdr_gather_plan_workspace_bytes(C.byref(p), nnz)), dtype=torch.uint8, device="cuda")
    row_start, entries = torch.empty(plan.rows + 1, dtype=torch.int32, device="cuda"), torch.full((nnz, 2), -1, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(L.zdr_gather_plan_build(C.byref(p), tv.data.data_ptr(), None, nnz, ws.data_ptr(), row_start.data_ptr(), entries.data_ptr(), stream))
    torch.cuda.synchronize()
    assert plan.nnz > 0 and int(row_start[-1]) == plan.nnz
    assert torch.equal(row_start, plan.row_start) and torch.equal(entries[:plan.nnz], plan.entries)


@pytest.mark.parametrize("filter", list(FILTERS))
def test_texel_project_passes_the_plan_through(filter):
    """One view: color = w c / w on the texels the view counts, so the cotangent that reaches the gather is, operation for operation,
    g' = (g / w) w there and 0 elsewhere.  The gradient of the default and the gradient through the plan are each held to ONE bar — the
    existing rule's, on this view and g' — of the float64 transpose of g'.  (g is 0 on the texels within NEAR of a switch of N, where
    the float64 reference may place its probes otherwise: tests/test_gpu_texel_aniso.py.)"""
    name, res, kw = "cbox_16x16_standard", (96, 64), FILTERS[filter]
    scene, cam = TP.case_scene(name, "bvh"), TP.camera(PC.CASES[name][1])
    theta = torch.rand(16, 16, 4, device="cuda")
    tv = scene.texel_view(theta, res=res, camera=cam, footprint=True)          # what texel_project makes, bit for bit
    view, fp = tv.data.cpu().numpy(), tv.footprint_data.cpu().numpy()
    gen = torch.Generator().manual_seed(6)
    base, g = torch.rand(res[1], res[0], 4, generator=gen).cuda(), torch.randn(16, 16, 4, generator=gen).cuda()
    if filter == "aniso":
        g = torch.where(torch.from_numpy(AR.exempt(fp, kw["footprint"], kw["max_aniso"])).cuda()[..., None], torch.zeros_like(g), g)
    w = tv.weight(1.0)
    seen = w > 0
    reach = (torch.where(seen[..., None], g, torch.zeros_like(g)) / torch.where(seen, w, torch.ones_like(w))[..., None]) * w[..., None]
    bar, r64 = adjoint_bar(filter, reach.cpu().numpy(), view, fp, res)
    for plan in (None, True):
        photo = base.clone().requires_grad_()
        scene.texel_project([(cam, photo)], theta, filter=filter, plan=plan, **kw).color.backward(g)
        err = float(np.abs(photo.grad.cpu().numpy().astype(np.float64) - r64).max())
        print(f"[gather plan] texel_project {filter}, plan={plan}: gradient vs float64 transpose {err:.3e}; bar {bar:.3e} "
              f"(largest |value| {float(np.abs(r64).max()):.3e})")
        assert err <= bar and np.abs(r64).max() > 0
    with pytest.raises(ValueError):
        scene.texel_project([(cam, base)], theta, plan=gather_plan(scene_view(name, res), res))


def test_wrong_plans_and_arguments_raise():
    name, res = "cbox_16x16_standard", (96, 64)
    tv = scene_view(name, res)
    photo = torch.rand(res[1], res[0], 4, device="cuda")
    with pytest.raises(ValueError):
        texel_gather(photo, tv, plan=gather_plan(tv, (48, 32)))                                   # another res
    with pytest.raises(ValueError):
        texel_gather(photo, tv, filter="mip", plan=gather_plan(tv, res, "bilinear"))             # another filter
    with pytest.raises(ValueError):
        texel_gather(photo, tv, filter="mip", footprint=2.0, plan=gather_plan(tv, res, "mip", footprint=1.0))      # another footprint
    with pytest.raises(ValueError):
        texel_gather(photo, tv, filter="aniso", max_aniso=4, plan=gather_plan(tv, res, "aniso", max_aniso=8))
    other = TexelView(tv.data.clone(), res, tv.footprint_data.clone())                           # the same size, other buffers
    for filter in FILTERS:
        with pytest.raises(ValueError):
            texel_gather(photo, other, filter=filter, plan=gather_plan(tv, res, filter, **FILTERS[filter]), **FILTERS[filter])
    texel_gather(photo, other, plan=True)
    first = other._gather_plans[next(iter(other._gather_plans))]
    assert texel_gather(photo, other, plan=True) is not None and other._gather_plans[next(iter(other._gather_plans))] is first
    other.data[0, 0, 0] += 0.0                                                                    # an in-place write: the plan is stale
    with pytest.raises(ValueError):
        texel_gather(photo, other, plan=first)
    texel_gather(photo, other, plan=True)
    assert other._gather_plans[next(iter(other._gather_plans))] is not first                      # built anew
    bare = TexelView(tv.data, res)
    with pytest.raises(ValueError):
        gather_plan(bare, res, "aniso")                                                           # no footprint buffer
    with pytest.raises(ValueError):
        texel_gather(photo, bare, filter="aniso", plan=True)
    with pytest.raises(ValueError):
        texel_gather(photo, tv.data, plan=True)                                                   # nowhere to keep the plan
    with pytest.raises(ValueError):
        gather_plan(tv, res, "nearest")
    with pytest.raises(ValueError):
        gather_plan(tv, res, "mip", footprint=float("nan"))
    with pytest.raises(ValueError):
        gather_plan(tv, (0, 4))
    plan = gather_plan(tv, res)
    with pytest.raises(ValueError):
        plan.apply(torch.zeros(3, 3, 4, device="cuda"))
    with pytest.raises(ValueError):
        plan.apply(torch.zeros(16, 16, 4, device="cuda"), d_pyramid=torch.zeros(1, 4, device="cuda"))


def test_the_c_entry_points_refuse_null_pointers_zero_sizes_and_a_bad_struct_size():
    L = N.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    a, b, c, d, e = (buf[k * 8192:].data_ptr() for k in range(5))

    def params(**kw):
        p = N.GatherPlanParams()
        p.struct_size = C.sizeof(N.GatherPlanParams)
        p.tex_h, p.tex_w, p.width, p.height, p.filter, p.levels, p.footprint, p.max_aniso = 4, 4, 3, 2, 2, 0, 1.0, 8
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    good = params()
    assert L.zdr_gather_plan_rows(C.byref(good)) == 6 + 3 and L.zdr_gather_plan_workspace_bytes(C.byref(good), 0) > 0
    bad = [params(struct_size=4), params(tex_h=0), params(tex_w=-1), params(width=0), params(height=0), params(filter=3), params(filter=-1), params(levels=-1),
           params(footprint=0.0), params(footprint=float("nan")), params(max_aniso=0), params(max_aniso=17)]
    for p in bad:
        assert L.zdr_gather_plan_rows(C.byref(p)) == 0 and L.zdr_gather_plan_workspace_bytes(C.byref(p), 0) == 0
        assert L.zdr_gather_plan_count(C.byref(p), a, b, c, None) == E_INVALID
        assert L.zdr_gather_plan_build(C.byref(p), a, b, 0, c, d, e, None) == E_INVALID
        assert L.zdr_gather_plan_apply(C.byref(p), a, b, c, d, e, None) == E_INVALID
    assert L.zdr_gather_plan_count(None, a, b, c, None) == E_INVALID
    for args in ((None, b, c), (a, None, c), (a, b, None), (a + 4, b, c)):           # a null view, footprint buffer (aniso) or workspace; misaligned
        assert L.zdr_gather_plan_count(C.byref(good), *args, None) == E_INVALID
    for args in ((None, b, 0, c, d, e), (a, b, 0, None, d, e), (a, b, 0, c, None, e), (a, b, 0, c, d, None), (a, b, 0, c, c, e)):
        assert L.zdr_gather_plan_build(C.byref(good), *args, None) == E_INVALID
    for args in ((None, b, c, d, e), (a, None, c, d, e), (a, b, None, d, e), (a, b, c, None, e), (a, b, c, d, None), (a, b, c, d, d)):
        assert L.zdr_gather_plan_apply(C.byref(good), *args, None) == E_INVALID
    bil = params(filter=0, footprint=0.0, max_aniso=0)                # a bilinear plan reads neither, and has no pyramid
    assert L.zdr_gather_plan_rows(C.byref(bil)) == 6
    assert L.zdr_gather_plan_build(C.byref(bil), a, None, 2 ** 31, c, d, e, None) == -3                 # ZDR_E_UNSUPPORTED: nnz above 2^31 - 1
    torch.cuda.synchronize()
