"""-m gpu: the UV tangents (Scene.texel_tangents_forward, texel_aovs(..., tangents=True), texel_footprint_forward(..., tangents=),
texel_view(..., footprint="uv"); include/zdr.h, zdr_scene_texel_tangents, zdr_texel_footprint_tangents) against the reference of
tests/texel_tangent_ref.py on the cases of tests/texel_tangent_cases.py.

The tangent buffer is held against the float64 reference under the bars of texel_tangent_cases (4 x the float32 reference's own error,
floor 4 float32 ulps of the channel's scale), ``orientation`` and the zero rows exactly; the aovs output must be the bits of
texel_aovs_forward, and both outputs the same bits from run to run, between the two acceleration structures and whatever the buffers
held.  The footprint from tangents is held against the float64 reference on the kernels' OWN buffers, and the quality condition — the UV
footprint gives the smallest error of the five gathers on a non-square texture — is checked on the kernels' own output.  Every figure is
printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import texel_aniso_cases as AC
import texel_aniso_ref as AR
import texel_project_cases as PC
import texel_project_ref as PR
import texel_tangent_cases as TT
import texel_tangent_ref as TR
from zdr_amd import Camera, Scene, TexelTangents, float3, texel_footprint_forward
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

INVALID = -1            # ZDR_E_INVALID of include/zdr.h
_scenes = {}


def bits(t):
    return t.contiguous().view(torch.int32)


def camera(cam):
    fov, o, t, up = cam
    return Camera(fov=fov, origin=float3(*o), target=float3(*t), up=float3(*up))


def case_scene(name, accel="auto"):
    make = TT.CASES[name][0]
    if (make, accel) not in _scenes:
        _scenes[(make, accel)] = Scene(make(), integrator="direct", accel=accel)
    return _scenes[(make, accel)]


def run_case(name, accel="auto", **kw):
    _, slots, material, hw = TT.CASES[name]
    out = case_scene(name, accel).texel_tangents_forward(material, hw, slots=slots, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(None)
def own_buffers(name):
    """(aovs, tangents, view, uv footprint) of a footprint case, the kernels' own, on the GPU"""
    case, cam, res = TT.FOOTPRINT_CASES[name]
    aovs, tan = run_case(case, "bvh")
    view = case_scene(case, "bvh").texel_view_forward(aovs, res, camera=camera(cam))
    fp = texel_footprint_forward(aovs, res, camera(cam), tangents=tan)
    torch.cuda.synchronize()
    return aovs, tan, view, fp


# ------------------------------------------------------------------------------------------- the tangent buffer
@pytest.mark.parametrize("name", list(TT.CASES))
def test_tangent_parity_with_the_float64_reference(name):
    aovs, tan = (t.cpu().numpy() for t in run_case(name))
    ref, keep = TT.reference(name)["data"], TT.compared(name)
    e, bars, m = TT.errors(name, tan), TT.bars(name), TT.MARGINS[name]
    rel = TT.area_relative_error(tan, aovs)
    print(f"[texel tangents parity] {name}: {int((~keep).sum())} of {keep.size} texels uncertain; kernel vs float64 tangent {e[0]:.3e} area {e[1]:.3e};  "
          f"float32 reference {m[0]:.3e} {m[1]:.3e};  bars {bars[0]:.3e} {bars[1]:.3e};  area against texel_size^2 {rel:.3e} (bar {TT.area_bar(name):.3e})")
    assert np.isfinite(tan).all()
    assert np.array_equal(tan[..., 7][keep], ref[..., 7][keep].astype(np.float32)), name                     # orientation: exact
    assert np.array_equal(TR.zero_rows(tan)[keep], TR.zero_rows(ref)[keep]), name                            # the zero rows: exact
    reached = aovs[..., 12] == 1
    assert np.array_equal(TR.zero_rows(tan)[reached], (aovs[..., 7] == 0)[reached]) and TR.zero_rows(tan)[~reached].all(), name
    for got_e, bar in zip(e, bars):
        assert got_e <= bar, (name, e, bars)
    assert rel <= TT.area_bar(name), (name, rel)
    if name in TT.ORIENTATION:
        assert reached.any() and (tan[..., 7][reached & keep] == TT.ORIENTATION[name]).all(), name
    else:
        assert TR.zero_rows(tan).all(), name                                                                  # 1 x 1, and a material no instance has


@pytest.mark.parametrize("name", ["soup_130", "cbox_16x64", "cbox_1x1", "cbox_no_instance"])
def test_the_same_bits_as_texel_aovs_from_run_to_run_and_between_the_accels(name):
    _, slots, material, hw = TT.CASES[name]
    aovs, tan = run_case(name, "brute")
    want = case_scene(name, "brute").texel_aovs_forward(material, hw, slots=slots)
    assert torch.equal(bits(aovs), bits(want)), name                                                         # the aovs output IS texel_aovs_forward's
    nbytes = int(N.lib().zdr_texel_aovs_workspace_bytes(*hw))
    for accel in ("brute", "bvh"):
        nan_a, nan_t = torch.full_like(aovs, float("nan")), torch.full_like(tan, float("nan"))
        ws = torch.full((nbytes,), 0xFF if accel == "brute" else 0x00, dtype=torch.uint8, device="cuda")
        a2, t2 = run_case(name, accel, out=nan_t, aovs_out=nan_a, workspace=ws)                             # whatever the three buffers held
        assert a2 is nan_a and t2 is nan_t
        assert torch.equal(bits(a2), bits(aovs)) and torch.equal(bits(t2), bits(tan)), (name, accel)


# ------------------------------------------------------------------------------------------- the footprint from tangents
@pytest.mark.parametrize("name", list(TT.FOOTPRINT_CASES))
def test_uv_footprint_parity_with_the_float64_reference(name):
    case, cam, res = TT.FOOTPRINT_CASES[name]
    aovs, tan, _, fp = own_buffers(name)
    pts, tn, got = aovs.cpu().numpy(), tan.cpu().numpy(), fp.cpu().numpy()
    ref = TT.footprint_reference(name, pts=pts, tangents=tn)                                                  # float64, on the kernels' own buffers
    vis, vref = TT.visible(name), TT.view_reference(name)
    err = TT.footprint_errors(got, ref)[vis].max(0)
    fail = TT.footprint_failing(name, got, ref)
    print(f"[uv footprint parity] {name}: visible {int(vis.sum())}, failing {int(fail.sum())}")
    for q, e, bar, margin in zip(AC.QUANTITIES, err, TT.footprint_bars(name, ref), TT.FOOTPRINT_MARGINS[name]):
        print(f"    {q}: kernel vs float64 largest {e:.3e}; float32 reference {margin:.3e}; bar {bar:.3e}")
    assert np.isfinite(got).all() and float(np.abs(got[vis]).sum()) > 0
    assert not fail.any(), (name, int(fail.sum()))
    assert (got[~PR.shaded(pts)] == 0).all() and (got[TR.zero_rows(tn)] == 0).all()                          # four zeros exactly
    again = texel_footprint_forward(aovs, res, camera(cam), tangents=tan, out=torch.full_like(fp, float("nan")))
    assert torch.equal(bits(again), bits(fp))                                                                 # the same bits, whatever out held
    assert int(vis.sum()) == {"cbox_16x64": 458, "cbox_64x16": 465}.get(name, int(vis.sum())) and vref["front"][vis].all()


def test_zero_tangent_rows_and_texels_behind_the_camera_give_four_zeros():
    name = "cbox_64x16"
    case, _, res = TT.FOOTPRINT_CASES[name]
    aovs, tan, _, fp = own_buffers(name)
    ys, xs = np.nonzero(TT.visible(name))
    dirty = tan.clone()
    dirty[ys[0], xs[0]] = 0.0; dirty[ys[1], xs[1]] = 0.0
    got = texel_footprint_forward(aovs, res, camera(TT.FOOTPRINT_CASES[name][1]), tangents=dirty)
    hit = torch.zeros(fp.shape[:2], dtype=torch.bool, device="cuda")
    hit[ys[0], xs[0]] = True; hit[ys[1], xs[1]] = True
    assert (got[hit] == 0).all() and (fp[hit][:, 3] > 0).all() and torch.equal(bits(got[~hit]), bits(fp[~hit]))
    inside = camera(PC.CAMERAS["inside"])                                                                  # stands in the box: texels lie behind it
    got = texel_footprint_forward(aovs, res, inside, tangents=tan).cpu().numpy()
    pts = aovs.cpu().numpy()
    front = PR.view_ref(pts, PC.CAMERAS["inside"], res, TT.oracle_scene(name))
    behind = PR.shaded(pts) & ~front["front"] & ~front["uncertain"]
    assert int(behind.sum()) > 50 and (got[behind] == 0).all() and np.isfinite(got).all()


# ------------------------------------------------------------------------------------------- quality on the kernels' own output
@pytest.mark.parametrize("name", TT.QUALITY_CASES)
def test_the_uv_view_gathers_best_of_the_five_on_a_non_square_texture(name):
    case, cam, res = TT.FOOTPRINT_CASES[name]
    _, slots, material, hw = TT.CASES[case]
    scene = case_scene(case, "bvh")
    mat = torch.zeros(hw[0], hw[1], 4, device="cuda")
    texels = scene.texel_aovs(mat, tangents=True)
    uv = scene.texel_view(mat, res=res, camera=camera(cam), texels=texels, footprint="uv")
    sq = scene.texel_view(mat, res=res, camera=camera(cam), texels=texels, footprint="square")
    assert uv.footprint_patch == "uv" and sq.footprint_patch == "square"
    for label, image in AC.images().items():
        img = torch.from_numpy(np.ascontiguousarray(image, np.float32)).cuda()
        truth = TT.truths(name)[label]
        row = {"bilinear": uv.gather(img), "mip 1": uv.gather(img, filter="mip"), "mip 0.5": uv.gather(img, filter="mip", footprint=0.5),
               "aniso square": sq.gather(img, filter="aniso"), "aniso uv": uv.gather(img, filter="aniso")}
        row = {k: TT.rmse(name, v.cpu().numpy(), truth) for k, v in row.items()}
        print(f"[uv quality, kernels] {name} {label}: " + "  ".join(f"{k} {v:.4f}" for k, v in row.items()))
        assert all(row["aniso uv"] < v for k, v in row.items() if k != "aniso uv"), (name, label, row)


# ------------------------------------------------------------------------------------------- plumbing
def test_plumbing_of_the_python_layer():
    name = "cbox_16x64"
    case, cam, res = TT.FOOTPRINT_CASES[name]
    hw = TT.CASES[case][3]
    scene, cam = case_scene(case, "bvh"), camera(cam)
    mat = torch.zeros(hw[0], hw[1], 4, device="cuda")
    plain = scene.texel_aovs(mat)
    assert plain.tangents is None
    with_t = scene.texel_aovs(mat, tangents=True)
    assert isinstance(with_t.tangents, TexelTangents) and torch.equal(bits(with_t.data), bits(plain.data))
    t = with_t.tangents
    assert t.data.shape == (hw[0], hw[1], 8) and t.dpdx.shape == (hw[0], hw[1], 3) and t.dpdy.shape == (hw[0], hw[1], 3)
    assert torch.equal(t.area, t.data[..., 3]) and torch.equal(t.orientation, t.data[..., 7])
    m = t.metric().cpu().numpy().astype(np.float64)
    d = t.data.cpu().numpy().astype(np.float64)
    want = np.stack([(d[..., 0:3] ** 2).sum(-1), (d[..., 0:3] * d[..., 4:7]).sum(-1), (d[..., 4:7] ** 2).sum(-1)], -1)
    assert m.shape == (hw[0], hw[1], 3) and np.abs(m - want).max() <= 8 * TT.EPS32 * np.abs(want).max()
    # footprint=True is today's square patch, bit for bit
    v_true = scene.texel_view(mat, res=res, camera=cam, texels=plain, footprint=True)
    assert v_true.footprint_patch == "square" and torch.equal(bits(v_true.footprint_data), bits(texel_footprint_forward(plain.data, res, cam)))
    assert scene.texel_view(mat, res=res, camera=cam, texels=plain).footprint_patch is None
    # "uv" computes the tangents itself without texels, and refuses texels that lack them
    own = scene.texel_view(mat, res=res, camera=cam, footprint="uv")
    assert own.footprint_patch == "uv" and torch.equal(bits(own.footprint_data), bits(texel_footprint_forward(with_t.data, res, cam, tangents=t.data)))
    assert not torch.equal(bits(own.footprint_data), bits(v_true.footprint_data))
    with pytest.raises(ValueError, match="tangents=True"):
        scene.texel_view(mat, res=res, camera=cam, texels=plain, footprint="uv")
    with pytest.raises(ValueError):
        scene.texel_view(mat, res=res, camera=cam, footprint="round")
    # a tangent tensor of the wrong shape, dtype or device
    for bad in (t.data[:, :-1], t.data[..., :4], t.data.double(), t.data.cpu()):
        with pytest.raises(ValueError):
            texel_footprint_forward(with_t.data, res, cam, tangents=bad)


def test_a_gather_plan_on_a_uv_view_gives_the_atomic_adjoint_and_the_same_bits_twice():
    name = "cbox_64x16"
    case, cam, res = TT.FOOTPRINT_CASES[name]
    hw = TT.CASES[case][3]
    scene = case_scene(case, "bvh")
    mat = torch.zeros(hw[0], hw[1], 4, device="cuda")
    view = scene.texel_view(mat, res=res, camera=camera(cam), footprint="uv")
    gen = torch.Generator().manual_seed(3)
    photo = torch.rand(res[1], res[0], 4, generator=gen).cuda()
    g = torch.rand(hw[0], hw[1], 4, generator=gen).cuda()
    grads = []
    for plan in (None, True, True):
        img = photo.clone().requires_grad_()
        out = view.gather(img, filter="aniso", plan=plan)
        out.backward(g)
        grads.append(img.grad.clone())
    v, f = view.data.cpu().numpy(), view.footprint_data.cpu().numpy()
    r64 = AR.gather_aniso_adjoint_ref(g.cpu().numpy(), v, f, res, 1.0, 8, 0, np.float64)
    r32 = AR.gather_aniso_adjoint_ref(g.cpu().numpy(), v, f, res, 1.0, 8, 0, np.float32)
    bar = AC.gather_bar(r32, r64)
    e_atomic, e_plan = (float(np.abs(x.cpu().numpy() - r64).max()) for x in grads[:2])
    print(f"[uv plan] atomic adjoint vs float64 {e_atomic:.3e}, plan {e_plan:.3e}, plan against atomic {float((grads[0] - grads[1]).abs().max()):.3e}; bar {bar:.3e}")
    assert float(grads[1].abs().sum()) > 0 and e_plan <= bar and e_atomic <= bar
    assert float((grads[0] - grads[1]).abs().max()) <= bar
    assert torch.equal(bits(grads[1]), bits(grads[2]))


def test_texel_project_passes_the_patch_through_to_each_view():
    name = "cbox_16x64"
    case, cam, res = TT.FOOTPRINT_CASES[name]
    hw = TT.CASES[case][3]
    scene = case_scene(case, "bvh")
    mat = torch.zeros(hw[0], hw[1], 4, device="cuda")
    gen = torch.Generator().manual_seed(5)
    cams = [camera(cam), camera(PC.CAMERAS["inside"])]
    views = [(c, torch.rand(res[1], res[0], 4, generator=gen).cuda()) for c in cams]
    got = scene.texel_project(views, mat, filter="aniso", footprint_patch="uv")
    texels = scene.texel_aovs(mat, tangents=True)
    num = weight = None
    for c, image in views:
        view = scene.texel_view(mat, res=res, camera=c, texels=texels, footprint="uv")
        w = view.weight(1.0)
        term = w[..., None] * view.gather(image, filter="aniso")
        num, weight = (term, w) if num is None else (num + term, weight + w)
    seen = weight > 0
    want = torch.where(seen[..., None], num / torch.where(seen, weight, torch.ones_like(weight))[..., None], torch.zeros_like(num))
    assert torch.equal(bits(got.color), bits(want)) and torch.equal(bits(got.weight), bits(weight)) and float(got.color.abs().sum()) > 0
    square = scene.texel_project(views, mat, filter="aniso")
    assert not torch.equal(bits(square.color), bits(got.color))
    with pytest.raises(ValueError):
        scene.texel_project(views, mat, filter="aniso", footprint_patch="round")
    with pytest.raises(ValueError, match="tangents=True"):
        scene.texel_project(views, mat, filter="aniso", footprint_patch="uv", texels=scene.texel_aovs(mat))


# ------------------------------------------------------------------------------------------- the C entry points
def test_the_c_entry_points_refuse_bad_arguments():
    L = N.lib()
    scene = case_scene("cbox_5x7")
    scene._upload_slots((0, None))
    H = W = 8
    n = H * W
    buf = torch.zeros(n * 16 + n * 8 + n * 2 + n * 4 + 64, dtype=torch.float32, device="cuda")
    aovs = buf.data_ptr()
    tan, ws, fp = aovs + 4 * n * 16, aovs + 4 * n * 24, aovs + 4 * n * 26
    st = scene._stream()
    call = lambda h, m, th, tw, a, t, w: L.zdr_scene_texel_tangents(h, m, th, tw, a, t, w, st)       # noqa: E731
    assert call(scene._handle, 0, H, W, aovs, tan, ws) == 0
    assert call(None, 0, H, W, aovs, tan, ws) == INVALID
    for a, t, w in ((None, tan, ws), (aovs, None, ws), (aovs, tan, None)):                               # null
        assert call(scene._handle, 0, H, W, a, t, w) == INVALID
    for a, t, w in ((aovs + 4, tan, ws), (aovs, tan + 8, ws), (aovs, tan, ws + 4)):                       # misaligned
        assert call(scene._handle, 0, H, W, a, t, w) == INVALID
    for a, t, w in ((aovs, aovs, ws), (aovs, aovs + 64 * n - 16, ws), (aovs, tan, tan), (aovs, tan, tan + 32 * n - 16), (aovs, tan, aovs + 16),
                    (tan + 16, tan, ws)):                                                                # overlapping
        assert call(scene._handle, 0, H, W, a, t, w) == INVALID, (a - aovs, t - aovs, w - aovs)
    for th, tw in ((0, W), (H, 0), (-1, W), (H, -3)):                                                    # size <= 0
        assert call(scene._handle, 0, th, tw, aovs, tan, ws) == INVALID
    for m in (-1, N.MAX_MATERIALS):                                                                      # material out of range
        assert call(scene._handle, m, H, W, aovs, tan, ws) == INVALID
    assert b"material" in L.zdr_last_error()
    torch.cuda.synchronize()

    p = N.TexelFootprintParams()
    p.struct_size = C.sizeof(N.TexelFootprintParams)
    p.tex_h, p.tex_w, p.width, p.height = H, W, 24, 16
    from zdr_amd.render import _camera_pod
    p.camera = _camera_pod(camera(TT.FOOTPRINT_CASES["cbox_16x64"][1]))
    foot = lambda a, t, o: L.zdr_texel_footprint_tangents(C.byref(p), a, t, o, st)                       # noqa: E731
    assert foot(aovs, tan, fp) == 0
    assert L.zdr_texel_footprint_tangents(None, aovs, tan, fp, st) == INVALID
    for a, t, o in ((None, tan, fp), (aovs, None, fp), (aovs, tan, None), (aovs + 4, tan, fp), (aovs, tan + 4, fp), (aovs, tan, fp + 8)):
        assert foot(a, t, o) == INVALID
    for a, t, o in ((aovs, tan, aovs), (aovs, tan, tan), (aovs, tan, tan + 32 * n - 16), (aovs, tan, aovs + 64 * n - 16)):
        assert foot(a, t, o) == INVALID
    for field, value in (("tex_h", 0), ("tex_w", -1), ("width", 0), ("height", -2), ("struct_size", 4)):
        keep = getattr(p, field)
        setattr(p, field, value)
        assert foot(aovs, tan, fp) == INVALID, field
        setattr(p, field, keep)
    p.camera.fov = float("nan")
    assert foot(aovs, tan, fp) == INVALID
    torch.cuda.synchronize()
    scene.check()
