"""The float64 / float32 reference of the texture-space views (tests/texel_project_ref.py) pinned on the host, before the GPU tests lean on
it: the classes every case must populate, the cap on uncertain texels, the gather's adjoint identity, a family with an exact answer, and
the precondition of the round trip with the renderer.  No GPU needed."""
import numpy as np
import pytest

import texel_cases as TC
import texel_lighting_cases as LC
import texel_project_cases as PC
import texel_project_ref as PR


@pytest.mark.parametrize("name", list(PC.CASES))
def test_every_case_populates_the_classes_it_claims(name):
    got = PC.classes(name)
    print(f"[texel project classes] {name}: reached, behind, outside, visible, occluded, seen from behind, uncertain = {got}")
    assert got == PC.CLASSES[name]
    reached, behind, outside, visible, occluded, back, _ = got
    assert behind + outside + visible + occluded == reached
    assert visible > 0 and occluded > 0 and outside > 0
    if "inside" in name:
        assert behind > 0
    else:
        assert back > 0


@pytest.mark.parametrize("name", list(PC.CASES))
def test_the_reference_alone_stays_far_below_the_uncertain_cap(name):
    unc, reached = PC.classes(name)[6], PC.classes(name)[0]
    assert unc <= PC.MAX_UNCERTAIN_REF * reached
    keep = PC.compared(name)
    assert np.array_equal(PC.reference(name, "float32")["data"][..., 0][keep], PC.reference(name)["data"][..., 0][keep])
    assert (PC.reference(name)["data"][~PC.reached(name)] == 0).all()


@pytest.mark.parametrize("name", list(PC.CASES))
def test_the_margins_are_the_float32_references_own_error(name):
    e = PC.errors(name, PC.reference(name, "float32")["data"])
    for got, margin in zip(e, PC.MARGINS[name]):
        assert got <= margin <= 1.01 * got + 1e-12, (name, e, PC.MARGINS[name])


def test_the_pixel_is_the_inverse_of_the_camera_ray():
    """a point on the ray of pixel (x, y) with jitter (jx, jy) projects to (x + jx, y + jy), at the depth it was put at"""
    res, cam = (24, 16), PC.CAMERAS["standard"]
    o, fwd, right, upp, tan, aspect = (a.astype(np.float64) for a in PR.camera_frame(cam, res))
    rng = np.random.default_rng(5)
    xy = rng.uniform(0, 1, (200, 2)) * np.array(res)
    px = (2.0 / res[0] * xy[:, 0] - 1.0) * tan
    py = (2.0 / res[1] * xy[:, 1] - 1.0) * aspect * tan
    d = right[None] * px[:, None] - upp[None] * py[:, None] + fwd[None]
    depth = rng.uniform(0.5, 9.0, 200)
    z, dist, wi, X, Y = PR.project(o[None] + depth[:, None] * d, PR.camera_frame(cam, res), res, np.float64)
    assert np.abs(X - xy[:, 0]).max() < 1e-9 and np.abs(Y - xy[:, 1]).max() < 1e-9 and np.abs(z - depth).max() < 1e-9


def synthetic_view(rng, n, res, visible_share=0.8):
    v = np.zeros((n, 1, 8), np.float32)
    v[:, 0, 0] = rng.uniform(0, 1, n) < visible_share
    v[:, 0, 2] = rng.uniform(0, res[0], n); v[:, 0, 3] = rng.uniform(0, res[1], n)
    return v


@pytest.mark.parametrize("res", [(24, 16), (1, 1), (2, 5)])
def test_the_reference_gathers_adjoint_identity_in_float64(res):
    rng = np.random.default_rng(11)
    view = synthetic_view(rng, 500, res)
    x, y = rng.normal(size=(res[1], res[0], 4)), rng.normal(size=(500, 1, 4))
    lhs = float((PR.gather_ref(x, view, np.float64) * y).sum())
    rhs = float((x * PR.gather_adjoint_ref(y, view, res, np.float64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    d = PR.gather_adjoint_ref(y, view[:, :, :] * np.array([0, 1, 1, 1, 1, 1, 1, 1], np.float32), res, np.float64)
    assert (d == 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_exact_family(dtype):
    """X, Y at pixel centres return the pixel bit for bit; a 1 x 1 image returns its pixel for every visible texel, wherever it lands"""
    rng = np.random.default_rng(3)
    w, h = 24, 16
    image = rng.normal(size=(h, w, 4)).astype(np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    view = np.zeros((h, w, 8), np.float32)
    view[..., 0] = 1; view[..., 2] = xs + 0.5; view[..., 3] = ys + 0.5
    assert np.array_equal(PR.gather_ref(image, view, dtype).astype(np.float32), image)
    one = rng.normal(size=(1, 1, 4)).astype(np.float32)
    v = synthetic_view(rng, 300, (1, 1))
    got = PR.gather_ref(one, v, dtype).astype(np.float32)
    on = v[:, 0, 0] == 1
    assert np.array_equal(got[on, 0], np.broadcast_to(one[0, 0], (int(on.sum()), 4))) and (got[~on] == 0).all()
    # the clamps: X = 0, 0.5, width - 0.5 and just below width read the border pixel alone
    edge = np.zeros((4, 1, 8), np.float32)
    edge[:, 0, 0] = 1; edge[:, 0, 3] = 0.5
    edge[:, 0, 2] = [0.0, 0.5, w - 0.5, np.nextafter(np.float32(w), np.float32(0))]
    got = PR.gather_ref(image, edge, dtype).astype(np.float32)
    assert np.array_equal(got[:2, 0], image[[0, 0], [0, 0]]) and np.array_equal(got[2:, 0], image[[0, 0], [w - 1, w - 1]])
    # a NaN behind an invisible texel is never read
    poisoned = image.copy(); poisoned[3, 4] = np.nan
    v = view.copy(); v[2:5, 3:6, 0] = 0
    assert not np.isnan(PR.gather_ref(poisoned, v, dtype)).any()


def test_the_oracles_first_hits_project_back_into_their_own_pixel():
    """the precondition of the GPU round trip: Cornell box, 24 x 16, spp 1, tent filter off"""
    res = (24, 16)
    pts, hit = PC.cbox_first_hits(res)
    view = PR.view_ref(pts, PC.CAMERAS["standard"], res, LC.oracle_scene(TC.cbox_arrays))
    d = view["data"]
    exempt = PC.round_trip_exempt(view, res) & hit
    ok = (d[..., 0] == 1) & (np.floor(d[..., 2]) == np.arange(res[0])[None, :]) & (np.floor(d[..., 3]) == np.arange(res[1])[:, None])
    print(f"[texel project round trip, oracle] hit pixels {int(hit.sum())}, exempt {int(exempt.sum())}, failing {int((hit & ~ok & ~exempt).sum())}")
    assert hit.sum() > 300
    assert exempt.sum() < 0.01 * hit.sum()
    assert not (hit & ~ok & ~exempt).any()
