"""The reference of the texture-space lighting (tests/texel_lighting_ref.py) on the host, and the cases the GPU test compares with it
(tests/texel_lighting_cases.py): the float64 reference against closed forms (Lambert's formula for the irradiance of a polygonal
light, the furnace under a constant sky), the float32 reference against the float64 one (the margins of
profiles/texel_lighting_margins.txt), and the bound on each case's uncertain texels.  Also: the bindings of zdr_scene_texel_lighting
exist.  No GPU."""
import os

import numpy as np
import pytest

import envmap_tables as ET
import texel_lighting_cases as LC
import texel_lighting_ref as LR
import texel_ref as R
from conftest import ROOT
from oracle import OracleScene
from zdr_amd import _native, geometry, scenes
from zdr_amd import envmap as E

STAT_SEED = 11          # chosen once: a fixed input of the two statistical tests


def lambert_irradiance(p, n, corners, radiance):
    """Irradiance at p (normal n) from a polygon of constant radiance that lies wholly above p's horizon: (L / 2) |sum_i beta_i Gamma_i . n|,
    beta_i the angle the i-th side subtends, Gamma_i the unit normal of the plane through p and that side (Lambert 1760)."""
    v = corners - p
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    total = 0.0
    for i in range(v.shape[0]):
        a, b = v[i], v[(i + 1) % v.shape[0]]
        g = np.cross(a, b)
        total += np.arccos(np.clip(a @ b, -1.0, 1.0)) * (g / np.linalg.norm(g)) @ n
    return 0.5 * abs(total) * radiance


def test_the_irradiance_under_a_quad_light_is_lamberts_formula():
    v, t = scenes.panel_mesh(2, 2)
    lv, lt = scenes.panel_mesh(1, 1)
    down = np.array([[0.5, 0, 0, 0.3], [0, -1, 0, 1.5], [0, 0, -0.4, -0.2], [0, 0, 0, 1]], np.float32)       # a 1.0 x 0.8 light facing down, 1.5 above
    emission = np.array([5.0, 3.0, 2.0], np.float32)
    A = geometry.from_arrays(np.concatenate([v, lv]), np.concatenate([t, lt + v.shape[0]]), [0, t.shape[0], t.shape[0] + lt.shape[0]],
                             np.stack([np.eye(4, dtype=np.float32).reshape(16), down.reshape(16)]), np.stack([np.zeros(3, np.float32), emission]))
    pts = np.ascontiguousarray(R.texel_aovs_ref(A, (0, None), 0, (4, 4), np.float32)["data"], np.float32)
    assert (pts[..., 12] == 1).all()
    spp = 1024
    ref = LR.texel_lighting_ref(A, OracleScene.from_arrays(A), pts, spp=spp, seed=STAT_SEED)
    corners = np.array([[-0.2, 1.5, -0.6], [0.8, 1.5, -0.6], [0.8, 1.5, 0.2], [-0.2, 1.5, 0.2]])
    worst = 0.0
    for y in range(4):
        for x in range(4):
            p, n = pts[y, x, 8:11].astype(np.float64), pts[y, x, 4:7].astype(np.float64)
            for ch in range(3):
                want = lambert_irradiance(p, n, corners, float(emission[ch]))
                se = np.sqrt(ref["var"][y, x, ch] / spp)
                worst = max(worst, abs(ref["data"][y, x, ch] - want) / se)
                assert abs(ref["data"][y, x, ch] - want) <= 4.0 * se, (x, y, ch, ref["data"][y, x, ch], want, se)
            # the light's back is all that closes the sky: openness = 1 - its form factor, the same formula with radiance 1 / pi
            closed = lambert_irradiance(p, n, corners, 1.0 / np.pi)
            se = np.sqrt(ref["var"][y, x, 3] / spp)
            worst = max(worst, abs(ref["data"][y, x, 3] - (1.0 - closed)) / se)
            assert abs(ref["data"][y, x, 3] - (1.0 - closed)) <= 4.0 * se, (x, y, ref["data"][y, x, 3], 1.0 - closed, se)
    print(f"[texel lighting ref] quad light, 16 texels at spp {spp}: largest |estimate - Lambert| = {worst:.2f} standard errors")


def test_a_constant_sky_gives_pi_times_its_radiance_and_full_openness():
    v, t = scenes.panel_mesh(1, 1)
    A = geometry.from_arrays(v, t)
    img = ET.make_map("constant", (16, 32))                             # radiance 2 everywhere
    prob, alias, pdf = ET.host_tables(img, False)
    env = (E.prepare_image(img), prob, alias, pdf, E.SAMPLE_MAP_W, E.SAMPLE_MAP_H)
    pts = np.ascontiguousarray(R.texel_aovs_ref(A, (0,), 0, (4, 4), np.float32)["data"], np.float32)
    spp = 256
    ref = LR.texel_lighting_ref(A, OracleScene.from_arrays(A), pts, spp=spp, seed=STAT_SEED, env=env)
    se = np.sqrt(ref["var"][..., :3] / spp)
    dev = np.abs(ref["data"][..., :3] - np.pi * 2.0) / se
    print(f"[texel lighting ref] furnace, 16 texels at spp {spp}: mean {ref['data'][..., :3].mean():.4f} (pi L = {2 * np.pi:.4f}), largest deviation {dev.max():.2f} standard errors")
    assert (dev <= 4.0).all()
    assert (ref["data"][..., 3] == 1.0).all()


@pytest.mark.parametrize("name", list(LC.CASES))
def test_at_most_one_percent_of_a_cases_reached_texels_is_uncertain(name):
    unc, reached = LC.reference(name)["uncertain"], LC.reached(name)
    print(f"[texel lighting ref] {name}: {int((unc & reached).sum())} of {int(reached.sum())} reached texels uncertain")
    assert not (unc & ~reached).any()
    assert (unc & reached).sum() <= LC.MAX_UNCERTAIN * reached.sum()


@pytest.mark.parametrize("name", list(LC.CASES))
def test_the_float32_reference_agrees_with_float64_within_the_bar(name):
    r64, r32 = LC.reference(name), LC.reference(name, "float32")
    keep = LC.compared(name)
    e = LC.error(name, r32["data"])
    print(f"[texel lighting ref] {name}: float32 vs float64 irradiance {e:.3e}; margin {LC.MARGINS[name]}; bar {LC.bar(name):.3e}; largest irradiance {LC.scale(name):.4e}")
    assert e <= LC.MARGINS[name] and LC.MARGINS[name] <= 1.02 * e + 1e-12      # the constant IS the measurement, rounded up
    assert not (LC.failing(name, r32["data"]) & keep).any()
    assert (r64["data"][~LC.reached(name)] == 0).all() and (r32["data"][~LC.reached(name)] == 0).all()
    assert r64["data"][..., :3].max() > 0


def test_the_cases_cover_what_they_are_meant_to():
    """light and shadow in every case, a texel no sample lit, both branches of the light sampler under the sun, a shorter reach of the
    openness rays under max_distance, and an spp that is no power of two"""
    for name in LC.CASES:
        ref = LC.reference(name)
        lit = ref["lit"][LC.reached(name)]
        assert (lit == 0).any() and (lit > 0).any(), name
    opn_far, opn_near = LC.reference("cbox_16x16")["data"][..., 3], LC.reference("cbox_16x16_ao")["data"][..., 3]
    assert (opn_near >= opn_far).all() and (opn_near > opn_far).any()
    env = LC.reference("env_panel_8x8")["data"][..., 3][LC.reached("env_panel_8x8")]
    assert (env < 1).any() and (env == 1).any()                       # under the blocker, and beside it
    assert LC.CASES["multi_24_spp9"][3] == 9


def test_the_margins_file_states_the_constants():
    txt = open(os.path.join(ROOT, "profiles", "texel_lighting_margins.txt")).read()
    for name in LC.CASES:
        line = [ln for ln in txt.splitlines() if ln.strip().startswith(name + " ")]
        assert line, name
        assert f"{LC.error(name, LC.reference(name, 'float32')['data']):.3e}" in line[0], (name, line[0])


def test_the_bindings_exist():
    for sym in ("zdr_texel_lighting_workspace_bytes", "zdr_scene_texel_lighting"):
        assert sym in _native.EXPORTS
    import zdr_amd
    assert hasattr(zdr_amd, "TexelLighting") and hasattr(zdr_amd.Scene, "texel_lighting") and hasattr(zdr_amd.Scene, "texel_lighting_forward")
    header = open(os.path.join(ROOT, "include", "zdr.h")).read()
    assert "zdr_scene_texel_lighting" in header and "zdr_texel_lighting_params" in header and "#define ZDR_ABI_VERSION 4" in header
