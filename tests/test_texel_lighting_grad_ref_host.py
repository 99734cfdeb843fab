"""The reference of the adjoint of the texture-space lighting (tests/texel_lighting_grad_ref.py) on the host, pinned by LINEARITY: with
the light list, the tables and visibility held fixed the float64 forward reference (tests/texel_lighting_ref.py) is linear in the
emissions and in the map, so its finite difference along a unit step is the adjoint's entry exactly, up to float64 rounding.  Also: the
cases' uncertain texels, the margins of profiles/texel_lighting_grad_margins.txt, and the bindings.  No GPU."""
import os

import numpy as np
import pytest

import texel_lighting_grad_cases as GC
from conftest import ROOT
from zdr_amd import _native

LINEAR = 1e-12          # of sum |terms|: float64 rounding of two forwards of some hundreds of samples and their difference


@pytest.mark.parametrize("name", [n for n in GC.CASES if "emission" in GC.targets(n)])
def test_a_unit_step_of_every_light_and_channel_is_the_adjoints_entry(name):
    """one forward per light, its three channels stepped together: channel ch of the irradiance reads only channel ch of an emission"""
    A = GC.CASES[name][0]()
    ref, g = GC.reference(name), GC.cotangent(name).astype(np.float64)
    e0 = A.inst_emission.astype(np.float64)
    base = GC.forward(name, emissions=e0)
    worst = 0.0
    for inst in GC.lights(name):
        e = e0.copy(); e[inst] = (e0[inst] + 1.0).astype(np.float32)      # the light table holds float32 emissions: the step as it arrives there
        step = e[inst] - e0[inst]
        d = GC.forward(name, emissions=e) - base
        for ch in range(3):
            fd, want, scale = float((g[..., ch] * d[..., ch]).sum()) / step[ch], float(ref["d_emission"][inst, ch]), float(ref["abs_emission"][inst, ch])
            worst = max(worst, abs(fd - want) / scale)
            assert abs(fd - want) <= LINEAR * scale, (name, inst, ch, fd, want, scale)
    print(f"[texel lighting grad ref] {name}: {len(GC.lights(name))} lights x 3 channels, largest |finite difference - adjoint| = {worst:.2e} of sum |terms|")


@pytest.mark.parametrize("name", [n for n in GC.CASES if "env" in GC.targets(n)])
def test_three_steps_of_a_float64_map_are_the_adjoints_inner_product(name):
    ref, g = GC.reference(name), GC.cotangent(name).astype(np.float64)
    tex = GC.CASES[name][4]()[0].astype(np.float64)
    emissions = GC.CASES[name][0]().inst_emission
    base = GC.forward(name, emissions=emissions, env_tex=tex)
    rng = np.random.default_rng(5)
    for k in range(3):
        delta = np.zeros_like(tex); delta[..., :3] = rng.uniform(0.0, 1.0, tex[..., :3].shape)      # non-negative: no accepted sample turns dark
        d = GC.forward(name, emissions=emissions, env_tex=tex + delta) - base
        fd, want = float((g[..., :3] * d).sum()), float((ref["d_env"].astype(np.float64) * delta).sum())
        scale = float((ref["abs_env"] * delta).sum())
        print(f"[texel lighting grad ref] {name} direction {k}: <d_out, dF> {fd:.12e}  <d_env, delta> {want:.12e}  difference {abs(fd - want) / scale:.2e} of sum |terms|")
        assert abs(fd - want) <= LINEAR * scale, (name, k, fd, want, scale)


@pytest.mark.parametrize("name", list(GC.CASES))
def test_untouched_entries_uncertain_texels_and_every_lights_column(name):
    ref, rch = GC.reference(name), GC.reached(name)
    unc = ref["uncertain"]
    print(f"[texel lighting grad ref] {name}: {int((unc & rch).sum())} of {int(rch.sum())} reached texels uncertain; terms per light "
          f"{[int(ref['n_emission'][i]) for i in GC.lights(name)]}")
    assert not (unc & ~rch).any() and (unc & rch).sum() <= GC.MAX_UNCERTAIN * rch.sum()
    assert (GC.cotangent(name)[unc] == 0).all()
    others = [i for i in range(ref["d_emission"].shape[0]) if i not in GC.lights(name)]
    assert (ref["d_emission"][others] == 0).all() and (ref["n_emission"][others] == 0).all()
    for i in GC.lights(name):
        assert (ref["d_emission"][i] != 0).all() and ref["n_emission"][i] > 0, (name, i)
    if "env" in GC.targets(name):
        assert (ref["d_env"][..., 3] == 0).all() and (ref["d_env"][..., :3] != 0).any()
        assert (ref["d_env"][ref["n_env"] == 0] == 0).all()
    else:
        assert ref["d_env"] is None
    assert GC.targets(name)


def test_the_cases_cover_what_they_are_meant_to():
    lit = GC.reference("env_panel_lit_16")
    assert ((lit["lit_env"] > 0) & (lit["lit_mesh"] > 0)).any()         # both branches of sample_light on one texel
    assert len(GC.lights("chandelier_24")) == 15 and len(GC.lights("multi_24_spp9")) == 3
    assert GC.CASES["multi_24_spp9"][3] == 9 and GC.CASES["cbox_16x16_spp1"][3] == 1
    assert GC.RANGES["cbox_16x16_pmj_tail"] == (1, 16) and "cbox_16x16_pmj_tail" in GC.SAMPLERS


@pytest.mark.parametrize("name", list(GC.CASES))
def test_the_margins_are_the_measurement_and_the_file_states_them(name):
    txt = open(os.path.join(ROOT, "profiles", "texel_lighting_grad_margins.txt")).read()
    line = [ln for ln in txt.splitlines() if ln.strip().startswith(name + " ")]
    assert line, name
    r32 = GC.reference(name, "float32")
    assert sorted(GC.MARGINS[name]) == sorted(GC.targets(name))
    for target in GC.targets(name):
        e = GC.error(name, target, GC.entries(r32, target)[0])
        print(f"[texel lighting grad ref] {name} {target}: float32 vs float64 {e:.3e}; margin {GC.MARGINS[name][target]}")
        assert e <= GC.MARGINS[name][target] <= 1.02 * e + 1e-12        # the constant IS the measurement, rounded up
        assert f"{e:.3e}" in line[0], (name, target, line[0])


def test_the_bindings_exist():
    for sym in ("zdr_texel_lighting_backward_workspace_bytes", "zdr_scene_texel_lighting_backward"):
        assert sym in _native.EXPORTS
    import zdr_amd
    assert hasattr(zdr_amd.Scene, "texel_lighting_backward") and hasattr(zdr_amd.Scene, "TexelLightingOperator")
    header = open(os.path.join(ROOT, "include", "zdr.h")).read()
    assert "zdr_scene_texel_lighting_backward" in header and "#define ZDR_ABI_VERSION 4" in header
    assert os.path.exists(_native.BAKEGRAD_LIB_PATH)
