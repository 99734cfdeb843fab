"""The preconditions test_gpu_many_lights.py rests on, checked on the CPU oracle alone at that file's resolution, spp and seeds:
the two scenes of many_lights.py drop no sample and stay below the clamp, the oracle's forward is linear in each light's emission,
and the lights beyond the emission-gradient kernels' on-chip table (list index >= 10) carry a large part of the gradient.

These are conditions on the inputs, not tolerances: a changed scene that misses one is to be changed again, not the condition."""
import numpy as np
import pytest

import oracle
from conftest import cbox_material_np, fd_material_np
from many_lights import (CAMERA, LDS_LIGHTS, NLIGHT, OSEED, OSPP, OW, chandelier_arrays, light_rows, oracle_terms, shares, stage30_arrays,
                         stage_material)
from test_gpu_emission_grad import cotangent                   # (importing it needs no GPU; its tests do)
from zdr_amd.scenes import CBOX_CAMERA


def params(integrator, camera, tex_hw):
    return oracle.make_params(integrator, OW, OW, OSPP, OSEED, camera, tex_hw)


@pytest.fixture(scope="module")
def chandelier():
    A = chandelier_arrays()
    return A, oracle.OracleScene.from_arrays(A)


@pytest.fixture(scope="module")
def stage():
    A = stage30_arrays()
    return A, oracle.OracleScene.from_arrays(A)


def material(name):
    return cbox_material_np() if name == "cbox" else fd_material_np(64, 0)


def test_the_chandelier_is_what_the_gpu_tests_take_it_for():
    A = chandelier_arrays()
    assert A.ninst == 17 and A.tris.shape[0] == 116
    rows = light_rows(A.inst_emission)
    assert rows == [1, 2, 3, 4, 5, 6] + list(range(8, 17)) and len(rows) == 15          # instance 7 is the blocker
    assert (A.inst_emission[1] == 20).all() and (A.inst_emission[0] == 0).all() and (A.inst_emission[7] == 0).all()
    assert len({tuple(e) for e in A.inst_emission[rows].tolist()}) == 15                # a distinct rgb per light
    counts = np.diff(A.inst_tri_begin)[rows[1:]]
    assert counts.tolist() == [2 * (1 + i % 3) * (1 + i % 2) for i in range(14)]
    assert int(A.tris.max()) < A.verts.shape[0] and int(A.tris.min()) >= 0


def test_the_stage_has_all_thirty_lights():
    A = stage30_arrays()
    assert A.ninst == 1 + NLIGHT and light_rows(A.inst_emission) == list(range(1, 1 + NLIGHT))
    assert A.inst_emission[1:].min() >= 20 and A.inst_emission[1:].max() <= 80
    assert len({tuple(e) for e in A.inst_emission[1:].tolist()}) == NLIGHT


@pytest.mark.parametrize("integrator", ["path", "direct"])
@pytest.mark.parametrize("mat_name", ["cbox", "fd64"])
def test_chandelier_preconditions(integrator, mat_name, chandelier):
    """No dropped sample and no clamp (oracle_terms asserts both for every render), every light carries at least 1 % of sum |term|
    and the lights beyond the table at least 25 %."""
    A, S = chandelier
    mat = material(mat_name)
    terms, base = oracle_terms(S, params(integrator, CBOX_CAMERA, mat.shape[:2]), mat, A.inst_emission, cotangent(OW, OW, 1))
    sh = shares(terms)[light_rows(A.inst_emission)]
    print(f"[many lights] chandelier {integrator} {mat_name}: image max {float(base[..., :3].max()):.4g}, shares {sh.min():.4f} - {sh.max():.4f}, "
          f"lights beyond the table {sh[LDS_LIGHTS:].sum():.4f}")
    assert sh.min() >= 0.01, sh
    assert sh[LDS_LIGHTS:].sum() >= 0.25, sh


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_stage_preconditions(integrator, stage):
    """At least 10 lights beyond the table carry 1e-3 of sum |term| each, and those carry at least half of it together."""
    A, S = stage
    mat = stage_material()
    terms, base = oracle_terms(S, params(integrator, CAMERA, mat.shape[:2]), mat, A.inst_emission, cotangent(OW, OW, 1))
    sh = shares(terms)[1:]
    big = [k for k in range(LDS_LIGHTS, NLIGHT) if sh[k] >= 1e-3]
    print(f"[many lights] stage {integrator}: image max {float(base[..., :3].max()):.4g}, {len(big)} lights beyond the table with share >= 1e-3 "
          f"carry {sh[big].sum():.4f}; {int((sh == 0).sum())} lights carry nothing")
    assert len(big) >= 10, sh
    assert sh[big].sum() >= 0.5, sh


@pytest.mark.parametrize("integrator", ["path", "direct"])
@pytest.mark.parametrize("scene_name,mat_name", [("chandelier", "cbox"), ("chandelier", "fd64"), ("stage", "rough")])
def test_the_oracles_forward_is_linear_in_each_emission(scene_name, integrator, mat_name, chandelier, stage):
    """I(row k doubled) - I(e) against I(row k tripled) - I(row k doubled), as <g, .>.  The bar is the image-sum bar of
    gpu_util.assert_image_parity, 1e-5 of <g, I>: the oracle sums a pixel's 16 float32 samples in float32, so each of the three images
    carries a rounding error of a few 1e-7 of its pixels, of either sign, and the sums over 2304 pixels stay far below that."""
    A, S = chandelier if scene_name == "chandelier" else stage
    mat = stage_material() if scene_name == "stage" else material(mat_name)
    p = params(integrator, CBOX_CAMERA if scene_name == "chandelier" else CAMERA, mat.shape[:2])
    g = cotangent(OW, OW, 1)
    rows = light_rows(A.inst_emission)
    some = [rows[0], rows[LDS_LIGHTS], rows[-1]] if scene_name == "chandelier" else [rows[16], rows[22], rows[29]]      # three of the four test_gpu_lightstage.py keeps
    t2, base = oracle_terms(S, p, mat, A.inst_emission, g, rows=some, factor=2.0)
    t3, _ = oracle_terms(S, p, mat, A.inst_emission, g, rows=some, factor=3.0)
    total = float((g[..., :3].astype(np.float64) * base[..., :3]).sum())
    worst = 0.0
    for k in some:
        first, second = t2[k], t3[k] - t2[k]
        worst = max(worst, float(np.abs(first - second).max()) / total)
        assert np.abs(first - second).max() <= 1e-5 * total, (k, first, second, total)
    assert np.abs(t2[some]).sum() > 0
    print(f"[many lights] {scene_name} {integrator} {mat_name}: linear to {worst:.3e} of <g, I>")
