"""Gradient of renders w.r.t. the lights' emissions, the parts a machine without a GPU can check: the C-ABI (header, binding and
library still agree on ABI 4 and declare, bind and export the new entry points), the emission-gradient kernels in the built code
object and their occupancy guards, and the argument checks of ``render(..., emissions=)`` that need no device."""
import os
import re

import pytest
import torch

from test_kernel_resources import LDS_BLOCK, kernels, waves_per_cu
from zdr_amd import _native, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("zdr_scene_set_emission_values", "zdr_render_backward_emission", "zdr_render_backward_materials_emission")


def header():
    return open(os.path.join(ROOT, "include", "zdr.h")).read()


def test_header_binding_and_library_still_agree_on_abi_4():
    h = int(re.search(r"#define ZDR_ABI_VERSION (\d+)", header()).group(1))
    assert h == 4 and _native.ABI_VERSION == 4
    assert _native.lib().zdr_abi_version() == 4


def test_the_emission_gradient_entry_points_are_declared_bound_and_exported():
    declared = set(re.findall(r"^int (zdr_\w+)\(", header(), re.M))
    lib = _native.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in declared and name in _native.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert declared <= set(_native.EXPORTS)


# k_path_bwd<SK, A, ENV, MT = true, EG = false, LG = true> and k_simple<ZDR_DIRECT, SK, A, BWD = true, STATS = false, ENV, MT = true, EG = false, LG = true>
PATH_LG = r"k_path_bwdILi([01])E(10BruteAccel|8BvhAccel)Lb([01])ELb1ELb0ELb1EE"
DIRECT_LG = r"k_simpleILi1ELi([01])E(10BruteAccel|8BvhAccel)Lb1ELb0ELb([01])ELb1ELb0ELb1EE"


def test_emission_gradient_kernels_are_built_for_both_samplers_both_accels_with_and_without_environment():
    names = list(kernels())
    for pattern in (PATH_LG, DIRECT_LG):
        got = {re.search(pattern, n).groups() for n in names if re.search(pattern, n)}
        assert got == {(sk, a, env) for sk in "01" for a in ("10BruteAccel", "8BvhAccel") for env in "01"}, (pattern, got)


def test_emission_gradient_path_kernels_keep_the_backward_budget():
    """The budget test_kernel_resources.py holds every k_path_bwd to: 128 VGPRs and 8 LDS blocks (BVH: with the traversal stack
    the launcher adds), 16 waves per CU for the brute-force kernel."""
    sel = {n: r for n, r in kernels().items() if re.search(PATH_LG, n)}
    assert len(sel) == 8
    for name, r in sel.items():
        print(name, r)
        assert r["vgpr_count"] <= 128, (name, r)
        if "BvhAccel" in name:
            assert r["group_segment_fixed_size"] + 10 * 256 <= 8 * LDS_BLOCK, (name, r)
        else:
            assert r["group_segment_fixed_size"] <= 8 * LDS_BLOCK, (name, r)
            assert waves_per_cu(r["group_segment_fixed_size"], r["vgpr_count"]) >= 16, (name, r)


def test_emissions_argument_is_checked_without_a_device():
    cpu = torch.device("cpu")
    ok = torch.zeros((3, 3))
    assert render.check_emissions(ok, 3, cpu) is ok
    for bad in (torch.zeros((2, 3)), torch.zeros((3, 4)), torch.zeros(9), torch.zeros((3, 3), dtype=torch.float64), [[0.0, 0.0, 0.0]] * 3):
        with pytest.raises(ValueError):
            render.check_emissions(bad, 3, cpu)
    with pytest.raises(ValueError, match="float32 tensor on cuda:0"):     # a host tensor for a scene on the GPU
        render.check_emissions(ok, 3, torch.device("cuda", 0))
    with pytest.raises(ValueError, match="envmap"):
        render.check_emissions(ok, 3, cpu, envmap=torch.zeros((4, 8, 3)))


def test_a_snapshot_of_emission_values_is_a_list_update_lights_takes_back():
    base = [None, 20.0, (6, 2, 1)]
    snap = render.EmissionValues(base, torch.zeros((3, 3)))
    assert list(snap) == base and len(snap) == 3 and snap.values.shape == (3, 3)
    assert render.default_material_slots(snap) == render.default_material_slots(base) == (0, None, None)
