"""Gradient of renders w.r.t. the environment map, the parts a machine without a GPU can check: the C-ABI (header, binding and
library agree on ABI 4 and export the new entry points), the environment-gradient kernels in the built code object and their
occupancy guards, and the torch-side preparation of the map that routes the gradient back to the caller's shape."""
import os
import re

import numpy as np
import pytest
import torch

from test_kernel_resources import LDS_BLOCK, kernels, waves_per_cu
from zdr_amd import _native, envmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("zdr_scene_set_envmap_texture", "zdr_render_backward_env", "zdr_render_backward_materials_env")


def header():
    return open(os.path.join(ROOT, "include", "zdr.h")).read()


def test_header_binding_and_library_agree_on_abi_4():
    h = int(re.search(r"#define ZDR_ABI_VERSION (\d+)", header()).group(1))
    assert h == 4 and _native.ABI_VERSION == 4
    assert _native.lib().zdr_abi_version() == 4


def test_the_environment_gradient_entry_points_are_declared_bound_and_exported():
    declared = set(re.findall(r"^int (zdr_\w+)\(", header(), re.M))
    lib = _native.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in declared and name in _native.EXPORTS, name
        getattr(lib, name)
    assert declared <= set(_native.EXPORTS)


# k_path_bwd<SK, A, ENV = true, MT = true, EG = true, LG = false> and k_simple<ZDR_DIRECT, SK, A, BWD = true, STATS = false, ENV, MT, EG = true, LG = false>
PATH_EG = r"k_path_bwdILi([01])E(10BruteAccel|8BvhAccel)Lb1ELb1ELb1ELb0EE"
DIRECT_EG = r"k_simpleILi1ELi([01])E(10BruteAccel|8BvhAccel)Lb1ELb0ELb1ELb1ELb1ELb0EE"


def test_environment_gradient_kernels_are_built_for_both_samplers_and_both_accels():
    names = list(kernels())
    for pattern in (PATH_EG, DIRECT_EG):
        got = {re.search(pattern, n).groups() for n in names if re.search(pattern, n)}
        assert got == {(sk, a) for sk in "01" for a in ("10BruteAccel", "8BvhAccel")}, (pattern, got)


def test_environment_gradient_path_kernels_keep_the_backward_budget():
    """The budget test_kernel_resources.py holds every k_path_bwd to: 128 VGPRs and 8 LDS blocks (BVH: with the traversal stack
    the launcher adds), 16 waves per CU for the brute-force kernel."""
    sel = {n: r for n, r in kernels().items() if re.search(PATH_EG, n)}
    assert len(sel) == 4
    for name, r in sel.items():
        assert r["vgpr_count"] <= 128, (name, r)
        if "BvhAccel" in name:
            assert r["group_segment_fixed_size"] + 10 * 256 <= 8 * LDS_BLOCK, (name, r)
        else:
            assert r["group_segment_fixed_size"] <= 8 * LDS_BLOCK, (name, r)
            assert waves_per_cu(r["group_segment_fixed_size"], r["vgpr_count"]) >= 16, (name, r)


def sky(h=3, c=3, seed=0):
    return np.random.default_rng(seed).uniform(0.1, 2.0, (h, 2 * h, c)).astype(np.float32)


@pytest.mark.parametrize("channels", [3, 4])
def test_torch_preparation_has_the_values_of_prepare_image(channels):
    img = sky(c=channels)
    got = envmap.prepare_tensor(torch.from_numpy(img))
    assert got.shape == (6, 6, 4)
    np.testing.assert_array_equal(got.numpy(), envmap.prepare_image(img))
    square = sky(h=4, c=channels)[:, :4]
    np.testing.assert_array_equal(envmap.prepare_tensor(torch.from_numpy(square)).numpy(), envmap.prepare_image(square))


def test_torch_preparation_routes_the_gradient_to_the_callers_shape():
    """1:2 RGB map: square row 2i and 2i + 1 are copies of row i, so row i receives the sum of their gradients; the alpha the
    preparation adds is a constant and sends nothing back."""
    env = torch.from_numpy(sky()).requires_grad_()
    g = torch.from_numpy(np.random.default_rng(1).normal(size=(6, 6, 4)).astype(np.float32))
    (envmap.prepare_tensor(env) * g).sum().backward()
    assert env.grad.shape == (3, 6, 3)
    np.testing.assert_allclose(env.grad.numpy(), (g[0::2, :, :3] + g[1::2, :, :3]).numpy(), rtol=0, atol=1e-6)
    # RGBA input: its alpha is the map's alpha and takes its gradient like the other channels
    env4 = torch.from_numpy(sky(c=4)).requires_grad_()
    (envmap.prepare_tensor(env4) * g).sum().backward()
    np.testing.assert_allclose(env4.grad.numpy(), (g[0::2] + g[1::2]).numpy(), rtol=0, atol=1e-6)


def test_torch_preparation_rejects_what_prepare_image_rejects():
    with pytest.raises(RuntimeError, match="1:2 or 1:1"):
        envmap.prepare_tensor(torch.zeros((10, 30, 3)))
    with pytest.raises(ValueError):
        envmap.prepare_tensor(torch.zeros((10, 20, 2)))
