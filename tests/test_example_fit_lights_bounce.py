"""-m gpu: examples/fit_lights.py --env --bounces 2 runs — a 16^2 texture, spp 8, 12 Adam steps: the sky is fitted to the direct plus
the bounced irradiance, both bakes given ``envmap=`` — and the loss falls.  The bounced term carries light and a gradient in the map.  No
bar on the recovered map."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def load_example():
    spec = importlib.util.spec_from_file_location("fit_lights", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "fit_lights.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_loss_falls_with_bounces():
    ex = load_example()
    losses = ex.run(tex=16, spp=8, iters=12, env=True, bounces=2, verbose=False)
    print(f"[fit_lights --env --bounces 2] loss {losses[0]:.4e} -> {losses[-1]:.4e}")
    assert len(losses) == 12 and all(l == l for l in losses)
    assert losses[-1] < 0.5 * losses[0]


def test_the_bounced_term_sees_the_map():
    """the wall throws light of the sky onto the floor: the bounced irradiance is positive and has a gradient in the map"""
    from zdr_amd import Scene
    ex = load_example()
    scene = Scene(ex.scene_arrays(wall=True), integrator="direct")
    scene.material_slots = (0, None, None, 1)
    mats = [torch.full((16, 16, 4), 0.5, device="cuda"), torch.full((4, 4, 4), 0.9, device="cuda")]
    sky = torch.from_numpy(ex.target_map()).cuda().requires_grad_(True)
    scene.add_envmap(sky.detach())
    irr = scene.texel_bounce(mats, 0, spp=8, bounces=2, envmap=sky).irradiance
    irr.sum().backward()
    torch.cuda.synchronize()
    print(f"[fit_lights --env --bounces 2] bounced irradiance: mean {float(irr.detach().mean()):.4e}; largest |d sky| {float(sky.grad.abs().max()):.4e}")
    assert float(irr.detach().sum()) > 0 and sky.grad.shape == sky.shape and float(sky.grad.abs().max()) > 0
    with pytest.raises(ValueError):
        ex.run(tex=16, spp=8, iters=1, env=False, bounces=2, verbose=False)
    scene.check()
