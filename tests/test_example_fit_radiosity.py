"""-m gpu: examples/fit_radiosity.py runs — a 32^2 texture, spp 8, two bounces, 30 Adam steps, with and without --emissions — and ends with
a loss below its first iteration's: the gradient of Scene.texel_bounce in the materials (and the emissions) points downhill through the
autograd route."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def load_example():
    spec = importlib.util.spec_from_file_location("fit_radiosity", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "fit_radiosity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("emissions", [False, True])
def test_the_example_ends_with_a_loss_below_its_first(emissions):
    losses = load_example().run(tex=32, spp=8, bounces=2, iters=30, emissions=emissions, verbose=False)
    print(f"[fit radiosity] emissions {emissions}: loss {losses[0]:.4e} -> {losses[-1]:.4e} over {len(losses)} iterations")
    assert len(losses) == 30 and np.isfinite(losses).all() and losses[0] > 0
    assert losses[-1] < losses[0]
