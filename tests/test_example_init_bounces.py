"""-m gpu: examples/optimize_texture.py --init-from-target --init-bounces runs — a 32^2 texture, a 64^2 render, spp 4, three Adam steps —
with finite losses, and the bounced term changes the start: the first iteration's loss differs from the one without it."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def load_example():
    spec = importlib.util.spec_from_file_location("optimize_texture", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "optimize_texture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_example_starts_from_the_target_with_the_bounced_term(tmp_path):
    ex = load_example()
    kw = dict(iters=3, res=64, spp=4, tex=32, init_from_target=True, verbose=False)
    plain = ex.run(**kw)
    bounced = ex.run(init_bounces=2, init_rounds=2, save_lighting=True, out=str(tmp_path), **kw)
    print(f"[init bounces] first iteration's loss {plain[0]:.4e} with the direct irradiance alone, {bounced[0]:.4e} with two bounces added")
    assert len(bounced) == 3 and np.isfinite(bounced).all() and np.isfinite(plain).all()
    assert bounced[0] > 0 and bounced[0] != plain[0]
    assert os.path.exists(os.path.join(str(tmp_path), "bounced.png"))
