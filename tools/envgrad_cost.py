#!/usr/bin/env python3
"""What the environment-map gradient costs: forward, backward and backward with d_env (zdr_render_backward_env) of one render call
(torch.cuda.Event around the call, as bench.py times), on
    cbox-sky    the Cornell box under a sun-and-sky map, path 512^2 spp 256 (brute force and BVH)
    env-only    the environment-only scene of tests/test_envmap.py (the floor alone, no mesh light): the camera rays that miss all
                land on a few texels per tile, the case where the scatter could pile its atomics onto a handful of cells
    c5-sky      c5 (1 M triangles, BVH) under the same map, path 1024^2 spp 256
    python tools/envgrad_cost.py [--configs cbox-sky,env-only,c5-sky] [--steps 5] [--warmup 2]
Prints one line per config and a JSON summary line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zdr_amd import envmap  # noqa: E402
from zdr_amd.scenes import cbox_material_np, cbox_models, fd_material_np, make_scene, tess1m_arrays  # noqa: E402
from material_cost import timed  # noqa: E402


def sun_sky(h=64, seed=0):
    """a sky of uniform noise with one small bright sun, (h, 2h, 3)"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.05, 0.6, (h, 2 * h, 3)).astype(np.float32)
    img[h // 6:h // 6 + 3, 5 * h // 4:5 * h // 4 + 4] = (300.0, 260.0, 200.0)
    return img


CONFIGS = {   # name: (scene factory, material, resolution, spp)
    "cbox-sky": (lambda: make_scene("path", accel="brute"), cbox_material_np, 512, 256),
    "cbox-sky-bvh": (lambda: make_scene("path", accel="bvh"), cbox_material_np, 512, 256),
    "env-only": (lambda: make_scene("path", models=[(cbox_models()[0][0], None, 0.0)]), lambda: fd_material_np(128, 1), 512, 256),
    "c5-sky": (lambda: make_scene("path", arrays=tess1m_arrays()), cbox_material_np, 1024, 256),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cbox-sky,cbox-sky-bvh,env-only,c5-sky")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sky", type=int, default=256, help="height of the 1:2 map (its square form is 2h x 2h)")
    args = ap.parse_args()
    out = {}
    for name in args.configs.split(","):
        make, mat_np, W, spp = CONFIGS[name]
        scene = make()
        scene.add_envmap(sun_sky(args.sky))
        m = torch.from_numpy(mat_np()).cuda()
        env = torch.from_numpy(envmap.prepare_image(sun_sky(args.sky))).cuda()
        img = torch.zeros((W, W, 4), device="cuda")
        cot = torch.ones((W, W, 4), device="cuda")
        g, d_env = torch.zeros_like(m), torch.zeros_like(env)
        fwd = timed(lambda: scene.render_forward(m, (W, W), spp, 0, out=img), args.steps, args.warmup)
        bwd = timed(lambda: scene.render_backward(cot, g, m, (W, W), spp, 0), args.steps, args.warmup)
        bwd_env = timed(lambda: scene.render_backward(cot, g, m, (W, W), spp, 0, d_env=d_env), args.steps, args.warmup)
        scene.check()
        print(f"{name:13s} {W}^2 spp {spp}  forward {fwd:8.3f} ms  backward {bwd:8.3f} ms  backward + d_env {bwd_env:8.3f} ms "
              f"({bwd_env / bwd - 1:+6.1%}; {bwd_env / fwd:4.2f} x forward, plain backward {bwd / fwd:4.2f} x)", flush=True)
        out[name] = {"forward_ms": fwd, "backward_ms": bwd, "backward_env_ms": bwd_env}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
