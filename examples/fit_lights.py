#!/usr/bin/env python3
"""Inverse lighting in texture space with zdr_amd: recover the emissions of two panel lights — and with --env a small environment map —
from a baked irradiance map, before any path tracing (README, "Texture-space lighting", "Gradients").

    python examples/fit_lights.py --tex 64 --spp 16 --iters 200 [--env]

A floor panel lies under two small emitting panels of different colour (with --env also under a sky with a warm spot).  The target is
``scene.texel_lighting(...)``'s irradiance with the KNOWN emissions (and map).  The fit starts from grey lights (and a grey map) and runs
Adam on

    sum coverage * |irradiance(E, env) - target|^2 / sum coverage

with ``irradiance = scene.texel_lighting(material, spp=..., texels=texels, emissions=E, envmap=env).irradiance``: one bake and its adjoint
per step, with the seed, the light list, the sampling tables and visibility held fixed, so the map from (E, env) to the irradiance is
linear and the loss a quadratic.  The loss is printed per iteration."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from zdr_amd import Scene, geometry
from zdr_amd.scenes import panel_mesh

EMISSIONS = ((17.0, 12.0, 4.0), (3.0, 9.0, 14.0))


def scene_arrays():
    """instance 0: the floor, [-1, 1]^2 facing up; instances 1 and 2: two panels facing down at it"""
    fv, ft = panel_mesh(4, 4)
    lv, lt = panel_mesh(1, 1)
    down = lambda s, x, y, z: np.array([[s, 0, 0, x], [0, -1, 0, y], [0, 0, -s, z], [0, 0, 0, 1]], np.float32).reshape(16)
    xforms = np.stack([np.eye(4, dtype=np.float32).reshape(16), down(0.3, -0.4, 0.8, -0.3), down(0.25, 0.5, 0.6, 0.4)])
    emission = np.array(((0.0, 0.0, 0.0),) + EMISSIONS, np.float32)
    nf = fv.shape[0]
    return geometry.from_arrays(np.concatenate([fv, lv, lv]), np.concatenate([ft, lt + nf, lt + nf + lv.shape[0]]),
                                [0, ft.shape[0], ft.shape[0] + lt.shape[0], ft.shape[0] + 2 * lt.shape[0]], xforms, emission)


def target_map(h=8):
    """an (h, 2h, 3) sky: blue towards the zenith, a warm spot"""
    v, u = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(2 * h) + 0.5) / (2 * h), indexing="ij")
    sky = np.stack([0.3 + 0.2 * v, 0.5 + 0.1 * v, 1.0 - 0.5 * v], -1)
    spot = np.exp(-(((u - 0.3) / 0.08) ** 2 + ((v - 0.25) / 0.12) ** 2))[..., None] * np.array([6.0, 4.0, 2.0])
    return np.ascontiguousarray(sky + spot, np.float32)


def run(tex=64, spp=16, iters=200, lr=0.5, env=False, seed=0, verbose=True):
    scene = Scene(scene_arrays(), integrator="direct")
    material = torch.full((tex, tex, 4), 0.5, device="cuda")
    texels = scene.texel_aovs(material)                              # geometry only: once
    coverage = texels.coverage[..., None]
    true_e = torch.tensor(((0.0, 0.0, 0.0),) + EMISSIONS, device="cuda")
    true_map = torch.from_numpy(target_map()).cuda()
    E = torch.full((3, 3), 5.0, device="cuda", requires_grad=True)    # (the floor's row is not a light's: ignored, gradient 0)
    params = [{"params": [E]}]
    sky = None
    if env:
        sky = torch.full_like(true_map, 0.5).requires_grad_(True)
        scene.add_envmap(sky.detach())                               # the sampling tables of the grey start: held fixed throughout
        params.append({"params": [sky], "lr": 0.1 * lr})             # radiances of order 1 against emissions of order 10
    bake = lambda e, m: scene.texel_lighting(material, spp=spp, seed=seed, texels=texels, emissions=e, envmap=m).irradiance
    with torch.no_grad():
        target = bake(true_e, true_map if env else None).clone()
    opt = torch.optim.Adam(params, lr=lr)
    losses = []
    for it in range(iters):
        opt.zero_grad()
        loss = (coverage * (bake(E, sky) - target).square()).sum() / coverage.sum().clamp_min(1.0)
        loss.backward()
        opt.step()
        with torch.no_grad():                                        # a light keeps a positive component, the map stays a radiance
            E.clamp_(min=1e-3)
            if env:
                sky.clamp_(min=0.0)
        losses.append(float(loss.detach()))
        if verbose:
            print(f"iteration {it:4d}  loss {losses[-1]:.6e}", flush=True)
    if verbose:
        print("emissions: fitted " + ", ".join("(" + ", ".join(f"{c:.2f}" for c in row) + ")" for row in E.detach()[1:].tolist())
              + "  true " + ", ".join(str(e) for e in EMISSIONS))
        if env:
            print(f"map: mean |fitted - true| {float((sky.detach() - true_map).abs().mean()):.4f} (mean of the true map {float(true_map.mean()):.4f})")
    scene.check()
    return losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tex", type=int, default=64)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.5)
    ap.add_argument("--env", action="store_true", help="also fit a small environment map")
    args = ap.parse_args()
    run(tex=args.tex, spp=args.spp, iters=args.iters, lr=args.lr, env=args.env)


if __name__ == "__main__":
    main()
