#!/usr/bin/env python3
"""Inverse lighting in texture space with zdr_amd: recover the emissions of two panel lights — and with --env a small environment map —
from a baked irradiance map, before any path tracing (README, "Texture-space lighting", "Gradients").

    python examples/fit_lights.py --tex 64 --spp 16 --iters 200 [--env [--bounces K]]

A floor panel lies under two small emitting panels of different colour (with --env also under a sky with a warm spot).  The target is
``scene.texel_lighting(...)``'s irradiance with the KNOWN emissions (and map).  The fit starts from grey lights (and a grey map) and runs
Adam on

    sum coverage * |irradiance(E, env) - target|^2 / sum coverage

with ``irradiance = scene.texel_lighting(material, spp=..., texels=texels, emissions=E, envmap=env).irradiance``: one bake and its adjoint
per step, with the seed, the light list, the sampling tables and visibility held fixed, so the map from (E, env) to the irradiance is
linear and the loss a quadratic.  The loss is printed per iteration.

With --env --bounces K a white wall stands beside the floor, and the target and the model become the irradiance that arrives directly
PLUS the one that arrives after 1 .. K Lambertian bounces, ``texel_lighting(...).irradiance + texel_bounce([floor, wall], bounces=K,
...).irradiance``, both given ``envmap=``: the sky is then fitted to the light the wall throws onto the floor as well (README, "Bounced
light", "Gradients").  The lights' emissions are fitted through the direct term alone."""
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


def scene_arrays(wall=False):
    """instance 0: the floor, [-1, 1]^2 facing up; instances 1 and 2: two panels facing down at it; ``wall``: instance 3, a wall that
    stands at x = -1 and faces the floor (+x)"""
    fv, ft = panel_mesh(4, 4)
    lv, lt = panel_mesh(1, 1)
    down = lambda s, x, y, z: np.array([[s, 0, 0, x], [0, -1, 0, y], [0, 0, -s, z], [0, 0, 0, 1]], np.float32).reshape(16)
    xforms = [np.eye(4, dtype=np.float32).reshape(16), down(0.3, -0.4, 0.8, -0.3), down(0.25, 0.5, 0.6, 0.4)]
    emission = ((0.0, 0.0, 0.0),) + EMISSIONS
    nf, nl = fv.shape[0], lv.shape[0]
    verts, tris = [fv, lv, lv], [ft, lt + nf, lt + nf + nl]
    begin = [0, ft.shape[0], ft.shape[0] + lt.shape[0], ft.shape[0] + 2 * lt.shape[0]]
    if wall:                                                         # the panel's +y (its front) turned to +x: x' = y - 1, y' = 1 - x, z' = z
        xforms.append(np.array([[0, 1, 0, -1], [-1, 0, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32).reshape(16))
        emission += ((0.0, 0.0, 0.0),)
        verts.append(lv); tris.append(lt + nf + 2 * nl); begin.append(begin[-1] + lt.shape[0])
    return geometry.from_arrays(np.concatenate(verts), np.concatenate(tris), begin, np.stack(xforms), np.array(emission, np.float32))


def target_map(h=8):
    """an (h, 2h, 3) sky: blue towards the zenith, a warm spot"""
    v, u = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(2 * h) + 0.5) / (2 * h), indexing="ij")
    sky = np.stack([0.3 + 0.2 * v, 0.5 + 0.1 * v, 1.0 - 0.5 * v], -1)
    spot = np.exp(-(((u - 0.3) / 0.08) ** 2 + ((v - 0.25) / 0.12) ** 2))[..., None] * np.array([6.0, 4.0, 2.0])
    return np.ascontiguousarray(sky + spot, np.float32)


def run(tex=64, spp=16, iters=200, lr=0.5, env=False, seed=0, verbose=True, bounces=None):
    if bounces is not None and not env:
        raise ValueError("--bounces fits the sky through the bounced light: it needs --env")
    scene = Scene(scene_arrays(wall=bounces is not None), integrator="direct")
    material = torch.full((tex, tex, 4), 0.5, device="cuda")
    if bounces is not None:                                          # the floor's material and the wall's, a white one
        wall = torch.full((4, 4, 4), 0.9, device="cuda")
        scene.material_slots = (0, None, None, 1)
        texels = scene.texel_aovs([material, wall], 0)
    else:
        texels = scene.texel_aovs(material)                          # geometry only: once
    coverage = texels.coverage[..., None]
    ninst = scene.inst_count
    true_e = torch.tensor((((0.0, 0.0, 0.0),) + EMISSIONS + ((0.0, 0.0, 0.0),))[:ninst], device="cuda")
    true_map = torch.from_numpy(target_map()).cuda()
    E = torch.full((ninst, 3), 5.0, device="cuda", requires_grad=True)    # (the rows of the floor and the wall are not a light's: ignored, gradient 0)
    params = [{"params": [E]}]
    sky = None
    if env:
        sky = torch.full_like(true_map, 0.5).requires_grad_(True)
        scene.add_envmap(sky.detach())                               # the sampling tables of the grey start: held fixed throughout
        params.append({"params": [sky], "lr": 0.1 * lr})             # radiances of order 1 against emissions of order 10
    if bounces is None:
        bake = lambda e, m: scene.texel_lighting(material, spp=spp, seed=seed, texels=texels, emissions=e, envmap=m).irradiance
    else:                                                            # direct + bounced: the second call finds the first one's emissions in the scene
        bake = lambda e, m: (scene.texel_lighting([material, wall], 0, spp=spp, seed=seed, texels=texels, emissions=e, envmap=m).irradiance
                             + scene.texel_bounce([material, wall], 0, spp=spp, bounces=bounces, seed=seed, texels=texels, envmap=m).irradiance)
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
    ap.add_argument("--bounces", type=int, default=None, help="with --env: add a wall and fit direct + bounced irradiance with this many bounces")
    args = ap.parse_args()
    run(tex=args.tex, spp=args.spp, iters=args.iters, lr=args.lr, env=args.env, bounces=args.bounces)


if __name__ == "__main__":
    main()
