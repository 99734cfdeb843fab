#!/usr/bin/env python3
"""Inverse texturing in texture space WITH interreflection, with zdr_amd: recover the albedo of the Cornell box from a baked radiosity map,
before any path tracing (README, "Bounced light", "Gradients").

    python examples/fit_radiosity.py --tex 64 --spp 16 --bounces 2 --iters 200 [--emissions]

The target is the texel radiosity  a* / pi x (texel_lighting + texel_bounce(a*))  of a KNOWN albedo a*.  The fit starts from grey and
runs Adam on

    sum coverage * |a / pi x (direct + bounced(a)) - target|^2 / sum coverage

with ``bounced = scene.texel_bounce(material, spp=..., bounces=..., texels=texels).irradiance``: the albedo enters twice, once in front and
once through the bounce, and the second route is differentiated by the adjoint of the bounced-light baker.  The seed, the walks, the
light list and visibility are held fixed, so per step the bounced term is a polynomial in the texels and its gradient is exact.
``--emissions`` also fits the light's emission, from grey, through both bakers' ``emissions=``.  The loss is printed per iteration."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from zdr_amd.scenes import make_scene

EMISSION = 20.0          # the Cornell box's light (zdr_amd/scenes.py)


def true_albedo(tex):
    """a smooth pattern in [0.25, 0.85], another per channel; roughness 0.5"""
    v, u = torch.meshgrid((torch.arange(tex) + 0.5) / tex, (torch.arange(tex) + 0.5) / tex, indexing="ij")
    rgb = torch.stack([0.55 + 0.3 * torch.sin(7.0 * u) * torch.cos(5.0 * v), 0.55 + 0.3 * torch.cos(9.0 * u + 4.0 * v), 0.55 + 0.3 * torch.sin(6.0 * v - 3.0 * u)], -1)
    return torch.cat([rgb, torch.full((tex, tex, 1), 0.5)], -1).float().cuda().contiguous()


def run(tex=64, spp=16, bounces=2, iters=200, lr=0.02, emissions=False, seed=0, verbose=True):
    scene = make_scene("direct")                                     # model 0: the box, slot 0; model 1: the light
    truth = true_albedo(tex)
    texels = scene.texel_aovs(truth)                                 # geometry only: once
    coverage = texels.coverage[..., None]
    true_e = torch.tensor(((0.0, 0.0, 0.0), (EMISSION,) * 3), device="cuda")
    E = torch.full((2, 3), 8.0, device="cuda", requires_grad=True) if emissions else None

    def radiosity(material, e):
        direct = scene.texel_lighting(material, spp=spp, seed=seed, texels=texels, emissions=e).irradiance
        bounced = scene.texel_bounce(material, spp=spp, bounces=bounces, seed=seed, texels=texels, emissions=e).irradiance
        return material[..., :3] / math.pi * (direct + bounced)
    with torch.no_grad():
        target = radiosity(truth, true_e if emissions else None).clone()
    material = torch.cat([torch.full((tex, tex, 3), 0.5, device="cuda"), truth[..., 3:]], -1).requires_grad_(True)
    params = [{"params": [material]}]
    if emissions:
        params.append({"params": [E], "lr": 25.0 * lr})              # emissions of order 10 against albedos of order 1
    opt = torch.optim.Adam(params, lr=lr)
    losses = []
    for it in range(iters):
        opt.zero_grad()
        loss = (coverage * (radiosity(material, E) - target).square()).sum() / coverage.sum().clamp_min(1.0)
        loss.backward()
        opt.step()
        with torch.no_grad():                                        # an albedo stays one, a light keeps a positive component
            material[..., :3].clamp_(0.0, 1.0)
            if emissions:
                E.clamp_(min=1e-3)
        losses.append(float(loss.detach()))
        if verbose:
            print(f"iteration {it:4d}  loss {losses[-1]:.6e}", flush=True)
    if verbose:
        lit = (coverage[..., 0] > 0) & (target.sum(-1) > 0)
        err = (material.detach()[..., :3] - truth[..., :3]).abs()[lit].mean()
        print(f"albedo: mean |fitted - true| over the {int(lit.sum())} lit texels {float(err):.4f} (grey start: {float((0.5 - truth[..., :3]).abs()[lit].mean()):.4f})")
        if emissions:
            print("emission: fitted (" + ", ".join(f"{c:.2f}" for c in E.detach()[1].tolist()) + f")  true ({EMISSION:.2f}, {EMISSION:.2f}, {EMISSION:.2f})")
    scene.check()
    return losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tex", type=int, default=64)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=2)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--emissions", action="store_true", help="also fit the light's emission")
    args = ap.parse_args()
    run(tex=args.tex, spp=args.spp, bounces=args.bounces, iters=args.iters, lr=args.lr, emissions=args.emissions, seed=args.seed)


if __name__ == "__main__":
    main()
