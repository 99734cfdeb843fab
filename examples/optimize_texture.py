#!/usr/bin/env python3
"""Inverse rendering with zdr_amd: recover the Cornell box's diffuse / roughness texture from a rendered target by gradient
descent — the workflow of the reference's example.py (render a ground truth, start from a random material, Adam on the
image loss through scene.render's PRB backward), on the assets this repository ships.

    python examples/optimize_texture.py --iters 200 --res 256 --spp 16 --out /tmp/zdr_example

--albedo-smoothness W adds W times a screen-space smoothness prior on the albedo the camera sees (scene.render_aovs: the first-hit
albedo buffer of the same camera samples, differentiable in the material; neighbours on another model or on the background do not count).
--denoise puts the feature-guided denoiser between the step's render and the loss (scene.render_denoised): the L1 loss of a noisy
render is a biased estimate of the loss of the converged image, the filtered render's less so.
--texel-prior W adds W times a smoothness prior in TEXTURE space that stops at chart borders: the mean over the covered texels of
|material - denoise(material, guides)|, the guides being scene.texel_aovs(material).as_guides() — the per-texel normal and instance
of the surface the texel lies on (seam padding included: texels that a lookup reaches take part).
--mask-unreached writes texture_diffuse.png with the texels that no lookup can ever read (reach 0: they never receive gradient and
stay random noise) black.
--fill-unreached writes texture_diffuse.png with every texel that lies on no model (coverage 0: the padding ring of each chart, which
gets only the bilinear spill of its neighbours' gradient, and the texels nothing reaches) filled from the covered texels by push-pull
(zdr_amd.push_pull): the covered texels stay as they are.  It takes precedence over --mask-unreached for the texels it fills.
--fill-param optimises theta with material = push_pull(theta, coverage): the holes are always the smooth continuation of their chart,
and the gradient that spills onto them is carried back to the covered texels (theta.grad is 0 elsewhere).
--save-lighting writes irradiance.png and openness.png, the texture-space lighting of the material (scene.texel_lighting: direct
irradiance and the open fraction of the hemisphere per texel), and prints the share of the reached texels that no light sample reached:
a texel in shadow gets only noise for a gradient, whatever its reach.
--init-from-target starts from the target photograph instead of from noise: the target is projected into texture space through the
camera (scene.texel_project) and divided by the direct irradiance of scene.texel_lighting — albedo = pi * color / irradiance, a
Lambertian guess that ignores indirect light — on the texels the camera sees and a light sample reached; every other texel is filled
from those by push-pull.  Roughness starts as it would have.  Prints the share of the reached texels that the camera sees and the
first iteration's loss.  --project-filter mip prefilters the photograph for that projection (a mip pyramid, the level taken from each
texel's on-screen size: scene.texel_project(..., filter="mip")), so that a texel that covers many pixels reads their mean, not one;
--project-filter aniso takes the level from the short axis of each texel's on-screen ellipse and averages probes along the long one
(filter="aniso"), which does not over-blur the walls seen at a grazing angle; --footprint-patch uv lets that ellipse follow the UV
mapping (the texel as the parallelogram of its UV tangents: scene.texel_project(..., footprint_patch="uv")) where a texture is not
square or a chart is stretched.
--init-bounces K (with --init-from-target) divides by the direct PLUS the bounced irradiance instead: albedo = pi * color / (direct +
bounced(albedo)), the bounced term being scene.texel_bounce with K Lambertian bounces.  It depends on the albedo, so the division is
iterated --init-rounds J times from a grey albedo.  With --save-lighting it also writes bounced.png and prints the share of the reached
texels without any light before and after the bounced term.
"""
import argparse
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
from PIL import Image

from zdr_amd import Camera, Scene, denoise as zdr_denoise, float3, push_pull

ASSETS = os.path.join(ROOT, "tests", "golden", "assets")


def load_material(diffuse_file, roughness_file):
    d = np.asarray(Image.open(diffuse_file))[..., :3]
    r = np.asarray(Image.open(roughness_file))[..., :1]
    return torch.from_numpy(np.ascontiguousarray((np.concatenate([d, r], -1).astype(np.float32) / 255.0) ** 2.2)).cuda()


def save_png(path, img):
    Image.fromarray((img[..., :3].clamp(0, 1) ** 0.454 * 255).to(torch.uint8).cpu().numpy()).save(path)


def albedo_smoothness_loss(f):
    """Mean absolute difference of the albedo of neighbouring pixels that see the same model (f: zdr_amd.Aovs)."""
    albedo = f.albedo / f.coverage.clamp_min(1e-6)[..., None]                              # the buffers are premultiplied by coverage
    inst, seen = f.instance.detach(), f.coverage.detach() > 0
    dx = (albedo[:, 1:] - albedo[:, :-1]).abs().sum(-1) * (seen[:, 1:] & seen[:, :-1] & (inst[:, 1:] == inst[:, :-1]))
    dy = (albedo[1:] - albedo[:-1]).abs().sum(-1) * (seen[1:] & seen[:-1] & (inst[1:] == inst[:-1]))
    return dx.mean() + dy.mean()


def texel_prior_loss(material, f, guides):
    """Mean over the covered texels of |material - its chart-aware filter| (f: zdr_amd.TexelAovs, guides: f.as_guides())."""
    smooth = zdr_denoise(material, guides, demodulate=False, sigma_depth=0, sigma_albedo=0)
    covered = f.coverage > 0
    return ((material - smooth).abs().sum(-1) * covered).sum() / covered.sum().clamp_min(1)


def run(iters=200, res=256, spp=16, tex=256, out=None, integrator="path", seed=0, verbose=True, albedo_smoothness=0.0, denoise=False,
        texel_prior=0.0, mask_unreached=False, save_lighting=False, fill_unreached=False, fill_param=False, init_from_target=False,
        project_filter="bilinear", footprint_patch="square", init_bounces=0, init_rounds=2):
    scene = Scene([(os.path.join(ASSETS, "cboxuv.obj"), None, float3(0.0)),
                   (os.path.join(ASSETS, "cbox-light.obj"), None, float3(17, 12, 4))], integrator=integrator)
    scene.camera = Camera(fov=50 / 180 * 3.1415926, origin=float3(-0.2, 2.6, 6.0), target=float3(-0.2, 2.6, -2.5), up=float3(0.0, 1.0, 0.0))
    material_gt = load_material(os.path.join(ASSETS, "cboxd.png"), os.path.join(ASSETS, "cboxr.png"))
    image_gt = scene.render(material_gt, res=(res, res), spp=max(256, 4 * spp))          # seed defaults to 0
    rng = random.Random(seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    theta = torch.rand((tex, tex, 4), device="cuda", generator=g).requires_grad_()
    opt = torch.optim.Adam([theta], lr=0.02)
    losses = []
    texels = scene.texel_aovs(theta.detach(), tangents=footprint_patch == "uv") if (texel_prior > 0.0 or mask_unreached or save_lighting or fill_unreached or fill_param or init_from_target) else None   # geometry only: once
    guides = texels.as_guides() if texel_prior > 0.0 else None
    if init_from_target:
        with torch.no_grad():
            photo = scene.texel_project([(scene.camera, image_gt)], theta.detach(), texels=texels, filter=project_filter, footprint_patch=footprint_patch)
            irradiance = scene.texel_lighting(theta.detach(), spp=max(64, spp), texels=texels).irradiance
            albedo = theta.detach().clone()
            albedo[..., :3] = 0.5                                  # the bounced light depends on the albedo: start grey, iterate
            for _ in range(max(int(init_rounds), 1) if init_bounces > 0 else 1):
                total = irradiance if init_bounces <= 0 else irradiance + scene.texel_bounce(albedo, spp=max(64, spp), bounces=init_bounces, texels=texels).irradiance
                known = (photo.weight > 0) & (total.sum(-1) > 0)
                guess = torch.zeros_like(theta)
                guess[..., :3] = (math.pi * photo.color[..., :3] / total.clamp_min(1e-8)).clamp(1e-3, 1.0)
                albedo[..., :3] = push_pull(guess, known)[..., :3].clamp(1e-3, 1.0)
            theta[..., :3] = albedo[..., :3]
            reached = texels.reach == 1
            if verbose:
                print(f"initialised from the target: the camera sees {int((reached & (photo.weight > 0)).sum())} of {int(reached.sum())} reached texels "
                      f"({float((reached & (photo.weight > 0)).sum()) / max(int(reached.sum()), 1):.1%}); {int(known.sum())} of them were lit", flush=True)
    material = theta
    for it in range(iters):
        opt.zero_grad()
        if fill_param:
            material = push_pull(theta, texels.coverage)
        step_seed = rng.randint(0, 2147483646)
        image = (scene.render_denoised if denoise else scene.render)(material, res=(res, res), spp=spp, seed=step_seed)
        loss = (image[..., :3] - image_gt[..., :3]).abs().mean()
        if albedo_smoothness > 0.0:
            loss = loss + albedo_smoothness * albedo_smoothness_loss(scene.render_aovs(material, res=(res, res), spp=spp, seed=step_seed))
        if texel_prior > 0.0:
            loss = loss + texel_prior * texel_prior_loss(material, texels, guides)
        loss.backward()
        opt.step()
        with torch.no_grad():
            theta.clamp_(1e-3, 1.0)                                                        # roughness / albedo stay physical
        losses.append(float(loss))
        if verbose and (it % 20 == 0 or it == iters - 1):
            print(f"iteration {it:4d}  L1 image loss {losses[-1]:.5f}", flush=True)
    if init_from_target and verbose and losses:
        print(f"first iteration's loss after the initialisation from the target: {losses[0]:.5f}", flush=True)
    material = push_pull(theta.detach(), texels.coverage) if fill_param else theta.detach()   # (a convex combination: stays within the clamp)
    if save_lighting:                                              # printed with or without --out; the images need it
        light = scene.texel_lighting(material.detach(), spp=max(64, spp), texels=texels)
        reached = texels.reach == 1
        unlit = reached & (light.irradiance.sum(-1) == 0)
        if verbose:
            print(f"texture-space lighting: {int(unlit.sum())} of {int(reached.sum())} reached texels ({float(unlit.sum()) / max(int(reached.sum()), 1):.1%}) "
                  "were reached by no light sample")
        bounce = scene.texel_bounce(material.detach(), spp=max(64, spp), bounces=init_bounces, texels=texels) if init_bounces > 0 else None
        if bounce is not None and verbose:
            dark = unlit & (bounce.irradiance.sum(-1) == 0)
            print(f"with {init_bounces} bounces: {int(dark.sum())} of {int(reached.sum())} reached texels ({float(dark.sum()) / max(int(reached.sum()), 1):.1%}) "
                  f"receive no light at all (before the bounced term: {float(unlit.sum()) / max(int(reached.sum()), 1):.1%})")
    if out:
        os.makedirs(out, exist_ok=True)
        save_png(os.path.join(out, "target.png"), image_gt)
        save_png(os.path.join(out, "result.png"), scene.render(material.detach(), res=(res, res), spp=max(256, 4 * spp)))
        if fill_unreached:
            save_png(os.path.join(out, "texture_diffuse.png"), texels.fill(material))
        else:
            save_png(os.path.join(out, "texture_diffuse.png"), material * (texels.reach[..., None] if mask_unreached else 1.0))
        if save_lighting:
            save_png(os.path.join(out, "irradiance.png"), light.irradiance / light.irradiance.max().clamp_min(1e-8))
            save_png(os.path.join(out, "openness.png"), light.openness[..., None].expand(-1, -1, 3))
            if bounce is not None:
                save_png(os.path.join(out, "bounced.png"), bounce.irradiance / light.irradiance.max().clamp_min(1e-8))
        duvdxy = scene.render_duvdxy(material.detach(), res=(res, res), spp=16)            # screen -> texture Jacobian (example.py)
        footprint = torch.det(duvdxy.reshape(res, res, 2, 2)).abs() * tex * tex
        Image.fromarray((footprint.clamp(0, 1) ** 0.454 * 255).to(torch.uint8).cpu().numpy()).save(os.path.join(out, "footprints.png"))
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--tex", type=int, default=256)
    ap.add_argument("--integrator", default="path")
    ap.add_argument("--out", default=None)
    ap.add_argument("--albedo-smoothness", type=float, default=0.0)
    ap.add_argument("--denoise", action="store_true")
    ap.add_argument("--texel-prior", type=float, default=0.0)
    ap.add_argument("--mask-unreached", action="store_true")
    ap.add_argument("--save-lighting", action="store_true")
    ap.add_argument("--fill-unreached", action="store_true")
    ap.add_argument("--fill-param", action="store_true")
    ap.add_argument("--init-from-target", action="store_true")
    ap.add_argument("--project-filter", choices=("bilinear", "mip", "aniso"), default="bilinear")
    ap.add_argument("--footprint-patch", choices=("square", "uv"), default="square")
    ap.add_argument("--init-bounces", type=int, default=0)
    ap.add_argument("--init-rounds", type=int, default=2)
    a = ap.parse_args()
    run(a.iters, a.res, a.spp, a.tex, a.out, a.integrator, albedo_smoothness=a.albedo_smoothness, denoise=a.denoise,
        texel_prior=a.texel_prior, mask_unreached=a.mask_unreached, save_lighting=a.save_lighting, fill_unreached=a.fill_unreached,
        fill_param=a.fill_param, init_from_target=a.init_from_target, project_filter=a.project_filter,
        footprint_patch=a.footprint_patch, init_bounces=a.init_bounces, init_rounds=a.init_rounds)
