#!/usr/bin/env python3
"""Pose refinement with zdr_amd: recover a camera that is off by a few pixels from a photograph, in texture space (README, "Camera
gradients").

    python examples/refine_camera.py --res 256 --tex 256 --iters 60

A photograph of the Cornell box is rendered from the TRUE camera and baked into texture space through it (``view.gather``): that bake
is theta, what a registered photograph of the same surface would have left in the texture.  The camera's origin and target are then
perturbed, and Adam recovers them on

    sum view.weight() * |view.gather(photo, filter="mip", footprint=F) - theta|^2 / sum view.weight()

with ``view = scene.texel_view(theta, res=..., camera=tensor)`` made anew each step from the camera TENSOR (10 float32 values on the
CPU: fov, origin, target, up; fov and up are held).  F is stepped 8 -> 4 -> 2 -> 1: a trilinear sample with a large footprint has a
useful gradient over many pixels, a bilinear one over a single pixel, so the coarse stages find the basin and the fine ones the pose.
Visibility is held fixed in the gradient (the interior derivative), and each backward copies 40 bytes to the host: one synchronisation
per step.  The pose error is printed per stage."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
from PIL import Image

from zdr_amd import Camera, Scene, float3

ASSETS = os.path.join(ROOT, "tests", "golden", "assets")
STAGES = (8.0, 4.0, 2.0, 1.0)


def load_material(diffuse_file, roughness_file):
    d = np.asarray(Image.open(diffuse_file))[..., :3]
    r = np.asarray(Image.open(roughness_file))[..., :1]
    return torch.from_numpy(np.ascontiguousarray((np.concatenate([d, r], -1).astype(np.float32) / 255.0) ** 2.2)).cuda()


def pose_error(cam, true):
    d = (cam.detach() - true).double()
    return float(d[1:4].norm()), float(d[4:7].norm())


def pixel_error(scene, material, texels, res, cam, true_view):
    """mean distance in pixels between where the camera puts a texel and where the true camera puts it, over the texels the true one sees:
    what smears a projected texture.  (Origin and target are not determined separately: the target may slide along the axis.)"""
    with torch.no_grad():
        view = scene.texel_view(material, res=(res, res), camera=cam.detach(), texels=texels)
        seen = true_view.visible > 0
        return float((view.pixel - true_view.pixel).norm(dim=-1)[seen].mean())


def run(res=256, tex=256, spp=64, iters=60, lr=0.004, shift=(0.12, -0.08, 0.1), aim=(-0.1, 0.06, 0.0), verbose=True):
    scene = Scene([(os.path.join(ASSETS, "cboxuv.obj"), None, float3(0.0)),
                   (os.path.join(ASSETS, "cbox-light.obj"), None, float3(17, 12, 4))], integrator="direct")
    true_camera = Camera(fov=50 / 180 * 3.1415926, origin=float3(-0.2, 2.6, 6.0), target=float3(-0.2, 2.6, -2.5), up=float3(0.0, 1.0, 0.0))
    scene.camera = true_camera
    material = load_material(os.path.join(ASSETS, "cboxd.png"), os.path.join(ASSETS, "cboxr.png"))
    if tex != material.shape[0]:
        material = torch.nn.functional.interpolate(material.permute(2, 0, 1)[None], size=(tex, tex), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).contiguous()
    photo = scene.render(material, res=(res, res), spp=spp).detach()
    texels = scene.texel_aovs(material)                              # geometry only: once
    true_view = scene.texel_view(material, res=(res, res), camera=true_camera, texels=texels)
    theta = true_view.gather(photo, filter="mip")
    true = true_camera.to_tensor()
    cam = true.clone()
    cam[1:4] += torch.tensor(shift); cam[4:7] += torch.tensor(aim)
    cam.requires_grad_()
    held = torch.zeros(10); held[1:7] = 1.0                          # fov and up are not refined
    history = [("start", *pose_error(cam, true), pixel_error(scene, material, texels, res, cam, true_view), float("nan"))]
    if verbose:
        print(f"perturbed pose: origin off by {history[0][1]:.4f}, target off by {history[0][2]:.4f} scene units; texels land {history[0][3]:.3f} pixels "
              f"from where the true camera puts them (mean over the texels it sees)", flush=True)
    for stage, footprint in enumerate(STAGES):
        opt = torch.optim.Adam([cam], lr=lr * 0.5 ** stage)          # Adam's step is about lr, whatever the gradient's size: halve it with the footprint
        for _ in range(iters):
            opt.zero_grad()
            view = scene.texel_view(material, res=(res, res), camera=cam, texels=texels)
            w = view.weight()
            loss = (w[..., None] * (view.gather(photo, filter="mip", footprint=footprint) - theta).square()).sum() / w.sum().detach().clamp_min(1.0)
            loss.backward()                                          # one synchronisation: 40 bytes to the host
            cam.grad *= held
            opt.step()
        history.append((f"footprint {footprint:g}", *pose_error(cam, true), pixel_error(scene, material, texels, res, cam, true_view), float(loss.detach())))
        if verbose:
            print(f"after {iters:3d} steps at footprint {footprint:g} (lr {lr * 0.5 ** stage:.5f}): origin off by {history[-1][1]:.5f}, target off by {history[-1][2]:.5f}, "
                  f"texels off by {history[-1][3]:.3f} pixels, loss {history[-1][4]:.3e}", flush=True)
    scene.check()
    return history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--tex", type=int, default=256)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--iters", type=int, default=60, help="Adam steps per footprint stage")
    ap.add_argument("--lr", type=float, default=0.004, help="Adam's step size of the first stage; halved from stage to stage")
    args = ap.parse_args()
    run(res=args.res, tex=args.tex, spp=args.spp, iters=args.iters, lr=args.lr)


if __name__ == "__main__":
    main()
