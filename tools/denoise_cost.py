#!/usr/bin/env python3
"""What the denoiser costs next to the render it post-processes: denoise forward + adjoint (5 levels, zdr_denoise + zdr_denoise_backward)
against render_forward + render_backward of the Cornell box (path integrator) at spp 16, and against the same filter written as torch
operations on the GPU (tests/denoise_ref.py in float32, forward + autograd) — what there was before the kernels.
Same process, same box; the sides ALTERNATE round by round (other work shares the host), each round is `--reps` calls between two
device events, and the median, minimum and maximum over the rounds are reported.
    python tools/denoise_cost.py [--sizes 512,1024] [--rounds 7] [--reps 10] [--warmup 3] [--out profiles/denoise_cost.txt]
The expectation it tests: the filter's two passes cost less than the render's two passes at spp 16 (if not, doubling the spp buys more)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from denoise_ref import denoise_ref  # noqa: E402
from zdr_amd.denoiser import denoise_backward, denoise_forward, workspace_bytes  # noqa: E402
from zdr_amd.scenes import cbox_material_np, make_scene  # noqa: E402

LEVELS, SPP = 5, 16
SIGMAS = dict(sigma_normal=0.25, sigma_depth=0.1, sigma_albedo=0.1)


def window(fn, reps):
    """ms per call of `reps` calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m = torch.from_numpy(cbox_material_np()).cuda()
    scene = make_scene("path")
    lines, out = [], {}
    for W in (int(s) for s in args.sizes.split(",")):
        img = torch.zeros((W, W, 4), device="cuda"); cot = torch.ones((W, W, 4), device="cuda"); g = torch.zeros_like(m)
        scene.render_forward(m, (W, W), SPP, 0, out=img)
        aovs = scene.render_aovs_forward(m, (W, W), SPP, 0)
        den, d_img = torch.empty_like(img), torch.empty_like(img)
        ws = torch.empty(workspace_bytes((W, W), LEVELS), dtype=torch.uint8, device="cuda")

        def filt():
            denoise_forward(img, aovs, levels=LEVELS, out=den, workspace=ws, **SIGMAS)
            denoise_backward(cot, aovs, levels=LEVELS, d_image=d_img, workspace=ws, **SIGMAS)

        def render():
            scene.render_forward(m, (W, W), SPP, 0, out=img)
            scene.render_backward(cot, g, m, (W, W), SPP, 0)

        def torch_ops():
            x = img.detach().clone().requires_grad_()
            denoise_ref(x, aovs, LEVELS, SIGMAS["sigma_normal"], SIGMAS["sigma_depth"], SIGMAS["sigma_albedo"], dtype=torch.float32).backward(cot)

        for _ in range(args.warmup):
            filt(); render()
        torch_ops()
        torch.cuda.synchronize()
        t = {"denoise": [], "render": [], "torch_ops": []}
        for _ in range(args.rounds):
            t["denoise"].append(window(filt, args.reps)); t["render"].append(window(render, args.reps)); t["torch_ops"].append(window(torch_ops, args.torch_reps))
        st = {k: stats(v) for k, v in t.items()}
        out[str(W)] = dict(st, levels=LEVELS, spp=SPP, denoise_over_render=st["denoise"]["median_ms"] / st["render"]["median_ms"],
                           torch_ops_over_denoise=st["torch_ops"]["median_ms"] / st["denoise"]["median_ms"])
        lines.append(f"cbox {W}^2: denoise fwd+adjoint L={LEVELS} {st['denoise']['median_ms']:8.3f} ms [{st['denoise']['min_ms']:.3f}, {st['denoise']['max_ms']:.3f}]   "
                     f"render fwd+bwd spp {SPP} {st['render']['median_ms']:8.3f} ms [{st['render']['min_ms']:.3f}, {st['render']['max_ms']:.3f}]   "
                     f"ratio {out[str(W)]['denoise_over_render']:.4f}   torch ops fwd+autograd {st['torch_ops']['median_ms']:8.3f} ms "
                     f"[{st['torch_ops']['min_ms']:.3f}, {st['torch_ops']['max_ms']:.3f}] = {out[str(W)]['torch_ops_over_denoise']:.1f} x the kernels")
        print(lines[-1], flush=True)
        scene.check()
    lines.append(json.dumps(out))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"tools/denoise_cost.py --sizes {args.sizes} --rounds {args.rounds} --reps {args.reps} on {torch.cuda.get_device_name(0)}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
