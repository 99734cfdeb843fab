#!/usr/bin/env python3
"""What the adjoint of the texture-space lighting costs: Scene.texel_lighting_backward against Scene.texel_lighting_forward with the same
arguments — the yardstick, code the adjoint does not touch.  Same process, same box; the two sides ALTERNATE round by round (other work
shares the host), each round is `--reps` calls between two device events, and the median, minimum and maximum over the rounds are
reported.
    python tools/texel_lighting_grad_cost.py [--workloads ...] [--rounds 7] [--reps 10] [--warmup 2] [--out profiles/texel_lighting_grad_cost.txt]
Workloads, all at 1024^2 texels and spp 16: the Cornell box (brute force) and the 1 M-triangle scene (BVH) with d_emission; the Cornell
geometry under a near-uniform sky and under a sun-and-sky map, both 256 x 512, with d_env.

Expectations, written down before any run.  Emission adjoint: at or below the forward, within the spread of the rounds — it draws the
same numbers and walks one any-hit ray per sample where the forward walks two.  Environment adjoint: at or below the forward plus the
float-atomic budget, the bytes actually added over 1.3 TB/s; the bytes are 48 (four taps x rgb x 4) per group of accepted environment
samples that goes to memory, counted by the kernel before and after its wave-level merge (words 1 and 2 of the workspace).  The sun map
must not cost more than the uniform sky by more than the difference of their budgets.  Prints one line per workload and a JSON summary
line; --out writes the same text to a file as well."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aov_cost import alternate, stats                                       # noqa: E402
from zdr_amd import _native as N                                            # noqa: E402
from zdr_amd.scenes import make_scene, tess1m_arrays                        # noqa: E402

ATOMIC_RATE = 1.3e12            # bytes of float atomic adds per second, chip-wide
GROUP_BYTES = 48                # four taps x rgb x 4 bytes


def uniform_sky(h=256):
    rng = np.random.default_rng(0)
    return (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (h, 2 * h, 3))).astype(np.float32)


def sun_sky(h=256):
    """a blue gradient and a sun of a few texels, about 35 degrees from the zenith, a few thousand times the sky"""
    v, u = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(2 * h) + 0.5) / (2 * h), indexing="ij")
    sky = np.stack([0.3 + 0.2 * v, 0.5 + 0.1 * v, 1.0 - 0.5 * v], -1)
    sun = np.exp(-(((u - 0.3) * 2 * h / 1.5) ** 2 + ((v - 35.0 / 180.0) * h / 1.5) ** 2))[..., None] * np.array([4000.0, 3600.0, 3000.0])
    return np.ascontiguousarray(sky + sun, np.float32)


# name: (texture size, spp, arrays, map, target)
WORKLOADS = {"cbox_1024": (1024, 16, None, None, "emission"), "tess1m_1024": (1024, 16, tess1m_arrays, None, "emission"),
             "cbox_uniform_sky": (1024, 16, None, uniform_sky, "env"), "cbox_sun_sky": (1024, 16, None, sun_sky, "env")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out, lines = {}, []
    for name in args.workloads.split(","):
        T, spp, arrays, env, target = WORKLOADS[name]
        scene = make_scene("direct", arrays=arrays() if arrays else None)
        if env:
            scene.add_envmap(env())
        slots = (0,) + (None,) * (scene.inst_count - 1)
        texels = scene.texel_aovs_forward(0, (T, T), slots=slots)
        light = torch.zeros((T, T, 4), device="cuda"); cot = torch.randn((T, T, 4), device="cuda")
        ws = torch.empty(N.lib().zdr_texel_lighting_workspace_bytes(T, T), dtype=torch.uint8, device="cuda")
        wsb = torch.empty(N.lib().zdr_texel_lighting_backward_workspace_bytes(scene._handle, T, T), dtype=torch.uint8, device="cuda")
        d_e = torch.zeros((scene.inst_count, 3), device="cuda") if target == "emission" else None
        d_env = torch.zeros(tuple(scene._envmap[0].shape), device="cuda") if target == "env" else None
        ta, tb = alternate(lambda: scene.texel_lighting_backward(texels, cot, spp=spp, seed=0, d_emission=d_e, d_env=d_env, workspace=wsb),
                           lambda: scene.texel_lighting_forward(texels, spp=spp, seed=0, out=light, workspace=ws), args.rounds, args.reps, args.warmup)
        a, b = stats(ta), stats(tb)
        torch.cuda.synchronize()
        header = wsb[:16].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF      # the last call's: shaded texels, accepted environment samples, groups
        before_ms, after_ms = 1e3 * header[1] * GROUP_BYTES / ATOMIC_RATE, 1e3 * header[2] * GROUP_BYTES / ATOMIC_RATE
        out[name] = {"texture": T, "spp": spp, "accel": scene.info()["accel"], "triangles": scene.info()["ntris"], "target": target, "shaded_texels": int(header[0]),
                     "env_samples": int(header[1]), "env_groups_after_merge": int(header[2]), "atomic_budget_ms_before_merge": before_ms, "atomic_budget_ms_after_merge": after_ms,
                     "texel_lighting_backward": a, "texel_lighting_forward": b, "ratio": a["median_ms"] / b["median_ms"]}
        lines.append(f"{name:17s} {scene.info()['ntris']:8d} triangles {out[name]['accel']:5s} texture {T}^2 spp {spp} d_{target:8s}  "
                     f"backward {a['median_ms']:8.3f} ms [{a['min_ms']:.3f}, {a['max_ms']:.3f}]   forward {b['median_ms']:8.3f} ms [{b['min_ms']:.3f}, {b['max_ms']:.3f}]   "
                     f"ratio {a['median_ms'] / b['median_ms']:.3f}   environment samples {int(header[1])}, groups after the merge {int(header[2])}: "
                     f"atomic budget {before_ms:.3f} -> {after_ms:.3f} ms")
        print(lines[-1], flush=True)
        scene.check()
    lines.append(json.dumps(out))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
