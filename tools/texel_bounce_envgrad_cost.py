#!/usr/bin/env python3
"""What the adjoint of the bounced light in the environment map costs: Scene.texel_bounce_backward_env against Scene.texel_bounce_forward
with the same arguments — the yardstick, code the adjoint does not touch.  Same process, same box; the two sides ALTERNATE round by round
(other work shares the host), each round is `--reps` calls between two device events, and the median, minimum and maximum over the rounds
are reported.
    python tools/texel_bounce_envgrad_cost.py [--workloads ...] [--rounds 7] [--reps 5] [--warmup 2] [--out profiles/texel_bounce_envgrad_cost.txt]
Workloads, all at 1024^2 texels and spp 16 under a 256 x 512 map, with one and with three bounces: the Cornell geometry under the
near-uniform sky and under the sun-and-sky map of tools/texel_lighting_grad_cost.py (a closed box: the samples are drawn and the shadow
rays walked, few are accepted); an OPEN scene — a floor, a wall and a tilted slab on it, nothing overhead — under the sun map, where the
map's light arrives.  One more row: all three gradients of the open scene with three bounces, texel_bounce_backward (d_materials and
d_emission) followed by texel_bounce_backward_env, against the forward.

The expectation, written down before the first run: on every row the adjoint costs at most the forward plus the float-atomic budget,
within the spread of the rounds — median(adjoint) <= median(forward) + budget + (max - min of the adjoint's rounds) + (max - min of the
forward's).  The budget is the lighting adjoint's: 48 bytes (four taps x rgb x 4) per group of accepted environment samples that goes to
memory, counted by the kernel after its wave-level merge (word 2 of the workspace; word 1 counts the samples before it), over 1.3 TB/s.
The reasoning: the adjoint walks the forward's rays with the forward's draws and keeps no records; what it adds is the merge in LDS and
the atomics.  Not known before the run: what the kernel's registers do to occupancy (tests/test_bounceenv_resources.py prints them
beside the forward's).  The three-gradient row is two replays of the walk: it is reported against the forward, and its expectation is
the sum of both adjoints' — twice the forward plus both budgets (the scatter budget of tools/texel_bounce_grad_cost.py, 64 bytes per
pushed vertex).  A row that misses the expectation is marked MISSED; it is reported, not tuned away.  Prints one line per row and a JSON
summary line; --out writes the same text to a file as well."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aov_cost import alternate, stats                                       # noqa: E402
from texel_lighting_grad_cost import sun_sky, uniform_sky                   # noqa: E402
from zdr_amd import Scene, geometry                                         # noqa: E402
from zdr_amd import _native as N                                            # noqa: E402
from zdr_amd.scenes import make_scene, panel_mesh                           # noqa: E402

ATOMIC_RATE = 1.3e12            # bytes of float atomic adds per second, chip-wide
GROUP_BYTES = 48                # four taps x rgb x 4 bytes
PUSH_BYTES = 64                 # one staging cell of texel_bounce_backward
T, SPP = 1024, 16


def open_arrays():
    """instance 0: a floor, [-1, 1]^2 facing up; instance 1: a wall at x = -0.6 that faces +x; instance 2: a slab above the floor's far
    side, tilted by 50 degrees, whose front looks down at the floor and across at the wall.  Nothing emits and nothing is overhead."""
    fv, ft = panel_mesh(8, 8)
    pv, pt = panel_mesh(2, 2)
    wall = np.array([[0, 1, 0, -0.6], [-0.7, 0, 0, 0.7], [0, 0, 0.9, 0], [0, 0, 0, 1]], np.float32)
    c, s = np.cos(np.radians(50.0)), np.sin(np.radians(50.0))
    slab = np.array([[0.5 * c, s, 0, 0.7], [-0.5 * s, c, 0, 0.45], [0, 0, 0.8, 0.1], [0, 0, 0, 1]], np.float32) @ np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)
    nf, npv = fv.shape[0], pv.shape[0]
    return geometry.from_arrays(np.concatenate([fv, pv, pv]), np.concatenate([ft, pt + nf, pt + nf + npv]),
                                [0, ft.shape[0], ft.shape[0] + pt.shape[0], ft.shape[0] + 2 * pt.shape[0]],
                                np.stack([np.eye(4, dtype=np.float32).reshape(16), wall.reshape(16), slab.reshape(16)]))


# name: (scene, map, bounces, all three gradients)
WORKLOADS = {}
for _scene, _env in (("cbox", "uniform_sky"), ("cbox", "sun_sky"), ("open", "sun_sky")):
    for _k in (1, 3):
        WORKLOADS[f"{_scene}_{_env}_k{_k}"] = (_scene, _env, _k, False)
WORKLOADS["open_sun_sky_k3_three_gradients"] = ("open", "sun_sky", 3, True)
MAPS = {"uniform_sky": uniform_sky, "sun_sky": sun_sky}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out, lines, scenes = {}, [], {}
    for name in args.workloads.split(","):
        which, env, K, three = WORKLOADS[name]
        if (which, env) not in scenes:
            if which == "cbox":
                scene = make_scene("direct")
                slots = (0,) + (None,) * (scene.inst_count - 1)
                sizes = [(T, T)]
            else:
                scene = Scene(open_arrays(), integrator="direct")
                slots = (0, 1, 1)
                sizes = [(T, T), (64, 64)]
            scene.add_envmap(MAPS[env]())
            gen = torch.Generator(device="cuda").manual_seed(0)
            mats = [torch.rand((h, w, 4), device="cuda", generator=gen) for h, w in sizes]
            scenes[(which, env)] = (scene, slots, mats, scene.texel_aovs_forward(0, (T, T), slots=slots))
        scene, slots, mats, texels = scenes[(which, env)]
        dims = np.ascontiguousarray(np.array([m.shape[:2] for m in mats], np.int32))
        bounced = torch.zeros((T, T, 4), device="cuda"); cot = torch.randn((T, T, 4), device="cuda")
        ws = torch.empty(N.lib().zdr_texel_bounce_workspace_bytes(T, T), dtype=torch.uint8, device="cuda")
        wse = torch.empty(N.lib().zdr_texel_bounce_backward_env_workspace_bytes(T, T), dtype=torch.uint8, device="cuda")
        d_env = torch.zeros(tuple(scene._envmap[0].shape), device="cuda")
        kw = dict(spp=SPP, bounces=K, seed=0, slots=slots)
        env_call = lambda: scene.texel_bounce_backward_env(texels, cot, mats, d_env=d_env, workspace=wse, **kw)
        pushed = 0
        if three:
            wsb = torch.empty(N.lib().zdr_texel_bounce_backward_workspace_bytes(scene._handle, T, T, dims.ctypes.data, dims.shape[0]), dtype=torch.uint8, device="cuda")
            d_m, d_e = [torch.zeros_like(m) for m in mats], torch.zeros((scene.inst_count, 3), device="cuda")

            def adjoint():
                scene.texel_bounce_backward(texels, cot, mats, d_materials=d_m, d_emission=d_e, workspace=wsb, **kw)
                env_call()
        else:
            adjoint = env_call
        ta, tb = alternate(adjoint, lambda: scene.texel_bounce_forward(texels, mats, out=bounced, workspace=ws, **kw), args.rounds, args.reps, args.warmup)
        a, b = stats(ta), stats(tb)
        torch.cuda.synchronize()
        header = wse[:16].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF      # the last call's: shaded texels, accepted environment samples, groups
        if three:
            pushed = int(wsb[:16].view(torch.int32).cpu().numpy().astype(np.int64)[1] & 0xFFFFFFFF)
        before_ms, after_ms = 1e3 * header[1] * GROUP_BYTES / ATOMIC_RATE, 1e3 * header[2] * GROUP_BYTES / ATOMIC_RATE
        scatter_ms = 1e3 * pushed * PUSH_BYTES / ATOMIC_RATE
        spread = (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"])
        expected = (2.0 if three else 1.0) * b["median_ms"] + after_ms + scatter_ms + spread
        met = a["median_ms"] <= expected
        info = scene.info()
        what = "texel_bounce_backward + texel_bounce_backward_env" if three else "texel_bounce_backward_env"
        out[name] = {"texture": T, "spp": SPP, "bounces": K, "map": env, "accel": info["accel"], "triangles": info["ntris"], "adjoint": what,
                     "shaded_texels": int(header[0]), "env_samples": int(header[1]), "env_groups_after_merge": int(header[2]),
                     "atomic_budget_ms_before_merge": before_ms, "atomic_budget_ms_after_merge": after_ms, "vertices_pushed": pushed, "scatter_budget_ms": scatter_ms,
                     "spread_ms": spread, "backward": a, "texel_bounce_forward": b, "ratio": a["median_ms"] / b["median_ms"], "expected_ms": expected, "met": bool(met)}
        lines.append(f"{name:32s} {info['ntris']:6d} triangles {info['accel']:5s} texture {T}^2 spp {SPP} bounces {K} {what:50s}  "
                     f"backward {a['median_ms']:8.3f} ms [{a['min_ms']:.3f}, {a['max_ms']:.3f}]   forward {b['median_ms']:8.3f} ms [{b['min_ms']:.3f}, {b['max_ms']:.3f}]   "
                     f"ratio {a['median_ms'] / b['median_ms']:.3f}   environment samples {int(header[1])}, groups after the merge {int(header[2])}: "
                     f"atomic budget {before_ms:.3f} -> {after_ms:.3f} ms" + (f", scatter budget {scatter_ms:.3f} ms" if three else "") + f", spread {spread:.3f} ms   "
                     f"expected <= {expected:.3f} ms: {'met' if met else 'MISSED'}")
        print(lines[-1], flush=True)
        scene.check()
    lines.append(json.dumps(out))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
