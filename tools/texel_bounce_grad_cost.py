#!/usr/bin/env python3
"""What the adjoint of the bounced light costs: Scene.texel_bounce_backward against Scene.texel_bounce_forward with the same arguments —
the yardstick, code the adjoint does not touch.  Same process, same box; the two sides ALTERNATE round by round (other work shares the
host), each round is `--reps` calls between two device events, and the median, minimum and maximum over the rounds are reported.
    python tools/texel_bounce_grad_cost.py [--workloads ...] [--rounds 7] [--reps 5] [--warmup 2] [--out profiles/texel_bounce_grad_cost.txt]
Workloads, all at 1024^2 texels and spp 16: the Cornell box (brute force) and the 1 M-triangle scene (BVH), with one and with three
bounces, with d_materials alone and with both targets; and the Cornell box with a 1 x 1 material, three bounces, both targets — every
gradient of the launch lands on one texel.

The expectation, written down before the first run: on every row the adjoint costs at most the forward plus the scatter budget, within
the spread of the rounds — median(adjoint) <= median(forward) + budget + (max - min of the adjoint's rounds) + (max - min of the
forward's).  The scatter budget is 64 bytes (one staging cell) per shaded vertex that is pushed, counted by the kernel (word 1 of the
workspace), over the 1.3 TB/s of float atomics the other cost tools use.  The reasoning: the forward walks the same rays with the same
draws, and the adjoint adds only LDS traffic (the records, two sweeps) and the pushes; the 1 x 1 material keeps its whole cell array in
LDS and adds almost nothing to memory.  Nobody has measured what the records' LDS does to occupancy: the LDS per wave is printed.  A row
that misses the expectation is marked MISSED; it is reported, not tuned away.  Prints one line per row and a JSON summary line; --out
writes the same text to a file as well."""
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
PUSH_BYTES = 64                 # one staging cell: four taps x four floats
STATIC_LDS = 4 * 7 * 64 + 4 * 3 * 32        # the scatter queue and the emission table (csrc/scene.h, csrc/bouncegrad.h)
RECORD_BYTES = 9 * 64 * 4                   # per vertex: ZDR_BGRAD_FIELDS fields x 64 lanes x 4 bytes

# name: (arrays, material size, bounces, both targets)
WORKLOADS = {}
for _scene, _arrays in (("cbox", None), ("tess1m", tess1m_arrays)):
    for _k in (1, 3):
        for _both in (False, True):
            WORKLOADS[f"{_scene}_k{_k}_{'both' if _both else 'mat'}"] = (_arrays, 1024, _k, _both)
WORKLOADS["cbox_k3_1x1_both"] = (None, 1, 3, True)
T, SPP = 1024, 16


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
        arrays, msize, K, both = WORKLOADS[name]
        if arrays not in scenes:
            scene = make_scene("direct", arrays=arrays() if arrays else None)
            slots = (0,) + (None,) * (scene.inst_count - 1)
            scenes[arrays] = (scene, slots, scene.texel_aovs_forward(0, (T, T), slots=slots))
        scene, slots, texels = scenes[arrays]
        m = torch.rand((msize, msize, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        dims = np.array([[msize, msize]], np.int32)
        bounced = torch.zeros((T, T, 4), device="cuda"); cot = torch.randn((T, T, 4), device="cuda")
        ws = torch.empty(N.lib().zdr_texel_bounce_workspace_bytes(T, T), dtype=torch.uint8, device="cuda")
        wsb = torch.empty(N.lib().zdr_texel_bounce_backward_workspace_bytes(scene._handle, T, T, dims.ctypes.data, 1), dtype=torch.uint8, device="cuda")
        d_m = torch.zeros_like(m)
        d_e = torch.zeros((scene.inst_count, 3), device="cuda") if both else None
        ta, tb = alternate(lambda: scene.texel_bounce_backward(texels, cot, [m], spp=SPP, bounces=K, seed=0, slots=slots, d_materials=d_m, d_emission=d_e, workspace=wsb),
                           lambda: scene.texel_bounce_forward(texels, [m], spp=SPP, bounces=K, seed=0, slots=slots, out=bounced, workspace=ws), args.rounds, args.reps, args.warmup)
        a, b = stats(ta), stats(tb)
        torch.cuda.synchronize()
        header = wsb[:16].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF      # the last call's: shaded texels, vertices pushed
        budget_ms = 1e3 * header[1] * PUSH_BYTES / ATOMIC_RATE
        spread = (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"])
        met = a["median_ms"] <= b["median_ms"] + budget_ms + spread
        info = scene.info()
        out[name] = {"texture": T, "spp": SPP, "bounces": K, "material": msize, "targets": "d_materials + d_emission" if both else "d_materials", "accel": info["accel"],
                     "triangles": info["ntris"], "shaded_texels": int(header[0]), "vertices_pushed": int(header[1]), "scatter_budget_ms": budget_ms, "spread_ms": spread,
                     "lds_bytes_per_wave_without_bvh_stacks": STATIC_LDS + K * RECORD_BYTES, "texel_bounce_backward": a, "texel_bounce_forward": b,
                     "ratio": a["median_ms"] / b["median_ms"], "met": bool(met)}
        lines.append(f"{name:18s} {info['ntris']:8d} triangles {info['accel']:5s} texture {T}^2 spp {SPP} bounces {K} material {msize}^2 {'d_materials + d_emission' if both else 'd_materials':24s}  "
                     f"backward {a['median_ms']:8.3f} ms [{a['min_ms']:.3f}, {a['max_ms']:.3f}]   forward {b['median_ms']:8.3f} ms [{b['min_ms']:.3f}, {b['max_ms']:.3f}]   "
                     f"ratio {a['median_ms'] / b['median_ms']:.3f}   vertices pushed {int(header[1])}: scatter budget {budget_ms:.3f} ms, spread {spread:.3f} ms   "
                     f"LDS per wave {STATIC_LDS + K * RECORD_BYTES} B (+ the BVH stacks)   expected <= {b['median_ms'] + budget_ms + spread:.3f} ms: {'met' if met else 'MISSED'}")
        print(lines[-1], flush=True)
        scene.check()
    lines.append(json.dumps(out))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
