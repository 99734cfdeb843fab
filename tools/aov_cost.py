#!/usr/bin/env python3
"""What the feature buffers cost: render_aovs_forward / render_aovs_backward against render_forward / render_backward of a COLLOCATED scene
of the same geometry — the kernels that do the same camera ray, first hit and texture lookup plus a BRDF, and store a quarter as much.
Same process, same box; the two sides ALTERNATE round by round (other work shares the host), each round is `--reps` calls between two
device events, and the median, minimum and maximum over the rounds are reported.
    python tools/aov_cost.py [--workloads cbox,tess1m] [--rounds 7] [--reps 20] [--warmup 3]
Workloads: cbox 512^2 spp 256 (brute force), the 1 M-triangle scene at 1024^2 spp 16 (BVH).  Prints one line per (workload, pass) and a JSON
summary line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zdr_amd.scenes import cbox_material_np, make_scene, tess1m_arrays  # noqa: E402

WORKLOADS = {"cbox": (512, 256, None), "tess1m": (1024, 16, tess1m_arrays)}     # name: (resolution, spp, arrays)


def window(fn, reps):
    """ms per call of `reps` calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(a, b, rounds, reps, warmup):
    """a and b timed in turns; returns their per-round ms"""
    for _ in range(warmup):
        a(); b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(a, reps)); tb.append(window(b, reps))
    return ta, tb


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cbox,tess1m")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    m = torch.from_numpy(cbox_material_np()).cuda()
    out = {}
    for name in args.workloads.split(","):
        W, spp, arrays = WORKLOADS[name]
        scene = make_scene("collocated", arrays=arrays() if arrays else None)
        img = torch.zeros((W, W, 4), device="cuda"); buf = torch.zeros((W, W, 16), device="cuda")
        cot = torch.ones((W, W, 4), device="cuda"); cot16 = torch.ones((W, W, 16), device="cuda")
        g = torch.zeros_like(m)
        passes = {
            "forward": (lambda: scene.render_aovs_forward(m, (W, W), spp, 0, out=buf), lambda: scene.render_forward(m, (W, W), spp, 0, out=img)),
            "backward": (lambda: scene.render_aovs_backward(cot16, g, m, (W, W), spp, 0), lambda: scene.render_backward(cot, g, m, (W, W), spp, 0)),
        }
        out[name] = {"resolution": W, "spp": spp, "accel": scene.info()["accel"]}
        for label, (aov, col) in passes.items():
            ta, tc = alternate(aov, col, args.rounds, args.reps, args.warmup)
            a, c = stats(ta), stats(tc)
            out[name][label] = {"aov": a, "collocated": c, "ratio": a["median_ms"] / c["median_ms"]}
            print(f"{name} {W}^2 spp {spp} {out[name]['accel']:5s} {label:8s} feature buffers {a['median_ms']:8.3f} ms [{a['min_ms']:.3f}, {a['max_ms']:.3f}]   "
                  f"collocated {c['median_ms']:8.3f} ms [{c['min_ms']:.3f}, {c['max_ms']:.3f}]   ratio {a['median_ms'] / c['median_ms']:.3f}", flush=True)
        scene.check()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
