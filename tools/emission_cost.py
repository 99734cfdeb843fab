#!/usr/bin/env python3
"""What the emission gradient costs: the backward without and with d_emission (zdr_render_backward_emission) of one render call
(torch.cuda.Event around the call, as bench.py times), on
    c3        the Cornell box, path 512^2 spp 256, brute force: ONE light, every term lands on three floats
    lights3   zdr_amd.scenes.multi_light_arrays(): three lights of different triangle counts and a blocker, path 512^2 spp 256
    c5        1 M triangles (BVH), path 1024^2 spp 256
    d3, d3_bvh, dlights3   the direct integrator at 512^2 spp 256: the Cornell box by brute force and with accel="bvh", and lights3's scene
The plain backward runs the kernels the parent commit runs (tools/isa_diff.py: instruction for instruction), so it is the baseline.
The two calls alternate, round by round, so that whatever else the box is doing lands on both; the medians, the spread of each and
the ratio are printed.
    python tools/emission_cost.py [--configs c3,lights3,c5] [--rounds 7] [--warmup 2] [--build]
--build: times a forced rebuild of the library first (needs no GPU).  Prints one line per config and a JSON summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zdr_amd import build  # noqa: E402
from zdr_amd.scenes import cbox_material_np, make_scene, multi_light_arrays, tess1m_arrays  # noqa: E402

CONFIGS = {   # name: (scene factory, resolution, spp)
    "c3": (lambda: make_scene("path", accel="brute"), 512, 256),
    "lights3": (lambda: make_scene("path", arrays=multi_light_arrays()), 512, 256),
    "c5": (lambda: make_scene("path", arrays=tess1m_arrays()), 1024, 256),
    "d3": (lambda: make_scene("direct", accel="brute"), 512, 256),
    "d3_bvh": (lambda: make_scene("direct", accel="bvh"), 512, 256),
    "dlights3": (lambda: make_scene("direct", arrays=multi_light_arrays()), 512, 256),
}


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,lights3,c5")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--build", action="store_true")
    args = ap.parse_args()
    out = {}
    if args.build:
        t = time.time()
        build.build(force=True)
        out["build_s"] = time.time() - t
        print(f"forced build of the library: {out['build_s']:.1f} s", flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is timed (a time from anything else would not be a measurement)")
    m = torch.from_numpy(cbox_material_np()).cuda()
    for name in args.configs.split(","):
        make, W, spp = CONFIGS[name]
        scene = make()
        cot = torch.ones((W, W, 4), device="cuda")
        g = torch.zeros_like(m)
        d_e = torch.zeros((scene.inst_count, 3), device="cuda")
        plain = lambda: scene.render_backward(cot, g, m, (W, W), spp, 0)
        emis = lambda: scene.render_backward(cot, g, m, (W, W), spp, 0, d_emission=d_e)
        for _ in range(args.warmup):
            plain(); emis()
        a, b = [], []
        for _ in range(args.rounds):
            a.append(once(plain)); b.append(once(emis))
        scene.check()
        ma, mb = float(np.median(a)), float(np.median(b))
        print(f"{name:8s} {W}^2 spp {spp}, {scene.light_count} light(s)  backward {ma:8.3f} ms [{min(a):.3f} .. {max(a):.3f}]  "
              f"backward + d_emission {mb:8.3f} ms [{min(b):.3f} .. {max(b):.3f}]  ratio {mb / ma:5.3f}", flush=True)
        out[name] = {"backward_ms": ma, "backward_emission_ms": mb, "ratio": mb / ma, "backward_all": a, "backward_emission_all": b}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
