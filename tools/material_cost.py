#!/usr/bin/env python3
"""What the material table costs: forward and backward ms of one render call (torch.cuda.Event around the call, as bench.py times),
one material through render_forward / render_backward against the material-table calls on the same mesh split in two instances,
with one material for both halves ([A], slots [0, 0, None]) and with one each ([A, B], slots [0, 1, None]).
    python tools/material_cost.py [--configs c3,c5] [--steps 10] [--warmup 3]
Prints one line per (config, variant) and a JSON summary line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zdr_amd import geometry  # noqa: E402
from zdr_amd.scenes import CONFIGS, cbox_material_np, cbox_models, fd_material_np, make_scene, tess1m_arrays  # noqa: E402


def split_in_two(a):
    """Instance 0's triangles in two instances, [0, n/2) and [n/2, n): same vertices, same order, the other instances unchanged."""
    b = [int(x) for x in a.inst_tri_begin]
    return geometry.from_arrays(a.verts, a.tris, [0, b[1] // 2] + b[1:], np.concatenate([a.inst_xform[:1], a.inst_xform]),
                                np.concatenate([a.inst_emission[:1], a.inst_emission]))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c5")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    a = torch.from_numpy(cbox_material_np()).cuda()
    b = torch.from_numpy(fd_material_np(1024, 1)).cuda()
    out = {}
    for name in args.configs.split(","):
        integrator, W, spp, kind, _ = CONFIGS[name]
        whole_arrays = tess1m_arrays() if kind == "tess1m" else geometry.assemble(cbox_models())
        whole = make_scene(integrator, arrays=whole_arrays)
        split = make_scene(integrator, arrays=split_in_two(whole_arrays))
        cot = torch.ones((W, W, 4), device="cuda")
        res = {}
        img = torch.zeros((W, W, 4), device="cuda")
        g = torch.zeros_like(a)
        res["legacy"] = (timed(lambda: whole.render_forward(a, (W, W), spp, 0, out=img), args.steps, args.warmup),
                         timed(lambda: whole.render_backward(cot, g, a, (W, W), spp, 0), args.steps, args.warmup))
        for label, mats, slots in (("[A]", [a], [0, 0, None]), ("[A, B]", [a, b], [0, 1, None])):
            split.material_slots = slots
            packed = mats[0] if len(mats) == 1 else torch.cat([m.reshape(-1, 4) for m in mats])
            dims = [tuple(m.shape[:2]) for m in mats]
            gp = torch.zeros_like(packed)
            res[label] = (timed(lambda: split.render_forward_materials(packed, (W, W), spp, 0, dims=dims, out=img), args.steps, args.warmup),
                          timed(lambda: split.render_backward_materials(cot, gp, packed, (W, W), spp, 0, dims=dims), args.steps, args.warmup))
        split.check(); whole.check()
        for k, (f, bw) in res.items():
            print(f"{name} {integrator} {W}^2 spp {spp} {k:8s} forward {f:8.3f} ms ({f / res['legacy'][0] - 1:+6.1%})   "
                  f"backward {bw:8.3f} ms ({bw / res['legacy'][1] - 1:+6.1%})", flush=True)
        out[name] = {k: {"forward_ms": v[0], "backward_ms": v[1]} for k, v in res.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
