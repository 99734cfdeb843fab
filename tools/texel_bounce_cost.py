#!/usr/bin/env python3
"""What the bounced light costs: Scene.texel_bounce_forward with one and with K bounces against the yardstick of
tools/texel_lighting_cost.py — render_forward of the DIRECT integrator at res = the texture's size and the same spp, which traces two
closest-hit rays and one shadow ray for every pixel — with Scene.texel_lighting_forward of the same arguments beside it.  The walk traces
K closest-hit and K shadow rays per sample, for the reached texels only.

The expectation, written down before the first run: on both workloads `bounces=1` costs at most the yardstick, and `bounces=K` at most
K times it.  A row that misses it is marked MISSED; it is reported, not tuned away.

Same process, same box; the sides ALTERNATE round by round (other work shares the host), each round is `--reps` calls per side between
two device events, and the median, minimum and maximum over the rounds are reported.
    python tools/texel_bounce_cost.py [--workloads cbox_1024,tess1m_1024] [--bounces 3] [--rounds 7] [--reps 5] [--warmup 2] [--out profiles/texel_bounce_cost.txt]
Workloads: the Cornell box at 1024^2 spp 16 (brute force) and the 1 M-triangle scene at 1024^2 spp 16 (BVH).  Prints one line per workload
and a JSON summary line; --out writes the same text to a file as well."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aov_cost import stats, window                                          # noqa: E402
from zdr_amd import _native as N                                            # noqa: E402
from zdr_amd.scenes import make_scene, tess1m_arrays                        # noqa: E402

WORKLOADS = {"cbox_1024": (1024, 16, None), "tess1m_1024": (1024, 16, tess1m_arrays)}   # name: (texture size, spp, arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cbox_1024,tess1m_1024")
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    K = args.bounces
    out, lines = {}, []
    for name in args.workloads.split(","):
        T, spp, arrays = WORKLOADS[name]
        scene = make_scene("direct", arrays=arrays() if arrays else None)
        slots = (0,) + (None,) * (scene.inst_count - 1)
        m = torch.rand((T, T, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        texels = scene.texel_aovs_forward(0, (T, T), slots=slots)
        bounced = torch.zeros((T, T, 4), device="cuda"); light = torch.zeros((T, T, 4), device="cuda"); img = torch.zeros((T, T, 4), device="cuda")
        ws = torch.empty(max(N.lib().zdr_texel_bounce_workspace_bytes(T, T), N.lib().zdr_texel_lighting_workspace_bytes(T, T)), dtype=torch.uint8, device="cuda")
        sides = {
            "bounce_1": lambda: scene.texel_bounce_forward(texels, [m], spp=spp, bounces=1, seed=0, slots=slots, out=bounced, workspace=ws),
            f"bounce_{K}": lambda: scene.texel_bounce_forward(texels, [m], spp=spp, bounces=K, seed=0, slots=slots, out=bounced, workspace=ws),
            "texel_lighting": lambda: scene.texel_lighting_forward(texels, spp=spp, seed=0, out=light, workspace=ws),
            "render_forward_direct": lambda: scene.render_forward(m, (T, T), spp, 0, out=img),
        }
        for _ in range(args.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, fn in sides.items():
                ms[k].append(window(fn, args.reps))
        st = {k: stats(v) for k, v in ms.items()}
        yard = st["render_forward_direct"]["median_ms"]
        r1, rk = st["bounce_1"]["median_ms"] / yard, st[f"bounce_{K}"]["median_ms"] / yard
        reach = float(texels[..., 12].mean())
        out[name] = {"texture": T, "spp": spp, "bounces": K, "accel": scene.info()["accel"], "triangles": scene.info()["ntris"], "reached": reach, **st,
                     "ratio_1": r1, f"ratio_{K}": rk, "expectation_1": 1.0, f"expectation_{K}": float(K), "met_1": r1 <= 1.0, f"met_{K}": rk <= K}
        show = lambda k: f"{st[k]['median_ms']:8.3f} ms [{st[k]['min_ms']:.3f}, {st[k]['max_ms']:.3f}]"
        lines.append(f"{name:12s} {scene.info()['ntris']:8d} triangles {out[name]['accel']:5s} texture {T}^2 spp {spp} reached {reach:.3f}   "
                     f"bounces=1 {show('bounce_1')}   bounces={K} {show(f'bounce_{K}')}   texel lighting {show('texel_lighting')}   "
                     f"render_forward direct {show('render_forward_direct')}   ratio 1: {r1:.3f} (expected <= 1: {'met' if r1 <= 1.0 else 'MISSED'})   "
                     f"ratio {K}: {rk:.3f} (expected <= {K}: {'met' if rk <= K else 'MISSED'})")
        print(lines[-1], flush=True)
        scene.check()
    lines.append(json.dumps(out))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
