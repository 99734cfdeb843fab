#!/usr/bin/env python3
"""What the texture-space lighting costs: Scene.texel_lighting_forward against render_forward of the DIRECT integrator at res = the
texture's size and the same spp.  The yardstick traces one camera ray, one shadow ray and one BSDF ray per sample, for every pixel; the
bake traces two any-hit rays per sample, for the reached texels only.  Same process, same box; the two sides ALTERNATE round by round
(other work shares the host), each round is `--reps` calls between two device events, and the median, minimum and maximum over the rounds
are reported.
    python tools/texel_lighting_cost.py [--workloads cbox_1024,tess1m_1024] [--rounds 7] [--reps 10] [--warmup 2] [--out profiles/texel_lighting_cost.txt]
Workloads: the Cornell box at 1024^2 spp 16 (brute force) and the 1 M-triangle scene at 1024^2 spp 16 (BVH).  Prints one line per workload
and a JSON summary line; --out writes the same text to a file as well."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aov_cost import alternate, stats                                       # noqa: E402
from zdr_amd import _native as N                                            # noqa: E402
from zdr_amd.scenes import make_scene, tess1m_arrays                        # noqa: E402

WORKLOADS = {"cbox_1024": (1024, 16, None), "tess1m_1024": (1024, 16, tess1m_arrays)}   # name: (texture size, spp, arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cbox_1024,tess1m_1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out, lines = {}, []
    for name in args.workloads.split(","):
        T, spp, arrays = WORKLOADS[name]
        scene = make_scene("direct", arrays=arrays() if arrays else None)
        slots = (0,) + (None,) * (scene.inst_count - 1)
        m = torch.rand((T, T, 4), device="cuda")
        texels = scene.texel_aovs_forward(0, (T, T), slots=slots)
        light = torch.zeros((T, T, 4), device="cuda"); img = torch.zeros((T, T, 4), device="cuda")
        ws = torch.empty(N.lib().zdr_texel_lighting_workspace_bytes(T, T), dtype=torch.uint8, device="cuda")
        ta, tb = alternate(lambda: scene.texel_lighting_forward(texels, spp=spp, seed=0, out=light, workspace=ws),
                           lambda: scene.render_forward(m, (T, T), spp, 0, out=img), args.rounds, args.reps, args.warmup)
        a, b = stats(ta), stats(tb)
        reach = float(texels[..., 12].mean())
        unlit = float(((light[..., :3].sum(-1) == 0) & (texels[..., 12] == 1)).sum() / texels[..., 12].sum().clamp_min(1))
        out[name] = {"texture": T, "spp": spp, "accel": scene.info()["accel"], "triangles": scene.info()["ntris"], "reached": reach, "unlit_of_reached": unlit,
                     "texel_lighting": a, "render_forward_direct": b, "ratio": a["median_ms"] / b["median_ms"]}
        lines.append(f"{name:12s} {scene.info()['ntris']:8d} triangles {out[name]['accel']:5s} texture {T}^2 spp {spp} reached {reach:.3f} unlit {unlit:.3f}   "
                     f"texel lighting {a['median_ms']:8.3f} ms [{a['min_ms']:.3f}, {a['max_ms']:.3f}]   "
                     f"render_forward direct {b['median_ms']:8.3f} ms [{b['min_ms']:.3f}, {b['max_ms']:.3f}]   ratio {a['median_ms'] / b['median_ms']:.3f}")
        print(lines[-1], flush=True)
        scene.check()
    lines.append(json.dumps(out))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
