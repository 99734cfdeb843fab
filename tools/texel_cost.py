#!/usr/bin/env python3
"""What the texture-space feature buffers cost: Scene.texel_aovs_forward against render_aovs_forward at res = the texture's size and
spp 1 — a call that writes the same bytes (16 floats per pixel) and traces one camera ray per texel.  Same process, same box; the two
sides ALTERNATE round by round (other work shares the host), each round is `--reps` calls between two device events, and the median,
minimum and maximum over the rounds are reported.
    python tools/texel_cost.py [--workloads cbox_1024,tess1m_1024,tess1m_2048] [--rounds 7] [--reps 20] [--warmup 3]
Workloads: the Cornell box at 1024^2 (30 triangles over a million texels: the wave-cooperative sweep and the row bands) and the
1 M-triangle scene at 1024^2 and 2048^2 (a few texels per triangle: the per-lane sweep and the atomics).  Prints one line per workload
and a JSON summary line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aov_cost import alternate, stats                                       # noqa: E402
from zdr_amd import _native as N                                            # noqa: E402
from zdr_amd.scenes import make_scene, tess1m_arrays                        # noqa: E402

WORKLOADS = {"cbox_1024": (1024, None), "tess1m_1024": (1024, tess1m_arrays), "tess1m_2048": (2048, tess1m_arrays)}   # name: (texture size, arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cbox_1024,tess1m_1024,tess1m_2048")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    out, scenes = {}, {}
    for name in args.workloads.split(","):
        T, arrays = WORKLOADS[name]
        if arrays not in scenes:
            scenes[arrays] = make_scene("collocated", arrays=arrays() if arrays else None)
        scene = scenes[arrays]
        slots = (0,) + (None,) * (scene.inst_count - 1)
        m = torch.rand((T, T, 4), device="cuda")
        tex = torch.zeros((T, T, 16), device="cuda"); buf = torch.zeros((T, T, 16), device="cuda")
        ws = torch.empty(N.lib().zdr_texel_aovs_workspace_bytes(T, T), dtype=torch.uint8, device="cuda")
        scene.texel_aovs_forward(0, (T, T), slots=slots, out=tex, workspace=ws)
        ta, tb = alternate(lambda: scene.texel_aovs_forward(0, (T, T), out=tex, workspace=ws),
                           lambda: scene.render_aovs_forward(m, (T, T), 1, 0, slots=slots, out=buf), args.rounds, args.reps, args.warmup)
        a, b = stats(ta), stats(tb)
        cov, reach = float(tex[..., 11].mean()), float(tex[..., 12].mean())
        out[name] = {"texture": T, "accel": scene.info()["accel"], "triangles": scene.info()["ntris"], "covered": cov, "reached": reach,
                     "texel_aovs": a, "render_aovs_spp1": b, "ratio": a["median_ms"] / b["median_ms"]}
        print(f"{name:12s} {scene.info()['ntris']:8d} triangles {out[name]['accel']:5s} texture {T}^2 covered {cov:.3f} reached {reach:.3f}   "
              f"texel buffers {a['median_ms']:8.3f} ms [{a['min_ms']:.3f}, {a['max_ms']:.3f}]   "
              f"render_aovs spp 1 {b['median_ms']:8.3f} ms [{b['min_ms']:.3f}, {b['max_ms']:.3f}]   ratio {a['median_ms'] / b['median_ms']:.3f}", flush=True)
        scene.check()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
