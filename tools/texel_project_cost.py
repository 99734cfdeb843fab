#!/usr/bin/env python3
"""What the texture-space views cost.  Same process, same box; the sides ALTERNATE round by round (other work shares the host), each round
is `--reps` calls between two device events, and the median, minimum and maximum over the rounds are reported.
    python tools/texel_project_cost.py [--parts view,gather,example] [--rounds 7] [--reps 20] [--warmup 3] [--out profiles/texel_project_cost.txt]
view     Scene.texel_view_forward against render_aovs_forward at res = the texture's size and spp 1 — the yardstick of tools/texel_cost.py:
         it traces one closest-hit ray per texel and writes twice the bytes.  The Cornell box at 1024^2 (brute force) and the 1 M-triangle
         scene at 1024^2 and 2048^2 (BVH), through the standard camera with an image of the texture's size.  Expectation: at or below it.
gather   texel_gather_forward and texel_gather_backward against `out.copy_` of an (H, W, 4) texture, at 2048^2 texels of the Cornell box's
         own view buffer, into a 1024^2 image (about 4 texels land on each pixel) and into a 64^2 image (the magnification case, about
         1000 texels per pixel).  Bytes a texel moves BY DESIGN: 32 of view buffer (the line is fetched whole) + 16 of colour or
         cotangent = 48, plus the image once.  Expectation: the forward reaches at least half of the copy's achieved bandwidth; for
         the adjoint the ratio of the magnified case to the 1024^2 case is reported next to the forward's — if it exceeds it by more than
         the spread, the atomics are a hotspot.
example  examples/optimize_texture.py --init-from-target against the default at 256^2, spp 16: the first iteration's loss and the loss
         after 50 iterations, over three seeds.  Recorded, not held to a bar.
Each part runs in a child process of its own under `timeout`; nothing is started after one fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TEXEL_BYTES, COPY_BYTES = 48, 32
VIEW_WORKLOADS = {"cbox_1024": (1024, False), "tess1m_1024": (1024, True), "tess1m_2048": (2048, True)}   # name: (texture size, the 1 M-triangle scene)


def rng_text(s):
    return f"{s['median_ms']:8.4f} ms [{s['min_ms']:.4f}, {s['max_ms']:.4f}]"


def part_view(args):
    import torch
    from aov_cost import alternate, stats
    from zdr_amd import _native as N
    from zdr_amd.scenes import make_scene, tess1m_arrays
    out, scenes = {}, {}
    for name, (T, big) in VIEW_WORKLOADS.items():
        if big not in scenes:
            scenes[big] = make_scene("collocated", arrays=tess1m_arrays() if big else None)
        scene = scenes[big]
        slots = (0,) + (None,) * (scene.inst_count - 1)
        m = torch.rand((T, T, 4), device="cuda")
        tex = scene.texel_aovs_forward(0, (T, T), slots=slots)
        view = torch.zeros((T, T, 8), device="cuda"); buf = torch.zeros((T, T, 16), device="cuda")
        ws = torch.empty(N.lib().zdr_texel_view_workspace_bytes(T, T), dtype=torch.uint8, device="cuda")
        ta, tb = alternate(lambda: scene.texel_view_forward(tex, (T, T), out=view, workspace=ws),
                           lambda: scene.render_aovs_forward(m, (T, T), 1, 0, slots=slots, out=buf), args.rounds, args.reps, args.warmup)
        a, b = stats(ta), stats(tb)
        reach = float(tex[..., 12].mean())
        traced = float(((view[..., 2] >= 0) & (view[..., 2] < T) & (view[..., 3] >= 0) & (view[..., 3] < T) & (view[..., 4] > 0)).float().mean())
        out[name] = {"texture": T, "accel": scene.info()["accel"], "triangles": scene.info()["ntris"], "reached": reach, "traced": traced,
                     "visible": float(view[..., 0].mean()), "texel_view": a, "render_aovs_spp1": b, "ratio": a["median_ms"] / b["median_ms"]}
        print(f"view   {name:12s} {scene.info()['ntris']:8d} triangles {out[name]['accel']:5s} texture {T}^2 reached {reach:.3f} traced {traced:.3f} visible {out[name]['visible']:.3f}   "
              f"texel view {rng_text(a)}   render_aovs spp 1 {rng_text(b)}   ratio {out[name]['ratio']:.3f}", flush=True)
        scene.check()
    print("RESULT " + json.dumps(out), flush=True)


def part_gather(args):
    import numpy as np
    import torch
    from aov_cost import stats, window
    from zdr_amd import texel_gather_backward, texel_gather_forward
    from zdr_amd.scenes import make_scene
    T = args.gather_size
    scene = make_scene("collocated")
    tex = scene.texel_aovs_forward(0, (T, T), slots=(0,) + (None,) * (scene.inst_count - 1))
    g = torch.rand(T, T, 4, device="cuda")
    x, cp, color = torch.rand(T, T, 4, device="cuda"), torch.empty(T, T, 4, device="cuda"), torch.empty(T, T, 4, device="cuda")
    out = {}
    for R in (1024, 64):
        view = scene.texel_view_forward(tex, (R, R))
        image, d_image = torch.rand(R, R, 4, device="cuda"), torch.zeros(R, R, 4, device="cuda")
        sides = {"forward": lambda: texel_gather_forward(image, view, out=color),
                 "adjoint": lambda: texel_gather_backward(g, view, (R, R), d_image=d_image),
                 "copy": lambda: cp.copy_(x)}
        for _ in range(args.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, fn in sides.items():
                t[k].append(window(fn, args.reps))
        st = {k: stats(v) for k, v in t.items()}
        n, visible = T * T, float(view[..., 0].mean())
        gbs = lambda k, b: b / (st[k]["median_ms"] * 1e-3) / 1e9   # noqa: E731
        bw = {"forward": gbs("forward", TEXEL_BYTES * n + 16 * R * R), "adjoint": gbs("adjoint", TEXEL_BYTES * n + 16 * R * R), "copy": gbs("copy", COPY_BYTES * n)}
        out[str(R)] = dict(st, texels=T, image=R, visible=visible, texels_per_pixel=visible * n / (R * R), gb_per_s=bw,
                           forward_over_copy_bandwidth=bw["forward"] / bw["copy"], adjoint_over_copy_bandwidth=bw["adjoint"] / bw["copy"])
        print(f"gather {T}^2 texels ({100 * visible:.1f} % visible) into a {R}^2 image ({out[str(R)]['texels_per_pixel']:.1f} visible texels per pixel): "
              f"forward {rng_text(st['forward'])} = {bw['forward']:7.1f} GB/s   adjoint {rng_text(st['adjoint'])} = {bw['adjoint']:7.1f} GB/s   "
              f"copy {rng_text(st['copy'])} = {bw['copy']:7.1f} GB/s   bandwidth over the copy's: forward {out[str(R)]['forward_over_copy_bandwidth']:.3f}, "
              f"adjoint {out[str(R)]['adjoint_over_copy_bandwidth']:.3f}", flush=True)
    f = out["64"]["forward"]["median_ms"] / out["1024"]["forward"]["median_ms"]
    a = out["64"]["adjoint"]["median_ms"] / out["1024"]["adjoint"]["median_ms"]
    spread = max((out[r]["adjoint"]["max_ms"] - out[r]["adjoint"]["min_ms"]) / out[r]["adjoint"]["median_ms"] for r in ("64", "1024"))
    out["magnified_over_1024"] = {"forward": f, "adjoint": a, "adjoint_spread": spread}
    ok = min(out[r]["forward_over_copy_bandwidth"] for r in ("64", "1024")) >= 0.5
    print(f"gather magnified (64^2) over 1024^2: forward {f:.3f}, adjoint {a:.3f} (run-to-run spread of the adjoint {spread:.3f}): "
          f"the atomics are {'a hotspot' if a > f * (1 + spread) else 'no hotspot'} under magnification", flush=True)
    print(f"gather expectation (the forward at least half of the copy's achieved bandwidth): {'met' if ok else 'NOT met'}", flush=True)
    scene.check()
    print("RESULT " + json.dumps(out), flush=True)


def part_example(args):
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("optimize_texture_cost", os.path.join(ROOT, "examples", "optimize_texture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = {}
    for init in (False, True):
        rows = []
        for seed in (0, 1, 2):
            losses = ex.run(iters=args.example_iters, res=256, spp=16, tex=256, seed=seed, verbose=False, init_from_target=init)
            rows.append((losses[0], float(np.mean(losses[-5:]))))
        key = "init_from_target" if init else "default"
        out[key] = {"first": [r[0] for r in rows], "last5_mean": [r[1] for r in rows]}
        print(f"example {key:16s} 256^2 spp 16, seeds 0 1 2: first-iteration loss " + " ".join(f"{r[0]:.5f}" for r in rows) +
              f"   mean loss of iterations {args.example_iters - 5}..{args.example_iters - 1} " + " ".join(f"{r[1]:.5f}" for r in rows), flush=True)
    print("RESULT " + json.dumps(out), flush=True)


PARTS = {"view": part_view, "gather": part_gather, "example": part_example}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="view,gather,example")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gather-size", type=int, default=2048)
    ap.add_argument("--example-iters", type=int, default=50)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds one part may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return PARTS[args.child](args)
    lines, results, device = [], {}, "?"
    for part in args.parts.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", part, "--rounds", str(args.rounds),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--gather-size", str(args.gather_size), "--example-iters", str(args.example_iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(f"texel_project_cost: the part {part} ended with status {r.returncode}; nothing more is started")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                results[part] = json.loads(line[7:])
            elif line.startswith(("view ", "gather ", "example ")):
                lines.append(line)
    lines.append(json.dumps(results))
    if args.out:
        import torch
        device = torch.cuda.get_device_name(0) if torch.cuda.is_available() else device
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"tools/texel_project_cost.py --parts {args.parts} --rounds {args.rounds} --reps {args.reps} on {device}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
