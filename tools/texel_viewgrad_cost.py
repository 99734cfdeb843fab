#!/usr/bin/env python3
"""What the camera gradients cost (README, "Camera gradients").  Same process, same box; the sides ALTERNATE round by round (other work
shares the host), each round is `--reps` calls between two device events, and the median, minimum and maximum over the rounds are
reported.  The yardsticks are kernels this feature did not touch.
    python tools/texel_viewgrad_cost.py [--parts dview,camera] [--rounds 7] [--reps 20] [--warmup 3] [--out profiles/texel_viewgrad_cost.txt]
dview    texel_gather_dview (bilinear) against texel_gather_forward at 2048^2 texels of the Cornell box's own view buffer, with a 1024^2
         image.  Bytes a texel moves BY DESIGN: 32 of view buffer + 16 of cotangent + 32 of d_view = 80 against the forward's 48.
         Expectation: within 80 / 48 = x 1.67 of the forward.  The mip filter (footprint 4) against texel_gather_mip_forward is
         recorded beside it, without a bar.
camera   Scene.texel_view_backward (96 bytes a texel, no ray) against Scene.texel_view_forward on the 1 M-triangle scene at 2048^2,
         through the standard camera with an image of the texture's size.  Expectation: at or below it.
Each part runs in a child process of its own under `timeout`; nothing is started after one fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DVIEW_BYTES, GATHER_BYTES = 80, 48


def rng_text(s):
    return f"{s['median_ms']:8.4f} ms [{s['min_ms']:.4f}, {s['max_ms']:.4f}]"


def part_dview(args):
    import torch
    from aov_cost import alternate, stats
    from zdr_amd import image_pyramid_forward, texel_gather_dview, texel_gather_forward, texel_gather_mip_forward
    from zdr_amd.scenes import make_scene
    T, R = args.size, 1024
    scene = make_scene("collocated")
    tex = scene.texel_aovs_forward(0, (T, T), slots=(0,) + (None,) * (scene.inst_count - 1))
    view = scene.texel_view_forward(tex, (R, R))
    image, g = torch.rand(R, R, 4, device="cuda"), torch.rand(T, T, 4, device="cuda")
    pyramid = image_pyramid_forward(image)
    color, d_view = torch.empty(T, T, 4, device="cuda"), torch.empty(T, T, 8, device="cuda")
    n, out = T * T, {}
    for name, new, old in (("bilinear", lambda: texel_gather_dview(image, view, g, out=d_view), lambda: texel_gather_forward(image, view, out=color)),
                           ("mip", lambda: texel_gather_dview(image, view, g, filter="mip", pyramid=pyramid, footprint=4.0, out=d_view),
                            lambda: texel_gather_mip_forward(image, pyramid, view, 4.0, out=color))):
        ta, tb = alternate(new, old, args.rounds, args.reps, args.warmup)
        a, b = stats(ta), stats(tb)
        out[name] = {"texels": T, "image": R, "visible": float(view[..., 0].mean()), "dview": a, "forward": b, "ratio": a["median_ms"] / b["median_ms"],
                     "dview_gb_per_s": DVIEW_BYTES * n / (a["median_ms"] * 1e-3) / 1e9, "forward_gb_per_s": GATHER_BYTES * n / (b["median_ms"] * 1e-3) / 1e9}
        print(f"dview  {name:8s} {T}^2 texels ({100 * out[name]['visible']:.1f} % visible), {R}^2 image: d_view {rng_text(a)} = {out[name]['dview_gb_per_s']:7.1f} GB/s   "
              f"forward gather {rng_text(b)} = {out[name]['forward_gb_per_s']:7.1f} GB/s   ratio {out[name]['ratio']:.3f}", flush=True)
    ok = out["bilinear"]["ratio"] <= DVIEW_BYTES / GATHER_BYTES
    print(f"dview  expectation (bilinear d_view within x {DVIEW_BYTES / GATHER_BYTES:.2f} of texel_gather_forward): {'met' if ok else 'NOT met'}", flush=True)
    scene.check()
    print("RESULT " + json.dumps(out), flush=True)


def part_camera(args):
    import torch
    from aov_cost import alternate, stats
    from zdr_amd import _native as N
    from zdr_amd.scenes import make_scene, tess1m_arrays
    T = args.size
    scene = make_scene("collocated", arrays=tess1m_arrays())
    tex = scene.texel_aovs_forward(0, (T, T), slots=(0,) + (None,) * (scene.inst_count - 1))
    view, d_view, d_cam = torch.zeros((T, T, 8), device="cuda"), torch.rand((T, T, 8), device="cuda"), torch.zeros(10, device="cuda")
    ws_f = torch.empty(N.lib().zdr_texel_view_workspace_bytes(T, T), dtype=torch.uint8, device="cuda")
    ws_b = torch.empty(N.lib().zdr_texel_view_backward_workspace_bytes(T, T), dtype=torch.uint8, device="cuda")
    ta, tb = alternate(lambda: scene.texel_view_backward(tex, d_view, (T, T), out=d_cam, workspace=ws_b),
                       lambda: scene.texel_view_forward(tex, (T, T), out=view, workspace=ws_f), args.rounds, args.reps, args.warmup)
    a, b = stats(ta), stats(tb)
    out = {"texture": T, "triangles": scene.info()["ntris"], "reached": float(tex[..., 12].mean()), "texel_view_backward": a, "texel_view_forward": b,
           "ratio": a["median_ms"] / b["median_ms"], "backward_gb_per_s": 96 * T * T / (a["median_ms"] * 1e-3) / 1e9}
    print(f"camera {out['triangles']:8d} triangles texture {T}^2 reached {out['reached']:.3f}: texel_view_backward {rng_text(a)} = {out['backward_gb_per_s']:7.1f} GB/s   "
          f"texel_view_forward {rng_text(b)}   ratio {out['ratio']:.3f}", flush=True)
    print(f"camera expectation (texel_view_backward at or below texel_view_forward): {'met' if out['ratio'] <= 1.0 else 'NOT met'}", flush=True)
    scene.check()
    print("RESULT " + json.dumps(out), flush=True)


PARTS = {"dview": part_dview, "camera": part_camera}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="dview,camera")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one part may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return PARTS[args.child](args)
    lines, results, device = [], {}, "?"
    for part in args.parts.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", part, "--rounds", str(args.rounds),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--size", str(args.size)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(f"texel_viewgrad_cost: the part {part} ended with status {r.returncode}; nothing more is started")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                results[part] = json.loads(line[7:])
            elif line.startswith(("dview ", "camera ")):
                lines.append(line)
    lines.append(json.dumps(results))
    if args.out:
        import torch
        device = torch.cuda.get_device_name(0) if torch.cuda.is_available() else device
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"tools/texel_viewgrad_cost.py --parts {args.parts} --rounds {args.rounds} --reps {args.reps} on {device}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
