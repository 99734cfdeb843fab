#!/usr/bin/env python3
"""What the prefiltered gather costs and what it buys.  Same process, same box; the sides ALTERNATE round by round (other work shares the
host), each round is `--reps` calls between two device events, and the median, minimum and maximum over the rounds are reported.
    python tools/texel_mip_cost.py [--parts pyramid,gather,quality,example] [--rounds 7] [--reps 20] [--warmup 3] [--out profiles/texel_mip_cost.txt]
pyramid  image_pyramid_forward and image_pyramid_backward of 1024^2 and 2048^2 images against `out.copy_` of the image and against
         push_pull_forward of a texture of the same size.  Expectation: at or below the push-pull forward — about a third of its bytes
         per pixel (16 read + 16/3 written against 86.7) in at most half the launches.
gather   at 2048^2 texels of the Cornell box's own view buffer, texel_gather_mip_forward against texel_gather_forward on the same view,
         and the full mip adjoint (zero d_pyramid, scatter, pyramid adjoint) against texel_gather_backward:
           a. a 64^2 image: every texel is magnified, f = 0.  Expectation, forward: within 48/32 of the bilinear gather (16 more view
              bytes per texel);
           b. a 1024^2 image with footprint 4, which forces fractional levels: eight taps against four.  Expectation, forward: <= 2 x.
         The adjoint is recorded, with the float-atomic budget: the bytes the scatter adds (16 per tap and visible texel) over 1.3 TB/s.
quality  texel_project of a spp-1024 Cornell render at 1024^2 into a 128^2 texture under both filters: RMSE over the texels both views see
         against the projection of the same render box-filtered to 128^2; "mip" with footprint 1 and with footprint 0.5 (one level sharper).
         Recorded.
example  examples/optimize_texture.py --init-from-target at 256^2, spp 16, 50 iterations under both filters: the first iteration's loss
         and the mean of the last five, over three seeds.  Recorded.
None of these is a test.  Each part runs in a child process of its own under `timeout`; nothing is started after one fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ATOMIC_BYTES_PER_S = 1.3e12          # the chip-wide rate of global float atomic adds, in added bytes


def rng_text(s):
    return f"{s['median_ms']:8.4f} ms [{s['min_ms']:.4f}, {s['max_ms']:.4f}]"


def rounds_of(sides, args):
    import torch
    from aov_cost import stats, window
    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            t[k].append(window(fn, args.reps))
    return {k: stats(v) for k, v in t.items()}


def met(ok):
    return "met" if ok else "**NOT met**"


def part_pyramid(args):
    import torch
    from zdr_amd import image_pyramid_backward, image_pyramid_forward
    from zdr_amd.mip import pyramid_layout, pyramid_pixels
    from zdr_amd.pushpull import push_pull_forward, workspace_bytes
    out = {}
    for R in (1024, 2048):
        image, cp, filled = torch.rand(R, R, 4, device="cuda"), torch.empty(R, R, 4, device="cuda"), torch.empty(R, R, 4, device="cuda")
        weight = (torch.rand(R, R, device="cuda") < 0.7).float()
        pyr, d_pyr, d_image = (torch.empty(pyramid_pixels((R, R)), 4, device="cuda"), torch.rand(pyramid_pixels((R, R)), 4, device="cuda"),
                               torch.zeros(R, R, 4, device="cuda"))
        ws = torch.empty(workspace_bytes((R, R)), dtype=torch.uint8, device="cuda")
        st = rounds_of({"pyramid": lambda: image_pyramid_forward(image, out=pyr),
                        "adjoint": lambda: image_pyramid_backward(d_pyr, (R, R), d_image=d_image),
                        "copy": lambda: cp.copy_(image),
                        "push_pull": lambda: push_pull_forward(image, weight, out=filled, workspace=ws)}, args)
        lay = pyramid_layout((R, R))
        L = len(lay) - 1
        tail = next(l for l, (w, h, _) in enumerate(lay) if max(w, h) <= 32)      # ZDR_MIP_TAIL_DIM: the first level the fused tail takes
        ok = max(st["pyramid"]["median_ms"], st["adjoint"]["median_ms"]) <= st["push_pull"]["median_ms"]
        out[str(R)] = dict(st, levels=L, launches=(tail + 1) // 2 + (1 if tail < L else 0), expectation_met=ok)
        print(f"pyramid {R}^2 ({L} levels, {out[str(R)]['launches']} launches): build {rng_text(st['pyramid'])}   adjoint {rng_text(st['adjoint'])}   "
              f"copy {rng_text(st['copy'])}   push-pull forward {rng_text(st['push_pull'])}   expectation (both at or below push-pull): {met(ok)}", flush=True)
    print("RESULT " + json.dumps(out), flush=True)


def part_gather(args):
    import torch
    from zdr_amd import (image_pyramid_backward, image_pyramid_forward, texel_gather_backward, texel_gather_forward, texel_gather_mip_backward,
                         texel_gather_mip_forward)
    from zdr_amd.mip import pyramid_pixels
    from zdr_amd.scenes import make_scene
    T = args.gather_size
    scene = make_scene("collocated")
    tex = scene.texel_aovs_forward(0, (T, T), slots=(0,) + (None,) * (scene.inst_count - 1))
    g, color = torch.rand(T, T, 4, device="cuda"), torch.empty(T, T, 4, device="cuda")
    out = {}
    for key, R, footprint, bound in (("a_64_magnified", 64, 1.0, 48.0 / 32.0), ("b_1024_footprint4", 1024, 4.0, 2.0)):
        view = scene.texel_view_forward(tex, (R, R))
        image, d_image = torch.rand(R, R, 4, device="cuda"), torch.zeros(R, R, 4, device="cuda")
        pyr, d_pyr = image_pyramid_forward(image), torch.zeros(pyramid_pixels((R, R)), 4, device="cuda")

        def full_adjoint():
            d_pyr.zero_()
            texel_gather_mip_backward(g, view, (R, R), footprint, d_image=d_image, d_pyramid=d_pyr)
            image_pyramid_backward(d_pyr, (R, R), d_image=d_image)
        st = rounds_of({"mip_forward": lambda: texel_gather_mip_forward(image, pyr, view, footprint, out=color),
                        "bilinear_forward": lambda: texel_gather_forward(image, view, out=color),
                        "mip_adjoint": full_adjoint,
                        "bilinear_adjoint": lambda: texel_gather_backward(g, view, (R, R), d_image=d_image)}, args)
        vis = view[..., 0] == 1
        s = (view[..., 6] * footprint)[vis]
        fractional = float(((s > 1) & (torch.frexp(s)[0] != 0.5)).float().mean())
        nvis = int(vis.sum())
        taps = nvis * 4 * (1.0 + fractional)
        budget_ms = 16.0 * taps / ATOMIC_BYTES_PER_S * 1e3
        ratio = st["mip_forward"]["median_ms"] / st["bilinear_forward"]["median_ms"]
        out[key] = dict(st, texels=T, image=R, footprint=footprint, visible=nvis / (T * T), fractional=fractional, forward_ratio=ratio, forward_bound=bound,
                        adjoint_ratio=st["mip_adjoint"]["median_ms"] / st["bilinear_adjoint"]["median_ms"], atomic_budget_ms=budget_ms, expectation_met=ratio <= bound)
        print(f"gather {key}: {T}^2 texels ({100 * nvis / (T * T):.1f} % visible, {100 * fractional:.1f} % of them with a fractional level) into a {R}^2 image, footprint {footprint}: "
              f"forward mip {rng_text(st['mip_forward'])}   bilinear {rng_text(st['bilinear_forward'])}   ratio {ratio:.3f} (expectation <= {bound:.2f}: {met(ratio <= bound)})   "
              f"full adjoint mip {rng_text(st['mip_adjoint'])}   bilinear {rng_text(st['bilinear_adjoint'])}   ratio {out[key]['adjoint_ratio']:.3f}   "
              f"float-atomic budget of the mip scatter ({taps / 1e6:.1f} M taps x 16 B over 1.3 TB/s) {budget_ms:.4f} ms", flush=True)
    scene.check()
    print("RESULT " + json.dumps(out), flush=True)


def part_quality(args):
    import torch
    from zdr_amd.scenes import cbox_material_np, make_scene
    R, T, spp = args.quality_res, 128, args.quality_spp
    scene = make_scene("path")
    material = torch.from_numpy(cbox_material_np()).cuda()
    render = scene.render(material, res=(R, R), spp=spp).detach()
    small = render.view(T, R // T, T, R // T, 4).mean((1, 3)).contiguous()
    theta = torch.rand(T, T, 4, device="cuda")
    texels = scene.texel_aovs(theta)
    ref = scene.texel_project([(scene.camera, small)], theta, texels=texels)
    out = {}
    # footprint 0.5 reads one level below: where scale is about 2 R / T it is the level whose pixels are the reference's own
    for name, flt, footprint in (("bilinear", "bilinear", 1.0), ("mip", "mip", 1.0), ("mip_footprint_0.5", "mip", 0.5)):
        got = scene.texel_project([(scene.camera, render)], theta, texels=texels, filter=flt, footprint=footprint)
        both = (got.weight > 0) & (ref.weight > 0)
        out[name] = {"rmse": float(((got.color - ref.color)[both][:, :3] ** 2).mean().sqrt()), "texels": int(both.sum())}
    view = scene.texel_view(theta, res=(R, R), texels=texels)
    out["median_scale"] = float(view.scale[view.visible == 1].median())
    print(f"quality texel_project of a spp-{spp} render at {R}^2 into a {T}^2 texture (median scale of the visible texels {out['median_scale']:.2f}), RMSE over "
          f"{out['mip']['texels']} texels against the projection of the render box-filtered to {T}^2: bilinear {out['bilinear']['rmse']:.5f}   mip {out['mip']['rmse']:.5f}   "
          f"mip with footprint 0.5 {out['mip_footprint_0.5']['rmse']:.5f}", flush=True)
    scene.check()
    print("RESULT " + json.dumps(out), flush=True)


def part_example(args):
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("optimize_texture_cost", os.path.join(ROOT, "examples", "optimize_texture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = {}
    for name in ("bilinear", "mip"):
        rows = []
        for seed in (0, 1, 2):
            losses = ex.run(iters=args.example_iters, res=256, spp=16, tex=256, seed=seed, verbose=False, init_from_target=True, project_filter=name)
            rows.append((losses[0], float(np.mean(losses[-5:]))))
        out[name] = {"first": [r[0] for r in rows], "last5_mean": [r[1] for r in rows]}
        print(f"example --init-from-target --project-filter {name:8s} 256^2 spp 16, seeds 0 1 2: first-iteration loss " + " ".join(f"{r[0]:.5f}" for r in rows) +
              f"   mean loss of iterations {args.example_iters - 5}..{args.example_iters - 1} " + " ".join(f"{r[1]:.5f}" for r in rows), flush=True)
    print("RESULT " + json.dumps(out), flush=True)


PARTS = {"pyramid": part_pyramid, "gather": part_gather, "quality": part_quality, "example": part_example}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="pyramid,gather,quality,example")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gather-size", type=int, default=2048)
    ap.add_argument("--quality-res", type=int, default=1024)
    ap.add_argument("--quality-spp", type=int, default=1024)
    ap.add_argument("--example-iters", type=int, default=50)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one part may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return PARTS[args.child](args)
    lines, results, device = [], {}, "?"
    for part in args.parts.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", part, "--rounds", str(args.rounds),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--gather-size", str(args.gather_size), "--quality-res", str(args.quality_res),
               "--quality-spp", str(args.quality_spp), "--example-iters", str(args.example_iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(f"texel_mip_cost: the part {part} ended with status {r.returncode}; nothing more is started")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                results[part] = json.loads(line[7:])
            elif line.startswith(("pyramid ", "gather ", "quality ", "example ")):
                lines.append(line)
    lines.append(json.dumps(results))
    if args.out:
        import torch
        device = torch.cuda.get_device_name(0) if torch.cuda.is_available() else device
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"tools/texel_mip_cost.py --parts {args.parts} --rounds {args.rounds} --reps {args.reps} on {device}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
