#!/usr/bin/env python3
"""What the anisotropic gather costs and what it buys.  Same process, same box; the sides ALTERNATE round by round (other work shares
the host), each round is `--reps` calls between two device events, and the median, minimum and maximum over the rounds are reported.
    python tools/texel_aniso_cost.py [--parts footprint,gather,quality] [--rounds 7] [--reps 20] [--warmup 3] [--out profiles/texel_aniso_cost.txt]
footprint  texel_footprint_forward at 2048^2 texels of the Cornell box's own texel buffer against `out.copy_` of an (H, W, 4) texture: the
           kernel reads 64 bytes a texel and writes 16, the copy reads 16 and writes 16.  Recorded.
gather     at 2048^2 texels of the Cornell box's own view and footprint buffers, texel_gather_aniso_forward against texel_gather_mip_forward
           on the same view, and the full anisotropic adjoint (zero d_pyramid, scatter, pyramid adjoint) against the full mip adjoint, for
           the cases of tools/texel_mip_cost.py:
             a. a 64^2 image: every texel is magnified, one probe at level 0;
             b. a 1024^2 image with footprint 4, which forces fractional levels and several probes.
           Nbar is the mean probe count of the visible texels.  Expectation, forward: within Nbar x the mip forward of the same case — it
           is Nbar trilinear samples.  The adjoint is recorded: its atomics are the known hotspot.
quality    texel_project of a spp-1024 Cornell render at 1024^2 into a 128^2 texture under the three filters: RMSE over the texels both
           views see against the projection of the same render box-filtered to 128^2 (the experiment of tools/texel_mip_cost.py, with a
           row for "aniso" at the default footprint).  Recorded.
None of these is a test.  Each part runs in a child process of its own under `timeout`; nothing is started after one fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from texel_mip_cost import met, rng_text, rounds_of          # noqa: E402


def part_footprint(args):
    import torch
    from zdr_amd import texel_footprint_forward
    from zdr_amd.scenes import make_scene
    T = args.gather_size
    scene = make_scene("collocated")
    tex = scene.texel_aovs_forward(0, (T, T), slots=(0,) + (None,) * (scene.inst_count - 1))
    fp, src, cp = torch.empty(T, T, 4, device="cuda"), torch.rand(T, T, 4, device="cuda"), torch.empty(T, T, 4, device="cuda")
    st = rounds_of({"footprint": lambda: texel_footprint_forward(tex, (1024, 1024), scene.camera, out=fp), "copy": lambda: cp.copy_(src)}, args)
    gbs = (64 + 16) * T * T / (st["footprint"]["median_ms"] * 1e-3) / 1e9
    out = dict(st, texels=T, ratio=st["footprint"]["median_ms"] / st["copy"]["median_ms"], gb_per_s=gbs)
    print(f"footprint {T}^2 texels: kernel {rng_text(st['footprint'])} ({gbs:.0f} GB/s of 80 B a texel)   copy of an (H, W, 4) texture {rng_text(st['copy'])}   "
          f"ratio {out['ratio']:.2f}", flush=True)
    print("RESULT " + json.dumps(out), flush=True)


def part_gather(args):
    import torch
    from zdr_amd import (image_pyramid_backward, image_pyramid_forward, texel_footprint_forward, texel_gather_aniso_backward, texel_gather_aniso_forward,
                         texel_gather_mip_backward, texel_gather_mip_forward)
    from zdr_amd.mip import pyramid_pixels
    from zdr_amd.scenes import make_scene
    T, max_aniso = args.gather_size, args.max_aniso
    scene = make_scene("collocated")
    tex = scene.texel_aovs_forward(0, (T, T), slots=(0,) + (None,) * (scene.inst_count - 1))
    g, color = torch.rand(T, T, 4, device="cuda"), torch.empty(T, T, 4, device="cuda")
    out = {}
    for key, R, footprint in (("a_64_magnified", 64, 1.0), ("b_1024_footprint4", 1024, 4.0)):
        view = scene.texel_view_forward(tex, (R, R))
        fp = texel_footprint_forward(tex, (R, R), scene.camera)
        image, d_image = torch.rand(R, R, 4, device="cuda"), torch.zeros(R, R, 4, device="cuda")
        pyr, d_pyr = image_pyramid_forward(image), torch.zeros(pyramid_pixels((R, R)), 4, device="cuda")

        def aniso_adjoint():
            d_pyr.zero_()
            texel_gather_aniso_backward(g, view, fp, (R, R), footprint, max_aniso, d_image=d_image, d_pyramid=d_pyr)
            image_pyramid_backward(d_pyr, (R, R), d_image=d_image)

        def mip_adjoint():
            d_pyr.zero_()
            texel_gather_mip_backward(g, view, (R, R), footprint, d_image=d_image, d_pyramid=d_pyr)
            image_pyramid_backward(d_pyr, (R, R), d_image=d_image)
        st = rounds_of({"aniso_forward": lambda: texel_gather_aniso_forward(image, pyr, view, fp, footprint, max_aniso, out=color),
                        "mip_forward": lambda: texel_gather_mip_forward(image, pyr, view, footprint, out=color),
                        "aniso_adjoint": aniso_adjoint, "mip_adjoint": mip_adjoint}, args)
        vis = view[..., 0] == 1
        # the probe count of tf_probes (csrc/texel_filter.h), over the whole buffer
        A, B = (fp[..., 3] * footprint)[vis], (fp[..., 2] * footprint)[vis]
        Bp = torch.maximum(torch.maximum(B, A / max_aniso), torch.ones_like(B))
        N = torch.where(A > 1, torch.ceil(A / Bp - 0.125).clamp(1, max_aniso), torch.ones_like(A))
        nbar, nvis = float(N.mean()), int(vis.sum())
        ratio = st["aniso_forward"]["median_ms"] / st["mip_forward"]["median_ms"]
        ok = ratio <= max(nbar, 1.0)
        out[key] = dict(st, texels=T, image=R, footprint=footprint, max_aniso=max_aniso, visible=nvis / (T * T), mean_probes=nbar,
                        probe_histogram=[int((N == k).sum()) for k in range(1, max_aniso + 1)], forward_ratio=ratio,
                        adjoint_ratio=st["aniso_adjoint"]["median_ms"] / st["mip_adjoint"]["median_ms"], expectation_met=ok)
        print(f"gather {key}: {T}^2 texels ({100 * nvis / (T * T):.1f} % visible, Nbar {nbar:.2f} at max_aniso {max_aniso}) into a {R}^2 image, footprint {footprint}: "
              f"forward aniso {rng_text(st['aniso_forward'])}   mip {rng_text(st['mip_forward'])}   ratio {ratio:.3f} (expectation <= Nbar: {met(ok)})   "
              f"full adjoint aniso {rng_text(st['aniso_adjoint'])}   mip {rng_text(st['mip_adjoint'])}   ratio {out[key]['adjoint_ratio']:.3f} (recorded)", flush=True)
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
    for name, flt, footprint in (("bilinear", "bilinear", 1.0), ("mip", "mip", 1.0), ("mip_footprint_0.5", "mip", 0.5), ("aniso", "aniso", 1.0),
                                 ("aniso_footprint_0.5", "aniso", 0.5)):
        got = scene.texel_project([(scene.camera, render)], theta, texels=texels, filter=flt, footprint=footprint)
        both = (got.weight > 0) & (ref.weight > 0)
        out[name] = {"rmse": float(((got.color - ref.color)[both][:, :3] ** 2).mean().sqrt()), "texels": int(both.sum())}
    view = scene.texel_view(theta, res=(R, R), texels=texels, footprint=True)
    vis = view.visible == 1
    out["median_major"], out["median_minor"] = float(view.footprint.major[vis].median()), float(view.footprint.minor[vis].median())
    print(f"quality texel_project of a spp-{spp} render at {R}^2 into a {T}^2 texture (median major / minor axis of the visible texels {out['median_major']:.2f} / "
          f"{out['median_minor']:.2f}), RMSE over {out['aniso']['texels']} texels against the projection of the render box-filtered to {T}^2: bilinear "
          f"{out['bilinear']['rmse']:.5f}   mip {out['mip']['rmse']:.5f}   mip with footprint 0.5 {out['mip_footprint_0.5']['rmse']:.5f}   aniso "
          f"{out['aniso']['rmse']:.5f}   aniso with footprint 0.5 {out['aniso_footprint_0.5']['rmse']:.5f}", flush=True)
    scene.check()
    print("RESULT " + json.dumps(out), flush=True)


PARTS = {"footprint": part_footprint, "gather": part_gather, "quality": part_quality}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="footprint,gather,quality")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gather-size", type=int, default=2048)
    ap.add_argument("--max-aniso", type=int, default=8)
    ap.add_argument("--quality-res", type=int, default=1024)
    ap.add_argument("--quality-spp", type=int, default=1024)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one part may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return PARTS[args.child](args)
    lines, results, device = [], {}, "?"
    for part in args.parts.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", part, "--rounds", str(args.rounds),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--gather-size", str(args.gather_size), "--max-aniso", str(args.max_aniso),
               "--quality-res", str(args.quality_res), "--quality-spp", str(args.quality_spp)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(f"texel_aniso_cost: the part {part} ended with status {r.returncode}; nothing more is started")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                results[part] = json.loads(line[7:])
            elif line.startswith(("footprint ", "gather ", "quality ")):
                lines.append(line)
    lines.append(json.dumps(results))
    if args.out:
        import torch
        device = torch.cuda.get_device_name(0) if torch.cuda.is_available() else device
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"tools/texel_aniso_cost.py --parts {args.parts} --rounds {args.rounds} --reps {args.reps} on {device}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
