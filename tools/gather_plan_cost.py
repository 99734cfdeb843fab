#!/usr/bin/env python3
"""What the gather plan costs and what it buys: the adjoint of a texel gather through a plan (zdr_amd/plan.py) against the atomic adjoint
of the same filter on the same inputs.  Same process, same box; the sides ALTERNATE round by round (other work shares the host), each
round is `--reps` calls between two device events, and the median, minimum and maximum over the rounds are reported.
    python tools/gather_plan_cost.py [--rows ...] [--rounds 7] [--reps 10] [--warmup 3] [--out profiles/gather_plan_cost.txt]
The setup is 2048^2 texels of the Cornell box's own view (and footprint) buffer.  Rows:
    bilinear_1024        bilinear, a 1024^2 image: two texels a pixel, short rows.  Recorded without a bar.
    bilinear_64          bilinear, a 64^2 image: every texel is magnified, 4,096 rows of thousands of entries — the atomics' hotspot
    mip_a_64             mip, a 64^2 image, footprint 1
    mip_b_1024_fp4       mip, a 1024^2 image, footprint 4: fractional levels, rows in the coarse levels
    aniso_a_64           aniso, as mip_a
    aniso_b_1024_fp4     aniso, as mip_b, max_aniso 8
Per row: the plan's build (wall clock around the call and a synchronise, median of `--builds`), nnz, the bytes of the plan, the apply
alone (outputs given, nothing zeroed), and the full adjoint — zero d_image, apply, pyramid adjoint — against the atomic full adjoint —
zero d_image and d_pyramid, scatter, pyramid adjoint.  Expectation, stated before measuring: the APPLY is at or below the atomic
adjoint on every magnified or coarse-level row (all but bilinear_1024).  The build is recorded with its ratio to one apply.
None of these is a test.  Each row runs in a child process of its own under `timeout`; nothing is started after one fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from texel_mip_cost import met, rng_text, rounds_of          # noqa: E402

ROWS = {"bilinear_1024": ("bilinear", 1024, 1.0, False), "bilinear_64": ("bilinear", 64, 1.0, True), "mip_a_64": ("mip", 64, 1.0, True),
        "mip_b_1024_fp4": ("mip", 1024, 4.0, True), "aniso_a_64": ("aniso", 64, 1.0, True), "aniso_b_1024_fp4": ("aniso", 1024, 4.0, True)}


def row(args):
    import torch
    from zdr_amd import (TexelView, image_pyramid_backward, texel_footprint_forward, texel_gather_aniso_backward, texel_gather_backward,
                         texel_gather_mip_backward)
    from zdr_amd.mip import pyramid_pixels
    from zdr_amd.scenes import make_scene
    flt, R, footprint, barred = ROWS[args.child]
    T, max_aniso = args.gather_size, args.max_aniso
    scene = make_scene("collocated")
    tex = scene.texel_aovs_forward(0, (T, T), slots=(0,) + (None,) * (scene.inst_count - 1))
    view = TexelView(scene.texel_view_forward(tex, (R, R)), (R, R), texel_footprint_forward(tex, (R, R), scene.camera) if flt == "aniso" else None)
    g = torch.randn(T, T, 4, device="cuda")
    d_image = torch.zeros(R, R, 4, device="cuda")
    d_pyr = None if flt == "bilinear" else torch.zeros(pyramid_pixels((R, R)), 4, device="cuda")
    kw = {} if flt == "bilinear" else {"footprint": footprint} if flt == "mip" else {"footprint": footprint, "max_aniso": max_aniso}
    builds = []
    for _ in range(args.builds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = view.gather_plan((R, R), flt, **kw)
        torch.cuda.synchronize()
        builds.append(1e3 * (time.perf_counter() - t0))
    build_ms = sorted(builds)[len(builds) // 2]

    def plan_adjoint():
        d_image.zero_()
        plan.apply(g, d_image, d_pyr)
        if d_pyr is not None:
            image_pyramid_backward(d_pyr, (R, R), d_image=d_image)

    def atomic_adjoint():
        d_image.zero_()
        if flt == "bilinear":
            return texel_gather_backward(g, view.data, (R, R), d_image=d_image)
        d_pyr.zero_()
        if flt == "mip":
            texel_gather_mip_backward(g, view.data, (R, R), footprint, d_image=d_image, d_pyramid=d_pyr)
        else:
            texel_gather_aniso_backward(g, view.data, view.footprint_data, (R, R), footprint, max_aniso, d_image=d_image, d_pyramid=d_pyr)
        image_pyramid_backward(d_pyr, (R, R), d_image=d_image)
    st = rounds_of({"apply": lambda: plan.apply(g, d_image, d_pyr), "plan_adjoint": plan_adjoint, "atomic_adjoint": atomic_adjoint}, args)
    counts = (plan.row_start[1:] - plan.row_start[:-1])
    ok = st["apply"]["median_ms"] <= st["atomic_adjoint"]["median_ms"]
    out = dict(st, filter=flt, texels=T, image=R, footprint=footprint, nnz=plan.nnz, rows=plan.rows, plan_bytes=plan.nbytes, longest_row=int(counts.max()),
               long_rows=int((counts >= 64).sum()), build_ms=build_ms, builds=builds, build_in_applies=build_ms / st["apply"]["median_ms"],
               apply_gb_per_s=24 * plan.nnz / (st["apply"]["median_ms"] * 1e-3) / 1e9, ratio=st["apply"]["median_ms"] / st["atomic_adjoint"]["median_ms"],
               full_ratio=st["plan_adjoint"]["median_ms"] / st["atomic_adjoint"]["median_ms"], barred=barred, expectation_met=ok if barred else None)
    print(f"plan {args.child}: {T}^2 texels into a {R}^2 image, {flt}, footprint {footprint}: nnz {plan.nnz} in {plan.rows} rows (longest {out['longest_row']}, "
          f"{out['long_rows']} of 64 or more), plan {plan.nbytes / 2 ** 20:.1f} MiB, build {build_ms:.2f} ms = {out['build_in_applies']:.0f} applies;   "
          f"apply {rng_text(st['apply'])} ({out['apply_gb_per_s']:.0f} GB/s of 24 B an entry)   full adjoint through the plan {rng_text(st['plan_adjoint'])}   "
          f"atomic full adjoint {rng_text(st['atomic_adjoint'])}   apply / atomic {out['ratio']:.3f} "
          + (f"(expectation <= 1: {met(ok)})" if barred else "(recorded)"), flush=True)
    scene.check()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--gather-size", type=int, default=2048)
    ap.add_argument("--max-aniso", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one row may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return row(args)
    lines, results, device = [], {}, "?"
    for name in args.rows.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(args.rounds),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--builds", str(args.builds), "--gather-size", str(args.gather_size),
               "--max-aniso", str(args.max_aniso)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(f"gather_plan_cost: the row {name} ended with status {r.returncode}; nothing more is started")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                results[name] = json.loads(line[7:])
            elif line.startswith("plan "):
                lines.append(line)
    lines.append(json.dumps(results))
    if args.out:
        import torch
        device = torch.cuda.get_device_name(0) if torch.cuda.is_available() else device
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"tools/gather_plan_cost.py --rows {args.rows} --rounds {args.rounds} --reps {args.reps} on {device}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
