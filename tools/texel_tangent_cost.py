#!/usr/bin/env python3
"""What the UV tangents cost.  Same process, same box; the sides ALTERNATE round by round (other work shares the host), each round is
`--reps` calls between two device events, and the median, minimum and maximum over the rounds are reported.
    python tools/texel_tangent_cost.py [--parts tangents,footprint] [--rounds 7] [--reps 20] [--warmup 3] [--out profiles/texel_tangent_cost.txt]
tangents   texel_tangents_forward against texel_aovs_forward at the same size, on the Cornell box at 1024^2 and the 1 M-triangle scene at
           2048^2.  The difference is one thread-per-texel launch: 8 bytes of key, 16 of the normal and a gathered 128-byte record read,
           32 bytes written.  Expectation: the difference of the medians is at or below texel_footprint_forward of the same texel count
           (one launch, 80 bytes a texel), measured in the same run.
footprint  texel_footprint_forward(..., tangents=) against the same call without, on the Cornell box's own texel buffer at 2048^2 and at
           1024^2.  By bytes 64 + 32 read and 16 written against 64 + 16: expectation at 2048^2, within x 1.4 of the square-patch call.
           The 1024^2 ratio is reported beside it: there the yardstick's 80 MiB may sit in the Infinity Cache where the new call's 112 do
           not.
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


def part_tangents(args):
    import torch
    from zdr_amd import _native as N
    from zdr_amd import texel_footprint_forward
    from zdr_amd.scenes import make_scene, tess1m_arrays
    out = {}
    for name, T, arrays in (("cbox_1024", 1024, None), ("tess1m_2048", 2048, tess1m_arrays)):
        scene = make_scene("collocated", arrays=arrays() if arrays else None)
        slots = (0,) + (None,) * (scene.inst_count - 1)
        tex, tan, fp = (torch.zeros((T, T, c), device="cuda") for c in (16, 8, 4))
        ws = torch.empty(N.lib().zdr_texel_aovs_workspace_bytes(T, T), dtype=torch.uint8, device="cuda")
        scene.texel_aovs_forward(0, (T, T), slots=slots, out=tex, workspace=ws)
        st = rounds_of({"tangents": lambda: scene.texel_tangents_forward(0, (T, T), out=tan, aovs_out=tex, workspace=ws),
                        "aovs": lambda: scene.texel_aovs_forward(0, (T, T), out=tex, workspace=ws),
                        "footprint": lambda: texel_footprint_forward(tex, (1024, 1024), scene.camera, out=fp)}, args)
        diff = st["tangents"]["median_ms"] - st["aovs"]["median_ms"]
        ok = diff <= st["footprint"]["median_ms"]
        out[name] = dict(st, texture=T, triangles=scene.info()["ntris"], difference_ms=diff, expectation_met=ok)
        print(f"tangents {name} ({scene.info()['ntris']} triangles, {T}^2 texels): texel_tangents_forward {rng_text(st['tangents'])}   texel_aovs_forward "
              f"{rng_text(st['aovs'])}   difference of the medians {diff:.4f} ms   texel_footprint_forward of the same texels {rng_text(st['footprint'])}   "
              f"expectation (difference at or below the footprint call): {met(ok)}", flush=True)
        scene.check()
        del scene
    print("RESULT " + json.dumps(out), flush=True)


def part_footprint(args):
    import torch
    from zdr_amd import texel_footprint_forward
    from zdr_amd.scenes import make_scene
    scene = make_scene("collocated")
    slots = (0,) + (None,) * (scene.inst_count - 1)
    out = {}
    for T in (2048, 1024):
        tex, tan = scene.texel_tangents_forward(0, (T, T), slots=slots)
        fp = torch.empty(T, T, 4, device="cuda")
        st = rounds_of({"uv": lambda: texel_footprint_forward(tex, (1024, 1024), scene.camera, out=fp, tangents=tan),
                        "square": lambda: texel_footprint_forward(tex, (1024, 1024), scene.camera, out=fp)}, args)
        ratio = st["uv"]["median_ms"] / st["square"]["median_ms"]
        gbs = (64 + 32 + 16) * T * T / (st["uv"]["median_ms"] * 1e-3) / 1e9
        out[str(T)] = dict(st, texels=T, ratio=ratio, gb_per_s=gbs)
        tail = f"expectation (within x 1.4): {met(ratio <= 1.4)}" if T == 2048 else "(reported: the yardstick may sit in the Infinity Cache)"
        if T == 2048:
            out[str(T)]["expectation_met"] = ratio <= 1.4
        print(f"footprint {T}^2 texels: from tangents {rng_text(st['uv'])} ({gbs:.0f} GB/s of 112 B a texel)   square patch {rng_text(st['square'])}   "
              f"ratio {ratio:.3f}   {tail}", flush=True)
    scene.check()
    print("RESULT " + json.dumps(out), flush=True)


PARTS = {"tangents": part_tangents, "footprint": part_footprint}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="tangents,footprint")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one part may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return PARTS[args.child](args)
    lines, results, device = [], {}, "?"
    for part in args.parts.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", part, "--rounds", str(args.rounds),
               "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(f"texel_tangent_cost: the part {part} ended with status {r.returncode}; nothing more is started")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                results[part] = json.loads(line[7:])
            elif line.startswith(("tangents ", "footprint ")):
                lines.append(line)
    lines.append(json.dumps(results))
    if args.out:
        import torch
        device = torch.cuda.get_device_name(0) if torch.cuda.is_available() else device
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"tools/texel_tangent_cost.py --parts {args.parts} --rounds {args.rounds} --reps {args.reps} on {device}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
