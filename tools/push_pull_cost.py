#!/usr/bin/env python3
"""What push-pull costs next to moving the texture once: zdr_push_pull and zdr_push_pull_backward on a material of the Cornell box with
its `coverage` as the weight, against `out.copy_(x)` of the same texture (16 bytes read + 16 written per texel: the yardstick of a
streaming pass) and against the same operator written as float32 torch operations on the GPU (tests/push_pull_ref.py, forward + transpose).
Same process, same box; the sides ALTERNATE round by round (other work shares the host), each round is `--reps` calls between two
device events, and the median, minimum and maximum over the rounds are reported.
    python tools/push_pull_cost.py [--sizes 1024,2048] [--rounds 7] [--reps 20] [--warmup 3] [--out profiles/push_pull_cost.txt]
Each size runs in a child process of its own under `timeout`; nothing is started after one fails.

Bytes per texel the implementation moves BY DESIGN (zdr_amd/csrc/zdr_pushpull.hip; level l has 4^-l of the texels, so the levels >= 1
together count 1/3 — the fused tail keeps the last few thousand texels in LDS, which changes nothing at these sizes):
  forward   level 0: push reads x, w (20); pull reads x, w (20) and writes out (16)                                   = 56
            level >= 1: written by push (p, a: 20), read by the next push (20), pull reads p, a and writes y (36),
            read as the coarser level by the next pull (16)                                                          = 92 / 3
  adjoint   level 0: gather reads g, w (20); spread reads g, w (20) and writes d_x (16)                              = 56
            level >= 1: written by gather (G, a, r: 24), read by the next gather (20), spread reads G, writes q (32),
            read as the parents by the next spread (q, r: 20)                                                        = 96 / 3
The expectation it tests: each pass reaches at least half of the copy's achieved bandwidth at 2048^2."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_BYTES, BWD_BYTES, COPY_BYTES = 56 + 92 / 3, 56 + 96 / 3, 32


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from push_pull_ref import push_pull_ref, push_pull_ref_transpose
    from zdr_amd.pushpull import push_pull_backward, push_pull_forward, workspace_bytes
    from zdr_amd.scenes import make_scene

    def window(fn, reps):
        """ms per call of `reps` calls between two device events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    W = args.child
    scene = make_scene("path")
    x = torch.rand(W, W, 4, device="cuda")
    g = torch.rand(W, W, 4, device="cuda")
    w = scene.texel_aovs(x).coverage.contiguous()
    out, d_x, cp = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    ws = torch.empty(workspace_bytes((W, W)), dtype=torch.uint8, device="cuda")
    sides = {
        "forward": lambda: push_pull_forward(x, w, out=out, workspace=ws),
        "adjoint": lambda: push_pull_backward(g, w, d_x=d_x, workspace=ws),
        "both": lambda: (push_pull_forward(x, w, out=out, workspace=ws), push_pull_backward(g, w, d_x=d_x, workspace=ws)),
        "copy": lambda: cp.copy_(x),
        "torch_ops": lambda: (push_pull_ref(x, w, dtype=torch.float32), push_pull_ref_transpose(g, w, dtype=torch.float32)),
    }
    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            t[k].append(window(fn, args.torch_reps if k == "torch_ops" else args.reps))
    st = {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for k, v in t.items()}
    n = W * W
    gbs = lambda k, b: b * n / (st[k]["median_ms"] * 1e-3) / 1e9   # noqa: E731
    bw = {"forward": gbs("forward", FWD_BYTES), "adjoint": gbs("adjoint", BWD_BYTES), "copy": gbs("copy", COPY_BYTES)}
    res = dict(st, size=W, covered=float(w.mean()), gb_per_s=bw, forward_over_copy_bandwidth=bw["forward"] / bw["copy"],
               adjoint_over_copy_bandwidth=bw["adjoint"] / bw["copy"], torch_ops_over_both=st["torch_ops"]["median_ms"] / st["both"]["median_ms"],
               device=torch.cuda.get_device_name(0))
    rng = lambda k: f"{st[k]['median_ms']:8.4f} ms [{st[k]['min_ms']:.4f}, {st[k]['max_ms']:.4f}]"   # noqa: E731
    print(f"cbox coverage {W}^2 ({100 * res['covered']:.1f} % covered): forward {rng('forward')} = {bw['forward']:7.1f} GB/s at {FWD_BYTES:.1f} B/texel   "
          f"adjoint {rng('adjoint')} = {bw['adjoint']:7.1f} GB/s at {BWD_BYTES:.1f} B/texel   forward + adjoint {rng('both')}   "
          f"copy {rng('copy')} = {bw['copy']:7.1f} GB/s at {COPY_BYTES} B/texel   "
          f"bandwidth over the copy's: forward {res['forward_over_copy_bandwidth']:.3f}, adjoint {res['adjoint_over_copy_bandwidth']:.3f}   "
          f"torch ops forward + transpose {rng('torch_ops')} = {res['torch_ops_over_both']:.1f} x the kernels", flush=True)
    scene.check()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one size may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    lines, results, device = [], {}, "?"
    for W in (int(s) for s in args.sizes.split(",")):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", str(W), "--rounds", str(args.rounds),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--torch-reps", str(args.torch_reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(f"push_pull_cost: the step at {W}^2 ended with status {r.returncode}; nothing more is started")
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                results[str(W)] = json.loads(line[7:])
                device = results[str(W)]["device"]
            elif line.startswith("cbox "):
                lines.append(line)
    last = results[str(max(int(k) for k in results))]
    ok = last["forward_over_copy_bandwidth"] >= 0.5 and last["adjoint_over_copy_bandwidth"] >= 0.5
    lines.append(f"expectation (each pass at least half of the copy's achieved bandwidth at {last['size']}^2): {'met' if ok else 'NOT met'}")
    print(lines[-1])
    lines.append(json.dumps(results))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"tools/push_pull_cost.py --sizes {args.sizes} --rounds {args.rounds} --reps {args.reps} on {device}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
