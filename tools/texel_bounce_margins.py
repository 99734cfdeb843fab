#!/usr/bin/env python3
"""Writes profiles/texel_bounce_margins.txt: the host table of tests/texel_bounce_cases.py (the float32 reference against the float64
one, the share of accepted environment samples, the fragility under moved barycentrics; no GPU involved) and, from a GPU, the kernels'
walks against the free-running float64 reference — the lines tests/test_gpu_texel_bounce.py prints: how many samples agree in nvert and
triangles, and the largest |u, v| differences per vertex index.  Recorded, not held to a bar.
    python tools/texel_bounce_margins.py [--out profiles/texel_bounce_margins.txt]
--edges APPENDS the same for BC.EDGE_CASES (tests/test_gpu_texel_bake_edges.py), with the kernels' own distance to the estimator's bar;
--edges --host-only appends the host table alone, --edges --gpu-only the kernels' lines alone.
--deep does what --edges does for BC.DEEP_CASES (tests/test_gpu_texel_deep_stack.py) and appends to profiles/texel_deep_stack.txt."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import texel_bounce_cases as BC                                  # noqa: E402


def estimator_line(BG, name, accel):
    """the kernels' beta and add against the float64 reference on the dump's own hits (test 1 of tests/test_gpu_texel_bounce.py)"""
    import numpy as np
    q, dump = BG.run_dump(name, accel)
    K = BC.bounces(name)
    ref = BC.run_reference(name, hits=dump)
    same = (ref["flags"] == dump["flags"]).all(1) & (ref["nvert"] == dump["nvert"])
    have = (np.arange(K)[None, :] < dump["nvert"][:, None]) & same[:, None] & ~ref["near"]
    eb = np.abs(dump["beta"].astype(np.float64) - ref["beta"]).max(-1)[have].max()
    ea = np.abs(dump["add"].astype(np.float64) - ref["add"]).max(-1)[have].max()
    return (f"[texel bounce estimator] {name} {accel}: samples {same.size}, flags differ on {int((~same).sum())}; kernel vs float64 on the dump's own hits: "
            f"beta {eb:.3e}, add {ea:.3e}; bar {BC.bar(name):.3e} ({max(eb, ea) / BC.bar(name):.3f} of it)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--edges", action="store_true")
    ap.add_argument("--deep", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    args = ap.parse_args()
    names = list(BC.DEEP_CASES) if args.deep else list(BC.EDGE_CASES) if args.edges else list(BC.CASES)
    out = args.out or os.path.join(ROOT, "profiles", "texel_deep_stack.txt" if args.deep else "texel_bounce_margins.txt")
    append = args.edges or args.deep
    lines = []
    if not args.gpu_only:
        lines += ([""] if append else []) + BC.table_lines(names)
    if not args.host_only:
        import texel_bounce_gpu as BG
        lines += ["", "the kernels' walks against the free-running float64 reference, on an MI355X: recorded, not held to a bar"]
        lines += ["  " + BG.walk_differences(name, accel)[1] for name in names for accel in BG.ACCELS]
        if append:
            lines += ["  " + estimator_line(BG, name, accel) for name in names for accel in BG.ACCELS]
    print("\n".join(lines))
    with open(out, "a" if append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
