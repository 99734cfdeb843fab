#!/usr/bin/env python3
"""Writes profiles/texel_bounce_grad_margins.txt: the table behind GR.MARGINS of tests/texel_bounce_grad_ref.py — per case of
tests/texel_bounce_cases.py the float32 reference of the bounced light's adjoint, every target's terms added in ascending and in
descending order, against the float64 reference on the same walks and decisions.  No GPU involved.
    python tools/texel_bounce_grad_margins.py [--out profiles/texel_bounce_grad_margins.txt]
--edges APPENDS the same for BC.EDGE_CASES (tests/test_gpu_texel_bake_edges.py) and, from a GPU, the kernels' own distance to their bars
against the float64 reference on the dump's own walks; --edges --host-only appends the host table alone, --edges --gpu-only the kernels'
lines alone.
--deep does what --edges does for BC.DEEP_CASES (tests/test_gpu_texel_deep_stack.py) and appends to profiles/texel_deep_stack.txt."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import texel_bounce_cases as BC                                   # noqa: E402
import texel_bounce_grad_ref as GR                                # noqa: E402


def kernel_lines(names):
    import numpy as np
    import test_gpu_texel_bounce_grad as T
    from texel_bounce_gpu import ACCELS
    lines = ["", "the kernels against the float64 reference on the dump's own walks, on an MI355X: largest error per target and its share of the bar"]
    for name in names:
        for accel in ACCELS:
            ref = T.dump_reference(name, accel)
            dm, de = T.run_backward(name, accel)
            bm, be = GR.bars(name, ref)
            em = max(float(np.abs(g[..., :3].astype(np.float64) - w[..., :3]).max()) for g, w in zip(dm, ref["d_materials"]))
            rows = GR.light_rows(name)
            ee = float(np.abs(de[rows].astype(np.float64) - ref["d_emission"][rows]).max()) if rows else 0.0
            lines.append(f"  [texel bounce grad] {name} {accel}: d_materials off by at most {em:.3e} (bar {bm:.3e}, {em / bm:.3f} of it)  "
                         f"d_emission off by at most {ee:.3e} (bar {be:.3e}, {ee / be:.3f} of it)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--edges", action="store_true")
    ap.add_argument("--deep", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", "texel_deep_stack.txt" if args.deep else "texel_bounce_grad_margins.txt")
    append = args.edges or args.deep
    if not append:
        lines = GR.table_lines()
    else:
        names = list(BC.DEEP_CASES) if args.deep else list(BC.EDGE_CASES)
        lines = [] if args.gpu_only else [""] + GR.table_lines(names)
        if not args.host_only:
            lines += kernel_lines(names)
    print("\n".join(lines))
    with open(out, "a" if append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
