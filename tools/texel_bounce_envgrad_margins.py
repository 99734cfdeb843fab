#!/usr/bin/env python3
"""Writes profiles/texel_bounce_envgrad_margins.txt: the table behind MARGINS of tests/texel_bounce_envgrad_ref.py — per case of
tests/texel_bounce_env_cases.py the float32 reference of the bounced light's adjoint in the environment map, every map texel's terms added
in ascending and in descending order, against the float64 reference on the same walks and decisions.  No GPU involved.
    python tools/texel_bounce_envgrad_margins.py [--out profiles/texel_bounce_envgrad_margins.txt]
--gpu APPENDS, from a GPU, the kernels' own distance to their bars against the float64 reference on the dump's own walks.
--deep does either for EC.DEEP_CASES (tests/test_gpu_texel_deep_stack.py) and appends to profiles/texel_deep_stack.txt."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import texel_bounce_env_cases as EC                               # noqa: E402
import texel_bounce_envgrad_ref as ER                             # noqa: E402


def kernel_lines(names):
    import numpy as np
    import test_gpu_texel_bounce_envgrad as T
    lines = ["", "the kernels against the float64 reference on the dump's own walks, on an MI355X: largest error and its share of the bar"]
    for name in names:
        for accel in T.ACCELS:
            ref = T.dump_reference(name, accel)
            got, header = T.run_backward(name, accel)
            e, b = float(np.abs(got[..., :3].astype(np.float64) - ref["d_env"][..., :3]).max()), ER.bar(name, ref)
            lines.append(f"  [texel bounce envgrad] {name} {accel}: d_env off by at most {e:.3e} (bar {b:.3e}, {e / b:.3f} of it); header: shaded texels {header[0]}, "
                         f"accepted environment samples {header[1]}, groups that went to memory {header[2]}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--deep", action="store_true")
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", "texel_deep_stack.txt" if args.deep else "texel_bounce_envgrad_margins.txt")
    names = list(EC.DEEP_CASES) if args.deep else list(EC.CASES)
    lines = kernel_lines(names) if args.gpu else ([""] if args.deep else []) + ER.table_lines(names)
    print("\n".join(lines))
    with open(out, "a" if args.gpu or args.deep else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
