#!/usr/bin/env python3
"""Writes profiles/texel_bounce_margins.txt: the host table of tests/texel_bounce_cases.py (the float32 reference against the float64
one, the share of accepted environment samples, the fragility under moved barycentrics; no GPU involved) and, from a GPU, the kernels'
walks against the free-running float64 reference — the lines tests/test_gpu_texel_bounce.py prints: how many samples agree in nvert and
triangles, and the largest |u, v| differences per vertex index.  Recorded, not held to a bar.
    python tools/texel_bounce_margins.py [--out profiles/texel_bounce_margins.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import texel_bounce_cases as BC                                  # noqa: E402
import texel_bounce_gpu as BG                                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texel_bounce_margins.txt"))
    args = ap.parse_args()
    lines = BC.table_lines()
    lines += ["", "the kernels' walks against the free-running float64 reference, on an MI355X: recorded, not held to a bar"]
    lines += ["  " + BG.walk_differences(name, accel)[1] for name in BC.CASES for accel in BG.ACCELS]
    print("\n".join(lines))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
