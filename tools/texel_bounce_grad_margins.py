#!/usr/bin/env python3
"""Writes profiles/texel_bounce_grad_margins.txt: the table behind GR.MARGINS of tests/texel_bounce_grad_ref.py — per case of
tests/texel_bounce_cases.py the float32 reference of the bounced light's adjoint, every target's terms added in ascending and in
descending order, against the float64 reference on the same walks and decisions.  No GPU involved.
    python tools/texel_bounce_grad_margins.py [--out profiles/texel_bounce_grad_margins.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import texel_bounce_grad_ref as GR                                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texel_bounce_grad_margins.txt"))
    args = ap.parse_args()
    lines = GR.table_lines()
    print("\n".join(lines))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
