#!/usr/bin/env python3
r"""Instructions of the path kernels that do no arithmetic the result needs: 64-bit address math, sign extensions for an address and
register-to-register copies.  Compiles csrc/zdr_kernels.hip to gfx950 assembly with the product's flags (hipcc -S, CPU only, the
command of tools/isa_diff.py) and prints, per kernel: the static counts, the runs of consecutive v_mov_b32 with the block they sit
in, every surviving 64-bit address instruction with its block, and the resource lines (NumVgprs, ScratchSize, Occupancy).
    python tools/isa_overhead.py                  the working tree, the two headline kernels and the two c5 kernels
    python tools/isa_overhead.py REV              a git revision instead of the tree
    python tools/isa_overhead.py --kernels=REGEX  kernels whose mangled name matches REGEX instead of the default four
    python tools/isa_overhead.py --runs=N         report v_mov runs of at least N instructions (default 6)
    python tools/isa_overhead.py --no-sites       leave the per-instruction list of address instructions out
    python tools/isa_overhead.py --keep=FILE      also keep the assembly in FILE;  --asm=FILE  read an assembly file instead of compiling
Counts are static (per kernel, not per trip): what they weigh is for the counters to say (SQ_INSTS_VALU, tools/pmc_custom.sh)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-munsafe-fp-atomics", "-fno-slp-vectorize", "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only"]
DEFAULT = r"^_Z6k_pathILi0E(10BruteAccel|8BvhAccel)Lb0ELb0ELb0EE|^_Z10k_path_bwdILi0E(10BruteAccel|8BvhAccel)Lb0ELb0ELb0ELb0EE"
ADDRESS = [("v_mad_u64_u32 + v_mad_i64_i32", re.compile(r"^v_mad_(u64_u32|i64_i32)\b")),
           ("v_lshl_add_u64", re.compile(r"^v_lshl_add_u64\b")),
           ("v_ashrrev_i32 v, 31, v", re.compile(r"^v_ashrrev_i32(_e\d+)?\s+v\d+,\s*31,"))]


def assemble(tree, out):
    subprocess.run([HIPCC, *FLAGS, "-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, "zdr_amd", "csrc"),
                    os.path.join(tree, "zdr_amd", "csrc", "zdr_kernels.hip"), "-o", out], check=True, capture_output=True)
    return parse(out)


def parse(out):
    kernels, name, block = {}, None, None
    for line in open(out):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and ".type" not in line:
            name = m.group(1); block = "entry"; kernels[name] = {"body": [], "res": {}}
        elif line.startswith(".Lfunc_end"):
            pass                                   # the resource comments of a kernel follow its end label
        elif name and re.match(r"^\.LBB\d+_\d+:", line):
            block = line.split(":")[0]
        elif name and re.match(r"^; %bb\.\d+", line):
            block = line[2:].split(":")[0].strip()
        elif name and line.startswith("\t") and not line.strip().startswith((";", ".")):
            kernels[name]["body"].append((block, line.strip().split(";")[0].strip()))
        elif name:
            m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy|NumSgprs): (\d+)", line)
            if m:
                kernels[name]["res"][m.group(1)] = int(m.group(2))
    return kernels


def report(name, k, min_run, sites):
    body = k["body"]
    demangled = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
    print(f"== {demangled}")
    print(f"   {name[:60]}...")
    valu = sum(i.startswith("v_") for _, i in body)
    print(f"   instructions / VALU: {len(body)} / {valu}")
    for label, rx in ADDRESS:
        print(f"   {label}: {sum(bool(rx.match(i)) for _, i in body)}")
    print(f"   v_mov_b32: {sum(i.startswith('v_mov_b32') for _, i in body)}")
    print(f"   scratch ops: {sum(i.startswith('scratch_') for _, i in body)}")
    print("   " + ", ".join(f"{key} {k['res'].get(key, '?')}" for key in ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy")))
    runs, n, start = [], 0, None
    for block, ins in body + [(None, "")]:
        if ins.startswith("v_mov_b32"):
            if n == 0:
                start = block
            n += 1
        else:
            if n >= min_run:
                runs.append((n, start))
            n = 0
    print(f"   v_mov_b32 runs of at least {min_run}: " + (", ".join(f"{n} in {b}" for n, b in runs) if runs else "none"))
    if sites:
        for block, ins in body:
            if any(rx.match(ins) for _, rx in ADDRESS):
                print(f"      {block:14s} {ins}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "1") for a in sys.argv[1:] if a.startswith("--"))
    pattern, min_run = re.compile(opt.get("kernels", DEFAULT)), int(opt.get("runs", "6"))
    with tempfile.TemporaryDirectory() as tmp:
        tree = ROOT
        if "asm" in opt:
            kernels, args = parse(opt["asm"]), [opt["asm"]]
        if args and "asm" not in opt:
            tree = os.path.join(tmp, "rev"); os.makedirs(tree)
            tar = subprocess.run(["git", "-C", ROOT, "archive", args[0], "zdr_amd/csrc", "include"], check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", tree], input=tar, check=True)
        if "asm" not in opt:
            kernels = assemble(tree, os.path.join(tmp, "k.s"))
        if "keep" in opt and "asm" not in opt:
            import shutil
            shutil.copy(os.path.join(tmp, "k.s"), opt["keep"])
    print(f"# {args[0] if args else 'working tree'}")
    for name in sorted(kernels):
        if pattern.search(name):
            report(name, kernels[name], min_run, "no-sites" not in opt)


if __name__ == "__main__":
    main()
