#!/usr/bin/env python3
r"""Instructions of the path kernels that do no arithmetic the result needs: 64-bit address math, sign extensions for an address and
register-to-register copies.  Compiles csrc/zdr_kernels.hip to gfx950 assembly with the product's flags (hipcc -S, CPU only, the
command of tools/isa_diff.py) and prints, per kernel: the static counts, the runs of consecutive v_mov_b32 with the block they sit
in, every surviving 64-bit address instruction with its block, and the resource lines (NumVgprs, ScratchSize, Occupancy).
Per kernel it also lists every scratch instruction with its block and offset ("loop": inside the persistent loop), and counts the
s_waitcnt vmcnt(0) and the v_readlane / v_writelane inside the persistent loop: the outermost loop that holds the most instructions,
found from the compiler's `in Loop: Header=` / `Parent Loop` comments (a nested loop's blocks count for the loop around it).
    python tools/isa_overhead.py                  the working tree, the two headline kernels and the two c5 kernels
    python tools/isa_overhead.py REV              a git revision instead of the tree
    python tools/isa_overhead.py --kernels=REGEX  kernels whose mangled name matches REGEX instead of the default four
    python tools/isa_overhead.py --runs=N         report v_mov runs of at least N instructions (default 6)
    python tools/isa_overhead.py --no-sites       leave the per-instruction lists (address and scratch instructions) out
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
WAIT_VM0 = re.compile(r"^s_waitcnt\b.*vmcnt\(0\)")


def assemble(tree, out):
    subprocess.run([HIPCC, *FLAGS, "-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, "zdr_amd", "csrc"),
                    os.path.join(tree, "zdr_amd", "csrc", "zdr_kernels.hip"), "-o", out], check=True, capture_output=True)
    return parse(out)


def loop_comment(k, block, line):
    """The loop a block sits in, from the comment on (or, for a header, the comment lines under) its label"""
    m = re.search(r"in Loop: Header=(BB\d+_\d+)", line)
    if m:
        k["loop_of"][block] = m.group(1)
    m = re.search(r"Parent Loop (BB\d+_\d+)", line)
    if m:
        k["parents"].setdefault(block.lstrip(".L"), []).append(m.group(1))
    if re.search(r"This (Inner )?Loop Header", line):
        k["loop_of"][block] = block.lstrip(".L")


def parse(out):
    kernels, name, block = {}, None, None
    for line in open(out):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and ".type" not in line:
            name = m.group(1); block = "entry"; kernels[name] = {"body": [], "res": {}, "loop_of": {}, "parents": {}}
        elif line.startswith(".Lfunc_end"):
            pass                                   # the resource comments of a kernel follow its end label
        elif name and re.match(r"^\.LBB\d+_\d+:", line):
            block = line.split(":")[0]
            loop_comment(kernels[name], block, line)
        elif name and re.match(r"^; %bb\.\d+", line):
            block = line[2:].split(":")[0].strip()
            loop_comment(kernels[name], block, line)
        elif name and re.match(r"^\s+; ", line) and "Loop" in line:
            loop_comment(kernels[name], block, line)
        elif name and line.startswith("\t") and not line.strip().startswith((";", ".")):
            ins = line.strip().split(";")[0].strip()
            if ins.startswith("scratch_") and "Folded" in line:         # a register spill, not an array in private memory
                ins += "    ; folded " + ("spill" if "Spill" in line else "reload")
            kernels[name]["body"].append((block, ins))
        elif name:
            m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy|NumSgprs): (\d+)", line)
            if m:
                kernels[name]["res"][m.group(1)] = int(m.group(2))
    return kernels


def persistent_loop(k):
    """(header of the outermost loop with the most instructions, the set of blocks inside it, nested loops included)"""
    def outermost(h):
        return (k["parents"].get(h) or [h])[0]      # the first Parent Loop comment of a header names the Depth=1 loop
    size = {}
    for block, _ in k["body"]:
        h = k["loop_of"].get(block)
        if h:
            size[outermost(h)] = size.get(outermost(h), 0) + 1
    if not size:
        return None, set()
    top = max(size, key=size.get)
    return top, {b for b, h in k["loop_of"].items() if outermost(h) == top}


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
    top, inside = persistent_loop(k)
    in_loop = [i for b, i in body if b in inside]
    print(f"   persistent loop {top}: {len(in_loop)} instructions, "
          f"s_waitcnt vmcnt(0) {sum(bool(WAIT_VM0.match(i)) for i in in_loop)}, "
          f"scratch ops {sum(i.startswith('scratch_') for i in in_loop)}")
    print(f"   v_readlane / v_writelane: {sum(i.startswith('v_readlane') for _, i in body)} / {sum(i.startswith('v_writelane') for _, i in body)}"
          f" (in the persistent loop {sum(i.startswith('v_readlane') for i in in_loop)} / {sum(i.startswith('v_writelane') for i in in_loop)})")
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
        for block, ins in body:
            if ins.startswith("scratch_"):
                print(f"      {block:14s} {'loop' if block in inside else '    '} {ins}")


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
