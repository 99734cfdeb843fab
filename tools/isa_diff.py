#!/usr/bin/env python3
r"""Which kernels does a source change actually touch?  Compiles csrc/zdr_kernels.hip of a git revision and of the working tree to gfx950
assembly (hipcc -S, CPU only) and compares every kernel's instruction stream, labels normalised, and its kernel descriptor
(the .amdhsa_ resource directives: VGPRs, SGPRs, LDS, scratch).  A kernel reported `identical` runs the
very same machine code: no timing is needed for it — and one that is NOT expected to change and does is the thing to time first.
(Round 4: a sampler change meant for the direct kernels shifted the register allocation of the BVH forward kernel and moved five spill
operations into its walk loop, +8 %; it had been A/B-timed on the Cornell box only.)
    python tools/isa_diff.py [rev]        rev defaults to HEAD; prints one line per kernel: identical | DIFFERENT (instructions, VALU, scratch ops old -> new)
    python tools/isa_diff.py --pair-appended-false [rev]
        for a change that appends a bool template parameter to kernel templates (the material-table mode of k_path, k_path_bwd and k_simple):
        a kernel of rev that is gone from the tree is compared with the instantiation whose template arguments end in one more `false`
        (mangled Lb0E inserted before the end of the template argument list) — the kernel the old launch now runs.
    python tools/isa_diff.py --pair-renamed='REGEX=>REPLACEMENT' [rev]        (may be given several times)
        for a kernel that was renamed or folded into another template: a mangled name of rev that is gone from the tree is rewritten with
        re.sub(REGEX, REPLACEMENT) and compared with the kernel of that name, e.g.
        '_Z19k_path_bwd_emissionI(\w+?Accel)(Lb\dE)E=>_Z10k_path_bwdI\1\2Lb1ELb0ELb1EE'.
    python tools/isa_diff.py --source=zdr_texel.hip --flags='-O3 -fno-slp-vectorize -ffp-contract=off' [rev]
        another translation unit of csrc/, under the options zdr_amd/build.py gives it (default: zdr_kernels.hip and its options)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--source=")), "zdr_kernels.hip")
FLAGS = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--flags=")), "-O3 -munsafe-fp-atomics -fno-slp-vectorize").split() + [
    "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only"]


def assemble(tree, out):
    subprocess.run([HIPCC, *FLAGS, "-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, "zdr_amd", "csrc"),
                    os.path.join(tree, "zdr_amd", "csrc", SOURCE), "-o", out], check=True, capture_output=True)
    kernels, name, res, rname = {}, None, {}, None
    for line in open(out):
        r = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)      # the kernel descriptor: registers, LDS, scratch, the enabled SGPR inputs
        if r:
            rname = r.group(1); res[rname] = []
        elif line.strip() == ".end_amdhsa_kernel":
            rname = None
        elif rname:
            res[rname].append(line.strip())
        m = re.match(r"^(_Z\w+):\s", line)
        if m and ".type" not in line:
            name = m.group(1); kernels[name] = []
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name and line.startswith("\t") and not line.strip().startswith((";", ".")):
            kernels[name].append(re.sub(r"\.?L?BB\d+_\d+", "L", line.strip()))
    for k in kernels:                                           # resources ride along as the tail of the instruction stream: `identical` covers both
        kernels[k] += ["; " + l for l in res.get(k, [])]
    return kernels


def stats(body):
    body = [l for l in body if not l.startswith("; ")]
    return len(body), sum(l.startswith("v_") for l in body), sum(l.startswith("scratch_") for l in body)


args = [a for a in sys.argv[1:] if not a.startswith("--")]
pair_appended_false = "--pair-appended-false" in sys.argv[1:]
pair_renamed = [a.split("=", 1)[1].split("=>", 1) for a in sys.argv[1:] if a.startswith("--pair-renamed=")]
rev = args[0] if args else "HEAD"
with tempfile.TemporaryDirectory() as tmp:
    old_tree = os.path.join(tmp, "old"); os.makedirs(old_tree)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "zdr_amd/csrc", "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", old_tree], input=tar, check=True)
    old = assemble(old_tree, os.path.join(tmp, "old.s"))
    new = assemble(ROOT, os.path.join(tmp, "new.s"))
demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().split("(")[0][:70]



def appended_false(name):
    """_Z6k_pathILi0E10BruteAccelLb0ELb0EEv... -> _Z6k_pathILi0E10BruteAccelLb0ELb0ELb0EEv...: the template argument list of a
    function template that returns void ends at the first `Ev`."""
    i = name.find("Ev")
    return name[:i] + "Lb0E" + name[i:] if i > 0 else None


if pair_appended_false:   # rename each old kernel the tree no longer has to its legacy-mode counterpart, when that exists
    for name in [n for n in old if n not in new]:
        twin = appended_false(name)
        if twin in new and twin not in old:
            old[twin] = old.pop(name)
for pattern, replacement in pair_renamed:
    for name in [n for n in old if n not in new]:
        twin = re.sub(pattern, replacement, name)
        if twin != name and twin in new and twin not in old:
            old[twin] = old.pop(name)
changed = 0
for name in sorted(set(old) | set(new)):
    if name not in old or name not in new:
        print(f"{'ADDED' if name in new else 'REMOVED':10s} {demangle(name)}"); changed += 1
    elif old[name] == new[name]:
        a = stats(old[name])
        vgprs = next((l.split()[-1] for l in old[name] if ".amdhsa_next_free_vgpr" in l), "?")
        print(f"identical  {demangle(name)}   instructions {a[0]}, VALU {a[1]}, scratch ops {a[2]}, VGPRs {vgprs}")
    else:
        changed += 1
        a, b = stats(old[name]), stats(new[name])
        print(f"DIFFERENT  {demangle(name)}   instructions {a[0]} -> {b[0]}, VALU {a[1]} -> {b[1]}, scratch ops {a[2]} -> {b[2]}")
print(f"{changed} of {len(set(old) | set(new))} kernels differ from {rev}")
