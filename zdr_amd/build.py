"""Ahead-of-time build of libzdr_hip.so (gfx950 only; no JIT, no multi-arch fat binary).

``python -m zdr_amd.build`` or ``zdr_amd.build.build()``.  hipcc cross-compiles without a GPU;
the resulting .so sits in-tree next to the sources so that it travels with the repository
snapshot to the GPU box.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(CSRC, "libzdr_hip.so")
# The texture-space kernels (zdr_texel.hip) are a library of their own that libzdr_hip.so names as a dependency and finds beside itself
# ($ORIGIN): libzdr_hip.so keeps exactly the code objects it had, path kernels first (tests/test_envmap_sampling_resources.py counts them).
TEXEL_LIB = os.path.join(CSRC, "libzdr_texel.so")
# The texture-space light baker (zdr_bake.hip) likewise: a third library, so that libzdr_texel.so keeps exactly its three kernels too.
BAKE_LIB = os.path.join(CSRC, "libzdr_bake.so")
# Push-pull hole filling (zdr_pushpull.hip): a fourth library, for the same reason.
PUSHPULL_LIB = os.path.join(CSRC, "libzdr_pushpull.so")
# Texture-space views of a camera, the gather through them and its adjoint (zdr_project.hip): a fifth library, for the same reason.
PROJECT_LIB = os.path.join(CSRC, "libzdr_project.so")
# The image pyramid, the mip gather and their adjoints (zdr_mip.hip): a sixth library, for the same reason.
MIP_LIB = os.path.join(CSRC, "libzdr_mip.so")
# The footprint ellipse, the anisotropic gather and its adjoint (zdr_aniso.hip): a seventh library, for the same reason.
ANISO_LIB = os.path.join(CSRC, "libzdr_aniso.so")
# The gather plan — the adjoints of the three gathers as CSR rows, built once and applied without atomics (zdr_plan.hip): an eighth library.
PLAN_LIB = os.path.join(CSRC, "libzdr_plan.so")
# Camera gradients — the derivative of a gather in the view buffer and the adjoint of the view buffer in the camera (zdr_viewgrad.hip): a ninth.
VIEWGRAD_LIB = os.path.join(CSRC, "libzdr_viewgrad.so")
# UV tangents — the per-texel tangent buffer and the footprint ellipse of a texel's true patch (zdr_tangent.hip): a tenth, so that
# libzdr_texel.so and libzdr_aniso.so keep exactly their three kernels each.
TANGENT_LIB = os.path.join(CSRC, "libzdr_tangent.so")
# The adjoint of the light baker in the emissions and the environment map (zdr_bakegrad.hip): an eleventh, so that libzdr_bake.so keeps
# exactly its ten kernels.
BAKEGRAD_LIB = os.path.join(CSRC, "libzdr_bakegrad.so")
# The bounced-light baker (zdr_bounce.hip): a twelfth, so that libzdr_bake.so keeps exactly its ten kernels too.
BOUNCE_LIB = os.path.join(CSRC, "libzdr_bounce.so")
# The adjoint of the bounced-light baker in the materials and the emissions (zdr_bouncegrad.hip): a thirteenth, so that libzdr_bounce.so
# keeps exactly its kernels.
BOUNCEGRAD_LIB = os.path.join(CSRC, "libzdr_bouncegrad.so")
# The adjoint of the bounced-light baker in the environment map (zdr_bounceenv.hip): a fourteenth, so that libzdr_bounce.so and
# libzdr_bouncegrad.so keep exactly their kernels.
BOUNCEENV_LIB = os.path.join(CSRC, "libzdr_bounceenv.so")
ARCH = "gfx950"


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the zdr HIP back end needs ROCm (no CPU fallback exists)")


def _sources():
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".cpp", ".h"))] + [
        os.path.join(ROOT, "include", "zdr.h")]


def source_hash() -> str:
    """sha256 over the kernel / host sources and the header, in name order: identifies the code a profile was taken on
    (profiles/pmc_traffic.json carries it; bench.py marks counter figures stale when it differs).  Works without git —
    the GPU box receives a snapshot, not a repository."""
    import hashlib
    h = hashlib.sha256()
    for path in _sources():
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def stale() -> bool:
    if not all(os.path.exists(p) for p in (LIB, TEXEL_LIB, BAKE_LIB, PUSHPULL_LIB, PROJECT_LIB, MIP_LIB, ANISO_LIB, PLAN_LIB, VIEWGRAD_LIB, TANGENT_LIB, BAKEGRAD_LIB, BOUNCE_LIB, BOUNCEGRAD_LIB, BOUNCEENV_LIB)):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(s) > t for s in _sources())


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not stale():
        return LIB
    hipcc = _hipcc()
    common = [f"--offload-arch={ARCH}", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    jobs = [
        # kernels: default contraction (FMA) for speed; NO fast-math (NaN policy, integrator.py:27).
        # -fno-slp-vectorize: hipcc otherwise packs scalar f32 math into v_pk_*_f32, which on gfx950
        # runs at the same FLOP rate as the scalar forms and pays extra moves to build register
        # pairs: measured 23.9 -> 17.7 ms on the cbox forward pass (profiles/r1_ab_flags.txt).
        ("zdr_kernels.hip", ["-O3", "-munsafe-fp-atomics", "-fno-slp-vectorize", *os.environ.get("ZDR_KERNEL_FLAGS", "").split()]),
        # host side: IEEE float32 for the per-triangle constants
        # (-D options of ZDR_KERNEL_FLAGS go to both halves: some macros size shared workspaces)
        ("zdr_api.cpp", ["-O2", "-ffp-contract=off", "-x", "hip", *[f for f in os.environ.get("ZDR_KERNEL_FLAGS", "").split() if f.startswith("-D")]]),
        # the denoiser's kernels, a translation unit of their own (linked last: the path kernels' code object stays the first in the
        # library); no fast-math either, and none of the measurement macros reach it
        ("zdr_denoise.hip", ["-O3", "-fno-slp-vectorize"]),
        # the environment-table kernels, likewise on their own and behind the denoiser's; no contraction: the weight map follows the
        # host's float32 operations one by one (zdr_amd/envmap.py)
        ("zdr_envmap.hip", ["-O3", "-fno-slp-vectorize", "-ffp-contract=off"]),
        # the texture-space rasteriser, last and linked into libzdr_texel.so; no contraction: two triangles that share an edge must
        # compute the same edge function, whatever it is inlined into (include/zdr.h, zdr_scene_texel_aovs)
        ("zdr_texel.hip", ["-O3", "-fno-slp-vectorize", "-ffp-contract=off"]),
        # the texture-space light baker, linked into libzdr_bake.so: the path kernels' device code (sample_light, the any-hit walks)
        # under the path kernels' flags, without the atomics option (it has no float atomic)
        ("zdr_bake.hip", ["-O3", "-fno-slp-vectorize"]),
        # push-pull hole filling, linked into libzdr_pushpull.so; no contraction: the result is defined by the operation order of
        # include/zdr.h (zdr_push_pull), and a level computes the same bits in the fused tail as in a launch of its own
        ("zdr_pushpull.hip", ["-O3", "-fno-slp-vectorize", "-ffp-contract=off"]),
        # texture-space views, linked into libzdr_project.so; no contraction: the gather's bits are defined by the operation order of
        # include/zdr.h (zdr_texel_gather), and the projection inverts the camera ray in plain float32; its adjoint scatters with float
        # atomics, which the option turns into global_atomic_add_f32 as in the path kernels
        ("zdr_project.hip", ["-O3", "-fno-slp-vectorize", "-ffp-contract=off", "-munsafe-fp-atomics"]),
        # the image pyramid and the mip gather, linked into libzdr_mip.so, under the flags of zdr_project.hip: the operation order of
        # include/zdr.h defines the bits (a level is the same in a fused launch as in one of its own), and the scatter's atomics
        # become global_atomic_add_f32
        ("zdr_mip.hip", ["-O3", "-fno-slp-vectorize", "-ffp-contract=off", "-munsafe-fp-atomics"]),
        # the footprint ellipse and the anisotropic gather, linked into libzdr_aniso.so, under the flags of zdr_mip.hip: a probe is the
        # mip gather's trilinear sample operation for operation, and one probe must give that gather's bits
        ("zdr_aniso.hip", ["-O3", "-fno-slp-vectorize", "-ffp-contract=off", "-munsafe-fp-atomics"]),
        # the gather plan, linked into libzdr_plan.so, under the flags of zdr_mip.hip without the atomics option (it has no float atomic):
        # a weight is the scatter kernels' own product, and the sums follow the operation order of include/zdr.h
        ("zdr_plan.hip", ["-O3", "-fno-slp-vectorize", "-ffp-contract=off"]),
        # camera gradients, linked into libzdr_viewgrad.so, under the flags of zdr_plan.hip (no float atomic here either): the taps and
        # lerps are the gathers' own, and the sums follow the operation order of include/zdr.h
        ("zdr_viewgrad.hip", ["-O3", "-fno-slp-vectorize", "-ffp-contract=off"]),
        # UV tangents, linked into libzdr_tangent.so, under the flags of zdr_aniso.hip without the atomics option (it has no float atomic):
        # the degenerate test is the rasteriser's and the ellipse the footprint kernel's, float for float (texel_setup.h, footprint.h)
        ("zdr_tangent.hip", ["-O3", "-fno-slp-vectorize", "-ffp-contract=off"]),
        # the adjoint of the light baker, linked into libzdr_bakegrad.so, under the flags of zdr_bake.hip plus the atomics option: its
        # sums into the emission accumulator and the environment map become global_atomic_add_f32
        ("zdr_bakegrad.hip", ["-O3", "-fno-slp-vectorize", "-munsafe-fp-atomics"]),
        # the bounced-light baker, linked into libzdr_bounce.so, under the flags of zdr_bake.hip (no float atomic here either): the
        # closest-hit and any-hit walks, surface_interact, the material lookup and sample_light of the path kernels
        ("zdr_bounce.hip", ["-O3", "-fno-slp-vectorize"]),
        # the adjoint of the bounced-light baker, linked into libzdr_bouncegrad.so, under the flags of zdr_bakegrad.hip: the walk of
        # zdr_bounce.hip once more, and its sums into the staging cells and the emission accumulator become global_atomic_add_f32
        ("zdr_bouncegrad.hip", ["-O3", "-fno-slp-vectorize", "-munsafe-fp-atomics"]),
        # the adjoint of the bounced-light baker in the environment map, linked into libzdr_bounceenv.so, under the flags of
        # zdr_bouncegrad.hip: the walk once more, and its sums into the map become global_atomic_add_f32
        ("zdr_bounceenv.hip", ["-O3", "-fno-slp-vectorize", "-munsafe-fp-atomics"]),
    ]
    procs = []
    for src, extra in jobs:
        obj = os.path.join(CSRC, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        cmd = [hipcc, *extra, *common, "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out}")
    bounceenv_obj = objs.pop()                              # (zdr_bounceenv.o: the last job)
    bouncegrad_obj = objs.pop()                             # (zdr_bouncegrad.o: the one before)
    bounce_obj = objs.pop()                                 # (zdr_bounce.o: the one before)
    bakegrad_obj = objs.pop()                               # (zdr_bakegrad.o: the one before)
    tangent_obj = objs.pop()                                # (zdr_tangent.o: the one before)
    viewgrad_obj = objs.pop()                               # (zdr_viewgrad.o: the one before)
    plan_obj = objs.pop()                                   # (zdr_plan.o: the one before)
    aniso_obj = objs.pop()                                  # (zdr_aniso.o: the one before)
    mip_obj = objs.pop()                                    # (zdr_mip.o: the one before)
    project_obj = objs.pop()                                # (zdr_project.o: the one before)
    pushpull_obj = objs.pop()                               # (zdr_pushpull.o: the one before)
    bake_obj = objs.pop()                                   # (zdr_bake.o: the one before)
    texel_obj = objs.pop()                                  # (zdr_texel.o: the one before that)
    links = [[hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", TEXEL_LIB, texel_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", BAKE_LIB, bake_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", PUSHPULL_LIB, pushpull_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", PROJECT_LIB, project_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", MIP_LIB, mip_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", ANISO_LIB, aniso_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", PLAN_LIB, plan_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", VIEWGRAD_LIB, viewgrad_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", TANGENT_LIB, tangent_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", BAKEGRAD_LIB, bakegrad_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", BOUNCE_LIB, bounce_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", BOUNCEGRAD_LIB, bouncegrad_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", BOUNCEENV_LIB, bounceenv_obj],
             [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB, *objs, "-Wl,--no-as-needed", "-L" + CSRC, "-lzdr_texel", "-lzdr_bake", "-lzdr_pushpull",
              "-lzdr_project", "-lzdr_mip", "-lzdr_aniso", "-lzdr_plan", "-lzdr_viewgrad", "-lzdr_tangent", "-lzdr_bakegrad", "-lzdr_bounce", "-lzdr_bouncegrad", "-lzdr_bounceenv",
              "-Wl,-rpath,$ORIGIN"]]
    for cmd in links:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
