"""The renders of tests/test_gpu_offsets.py, as functions that the test calls in its own process (default addressing) and that this file,
run as a script in a fresh child process with ZDR_WIDE_OFFSETS=1, computes again with 64-bit addressing everywhere the kernels have both
forms (the variable is read by the library at every launch):
    python tests/helpers/offsets_cases.py same OUT.npz            the Cornell-box renders, dumps and gradients
    python tests/helpers/offsets_cases.py boundary SIDE OUT.npz   one render with a SIDE x SIDE material
Every result is a dict of numpy arrays."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, SPP = 64, 8                      # 64 items: every wave draws exactly one, so the image is deterministic
BW, BSPP = 32, 4                    # the boundary renders


def split_arrays():
    """The Cornell box with cboxuv.obj's triangles in two instances (as tests/test_gpu_materials.py)."""
    from zdr_amd import geometry
    from zdr_amd.scenes import cbox_models
    a = geometry.assemble(cbox_models())
    b = a.inst_tri_begin
    n = int(b[1]); k = n // 2
    return geometry.from_arrays(a.verts, a.tris, [0, k, n, int(b[2])], np.concatenate([a.inst_xform[:1], a.inst_xform]),
                                np.concatenate([a.inst_emission[:1], a.inst_emission]))


def same_answers():
    import torch
    from path_trace import all_queries
    from zdr_amd.scenes import cbox_material_np, make_scene
    out = {}
    mat = torch.from_numpy(cbox_material_np()).cuda()
    ones = torch.ones((W, W, 4), device="cuda")
    q = torch.from_numpy(all_queries(W, W, SPP)).cuda()
    for accel in ("auto", "bvh"):                       # auto: brute force on the Cornell box
        for integrator in ("path", "direct", "collocated"):
            scene = make_scene(integrator, accel=accel)
            out[f"image_{integrator}_{accel}"] = scene.render_forward(mat, (W, W), SPP, 0).cpu().numpy()
            if integrator == "path":
                g = torch.zeros_like(mat)
                scene.render_backward(ones, g, mat, (W, W), SPP, 0)
                out[f"grad_{accel}"] = g.cpu().numpy()
                out[f"dump_{accel}"] = scene.path_dump(mat, q, (W, W), SPP, 1, d_image=ones).cpu().numpy()   # the backward's paths: seed + 1
            scene.check()
    # a material table with two materials of different sizes
    scene = make_scene("path", arrays=split_arrays())
    scene.material_slots = [0, 1, None]
    small = torch.nn.functional.avg_pool2d(mat.permute(2, 0, 1)[None], 16)[0].permute(1, 2, 0).contiguous()
    out["image_table"] = scene.render_forward_materials([small, mat], (W, W), SPP, 0).cpu().numpy()
    scene.check()
    return out


# The checked-in cboxuv.obj keeps its texture coordinates inside [0.0056, 0.9944] x [0.0056, 0.8767], so no lookup of the Cornell box
# reaches the last rows of a texture — and the texels beyond 2^31 bytes of a 11,586^2 material are its last row and a half.  The
# boundary renders therefore stretch v of the box to [0, 1] (same geometry, same u) and look, through a narrow lens, at the strip of the
# floor along its front edge, where the stretched v runs from 0 upwards: 1e-4 in v is 1.5e-3 scene units there.
V_MIN, V_MAX = 0.005635, 0.876629
BOUNDARY_FOV = 0.004
BOUNDARY_ORIGIN, BOUNDARY_TARGET = (0.0, 1.0, 1.5), (0.0, -0.158, -0.2452)


def boundary_arrays():
    from zdr_amd import geometry
    from zdr_amd.scenes import cbox_models
    a = geometry.assemble(cbox_models())
    verts = a.verts.copy()
    used = np.unique(a.tris[:int(a.inst_tri_begin[1])])
    verts[used, 4] = np.clip((verts[used, 4] - np.float32(V_MIN)) / np.float32(V_MAX - V_MIN), 0.0, 1.0)
    return geometry.from_arrays(verts, a.tris, [int(x) for x in a.inst_tri_begin], a.inst_xform, a.inst_emission)


def boundary_camera():
    from zdr_amd import Camera, float3
    return Camera(fov=BOUNDARY_FOV, origin=float3(*BOUNDARY_ORIGIN), target=float3(*BOUNDARY_TARGET), up=float3(0.0, 1.0, 0.0))


def boundary(side):
    import torch
    from path_trace import all_queries
    from zdr_amd.scenes import make_scene
    gen = torch.Generator(device="cuda"); gen.manual_seed(1234)
    mat = torch.rand((side, side, 4), generator=gen, device="cuda")
    scene = make_scene("path", arrays=boundary_arrays())
    scene.camera = boundary_camera()
    image = scene.render_forward(mat, (BW, BW), BSPP, 0).cpu().numpy()
    dump = scene.path_dump(mat, torch.from_numpy(all_queries(BW, BW, BSPP)).cuda(), (BW, BW), BSPP, 0).cpu().numpy()
    scene.check()
    return {"image": image, "dump": dump}


if __name__ == "__main__":
    if sys.argv[1] == "same":
        np.savez(sys.argv[2], **same_answers())
    else:
        np.savez(sys.argv[3], **boundary(int(sys.argv[2])))
