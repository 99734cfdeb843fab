"""What the GPU tests of the bounced light (tests/test_gpu_texel_bounce.py) and the tool that records their figures
(tools/texel_bounce_margins.py) share: a scene per case and accelerator, the forward call, the dump of every sample of a case in the order
of the reference's rows, and the comparison of the kernels' walks with the free-running float64 reference.  Needs a GPU; not a test."""
import numpy as np
import torch

import texel_bounce_cases as BC
import texel_bounce_ref as BR
from zdr_amd import Scene
from zdr_amd import _native as N

ACCELS = ["brute", "bvh"]
_scenes = {}


def case_scene(name, accel):
    make, env = BC.case(name)[0], BC.case(name)[6]
    key = (make, env, accel, BC.SAMPLERS.get(name))
    if key not in _scenes:
        scene = Scene(make(), integrator="direct", accel=accel)
        if name in BC.SAMPLERS:                                   # a handle of its own, with the tables the reference draws from
            scene.set_pmj02bn_tables(*BC.pmj_tables(name))
        if env:                                                   # the tables the reference uses, as they are
            tex, prob, alias, pdf, mw, mh = env()
            N.check(N.lib().zdr_scene_set_envmap(scene._handle, tex.ctypes.data, tex.shape[0], tex.shape[1], prob.ctypes.data, alias.ctypes.data,
                                                 pdf.ctypes.data, mw, mh))
            scene.env_count = 1
            scene._envmap = (tex, prob, alias, pdf)
        assert scene.info()["accel"] == accel
        _scenes[key] = scene
    return _scenes[key]


def case_args(name, mats=None):
    return (torch.from_numpy(BC.points(name)).cuda(), [torch.from_numpy(m).cuda() for m in (BC.materials(name) if mats is None else mats)])


def case_kw(name, **kw):
    kw.setdefault("samples", BC.RANGES.get(name))
    kw.setdefault("bounces", BC.bounces(name))
    return dict(spp=BC.case(name)[4], seed=BC.SEED, sampler="pmj02bn" if name in BC.SAMPLERS else None, slots=BC.case(name)[1], **kw)


def run_forward(name, accel, mats=None, **kw):
    pts, m = case_args(name, mats)
    out = case_scene(name, accel).texel_bounce_forward(pts, m, **case_kw(name, **kw))
    torch.cuda.synchronize()
    return out.cpu().numpy()


_dumps = {}


def run_dump(name, accel, **kw):
    """the dump of every sample of the case, in the order of the reference's rows, parsed; computed once per (case, accelerator, arguments)"""
    key = (name, accel, tuple(sorted(kw.items())))
    if key not in _dumps:
        pts, m = case_args(name)
        ckw = case_kw(name, **kw)
        begin, end = ckw["samples"] if ckw["samples"] is not None else (0, ckw["spp"])
        q = BC.reference(name)["queries"] if (kw.get("samples") is None) else None
        if q is None:
            full = BC.reference(name)["queries"]
            q = full[(full[:, 2] >= begin) & (full[:, 2] < end)]
        rows = case_scene(name, accel).texel_bounce_dump(pts, m, torch.from_numpy(np.ascontiguousarray(q)), **ckw)
        torch.cuda.synchronize()
        _dumps[key] = (q, BR.parse_dump(rows.cpu().numpy(), ckw["bounces"]))
    return _dumps[key]


def walk_differences(name, accel):
    """(agree, line): the samples whose nvert and triangles agree with the free-running reference, and the line of
    profiles/texel_bounce_margins.txt with the largest |u, v| differences per vertex index over them"""
    q, dump = run_dump(name, accel)
    ref = BC.reference(name)
    agree = BR.triangles_equal(ref, dump)
    duv = []
    for k in range(BC.bounces(name)):
        m = agree & (dump["nvert"] > k)
        duv.append(float(np.abs(dump["uv"][m, k].astype(np.float64) - ref["uv"][m, k]).max()) if m.any() else 0.0)
    return agree, (f"[texel bounce walk] {name} {accel}: nvert and triangles agree on {int(agree.sum())} of {agree.size} samples; "
                   "largest |u, v| difference per vertex index: " + ", ".join(f"{d:.2e}" for d in duv))
