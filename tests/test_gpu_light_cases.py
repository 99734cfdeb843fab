"""-m gpu: the light side of a path vertex point by point.  Every row of every family of tests/light_cases.py through zdr_light_dump — lane i
calls sample_light, sample_light_pdf, env_sampled_light_pdf, env_lookup, uv_to_direction, direction_to_uv, env_pdf_scale,
balanced_heuristic, offset_ray_origin, sample_uniform_triangle, tent_warp1 and surface_interact on the scene's own tables — and every output
of every row judged by the float64 reference: bit for bit where float32 is exact, under the bound of its own conditioning elsewhere
(K, KT from CPU measurements only).  Then what the outputs must satisfy among themselves: the pdf of a sampled direction, looked up again."""
import functools

import numpy as np
import pytest
import torch

import light_cases as lc
from gpu_util import make_scene
from zdr_amd import _native

pytestmark = pytest.mark.gpu
CASES = [(name, scene) for name, scenes in lc.PLAN for scene in scenes]


@functools.lru_cache(None)
def scene(name):
    s = make_scene("path", arrays=lc.scene_arrays(name), accel=lc.ACCEL.get(name, "auto"))
    if name.endswith("_env"):                 # the hand-made 8 x 4 sample map: the tables go in as they are
        tex, prob, alias, pdf = lc.env_tables()
        _native.check(_native.lib().zdr_scene_set_envmap(s._handle, tex.ctypes.data, tex.shape[0], tex.shape[1], prob.ctypes.data, alias.ctypes.data,
                                                         pdf.ctypes.data, lc.MAP_W, lc.MAP_H))
        s.env_count = 1
    T = lc.tables(name)
    assert s.info()["light_count"] == T.light_count
    return s


def dump(scene_name, mode, rows):
    s = scene(scene_name)
    out = s.light_dump(mode, torch.from_numpy(np.array(rows, np.float32)))
    s.check()
    return out.cpu().numpy()


@functools.lru_cache(None)
def answers(name, scene_name):
    mode, rows = lc.family(name, scene_name)
    o = dump(scene_name, mode, rows)
    o.setflags(write=False)
    return o


def report_hit(o):
    return o[:, 0].view(np.int32).astype(np.int64), o[:, 1].view(np.int32).astype(np.int64), o[:, 2].copy(), o[:, 3].copy()


# ----------------------------------------------------------------------------- a. every family, every row
@pytest.mark.parametrize("name,scene_name", CASES)
def test_every_row_is_exact_or_inside_its_bound(name, scene_name):
    o = answers(name, scene_name)
    mode, rows = lc.family(name, scene_name)
    hit = None
    if name == "interact":
        hit = report_hit(o)
        S = lc.oracle_scene(scene_name)                           # the walk is judged by tests/ray_cases.py; here only that the report names a triangle of the scene
        inst, prim = hit[0], hit[1]
        h = inst >= 0
        assert (inst[h] < S.ninst).all() and (prim[h] >= 0).all() and (prim[h] < np.diff(lc.tables(scene_name).begin)[inst[h]]).all()
        assert h.mean() > 0.5
        wide = dump(scene_name, "interact_wide", rows)
        assert np.array_equal(o.view(np.uint32), wide.view(np.uint32))                  # surface_interact<false> reads the same record
    v = lc.judge(name, scene_name, o, hit=hit)
    v.assert_all_inside(f"{name}/{scene_name}")
    if mode == "sample":
        assert not o[:, 11:].any()
        c, ref = lc.reference(name, scene_name)
        mesh = ~ref["env"]
        assert (o[mesh, 8:10] == -1).all()
    if mode == "pdf":
        assert np.array_equal(o[:, 0].view(np.uint32), o[:, 1].view(np.uint32))         # narrow against wide, bit for bit
        slot = o[:, 2].view(np.int32)
        assert (slot >= 0).all() and (slot < lc.tables(scene_name).P.shape[0]).all()
    print(f"[light] {name}/{scene_name}: accepted under a flipped decision {int(v.used.sum())} of {len(v.ok)} rows")
    assert v.used.mean() <= lc.OPEN_CAP


# ------------------------------------------------------- b. consistency, from what the kernels themselves return
@pytest.mark.parametrize("scene_name", ["cbox_env", "quad_env"])
def test_the_pdf_and_radiance_of_an_environment_sample_are_found_again_from_its_direction(scene_name):
    """For every row that took the environment branch: env_sampled_light_pdf(wi) is the sampled pdf and env_lookup(direction_to_uv(wi))
    the sampled radiance — the two sides of the MIS weight.  Both answers are judged against the float64 value at the sampled map
    coordinates; the way back carries wi's own bound.  Rows whose wi lies within that bound of a border of the sample map or of a
    texel footprint (an open decision of either way) are counted, not judged.  Before direction_to_uv wrapped u into [0, 1), every row
    with wi.x < 0 failed here."""
    for name in ("sample", "alias") if scene_name == "quad_env" else ("sample",):
        T = lc.tables(scene_name)
        mode, rows = lc.family(name, scene_name)
        o = answers(name, scene_name)
        c, ref = lc.reference(name, scene_name)
        env = ref["env"]
        back = np.zeros((len(rows), 16), np.float32)
        back[:, 0:3] = o[:, 0:3]
        back[:, 3:5] = 0.5
        b = dump(scene_name, "env", back)
        cb = lc.Ctx()
        d = [lc.Num(cb, ref["wi"][k].v, ref["wi"][k].e) for k in range(3)]
        rb = lc.eval_env(cb, T, back, d=d)
        opened, lookup_open = np.zeros(len(rows), bool), np.zeros(len(rows), bool)
        for sites, mask in ((cb.open, opened), (c.open, opened)):
            for site, m in sites.items():
                if site.startswith("back_"):
                    continue
                (lookup_open if site.startswith("tex_") else mask).__ior__(np.broadcast_to(m, mask.shape))
        with np.errstate(all="ignore"):
            e_pdf = rb["pdf"].e + ref["pdf"].e
            judged = env & ~opened & np.isfinite(e_pdf)
            d_pdf = np.abs(b[:, 2].astype(np.float64) - o[:, 4].astype(np.float64))
            bad = judged & ~(d_pdf <= e_pdf)
            left = judged & (o[:, 0] < 0)
            print(f"[light] {name}/{scene_name}: environment rows {int(env.sum())}, judged {int(judged.sum())} ({int(left.sum())} with wi.x < 0), near a border {int((env & opened).sum())}; "
                  f"pdf found again: worst difference / bound {np.where(judged, d_pdf / np.where(e_pdf > 0, e_pdf, 1), 0).max():.3f}, outside {int(bad.sum())}")
            assert judged.sum() >= 200 and left.sum() >= 0.3 * judged.sum()      # (the lattice points of the family sit ON the map's borders: exact going out, open coming back)
            assert not bad.any(), np.flatnonzero(bad)[:8].tolist()
            for k in range(3):
                e_l = rb["lookup"][k].e + ref["eval"][k].e
                d_l = np.abs(b[:, 3 + k].astype(np.float64) - o[:, 5 + k].astype(np.float64))
                bad = judged & ~lookup_open & np.isfinite(e_l) & ~(d_l <= e_l)
                assert not bad.any(), (k, np.flatnonzero(bad)[:8].tolist())


@pytest.mark.parametrize("scene_name", ["cbox", "stage", "chandelier", "cbox_env"])
def test_the_pdf_of_a_mesh_sample_is_found_again_from_its_point(scene_name):
    """sample_light_pdf(origin, inst, slot, p) at the point a mesh sample chose is the sample's pdf: the point is the float64 one rounded
    to float32 (the hook returns wi and dist, not p), its rounding part of the bound."""
    T = lc.tables(scene_name)
    mode, rows = lc.family("sample", scene_name)
    o = answers("sample", scene_name)
    c, ref = lc.reference("sample", scene_name)
    mesh = ~ref["env"]
    tri = np.where(mesh, ref["tri"], 0)
    q = np.zeros((len(rows), 16), np.float32)
    q[:, 0:3] = rows[:, 0:3]
    q[:, 3:6] = np.stack([ref["p"][k].v for k in range(3)], 1).astype(np.float32)
    q[:, 6], q[:, 7] = T.tri_inst[tri].astype(np.int32).view(np.float32), tri.astype(np.int32).view(np.float32)
    b = dump(scene_name, "pdf", q)
    cb = lc.Ctx()
    p = [lc.Num(cb, ref["p"][k].v, lc.U * np.abs(ref["p"][k].v)) for k in range(3)]
    rb = lc.eval_pdf(cb, T, q, p=p)
    opened = np.zeros(len(rows), bool)
    for m in c.open.values():
        opened |= np.broadcast_to(m, opened.shape)
    with np.errstate(all="ignore"):
        e = rb["pdf"].e + ref["pdf"].e
        judged = mesh & ~opened & np.isfinite(e)
        d = np.abs(b[:, 0].astype(np.float64) - o[:, 4].astype(np.float64))
        bad = judged & ~(d <= e)
        print(f"[light] sample/{scene_name}: mesh rows {int(mesh.sum())}, judged {int(judged.sum())}; pdf found again: worst difference / bound "
              f"{np.where(judged, d / np.where(e > 0, e, 1), 0).max():.3f}, outside {int(bad.sum())}")
        assert judged.sum() >= 0.7 * mesh.sum()
        assert not bad.any(), np.flatnonzero(bad)[:8].tolist()


# ------------------------------------------------------------------------------------- c. the hook itself
@pytest.mark.parametrize("n", [1, 63, 65])
def test_rows_beyond_n_are_untouched(n):
    L = _native.lib()
    for scene_name, mode, fam in (("cbox_env", 0, "sample"), ("cbox", 1, "pdf"), ("cbox_env", 2, "env"), ("quad", 3, "misc"), ("cbox", 4, "interact"), ("terrain", 5, "interact")):
        s = scene(scene_name)
        full = lc.family(fam, scene_name)[1][:128]
        rows = torch.from_numpy(np.array(full)).to(s.device)
        out = torch.full((128, 16), -777.0, device=s.device)
        assert L.zdr_light_dump(s._handle, mode, rows.data_ptr(), n, out.data_ptr(), None) == 0
        s.check()
        o = out.cpu().numpy()
        assert (o[n:] == -777.0).all(), (mode, n)
        ref = dump(scene_name, list(s.LIGHT_MODES)[mode], full)
        assert np.array_equal(o[:n].view(np.uint32), ref[:n].view(np.uint32)), (mode, n)      # a row's answer does not depend on n


def test_a_row_that_names_no_triangle_reads_nothing():
    rows = np.zeros((4, 16), np.float32)
    rows[:, 6] = np.array([-1, 0, 10 ** 6, 0], np.int32).view(np.float32)
    rows[:, 7] = np.array([0, -1, 0, 10 ** 8], np.int32).view(np.float32)
    o = dump("cbox", "pdf", rows)
    assert np.isnan(o[:, 0:2]).all() and (o[:, 2].view(np.int32) == -1).all()


def test_light_dump_arguments():
    L = _native.lib()
    s, plain = scene("cbox_env"), scene("cbox")
    rows = torch.zeros((64, 16), device=s.device); rows[:, 1] = 1
    out = torch.zeros((64, 16), device=s.device)
    good = [s._handle, 0, rows.data_ptr(), 64, out.data_ptr(), None]
    for mode in range(6):
        args = list(good); args[1] = mode
        assert L.zdr_light_dump(*args) == 0
    torch.cuda.synchronize()
    for k in (0, 2, 4):
        args = list(good); args[k] = None
        assert L.zdr_light_dump(*args) == -1 and b"null" in L.zdr_last_error(), k                   # ZDR_E_INVALID
    for mode in (-1, 6, 99):
        args = list(good); args[1] = mode
        assert L.zdr_light_dump(*args) == -1 and b"mode" in L.zdr_last_error(), mode
    args = list(good); args[0] = plain._handle; args[1] = 2
    assert L.zdr_light_dump(*args) == -1 and b"environment" in L.zdr_last_error()                    # ZDR_LIGHT_ENV without a map
    args = list(good); args[3] = 0; args[2] = None; args[4] = None
    assert L.zdr_light_dump(*args) == 0                                                              # n = 0: nothing to read or write
    args[1] = 7
    assert L.zdr_light_dump(*args) == -1                                                             # ... but the mode is still checked
    assert s.light_dump("misc", torch.empty((0, 16))).shape == (0, 16)
    with pytest.raises(KeyError):
        s.light_dump("nonsense", rows)
    s.check(); plain.check()
