"""-m gpu: the bilinear texture lookup and its adjoint row by row.  The cases of tests/texture_cases.py through zdr_texture_lookup and
zdr_texture_scatter — lane i calls read_bsdf, read_bsdf_in and env_lookup; the waves call scatter_push / scatter_finish with the ballots the
case deals them, and the fold of the backward calls follows — judged by the float64 reference: the exact family bit for bit in every
storage regime and all three forms, the general families texel by texel and row by row under bounds whose K comes from CPU measurements
only.  No texel and no row is exempt."""
import functools

import numpy as np
import pytest
import torch

import texture_cases as tc
from gpu_util import make_scene
from zdr_amd import _native

pytestmark = pytest.mark.gpu
F64 = np.float64


@functools.lru_cache(None)
def scene(env=False):
    s = make_scene("path")                   # the hooks read no geometry: the scene names the device and holds the map
    if env:                                  # a 16 x 32 map, made square as add_envmap makes it; the texels are replaced per case
        s.add_envmap(np.random.default_rng(5).uniform(0.1, 2.0, (16, 32, 3)).astype(np.float32))
        assert s._envmap[0].shape[:2] == tc.ENV_SIZE
    return s


def packed(arrays):
    return torch.from_numpy(np.concatenate([a.reshape(-1, 4) for a in arrays])).cuda()


def scatter(case, form, rows=None, prefill=True):
    """-> ({entry: gradient (h, w, 4) float32}, copies) of one zdr_texture_scatter call"""
    s = scene(case.env)
    d = packed(case.prefill if prefill else [np.zeros_like(p) for p in case.prefill])
    d_env = None
    if case.env:
        d_env = torch.from_numpy(case.env_prefill if prefill else np.zeros_like(case.env_prefill)).cuda().contiguous()
    copies = s.texture_scatter(form, case.sizes, torch.from_numpy(case.rows() if rows is None else rows), tc.ROUNDS, d, d_env)
    s.check()
    flat, out, off = d.cpu().numpy(), {}, 0
    for k, (h, w) in enumerate(case.sizes):
        out[k] = flat[off:off + h * w].reshape(h, w, 4)
        off += h * w
    if case.env:
        out[tc.ENV_ENTRY] = d_env.cpu().numpy()
    return out, copies


def lookup(case):
    """-> (n_active, 20) float32 of one zdr_texture_lookup call over the case's active material rows, and their indices"""
    s = scene(case.env)
    if case.env:
        s.set_envmap_texture(torch.from_numpy(case.env_texture).cuda())
    i = np.flatnonzero((case.mat >= 0) & (case.mat < len(case.sizes)))
    rows = np.zeros((i.size, 3), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2] = case.u[i], case.v[i], case.mat[i].view(np.float32)
    out = s.texture_lookup(packed(case.textures), case.sizes, torch.from_numpy(rows))
    s.check()
    return out.cpu().numpy(), i


def assert_copies(case, form, copies):
    want = case.copies(single=(form == "single"))
    got = {k: int(c) for k, c in enumerate(copies) if c}
    assert got == want, (case.name, form, got, want)


EXACT = [("single", (s,), False) for s in tc.EXACT_SIZES] + [("table", ((2, 3), s, (1, 1)), False) for s in tc.EXACT_SIZES] + \
        [("table", tuple(tc.TABLES["lds"]), False)] + [("table_env", (s, (3, 5)), True) for s in tc.EXACT_SIZES]


# ----------------------------------------------------------------------------- a., e. the exact family, bit for bit
@pytest.mark.parametrize("form,sizes,env", EXACT, ids=lambda x: x if isinstance(x, str) else ("+".join("%dx%d" % s for s in x) if isinstance(x, tuple) else ""))
def test_exact_family_equals_the_reference_bit_for_bit(form, sizes, env):
    """Every push pattern (wave b deals by PATTERNS[b % 8]), every regime, any number of copies: the float64 answer, and the same bits twice."""
    case = tc.exact_case(sizes, env)
    got, copies = scatter(case, form)
    assert_copies(case, form, copies)
    again, _ = scatter(case, form)
    for k, size, is_env in case.entries():
        ref, _ = case.reference(k)
        bad = np.argwhere(got[k].astype(F64) != ref)
        assert not len(bad), (case.name, form, k, f"{len(bad)} of {ref.size} values differ", bad[:4].tolist(), got[k][tuple(bad[0])], ref[tuple(bad[0])])
        assert got[k].tobytes() == again[k].tobytes(), (case.name, form, k, "two runs differ")


def test_exact_lookup_and_adjointness():
    """c., d. on the exact family: the four forms of the lookup are the float64 value, and sum g . lookup = sum texels . scatter exactly."""
    for sizes, env in [(((2, 3), s, (1, 1)), False) for s in tc.EXACT_SIZES] + [(((17, 33), (3, 5)), True)]:
        case = tc.exact_case(sizes, env)
        out, i = lookup(case)
        grads, _ = scatter(case, "table_env" if env else "table", prefill=False)
        lhs = rhs = 0.0
        for k, size, is_env in case.entries():
            j = case.of(k)
            val, _ = tc.ref_lookup(case.tex(k), case.u[j], case.v[j], env=is_env)
            if is_env:
                s = scene(True)
                rows = np.zeros((j.size, 3), np.float32)
                rows[:, 0], rows[:, 1] = case.u[j], case.v[j]
                e = s.texture_lookup(packed(case.textures), case.sizes, torch.from_numpy(rows)).cpu().numpy()[:, 16:20]
                assert not e[:, 3].any()
                np.testing.assert_array_equal(e[:, :3].astype(F64), val[:, :3], err_msg=case.name + " env_lookup")
                lhs += float((case.g[j, :3].astype(F64) * e[:, :3]).sum())
                rhs += float((case.tex(k)[..., :3].astype(F64) * grads[k][..., :3]).sum())
                continue
            sel = np.flatnonzero(case.mat[i] == k)
            for f in range(4):
                np.testing.assert_array_equal(out[sel, 4 * f:4 * f + 4].astype(F64), val, err_msg=f"{case.name} material {k} form {f}")
            lhs += float((case.g[j].astype(F64) * out[sel, 0:4]).sum())
            rhs += float((case.tex(k).astype(F64) * grads[k]).sum())
        assert lhs == rhs and lhs != 0.0, (case.name, lhs, rhs)


# ----------------------------------------------------------------------------- b., c., d. the general families
@pytest.mark.parametrize("family", tc.UV_FAMILIES)
def test_general_family_is_inside_its_bounds(family):
    """Every texel of every gradient and every row of every lookup inside its bound; narrow = wide and read_bsdf_in = read_bsdf bit for
    bit; adjointness within the sum of the two bounds; a material without rows keeps its pre-fill exactly."""
    worst = {"scatter": 0.0, "lookup": 0.0, "env_lookup": 0.0, "adjoint": 0.0}
    failures = []
    for fam, case, single in tc.all_general_cases():
        if fam != family:
            continue
        form = "single" if single else ("table_env" if case.env else "table")
        assert tc.input_conditions(case) is None
        got, copies = scatter(case, form)
        assert_copies(case, form, copies)
        zero, _ = scatter(case, form, prefill=False)
        out, i = lookup(case)
        assert out[:, 0:4].tobytes() == out[:, 4:8].tobytes(), (case.name, "read_bsdf: narrow and wide differ")
        assert out[:, 8:12].tobytes() == out[:, 12:16].tobytes(), (case.name, "read_bsdf_in: narrow and wide differ")
        same = out[:, 0:4].view(np.uint32) == out[:, 8:12].view(np.uint32)
        assert same.all(), (case.name, "read_bsdf_in differs from read_bsdf", int((~same).sum()), out[~same.all(1)][:2])
        lhs = rhs = slack = 0.0
        for k, size, is_env in case.entries():
            j = case.of(k)
            ref, bound = case.reference(k)
            r = tc.ratio(np.abs(got[k].astype(F64) - ref), bound)
            worst["scatter"] = max(worst["scatter"], r)
            if not r <= 1.0:
                failures.append((case.name, form, "scatter", k, r))
            if not j.size:
                assert got[k].tobytes() == case.pre(k).tobytes(), (case.name, k, "a material without rows lost its pre-fill")
            val, lb = tc.ref_lookup(case.tex(k), case.u[j], case.v[j], env=is_env)
            zref, zbound = tc.ref_scatter(size, case.u[j], case.v[j], case.g[j], np.zeros_like(case.pre(k)), env=is_env)
            if is_env:
                rows = np.zeros((j.size, 3), np.float32)
                rows[:, 0], rows[:, 1] = case.u[j], case.v[j]
                lk = scene(True).texture_lookup(packed(case.textures), case.sizes, torch.from_numpy(rows)).cpu().numpy()[:, 16:19]
                val, lb, key, c = val[:, :3], lb[:, :3], "env_lookup", 3
            else:
                lk, key, c = out[np.flatnonzero(case.mat[i] == k), 0:4], "lookup", 4
            r = tc.ratio(np.abs(lk.astype(F64) - val), lb)
            worst[key] = max(worst[key], r)
            if not r <= 1.0:
                failures.append((case.name, form, key, k, r))
            lhs += float((case.g[j, :c].astype(F64) * lk).sum())
            rhs += float((case.tex(k)[..., :c].astype(F64) * zero[k][..., :c]).sum())
            slack += float((np.abs(case.g[j, :c]).astype(F64) * lb).sum()) + float((np.abs(case.tex(k)[..., :c]).astype(F64) * zbound[..., :c]).sum())
        r = abs(lhs - rhs) / slack if slack else 0.0
        worst["adjoint"] = max(worst["adjoint"], r)
        if not r <= 1.0:
            failures.append((case.name, form, "adjoint", lhs, rhs, slack))
    for name, r in worst.items():
        print(f"[texture] {family:13s} {name:10s} worst error / bound {r:.3f}")
    assert not failures, failures


# ----------------------------------------------------------------------------- f. arguments
def test_texture_hook_arguments():
    s, e = scene(), scene(True)
    L = _native.lib()
    INVALID = -1
    dims = np.array([[3, 5], [2, 2]], np.int32)
    tex = torch.ones((19, 4), device="cuda")
    rows = torch.zeros((64, 8), device="cuda")
    grad = torch.full((19, 4), 7.0, device="cuda")
    d_env = torch.full(tc.ENV_SIZE + (4,), 7.0, device="cuda")
    out = torch.full((64, 20), 7.0, device="cuda")
    copies = np.zeros(16, np.int32)

    def sc(scn=s, form=1, d=dims, nmat=2, r=rows, n=64, rounds=1, g=grad, ge=None):
        return L.zdr_texture_scatter(scn._handle, form, None if d is None else d.ctypes.data, nmat, None if r is None else r.data_ptr(), n, rounds,
                                     None if g is None else g.data_ptr(), None if ge is None else ge.data_ptr(), copies.ctypes.data, None)

    def lk(d=dims, nmat=2, t=tex, r=rows, n=64, o=out):
        return L.zdr_texture_lookup(s._handle, None if t is None else t.data_ptr(), None if d is None else d.ctypes.data, nmat,
                                    None if r is None else r.data_ptr(), n, None if o is None else o.data_ptr(), None)
    assert sc() == 0 and lk() == 0
    torch.cuda.synchronize()
    grad.fill_(7.0); out.fill_(7.0)
    bad_mat = rows.clone(); bad_mat.view(torch.int32)[5, 6] = 2
    bad_lookup = rows.clone(); bad_lookup.view(torch.int32)[5, 2] = 2
    negative = rows.clone(); negative.view(torch.int32)[5, 2] = -1
    env_row = rows.clone(); env_row.view(torch.int32)[5, 6] = tc.ENV_ENTRY
    assert sc(r=bad_mat) == INVALID and b"material" in L.zdr_last_error()
    assert sc(r=env_row) == INVALID                                          # entry 15 is no material outside the third form
    assert sc(d=np.array([[3, 5], [0, 2]], np.int32)) == INVALID
    assert sc(d=np.ones((17, 2), np.int32), nmat=17) == INVALID and sc(nmat=0) == INVALID
    assert sc(form=0) == INVALID and sc(form=3) == INVALID                   # the single form takes one material
    assert sc(form=2, ge=d_env) == INVALID and b"no environment map" in L.zdr_last_error()
    assert sc(scn=e, form=2, d=np.ones((16, 2), np.int32), nmat=16, ge=d_env) == INVALID
    assert sc(scn=e, form=2, ge=None) == INVALID
    assert sc(r=None) == INVALID and sc(g=None) == INVALID and sc(d=None) == INVALID and sc(rounds=0) == INVALID
    assert L.zdr_texture_scatter(None, 1, dims.ctypes.data, 2, rows.data_ptr(), 64, 1, grad.data_ptr(), None, None, None) == INVALID
    assert lk(r=bad_lookup) == INVALID and lk(r=negative) == INVALID
    assert lk(d=np.array([[3, 5], [2, -1]], np.int32)) == INVALID and lk(nmat=17) == INVALID
    assert lk(t=None) == INVALID and lk(r=None) == INVALID and lk(o=None) == INVALID and lk(d=None) == INVALID
    torch.cuda.synchronize()
    assert (grad == 7.0).all() and (out == 7.0).all() and (d_env == 7.0).all()      # nothing was launched
    assert sc(n=0, r=None, g=None) == 0 and lk(n=0, t=None, r=None, o=None) == 0    # n = 0: nothing to read or write
    assert sc(scn=e, form=2, r=env_row, ge=d_env) == 0                       # ... and with a map, entry 15 is the map
    torch.cuda.synchronize()
    assert (grad == 7.0).all() and (d_env == 7.0).all()                      # (zero gradients: += 0)
