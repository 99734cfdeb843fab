"""-m gpu: the kernels fetch their records and texels through a scalar base and a 32-bit byte offset (scene.h, load_at) and keep a
64-bit form for buffers of the caller's that do not end within 4 GiB (RenderCfg::wide_offsets).  Both forms must give the same answers,
bit for bit, and the narrow one must be right up to its last byte: a material just over 2 GiB (an offset that a sign extension would
ruin) and one just over 4 GiB (which has to take the wide form by itself).

ZDR_WIDE_OFFSETS=1 forces the wide form; the library reads it at launch, so the forced renders run in a fresh child process
(tests/helpers/offsets_cases.py, which also holds the renders themselves: the same functions run here and there)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import offsets_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

ACCELS = ("auto", "bvh")


def in_child(tmp_path_factory, *args):
    """The renders of offsets_cases.py in a fresh process with the 64-bit form forced."""
    out = str(tmp_path_factory.mktemp("offsets") / "wide.npz")
    env = dict(os.environ, ZDR_WIDE_OFFSETS="1", ZDR_LOG_OFFSETS="1")
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, "tests", "helpers", "offsets_cases.py"), *args, out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    logged = [line for line in r.stderr.splitlines() if line.startswith("[zdr offsets]")]
    assert logged and all("wide=1" in line for line in logged), logged[:3]      # the child really ran the wide form, at every launch
    return dict(np.load(out))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def narrow():
    return cases.same_answers()


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    return in_child(tmp_path_factory, "same")


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("integrator", ["path", "direct", "collocated"])
def test_images_are_the_same_bit_for_bit(integrator, accel, narrow, wide):
    key = f"image_{integrator}_{accel}"
    assert np.abs(narrow[key][..., :3]).sum() > 0
    assert same_bits(narrow[key], wide[key])


def test_material_table_image_is_the_same_bit_for_bit(narrow, wide):
    assert np.abs(narrow["image_table"][..., :3]).sum() > 0
    assert same_bits(narrow["image_table"], wide["image_table"])


@pytest.mark.parametrize("accel", ACCELS)
def test_backward_paths_are_the_same_bit_for_bit(accel, narrow, wide):
    """Every vertex of all 64 x 64 x 8 paths of the backward pass, per-vertex gradients included."""
    from path_trace import Trace
    tr = Trace(narrow[f"dump_{accel}"])
    assert tr.n == cases.W * cases.W * cases.SPP and (tr.grad[tr.live] != 0).any()
    assert same_bits(narrow[f"dump_{accel}"], wide[f"dump_{accel}"])


@pytest.fixture(scope="module")
def oracle_gradient(narrow):
    """The oracle's gradient and the paths that measurably took another branch than the oracle's (gpu_util.Flips), from the dumps of
    the default form (the forced form's are asserted equal to them above)."""
    import oracle
    from gpu_util import Flips, make_scene, oracle_params
    from path_trace import Trace, all_queries
    from zdr_amd import geometry
    from zdr_amd.scenes import cbox_material_np, cbox_models
    A = geometry.assemble(cbox_models())
    S, Sf = oracle.OracleScene.from_arrays(A), oracle.OracleScene.from_arrays(A, variant="fma")
    mat = cbox_material_np()
    scene = make_scene("path")
    W, spp = cases.W, cases.SPP
    ones = np.ones((W, W, 4), np.float32)
    p = oracle_params(scene, W, W, spp, 1, mat.shape[:2])
    q = all_queries(W, W, spp)
    ref, fma = Trace(S.path_dump(p, mat, q, d_image=ones)), Trace(Sf.path_dump(p, mat, q, d_image=ones))
    flips = {accel: Flips(scene, S, Sf, mat, (W, W), spp, 1, cot=ones, what=f"offsets backward {accel}", traces=(Trace(narrow[f"dump_{accel}"]), ref, fma))
             for accel in ACCELS}
    return S.render_backward(p, ones, mat), Sf.render_backward(p, ones, mat), flips


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("form", ["narrow", "wide"])
def test_material_gradient_matches_the_oracle(form, accel, narrow, wide, oracle_gradient):
    from gpu_util import assert_grad_parity
    gref, gfloor, flips = oracle_gradient
    got = (narrow if form == "narrow" else wide)[f"grad_{accel}"]
    assert_grad_parity(got, gref, f"offsets {form} {accel}", floor=gfloor, flips=flips[accel])


# ---- the boundaries ------------------------------------------------------------------------------------------------------
def texel_bytes_reached(dump, side):
    """Highest byte offset of a texel in the bilinear footprint of a primary vertex (read_bsdf: texel (x, y) at x + w y, 16 bytes)."""
    from path_trace import Trace
    tr = Trace(dump)
    uv = tr.uv[:, 0][tr.live[:, 0]]
    assert len(uv) > 0
    px = uv[:, 0] * np.float32(side - 1); py = (np.float32(1.0) - uv[:, 1]) * np.float32(side - 1)
    x1 = np.clip(px.astype(np.int64) + 1, 0, side - 1); y1 = np.clip(py.astype(np.int64) + 1, 0, side - 1)
    return int((x1 + side * y1).max()) * 16


@pytest.mark.parametrize("side,limit,wide_by_itself", [(11586, 1 << 31, False), (16400, 1 << 32, True)])
def test_materials_just_over_2_and_4_gib(side, limit, wide_by_itself, tmp_path_factory, monkeypatch, capfd):
    """A float32 material of side x side x 4: 11,586^2 ends 282,688 bytes past 2^31, 16,400^2 ends 8,392,704 bytes past 2^32.
    The scene is the Cornell box with v stretched to [0, 1] and a lens on the floor's front edge (offsets_cases.py: the fixture's own
    coordinates stop at v = 0.0056, 65 rows short of the last row of the smaller texture), so that primary vertices look up texels beyond
    the boundary — asserted from their uv."""
    import torch
    assert side * side * 16 > limit
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * (1 << 30):
        pytest.skip(f"needs 16 GiB of free device memory, {free / (1 << 30):.1f} GiB are free")
    monkeypatch.delenv("ZDR_WIDE_OFFSETS", raising=False)
    monkeypatch.setenv("ZDR_LOG_OFFSETS", "1")
    capfd.readouterr()
    default = cases.boundary(side)
    torch.cuda.empty_cache()
    logged = [line for line in capfd.readouterr().err.splitlines() if line.startswith("[zdr offsets]")]
    assert logged and all(f"wide={int(wide_by_itself)}" in line for line in logged), logged      # which form the library chose by itself
    reached = texel_bytes_reached(default["dump"], side)
    print(f"[offsets] {side}^2: highest texel of a primary vertex at byte {reached}, boundary {limit}")
    assert reached >= limit
    assert np.abs(default["image"][..., :3]).sum() > 0
    forced = in_child(tmp_path_factory, "boundary", str(side))
    assert same_bits(default["image"], forced["image"])
    assert same_bits(default["dump"], forced["dump"])
