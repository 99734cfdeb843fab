"""The checker of tests/envmap_tables.py on the host: it accepts the tables zdr_amd/envmap.py builds for every map family, rejects
tables broken on purpose, and its measured constants hold for the maps built here.  Also: the bindings and keywords of the on-device
rebuild exist (zdr_scene_update_envmap_sampling).  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import envmap_tables as T
from conftest import ROOT
from zdr_amd import _native
from zdr_amd import envmap as E

W, H = T.W, T.H
SHAPE = (16, 32)


@pytest.fixture(scope="module")
def host():
    """{(family, compensate_mis): (image, prob, alias, pdf)} at the smallest shape"""
    out = {}
    for family in T.FAMILIES:
        img = T.make_map(family, SHAPE)
        for comp in (True, False):
            out[family, comp] = (img,) + T.host_tables(img, comp)
    return out


def test_host_tables_are_build_tables_bit_for_bit():
    """the memoised weight map of T.host_tables changes nothing"""
    img = T.make_map("sun_sky", SHAPE)
    for a, b in zip(T.host_tables(img, True), E.build_tables(E.prepare_image(img), compensate_mis=True)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("family", T.FAMILIES)
def test_the_checker_accepts_the_host_tables_and_the_constants_cover_them(family, host):
    for comp in (True, False):
        img, prob, alias, pdf = host[family, comp]
        q = T.check_tables(prob, alias, pdf, bar=T.Q_BAR)
        a = T.agreement(T.pdf64(img, comp), pdf) if family != "constant" else float("nan")
        print(f"[envmap tables] {family} compensate_mis {int(comp)}: table residual {q:.3e} (measured {T.Q_MEASURED:.3e}), "
              f"host float32 vs float64 pdf {a:.3e} (measured {T.AGREE_MEASURED:.3e}), pdf == 0: {float((pdf == 0).mean()):.3f}")
        assert q <= T.Q_MEASURED                                     # the constants are maxima over these maps and more
        if family != "constant":
            assert a <= T.AGREE_MEASURED
    assert T.Q_BAR == max(4.0 * T.Q_MEASURED, 2.0 ** -20) and T.AGREE_BAR == 4.0 * T.AGREE_MEASURED and T.AGREE_MEASURED > 0.0


def test_the_families_are_what_they_are_meant_to_be(host):
    assert (host["black", True][3] == 1.0).all() and (host["black", True][1] == 1.0).all()      # every total 0: uniform
    assert float((host["sun_sky", True][3] == 0).mean()) > 0.5                                    # compensation zeroes most of the map
    assert float((host["black_rows", True][3] == 0).mean()) > 0.5
    assert float((host["random_hdr", False][3] == 0).mean()) == 0.0


def test_the_margins_file_states_the_constants():
    txt = open(os.path.join(ROOT, "profiles", "envmap_sampling_margins.txt")).read()
    q = float(re.search(r"^Q_MEASURED = (\S+)", txt, re.M).group(1)); a = float(re.search(r"^AGREE_MEASURED = (\S+)", txt, re.M).group(1))
    assert q <= T.Q_MEASURED <= 1.01 * q and a <= T.AGREE_MEASURED <= 1.01 * a, (q, T.Q_MEASURED, a, T.AGREE_MEASURED)


def _broken(host, family="sun_sky"):
    img, prob, alias, pdf = host[family, True]
    return prob.copy(), alias.copy(), pdf.copy()


def _zero_texel_in_a_live_row(pdf):
    p = pdf.reshape(H, W)
    y = int(np.argmax((p.sum(axis=1) > 0) & ((p == 0).sum(axis=1) > 0)))
    assert p[y].sum() > 0 and (p[y] == 0).any()
    return y, int(np.argmax(p[y] == 0)), int(np.argmax(p[y]))


def test_the_checker_rejects_an_alias_that_points_at_a_texel_without_density(host):
    prob, alias, pdf = _broken(host)
    y, x0, xmax = _zero_texel_in_a_live_row(pdf)
    i = H + y * W + int(np.argmax((pdf.reshape(H, W)[y] > 0) & (prob[H + y * W:H + (y + 1) * W] < 1)))
    assert prob[i] < 1
    alias[i] = x0
    with pytest.raises(AssertionError, match="pdf 0"):
        T.check_tables(prob, alias, pdf, bar=T.Q_BAR)


def test_the_checker_rejects_a_zero_weight_entry_that_keeps_itself(host):
    prob, alias, pdf = _broken(host)
    y, x0, xmax = _zero_texel_in_a_live_row(pdf)
    prob[H + y * W + x0] = 1.0; alias[H + y * W + x0] = x0
    with pytest.raises(AssertionError, match="pdf 0"):
        T.check_tables(prob, alias, pdf, bar=T.Q_BAR)


def test_the_checker_rejects_a_prob_above_one(host):
    prob, alias, pdf = _broken(host, "random_hdr")
    prob[H + 5 * W + 7] = np.float32(1.0 + 2.0 ** -20)
    with pytest.raises(AssertionError, match=r"prob outside \[0, 1\]"):
        T.check_tables(prob, alias, pdf, bar=T.Q_BAR)
    prob[H + 5 * W + 7] = np.nan
    with pytest.raises(AssertionError, match=r"prob outside \[0, 1\]"):
        T.check_tables(prob, alias, pdf, bar=T.Q_BAR)
    alias[3] = H
    with pytest.raises(AssertionError):
        T.check_tables(_broken(host, "random_hdr")[0], alias, pdf, bar=T.Q_BAR)


def test_the_checker_rejects_a_row_table_swapped_with_its_neighbours(host):
    prob, alias, pdf = _broken(host, "random_hdr")
    a, b = slice(H + 100 * W, H + 101 * W), slice(H + 101 * W, H + 102 * W)
    for t in (prob, alias):
        t[a], t[b] = t[b].copy(), t[a].copy()
    with pytest.raises(AssertionError, match="disagree"):
        T.check_tables(prob, alias, pdf, bar=T.Q_BAR)


def test_the_checker_rejects_a_scaled_pdf(host):
    prob, alias, pdf = _broken(host, "random_hdr")
    with pytest.raises(AssertionError, match="mean"):
        T.check_tables(prob, alias, pdf * np.float32(1.01), bar=T.Q_BAR)
    i = int(np.argmin(np.where(pdf > 0, pdf, np.inf)))               # the smallest positive density, negated: the mean hardly moves
    pdf[i] = -pdf[i]
    with pytest.raises(AssertionError):
        T.check_tables(prob, alias, pdf, bar=T.Q_BAR)


def test_the_bindings_and_the_keywords_of_the_device_rebuild_exist():
    from zdr_amd.render import Scene
    hdr = open(os.path.join(ROOT, "include", "zdr.h")).read()
    for name in ("zdr_scene_update_envmap_sampling", "zdr_scene_get_envmap_sampling"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _native.EXPORTS, name
        assert hasattr(_native.lib(), name), name
    assert int(re.search(r"#define ZDR_ABI_VERSION (\d+)", hdr).group(1)) == 4
    sig = inspect.signature(Scene.update_envmap_sampling).parameters
    assert list(sig)[1:] == ["image", "compensate_mis", "on_device"] and sig["on_device"].default is False and sig["compensate_mis"].default is True
    assert inspect.signature(Scene.render).parameters["update_sampling"].default is False
    assert inspect.signature(Scene.render).parameters["update_sampling"].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(Scene.envmap_sampling_tables)


def test_a_library_without_the_table_kernels_would_still_load():
    """zdr_api.cpp references the launcher weakly (csrc/envsample.h), like the denoiser's: the host-only link of
    tests/test_host_sanitizers.py has no zdr_envmap.o"""
    api = open(os.path.join(ROOT, "zdr_amd", "csrc", "zdr_api.cpp")).read()
    assert "if (!zdr_launch_envmap_sampling)" in api
