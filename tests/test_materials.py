"""CPU-side checks of the material slots (one material per model, include/zdr.h zdr_scene_set_material_slots and
zdr_render_*_materials): the C-ABI exports and the binding, and the slot-table validation of zdr_amd/render.py."""
import os
import re

import pytest

from conftest import ROOT
from zdr_amd import _native
from zdr_amd.render import check_material_slots, default_material_slots, resolve_material_slots

NEW = ("zdr_scene_set_material_slots", "zdr_render_forward_materials", "zdr_render_backward_materials")


def test_material_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "zdr.h")).read()
    assert int(re.search(r"#define ZDR_MAX_MATERIALS (\d+)", hdr).group(1)) == _native.MAX_MATERIALS == 16
    L = _native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _native.EXPORTS
        assert getattr(L, name).argtypes, name          # bound with a signature, not called through ctypes' defaults


def test_slot_table_of_the_wrong_length_is_refused():
    with pytest.raises(ValueError):
        check_material_slots([0, None], 3)
    with pytest.raises(ValueError):
        check_material_slots([0, None, None, 1], 3)
    with pytest.raises(ValueError):
        check_material_slots(0, 1)
    assert check_material_slots([0, None, 1], 3) == (0, None, 1)


def test_slot_values_outside_the_table_are_refused():
    for bad in (-1, 16, 1.0, True, "0"):
        with pytest.raises(ValueError):
            check_material_slots([bad, None], 2)
    assert check_material_slots([15, None], 2) == (15, None)


def test_a_slot_past_the_list_of_materials_is_refused():
    slots = check_material_slots([0, 2, None], 3)
    with pytest.raises(ValueError):
        resolve_material_slots(slots, [0, 0, 20], 2)
    assert resolve_material_slots(slots, [0, 0, 20], 3) == (0, 2, None)


def test_more_than_sixteen_materials_are_refused():
    with pytest.raises(ValueError):
        resolve_material_slots(check_material_slots([0], 1), [0], 17)
    with pytest.raises(ValueError):
        resolve_material_slots(None, [0] * 17, 17)
    with pytest.raises(ValueError):
        resolve_material_slots(None, [0], 0)


def test_default_mapping_gives_the_kth_non_emitting_model_material_k():
    emissions = [0.0, 20.0, None, (0, 0, 1), (0, 0, 0)]
    assert default_material_slots(emissions) == (0, None, 1, None, 2)
    assert resolve_material_slots(None, emissions, 3) == (0, None, 1, None, 2)
    for n in (1, 2, 4):                                   # the list must hold one material per non-emitting model
        with pytest.raises(ValueError):
            resolve_material_slots(None, emissions, n)
