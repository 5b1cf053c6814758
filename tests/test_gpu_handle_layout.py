"""The handle of csrc/offk_api.hip -- its workspace regions and the six unit parameters per site -- held to a recorded golden,
tests/golden/handle_layout.json (tools/record_handle_layout.py wrote it from the library as it was while regions and gradient slots were
string maps; the enum-indexed tables that replaced them have to give the same answers, value for value and character for character):

  (a) per handle -- (batch, length) of HANDLES x both variants x both precisions -- offk_workspace_bytes, offk_train_workspace_bytes and
      offk_unit_grad_floats; (offset, bytes) of every workspace region by name, or the code and the whole offk_last_error text where the
      handle has no such region (and for two names no handle has); (offset, count) of offk_unit_grad_slot for every unit-parameter key
      with and without "module.", or the code and text where the variant has no such parameter; offk_missing_weights of the fresh handle;
  (b) on the (1, 2) handles, the trail of a missing weight: every weight set but one (LEFT_OUT), then offk_missing_weights and what
      offk_off_units, offk_pw_reduce at that site, offk_sobel_tdiff_all and offk_off_units_backward answer -- on real device buffers
      of the right sizes: an entry that does not need the key runs -- and what binding a parameter, setting the same key and binding a
      key that cannot be bound return.

No workspace is allocated and nothing is launched for (a); offk_create needs the device, so none of this can run without one."""
import json
import os

import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib, spec

from .handle_layout import (GOLDEN_FILE, handle_id, HANDLE_IDS, HANDLES, left_out_keys, NEVER_REGIONS, PRECISIONS, record_layout,
                            record_trail, region_names, TRAIL_HANDLE, TRAIL_IDS, unit_keys, VARIANTS)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, GOLDEN_FILE)) as f:
        return json.load(f)


def test_golden_lists_the_cases(golden):
    assert sorted(golden["layout"]) == sorted(HANDLE_IDS) and sorted(golden["trail"]) == sorted(TRAIL_IDS)
    for hid, row in golden["layout"].items():
        assert sorted(row["regions"]) == sorted(region_names()) and sorted(row["grad_slots"]) == sorted(unit_keys()), hid
        absent = sorted(n for n, v in row["regions"].items() if v[0] != 0)
        # what a handle lacks: the two names nobody has, and the per-tile sums of xv_7 without the pool-first 7-head (below its gate of 96 pairs)
        b, l = (int(x[1:]) for x in hid.split("|")[0].split("_")[:2])
        pool_first = b * (l - 1) >= 96 and "poolfirst0" not in hid
        assert absent == sorted(NEVER_REGIONS + (() if pool_first else ("poolpart_7t",))), hid
        assert all(v == [-1, "unknown workspace region: " + n] for n, v in row["regions"].items() if v[0] != 0), hid
        assert all(v[1] % 256 == 0 for v in row["regions"].values() if v[0] == 0), hid
        lacking = [k for k, v in row["grad_slots"].items() if v[0] != 0]
        assert all(spec.SOBEL_KEY in k or ("|flow|" in hid and "motion_spatial_grad_" in k) for k in lacking), hid
        assert len(lacking) == (2 + 36 if "|flow|" in hid else 2), hid
    for hid, trail in golden["trail"].items():
        assert sorted(trail) == sorted(["without " + k for k in left_out_keys(hid.split("|")[1])] + ["bind"]), hid
        for left, row in trail.items():
            if left != "bind":
                assert row["missing"] == [1, left[len("without "):]] and row["offk_off_units"] == [-3, "weight not set: " + left[len("without "):]]


@pytest.mark.parametrize("case", [(b, l, pf, v, p) for b, l, pf in HANDLES for v in VARIANTS for p in PRECISIONS], ids=HANDLE_IDS)
def test_layout_is_the_recorded_one(golden, case):
    got = record_layout(_lib.load(), *case)
    want = golden["layout"][handle_id(*case)]
    for k in sorted(want):
        if isinstance(want[k], dict):
            for name in sorted(want[k]):
                assert got[k][name] == want[k][name], (k, name, got[k][name], want[k][name])
    assert got == want


@pytest.mark.parametrize("case", [(v, p) for v in VARIANTS for p in PRECISIONS], ids=TRAIL_IDS)
def test_missing_weight_and_bind_trail_is_the_recorded_one(golden, case):
    got = record_trail(_lib.load(), *case)
    want = golden["trail"][handle_id(*TRAIL_HANDLE, *case)]
    for left in sorted(want):
        assert got[left] == want[left], (left, got[left], want[left])
    assert got == want
