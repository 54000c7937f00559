"""The hsr_plan_* entry points are exported by the C-ABI library and declared by hsr_env_amd.sim, refuse a NULL planner (hsr_batch_plan_create:
a NULL batch) with HSR_EINVAL before they touch a device and name themselves in the message; hsr_plan_spec has the header's layout.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import pytest

from hsr_env_amd.sim import PROTOTYPES, PlanSpec

ROOT = Path(__file__).resolve().parents[1]
CALLS = {
    "hsr_plan_reset_dev": lambda f: f(None, None),
    "hsr_plan_shift_dev": lambda f: f(None, None),
    "hsr_plan_begin_dev": lambda f: f(None),
    "hsr_plan_sample_dev": lambda f: f(None, 0, 0, 0, None),
    "hsr_plan_accumulate_dev": lambda f: f(None, 0),
    "hsr_plan_add_cost_dev": lambda f: f(None, None),
    "hsr_plan_update_dev": lambda f: f(None),
    "hsr_plan_action_dev": lambda f: f(None, None),
    "hsr_plan_costs_dev": lambda f: f(None, None, None),
    "hsr_plan_state_dev": lambda f: f(None, None, None),
    "hsr_plan_best_dev": lambda f: f(None, None, None),
    "hsr_plan_failed": lambda f: f(None, None),
}


@pytest.fixture(scope="module")
def lib():
    from hsr_env_amd.build import build_lib
    lib = C.CDLL(str(build_lib()))
    lib.hsr_last_error.restype = C.c_char_p
    return lib


def test_every_planner_symbol_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hsrsim.h").read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hsr_(?:batch_)?plan_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(list(CALLS) + ["hsr_batch_plan_create", "hsr_plan_destroy"])
    for name in declared:
        assert hasattr(lib, name) and name in PROTOTYPES, name


@pytest.mark.parametrize("name", sorted(CALLS))
def test_planner_entry_points_refuse_a_null_planner(lib, name):
    f = getattr(lib, name)
    f.restype, f.argtypes = PROTOTYPES[name]
    assert CALLS[name](f) == -1
    assert name.encode() in lib.hsr_last_error()


def test_create_refuses_null_arguments_and_destroy_takes_null(lib):
    f = lib.hsr_batch_plan_create
    f.restype, f.argtypes = PROTOTYPES["hsr_batch_plan_create"]
    out = C.c_void_p()
    assert f(None, C.byref(PlanSpec()), C.byref(out)) == -1 and not out.value
    lib.hsr_plan_destroy.restype, lib.hsr_plan_destroy.argtypes = PROTOTYPES["hsr_plan_destroy"]
    lib.hsr_plan_destroy(None)


def test_the_spec_has_the_headers_layout():
    """include/hsrsim.h: hsr_plan_spec, in the header's order."""
    names = ["seed", "env_offset", "groups", "samples", "horizon", "elites", "goal_body", "geofence", "gamma", "alpha", "init_std", "min_std"]
    assert [n for n, _ in PlanSpec._fields_] == names
    assert [t for _, t in PlanSpec._fields_] == [C.c_uint64, C.c_uint32] + [C.c_int32] * 5 + [C.c_float] * 5
    assert [getattr(PlanSpec, n).offset for n in names] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48]
    assert C.sizeof(PlanSpec) == 56
    text = (ROOT / "include" / "hsrsim.h").read_text()
    body = re.search(r"typedef struct hsr_plan_spec \{(.*?)\} hsr_plan_spec;", text, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == names
