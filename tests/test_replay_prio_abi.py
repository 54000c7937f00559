"""The hsr_replay_priority_* entry points are exported by the C-ABI library and declared by hsr_env_amd.sim, refuse a NULL replay with
HSR_EINVAL before they touch a device and name themselves in the message; hsr_priority_spec has the header's layout.  No GPU."""
import ctypes as C

import pytest

from hsr_env_amd.sim import PROTOTYPES, PrioritySpec, ReplaySeqOut

CALLS = {
    "hsr_replay_priority_enable": lambda f: f(None, C.byref(PrioritySpec(1.0, 1e-6, 1e6, 256))),
    "hsr_replay_priority_state": lambda f: f(None, None, None, None),
    "hsr_replay_priority_sample_dev": lambda f: f(None, 0, 4, 0.5, *[None] * 9),
    "hsr_replay_priority_sample_seq_dev": lambda f: f(None, 0, 4, 2, 0.5, 0.9, C.byref(ReplaySeqOut()), None),
    "hsr_replay_priority_update_dev": lambda f: f(None, 0, 4, None, None),
    "hsr_replay_priority_read_dev": lambda f: f(None, None),
}


@pytest.fixture(scope="module")
def lib():
    from hsr_env_amd.build import build_lib
    lib = C.CDLL(str(build_lib()))
    lib.hsr_last_error.restype = C.c_char_p
    return lib


@pytest.mark.parametrize("name", sorted(CALLS))
def test_priority_entry_points_refuse_a_null_replay(lib, name):
    f = getattr(lib, name)
    f.restype, f.argtypes = PROTOTYPES[name]
    assert CALLS[name](f) == -1
    assert name.encode() in lib.hsr_last_error()


def test_the_spec_is_three_floats_and_an_int():
    """include/hsrsim.h: hsr_priority_spec, in the header's order."""
    assert [(n, t) for n, t in PrioritySpec._fields_] == [("p_init", C.c_float), ("p_min", C.c_float), ("p_max", C.c_float), ("max_batch", C.c_int32)]
    assert C.sizeof(PrioritySpec) == 16
    assert [getattr(PrioritySpec, n).offset for n, _ in PrioritySpec._fields_] == [0, 4, 8, 12]
