"""The lane plan (misti_lanes.cpp: lane_plan): which stream-priority level each lane of a pool goes on.  The HIP runtime keeps one
pool of GPU_MAX_HW_QUEUES hardware queues per priority level, so a pool that does not fit into one level's queues is dealt over
the levels.  Pure host code, reached through the library's internal entry point misti_lane_plan_ - no device is needed."""
import ctypes as C

import pytest

from misti_amd import _lib

CAP = 22                       # the pool's cap of distinct hardware queues (misti_lanes.cpp)


def plan(n_lanes, q, n_levels, cap=CAP):
    """lane_plan itself (q > 0), or what misti_create_lanes would do in this environment (q == 0)."""
    lib = _lib.load()
    fn = lib.misti_lane_plan_
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * n_lanes)(*([-1] * n_lanes))
    assert fn(n_lanes, q, n_levels, cap, out) == 0, lib.misti_last_error()
    return list(out)


def queues(levels, q, n_levels):
    """Distinct hardware queues of a plan: a level with n lanes occupies min(n, q) of its q queues."""
    return sum(min(levels.count(l), q) for l in range(n_levels))


def deepest(levels, q, n_levels):
    """Most lanes on one queue: the runtime deals a level's streams over the level's queues."""
    return max(-(-levels.count(l) // q) for l in range(n_levels))


CASES = [(20, 22, 3), (20, 4, 3), (20, 4, 1), (24, 22, 3), (64, 4, 3), (1, 4, 3)]


@pytest.mark.parametrize("n,q,n_levels", CASES)
def test_every_lane_has_a_level_in_range_and_the_plan_repeats(n, q, n_levels):
    a = plan(n, q, n_levels)
    assert len(a) == n and all(0 <= l < n_levels for l in a)
    assert a == plan(n, q, n_levels) == plan(n, q, n_levels)
    assert queues(a, q, n_levels) <= CAP


def test_a_queue_for_every_lane_keeps_the_default_level():
    """20 lanes at 22 queues: the pool as it was before there was a plan."""
    assert plan(20, 22, 3) == [0] * 20


def test_twenty_lanes_at_four_queues_reach_twelve_queues():
    a = plan(20, 4, 3)
    assert queues(a, 4, 3) == 12 and deepest(a, 4, 3) <= 2
    assert len(set(a[:3])) == 3                      # consecutive lanes on different levels: round-robin issue reaches every level at once


def test_one_level_is_one_level():
    assert plan(20, 4, 1) == [0] * 20


def test_the_cap_of_22_queues_holds_over_all_levels():
    a = plan(24, 22, 3)
    assert queues(a, 22, 3) == 22
    assert a == [0] * 24                             # 22 queues on the default level, shared by 24 lanes: as before
    b = plan(24, 8, 3)                               # 8 + 8 + 6 queues
    assert queues(b, 8, 3) == 22 and deepest(b, 8, 3) == 2


def test_many_lanes_and_one_lane():
    a = plan(64, 4, 3)
    assert queues(a, 4, 3) == 12 and deepest(a, 4, 3) == -(-64 // 12)
    assert plan(1, 4, 3) == [0]


def test_the_default_level_is_filled_first():
    """A pool that fits into the default level's queues stays there; a slightly larger one puts only the overflow elsewhere."""
    assert plan(4, 4, 3) == [0] * 4
    a = plan(6, 4, 3)
    assert [a.count(l) for l in range(3)] == [4, 2, 0] and queues(a, 4, 3) == 6


def test_environment(monkeypatch):
    """What misti_create_lanes reads when a pool is created: the queue limit the environment names (else HIP's 4) and
    MISTI_LANE_PRIORITIES=0."""
    _lib.load()                                      # the library's constructor may set GPU_MAX_HW_QUEUES: before the patches below
    monkeypatch.delenv("MISTI_LANE_PRIORITIES", raising=False)
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")
    assert plan(20, 0, 3) == plan(20, 4, 3) and len(set(plan(20, 0, 3))) == 3
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "22")
    assert plan(20, 0, 3) == [0] * 20
    monkeypatch.delenv("GPU_MAX_HW_QUEUES")
    assert plan(20, 0, 3) == plan(20, 4, 3)
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")
    monkeypatch.setenv("MISTI_LANE_PRIORITIES", "0")
    assert plan(20, 0, 3) == [0] * 20
    assert plan(64, 0, 3) == [0] * 64
    monkeypatch.setenv("MISTI_LANE_PRIORITIES", "1")
    assert plan(20, 0, 3) == plan(20, 4, 3)


def test_bad_arguments_are_errors():
    lib = _lib.load()
    out = (C.c_int * 4)()
    assert lib.misti_lane_plan_(0, 4, 3, CAP, out) == -1
    assert lib.misti_lane_plan_(4, 4, 0, CAP, out) == -1
    assert lib.misti_lane_plan_(4, 4, 3, CAP, None) == -1
