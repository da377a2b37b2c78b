"""The engine's quiescence gate, entry point by entry point.

Every call that needs the engine quiet refuses with RL_ESTATE while (a) a batch is in flight,
(b) a restore is open, (c) a routed set plan is open or (d) a routed adjust plan is open, and says
which of the four in rl_last_error. The texts below are the literals of rl_engine.cpp: an entry
point that words its refusal differently, or checks in another order, fails here. After each
state is closed a one-key rl_peek succeeds.
"""
import ctypes as C

import numpy as np
import pytest

import hiprl

pytestmark = pytest.mark.gpu

ESTATE = -5
T = 1_700_000_000

IN_FLIGHT = "{} while a batch is in flight (call rl_wait)"
RESTORING = "{} between rl_restore_begin and rl_restore_end"
SET_PLAN = "{} while a routed set plan is open (call rl_set_routed_commit)"
ADJ_PLAN = "{} while a routed adjust plan is open (call rl_adjust_routed_commit)"
PLAN_OPEN = "{}: a plan is open (call {})"

QUIET = ("rl_snapshot_begin", "rl_restore_begin", "rl_merge", "rl_resize", "rl_peek", "rl_forget", "rl_set",
         "rl_adjust", "rl_peek_device", "rl_peek_routed", "rl_rule_stats_read", "rl_cache_stats_read", "rl_census")
PLANS = ("rl_set_routed_plan", "rl_adjust_routed_plan")


@pytest.fixture(scope="module")
def world():
    e = hiprl.Engine(log2_slots=(12, 12, 12, 12), max_batch_desc=4096)
    e.load_rules([(10, hiprl.MINUTE)])
    b = hiprl.build_batch([("gate", [[("k", "v")]], [0], 1, T)])
    hdr = e.snapshot_begin()  # of the empty table: what rl_restore_begin and rl_merge take
    e.snapshot_end()
    yield e, b, hdr
    e.close()


def calls(e, b, hdr):
    """name -> a call of every entry point behind the gate, with arguments that pass what it checks first."""
    lib, h = e.lib, e.h
    s = hiprl._batch_struct(b)
    keep = [s]  # the structs the closures point into
    reply = np.zeros(1, hiprl.PEEK_DTYPE)
    delta = np.ones(1, np.int32)
    stat = np.zeros(1, hiprl.RULE_STAT_DTYPE)
    lg = (C.c_uint32 * 4)(12, 12, 12, 12)
    snap, cstats, mrep, arep = hiprl.RlSnapshotHeader(), hiprl.RlCacheStats(), hiprl.RlMergeReport(), hiprl.RlAdjustReport()
    census = hiprl.RlCensusReport()
    census.struct_size = C.sizeof(hiprl.RlCensusReport)
    keep += [reply, delta, stat, lg, snap, cstats, mrep, arep, census]
    return keep, {
        "rl_snapshot_begin": lambda: lib.rl_snapshot_begin(h, C.byref(snap)),
        "rl_restore_begin": lambda: lib.rl_restore_begin(h, C.byref(hdr)),
        "rl_merge": lambda: lib.rl_merge(h, C.byref(hdr), None, 0, T, C.byref(mrep)),
        "rl_resize": lambda: lib.rl_resize(h, lg),
        "rl_peek": lambda: lib.rl_peek(h, C.byref(s), reply.ctypes.data),
        "rl_forget": lambda: lib.rl_forget(h, C.byref(s), reply.ctypes.data),
        "rl_set": lambda: lib.rl_set(h, C.byref(s), reply.ctypes.data, None),
        "rl_adjust": lambda: lib.rl_adjust(h, C.byref(s), delta.ctypes.data, 0, None, C.byref(arep)),
        "rl_peek_device": lambda: lib.rl_peek_device(h, C.byref(s), None),
        "rl_peek_routed": lambda: lib.rl_peek_routed(h, None, 0, None, 0),
        "rl_rule_stats_read": lambda: lib.rl_rule_stats_read(h, 0, 1, stat.ctypes.data, 0),
        "rl_cache_stats_read": lambda: lib.rl_cache_stats_read(h, C.byref(cstats), 0),
        "rl_census": lambda: lib.rl_census(h, T, C.byref(census)),
        "rl_set_routed_plan": lambda: lib.rl_set_routed_plan(h, None, None, 0, None),
        "rl_adjust_routed_plan": lambda: lib.rl_adjust_routed_plan(h, None, 0, None),
        "rl_submit": lambda: lib.rl_submit(h, C.byref(s), None, None),
        "rl_set_routed_commit": lambda: lib.rl_set_routed_commit(h, 1),
        "rl_adjust_routed_commit": lambda: lib.rl_adjust_routed_commit(h, 1, C.byref(arep)),
    }


def refused(e, call, text):
    assert call() == ESTATE
    assert e.lib.rl_last_error(e.h).decode() == text


def peek_works(e, b):
    out = e.peek(b)
    assert out.shape == (1,) and not int(out["flags"][0]) & hiprl.PEEK_BAD


def test_batch_in_flight(world):
    e, b, hdr = world
    keep, f = calls(e, b, hdr)
    e.submit_host_async(b)
    for name in QUIET + PLANS:
        refused(e, f[name], IN_FLIGHT.format(name))
    e.wait()
    peek_works(e, b)


def test_open_restore(world):
    e, b, hdr = world
    keep, f = calls(e, b, hdr)
    e.restore_begin(hdr)
    for name in QUIET + PLANS:
        refused(e, f[name], "a restore is open (call rl_restore_end)" if name == "rl_restore_begin"
                else RESTORING.format(name))
    refused(e, f["rl_submit"], RESTORING.format("submit"))
    e.restore_end()
    peek_works(e, b)


@pytest.mark.parametrize("kind", ["set", "adjust"])
def test_open_routed_plan(world, kind):
    e, b, hdr = world
    keep, f = calls(e, b, hdr)
    commit, other = f"rl_{kind}_routed_commit", "rl_adjust_routed_commit" if kind == "set" else "rl_set_routed_commit"
    assert f[f"rl_{kind}_routed_plan"]() == 0  # n = 0: a plan is open and nothing ran
    for name in QUIET:
        refused(e, f[name], (SET_PLAN if kind == "set" else ADJ_PLAN).format(name))
    for name in PLANS:
        refused(e, f[name], PLAN_OPEN.format(name, commit))
    refused(e, f["rl_submit"], (SET_PLAN if kind == "set" else ADJ_PLAN).format("submit"))
    # the other form's commit names this one's and leaves the plan open
    refused(e, f[other], f"{other}: the open plan is a routed {kind}'s (call {commit})")
    assert f[commit]() == 0
    refused(e, f[commit], f"{commit} without an open plan (call rl_{kind}_routed_plan)")
    peek_works(e, b)
