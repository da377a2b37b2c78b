"""Routed refund (rl_hip.h "Routed refund"), CPU only: the library's four entry points and their
prototypes in the header against the Python binding, the ABI version the change left alone,
Router.refund's argument errors, and the model (routed_refund_model.py) against RefundOracle on the
concatenated batch and against hand-written cases."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import hiprl
import routing
from refund_model import RefundOracle
from routed_refund_model import RoutedRefundOracle

ROOT = Path(__file__).resolve().parents[1]
NEW = ("rl_refund_route_owed", "rl_refund_routed_plan", "rl_refund_routed_commit", "rl_router_refund")
F, LC, NILF, PS = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND
NIL = hiprl.NIL_RULE
S, M, H, D = hiprl.SECOND, hiprl.MINUTE, hiprl.HOUR, hiprl.DAY
T0 = 1_700_000_000
# rule 1 rejects whatever asks more than 1 a day (the "global" descriptor of the hand cases); rule 5
# is shadowed: over its limit it rejects nothing
RULES = [(10, M), (1, D), (1 << 30, H), (4, S), (10000, M), (2, M, True)]


def test_library_exports_the_routed_refund_entry_points():
    lib = hiprl.load_library()
    names = {n for n, _, _ in hiprl.ABI}
    for f in NEW:
        assert hasattr(lib, f), f
        assert f in names
    # null arguments are refused before anything touches the GPU
    assert lib.rl_refund_route_owed(None, None, None, None, None, None) == -1
    assert lib.rl_refund_routed_plan(None, None, 0, None) == -1
    assert lib.rl_refund_routed_commit(None, 1, None) == -1
    assert lib.rl_router_refund(None, None, None, None, None, None, None) == -1
    assert lib.rl_abi_version() == 7
    for m in ("refund_route_owed", "refund_routed_plan", "refund_routed_commit"):
        assert hasattr(hiprl.Engine, m), m
    assert hasattr(hiprl.Router, "refund")
    assert C.sizeof(hiprl.RlRefundReport) == 64


def test_prototypes_and_abi_version_match_header(tmp_path):
    # the header's prototypes are assignable to the shapes its "Routed refund" section documents (a
    # mismatch is a compile error under -Werror), and the version did not move
    src = tmp_path / "rr.c"
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n'
                   'int (*f_owed)(rl_engine*, const rl_batch*, const rl_status*, uint32_t*, uint32_t*, uint32_t*) = '
                   'rl_refund_route_owed;\n'
                   'int (*f_plan)(rl_engine*, const void*, uint32_t, rl_peek_reply*) = rl_refund_routed_plan;\n'
                   'int (*f_commit)(rl_engine*, int, rl_refund_report*) = rl_refund_routed_commit;\n'
                   'int (*f_ref)(rl_router*, const rl_batch*, const rl_status* const*, const uint32_t*, '
                   'uint32_t* const*, rl_peek_reply* const*, rl_refund_report* const*) = rl_router_refund;\n'
                   'int main(){printf("%u %u %u %u", (unsigned)RL_ABI_VERSION, (unsigned)RL_ROUTE_RECORD_BYTES, '
                   '(unsigned)RL_REFUND_KEEP_CACHE, (unsigned)sizeof(rl_refund_report)); return 0;}\n')
    obj = tmp_path / "rr.o"
    subprocess.run(["gcc", "-Wall", "-Werror", "-c", "-I", str(ROOT / "include"), str(src), "-o", str(obj)], check=True)
    exe = tmp_path / "rr"
    subprocess.run(["gcc", str(obj), "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [hiprl.ABI_VERSION, hiprl.ROUTE_RECORD_BYTES, hiprl.REFUND_KEEP_CACHE, 64]
    assert hiprl.ABI_VERSION == 7 and hiprl.load_library().rl_abi_version() == 7
    abi = {n: (a, r) for n, a, r in hiprl.ABI}
    assert abi["rl_refund_route_owed"] == ([C.c_void_p, C.POINTER(hiprl.RlBatch)] + [C.c_void_p] * 4, C.c_int)
    assert abi["rl_refund_routed_plan"] == ([C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p], C.c_int)
    assert abi["rl_refund_routed_commit"] == ([C.c_void_p, C.c_int, C.POINTER(hiprl.RlRefundReport)], C.c_int)
    assert len(abi["rl_router_refund"][0]) == 7


class FakeRouter:
    """Router.refund's checks run before the library is called: a stand-in with no handle shows that
    none of the refused calls reaches it."""
    n = 2
    h = None
    refund = hiprl.Router.refund

    class lib:
        @staticmethod
        def rl_router_refund(*a):
            raise AssertionError("the call reached the library")


def test_router_refund_argument_errors():
    r = FakeRouter()
    b = hiprl.build_batch([("d", [[("k", "a")], [("k", "b")]], [0, 1], 3, T0)])
    st = np.zeros(2, hiprl.STATUS_DTYPE)
    for args, kw in [(([b], [st, st]), {}),  # one batch for two engines
                     (([b, b], [st]), {}),  # one status array
                     (([b, b], [st, st]), dict(keep_cache=[True])),  # one flag
                     (([b, b], [st, st[:1]]), {}),  # a status short
                     (([b, b], [st, np.zeros((2, 1), hiprl.STATUS_DTYPE)]), {}),  # not one-dimensional
                     (([b, b], [st, np.zeros(2, np.uint32)]), {})]:  # not statuses
        with pytest.raises(ValueError, match="rl_router_refund"):
            r.refund(*args, **kw)


# ---- the model ---------------------------------------------------------------------------------------
def req(keys, rules, hits, t=T0 + 7):
    return ("rr", [[("k", str(k))] for k in keys], rules, hits, t)


def string(name, rule, t=T0 + 7):
    b = hiprl.build_batch([req([name], [rule], 1, t)])
    d = hiprl.UNIT_DIVIDER[RULES[rule][1]]
    return b.prefix(0) + str(t // d * d).encode()


def stream(seed, n_req):
    rng = np.random.default_rng(seed)
    reqs = []
    for _ in range(n_req):
        nd = int(rng.integers(1, 4))
        rules = [int(rng.choice([0, 2, 3, 4, 5, NIL])) for _ in range(nd)]
        reqs.append(req([int(20 * rng.random() ** 2) for _ in range(nd)], rules, int(rng.integers(0, 9)),
                        T0 + int(rng.integers(0, 2))))
    reqs.sort(key=lambda r: r[4])
    return hiprl.build_batch(reqs)


@pytest.mark.parametrize("local_cache,split", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("keep", [False, True])
def test_model_equals_the_refund_oracle_on_the_concatenated_batch(local_cache, split, keep):
    a = RefundOracle(RULES, local_cache=local_cache, per_second_split=split)
    m = RoutedRefundOracle(RULES, local_cache=local_cache, per_second_split=split)
    rejected = unfrozen = 0
    for step in range(4):
        row = [stream(10 * step + g, 60 if g != 1 else 0) for g in range(3)]  # origin 1 passes nothing
        cat = routing.concat_batches(row)
        st, thr = a.submit(cat)
        st2, thr2 = m.submit(cat)
        assert np.array_equal(st, st2) and np.array_equal(thr, thr2)
        want_amounts, want = a.refund(cat, st, keep)
        cuts = np.cumsum([0] + [b.n_desc for b in row])
        amounts, outs, origin, owner = m.refund_routed(row, [st[cuts[g]:cuts[g + 1]] for g in range(3)], keep)
        assert sum(amounts, []) == want_amounts
        assert {f: sum(o[f] for o in origin) for f in ("descriptors", "rejected_req", "skipped")} == \
            {f: want[f] for f in ("descriptors", "rejected_req", "skipped")}
        assert owner == {f: want[f] for f in ("absent", "refunded", "floored", "unfrozen")}
        # the world identity that replaces the lone engine's per-report one
        assert sum(o["descriptors"] - o["skipped"] for o in origin) == owner["absent"] + owner["refunded"]
        assert a.redis == m.redis and a.lcache == m.lcache
        for g, b in enumerate(row):
            assert [bool(int(f) & NILF) for f in outs[g]["flags"]] == [x == 0 for x in amounts[g]]
        rejected += want["rejected_req"]
        unfrozen += want["unfrozen"]
    assert rejected >= 40 and (unfrozen >= 1) == (local_cache and not keep), (rejected, unfrozen)


def rejected_pair(m, name, hits, who):
    """A request of `hits` on `name` (rule 4: 10000 a minute) and on origin `who`'s global key, which
    is over its limit of 1 a day from the second request on."""
    b = hiprl.build_batch([req([name, f"g{who}"], [4, 1], hits)])
    st, _ = m.submit(b)
    return b, st


def test_model_floors_once_across_origins():
    # a counter of 9 owed 6 by origin 0 and 6 by origin 1 ends at 0, floored once, in either order
    for order in ((0, 1), (1, 0)):
        m = RoutedRefundOracle(RULES)
        for who in (0, 1):
            m.submit(hiprl.build_batch([req([f"g{who}"], [1], 1)]))
        pairs = [rejected_pair(m, "nine", 6, who) for who in order]
        key = string("nine", 4)
        assert m.redis[0][key][0] == 12
        m.redis[0][key][0] = 9  # (on the device: a Router.adjust of -3 between the step and the refund)
        amounts, outs, origin, owner = m.refund_routed([p[0] for p in pairs], [p[1] for p in pairs])
        assert amounts == [[6, 6], [6, 6]] and m.redis[0][key][0] == 0
        assert [int(o["count"][0]) for o in outs] == [9, 9], "every duplicate reports the state before the call"
        assert owner == dict(absent=0, refunded=4, floored=1, unfrozen=0)
        assert origin == [dict(descriptors=2, rejected_req=1, skipped=0)] * 2


def test_model_amounts_above_int32():
    for h in (2**31, 2**32 - 1):
        m = RoutedRefundOracle(RULES)
        b = hiprl.build_batch([req(["big", "other"], [2, 4], h)])  # 2^30 an hour: over its limit at once
        st, _ = m.submit(b)
        assert int(st["code_flags"][0]) & 0xFF == 2 and m.redis[0][string("big", 2)][0] == h
        empty = hiprl.build_batch([])
        amounts, outs, origin, owner = m.refund_routed([empty, b], [st[:0], st])
        assert amounts == [[], [h, h]] and owner == dict(absent=0, refunded=2, floored=0, unfrozen=0)
        assert m.redis[0][string("big", 2)][0] == 0 and m.redis[0][string("other", 4)][0] == 0
        assert origin[0] == dict(descriptors=0, rejected_req=0, skipped=0)


def test_model_keep_flag_on_one_origin_only():
    # a key frozen at 12 / 10 and owed 6 by each of two origins: released when either comes without
    # the flag, frozen still when both carry it
    for keeps, released in (([True, False], True), ([False, True], True), ([False, False], True), ([True, True], False)):
        m = RoutedRefundOracle(RULES, local_cache=True)
        for who in (0, 1):
            m.submit(hiprl.build_batch([req([f"g{who}"], [1], 1)]))
        bs = [hiprl.build_batch([req(["fr", f"g{who}"], [0, 1], 6)]) for who in (0, 1)]
        sts = [m.submit(b)[0] for b in bs]
        key = string("fr", 0)
        assert m.redis[0][key][0] == 12 and key in m.lcache
        amounts, outs, origin, owner = m.refund_routed(bs, sts, keeps)
        assert amounts == [[6, 6], [6, 6]] and m.redis[0][key][0] == 0
        # (each origin's global key, frozen at 7 / 1 and back at 1, is released by its own record alone)
        assert (key not in m.lcache) == released and owner["unfrozen"] == int(released) + keeps.count(False), keeps
        assert int(outs[1]["flags"][0]) == F | LC and int(outs[0]["flags"][0]) == F | LC


def test_model_local_cache_hit_and_nil_inside_a_rejected_request():
    m = RoutedRefundOracle(RULES, local_cache=True)
    m.submit(hiprl.build_batch([req(["hot"], [0], 11), req(["g0"], [1], 1)]))  # "hot" frozen at 11 / 10
    b = hiprl.build_batch([req(["hot", "x", "cold", "g0"], [0, NIL, 4, 1], 5)])
    st, _ = m.submit(b)
    flags = [int(c) >> 8 for c in st["code_flags"]]
    assert flags[0] & 2 and not flags[2] & 2, "the first descriptor is a local-cache hit"
    amounts, outs, origin, owner = m.refund_routed([b], [st])
    assert amounts == [[0, 0, 5, 5]]
    assert [int(f) for f in outs[0]["flags"][:2]] == [NILF, NILF], "neither was asked"
    assert origin == [dict(descriptors=4, rejected_req=1, skipped=2)] and owner["refunded"] == 2
    assert m.redis[0][string("hot", 0)][0] == 11 and m.redis[0][string("cold", 4)][0] == 0


def test_model_shadowed_over_limit_rejects_nothing():
    m = RoutedRefundOracle(RULES)
    b = hiprl.build_batch([req(["sh", "y"], [5, 4], 3)])
    st, _ = m.submit(b)
    cf = int(st["code_flags"][0])
    assert cf & 0xFF == 1 and (cf >> 8) & 4, "over 2 a minute, reported OK with the shadow flag"
    amounts, outs, origin, owner = m.refund_routed([b], [st])
    assert amounts == [[0, 0]] and origin == [dict(descriptors=2, rejected_req=0, skipped=2)]
    assert owner == dict(absent=0, refunded=0, floored=0, unfrozen=0) and m.redis[0][string("y", 4)][0] == 3
