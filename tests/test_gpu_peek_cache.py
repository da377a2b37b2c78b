"""HipRateLimitCache::Peek / Forget (rl_cache.hpp) through the batcher's queue (tests/cshim_peek):
on the reference's integration stream a peek reports what Redis GET and the local cache hold, a
forget unblocks the key, and a peek racing concurrent callers sits at one place of the serial
order — the place the trace hook reports."""
import ctypes as C
import threading
from pathlib import Path

import pytest

import hiprl

pytestmark = pytest.mark.gpu
SHIM = Path(__file__).resolve().parent / "cshim_peek" / "librl_peek_shim.so"
OK, OVER_LIMIT = 1, 2


def _lib():
    if not SHIM.exists():
        raise RuntimeError(f"{SHIM} missing (built by __graft_entry__.build())")
    lib = C.CDLL(str(SHIM))
    vp, u32, u64, cp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p
    lib.rlp_create.argtypes, lib.rlp_create.restype = [C.c_int, u32], vp
    lib.rlp_destroy.argtypes = [vp]
    lib.rlp_set_time.argtypes = [vp, C.c_int64]
    lib.rlp_add_rule.argtypes, lib.rlp_add_rule.restype = [vp, u32, u32], C.c_int
    lib.rlp_do_limit.argtypes = [vp, cp, cp, cp, C.c_int, u32, C.POINTER(u32), C.POINTER(u64), C.POINTER(u32)]
    lib.rlp_peek.argtypes = [vp, C.c_int, cp, cp, cp, C.c_int, C.POINTER(u32), C.POINTER(u64), C.POINTER(u32)]
    lib.rlp_total_hits.argtypes, lib.rlp_total_hits.restype = [vp, C.c_int], u64
    lib.rlp_trace_control.restype = u32
    lib.rlp_error.argtypes, lib.rlp_error.restype = [vp], cp
    return lib


class Cache:
    def __init__(self, local_cache, window_us=0):
        self.lib = _lib()
        self.h = self.lib.rlp_create(int(local_cache), window_us)
        assert self.h, "HipRateLimitCache construction failed"

    def do_limit(self, domain, key, value, rule, hits):
        """-> (code, remaining, throttle), (seq, pos)"""
        out, seq, pos = (C.c_uint32 * 3)(), C.c_uint64(), C.c_uint32()
        rc = self.lib.rlp_do_limit(self.h, domain.encode(), key.encode(), value.encode(), -1 if rule is None else rule,
                                   hits, out, C.byref(seq), C.byref(pos))
        if rc:
            raise hiprl.RedisError(self.lib.rlp_error(self.h).decode())
        return tuple(out), (seq.value, pos.value)

    def peek(self, domain, key, value, rule, forget=False):
        """-> dict(Found, LocalCached, Count, TtlSeconds, CachedSeconds), (seq, pos)"""
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        rc = self.lib.rlp_peek(self.h, int(forget), domain.encode(), key.encode(), value.encode(),
                               -1 if rule is None else rule, out, C.byref(seq), C.byref(pos))
        if rc:
            raise hiprl.RedisError(self.lib.rlp_error(self.h).decode())
        return dict(zip(["Found", "LocalCached", "Count", "TtlSeconds", "CachedSeconds"], out)), (seq.value, pos.value)

    def close(self):
        self.lib.rlp_destroy(self.h)


def test_peek_and_forget_on_the_integration_stream(golden):
    s = next(x for x in golden["streams"] if x["local_cache"])
    assert s["rules"][1] == [20, hiprl.MINUTE]
    m = Cache(True)
    ids = [m.lib.rlp_add_rule(m.h, L, u) for L, u in s["rules"]]
    pairs = [(r, e) for r, e in zip(s["requests"], s["expect"]) if r["rules"] == [1]]
    assert len(pairs) == 25
    req0 = pairs[0][0]
    (key, value), = req0["descriptors"][0]
    now = req0["now"]
    m.lib.rlp_set_time(m.h, now)
    total = 0
    for k, (req, exp) in enumerate(pairs[:22]):
        assert req["now"] == now and req["descriptors"] == req0["descriptors"]
        (code, rem, _), _ = m.do_limit(req["domain"], key, value, ids[1], req["hits"])
        assert [code, rem] == exp["statuses"][0][:2], exp["src"]
        total += max(1, req["hits"])
        if k == 9:  # mid-stream: ten hits counted, nothing frozen, and the peek spends nothing
            st, _ = m.peek(req["domain"], key, value, ids[1])
            assert st == dict(Found=1, LocalCached=0, Count=10, TtlSeconds=60, CachedSeconds=0), st
    # request 21 went over (count 21) and froze the key; request 22 was a local-cache hit: no INCRBY
    st, _ = m.peek(req0["domain"], key, value, ids[1])
    assert (st["Found"], st["LocalCached"], st["Count"]) == (1, 1, 21), st
    assert st["TtlSeconds"] == 60 and st["CachedSeconds"] == 60, st
    assert m.lib.rlp_total_hits(m.h, ids[1]) == total  # Peek adds no hits
    # other keys, other rules, a nil limit: absent
    assert m.peek(req0["domain"], key, value + "x", ids[1])[0]["Found"] == 0
    assert m.peek(req0["domain"], key, value, None)[0]["Found"] == 0
    # Forget reports the state it clears; the key is unblocked: the next DoLimit counts from 0
    st2, _ = m.peek(req0["domain"], key, value, ids[1], forget=True)
    assert st2 == st
    st3, _ = m.peek(req0["domain"], key, value, ids[1])
    assert st3 == dict(Found=0, LocalCached=0, Count=0, TtlSeconds=0, CachedSeconds=0), st3
    (code, rem, _), _ = m.do_limit(req0["domain"], key, value, ids[1], 1)
    assert (code, rem) == (OK, 19)
    assert m.peek(req0["domain"], key, value, ids[1])[0]["Count"] == 1
    # a rule first seen by Peek is registered as DoLimit registers it
    new = m.lib.rlp_add_rule(m.h, 7, hiprl.HOUR)
    assert m.peek("fresh", "k", "v", new)[0]["Found"] == 0
    (code, rem, _), _ = m.do_limit("fresh", "k", "v", new, 3)
    assert (code, rem) == (OK, 4)
    st, _ = m.peek("fresh", "k", "v", new)
    assert (st["Found"], st["Count"], st["TtlSeconds"]) == (1, 3, 3600)
    m.close()


def test_peek_racing_concurrent_callers_has_one_place_in_the_serial_order():
    """8 threads add hits to one key while the main thread peeks it: every peek's count is the sum
    of the hits of exactly the calls traced before it."""
    T, n = 8, 60
    m = Cache(False, window_us=300)
    rule = m.lib.rlp_add_rule(m.h, 1 << 30, hiprl.HOUR)
    ctl = m.lib.rlp_trace_control()
    m.lib.rlp_set_time(m.h, 1_700_000_000)
    calls = [[] for _ in range(T)]  # (seq, pos, hits)

    def run(t):
        for i in range(n):
            hits = 1 + (t + i) % 4
            _, (seq, pos) = m.do_limit("race", "k", "shared", rule, hits)
            calls[t].append((seq, pos, hits))

    th = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    peeks = []
    while any(x.is_alive() for x in th) and len(peeks) < 200:
        st, (seq, pos) = m.peek("race", "k", "shared", rule)
        peeks.append((seq, pos, st))
    for x in th:
        x.join()
    st, (seq, pos) = m.peek("race", "k", "shared", rule)
    peeks.append((seq, pos, st))
    flat = [c for per in calls for c in per]
    assert len({(s_, p_) for s_, p_, _ in flat}) == T * n  # every call has a place of its own
    assert peeks[-1][2]["Count"] == sum(h for _, _, h in flat)
    mid = 0
    for seq, pos, st in peeks:
        assert pos == ctl and seq != 2**64 - 1
        before = sum(h for s_, _, h in flat if s_ < seq)  # the batches gathered before the peek
        assert st["Count"] == before and st["Found"] == (before > 0), (seq, st, before)
        mid += 0 < before < peeks[-1][2]["Count"]
    assert mid > 0, "no peek landed among the callers' batches"
    m.close()
