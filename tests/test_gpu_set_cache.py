"""HipRateLimitCache::Set (rl_cache.hpp) through the batcher's queue (tests/cshim_set): a Set
between concurrent DoLimit callers sits at one place of the serial order — the place the trace hook
reports — for counter-only (keep_cache) and cache-only (keep_counter) writes, and a Set that pushes
a home unit over the auto-grow watermark is followed by a grow."""
import ctypes as C
import threading
from pathlib import Path

import pytest

import hiprl

pytestmark = pytest.mark.gpu
SHIM = Path(__file__).resolve().parent / "cshim_set" / "librl_set_shim.so"
OK, OVER_LIMIT = 1, 2
NAMES = ["Found", "LocalCached", "Count", "TtlSeconds", "CachedSeconds"]


def _lib():
    if not SHIM.exists():
        raise RuntimeError(f"{SHIM} missing (built by __graft_entry__.build())")
    lib = C.CDLL(str(SHIM))
    vp, u32, u64, cp, pu32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint32)
    lib.rls_create.argtypes, lib.rls_create.restype = [C.c_int, u32, pu32, u32, pu32], vp
    lib.rls_destroy.argtypes = [vp]
    lib.rls_set_time.argtypes = [vp, C.c_int64]
    lib.rls_add_rule.argtypes, lib.rls_add_rule.restype = [vp, u32, u32], C.c_int
    lib.rls_do_limit.argtypes = [vp, cp, cp, cp, C.c_int, u32, pu32, C.POINTER(u64), pu32]
    lib.rls_peek.argtypes = [vp, cp, cp, cp, C.c_int, pu32, C.POINTER(u64), pu32]
    lib.rls_set.argtypes = [vp, cp, cp, cp, C.c_int, pu32, C.c_int, C.c_int, pu32, C.POINTER(u64), pu32]
    lib.rls_occupancy.argtypes = [vp, pu32]
    lib.rls_resizes.argtypes, lib.rls_resizes.restype = [vp], u64
    lib.rls_trace_control.restype = u32
    lib.rls_error.argtypes, lib.rls_error.restype = [vp], cp
    return lib


class Cache:
    def __init__(self, local_cache, window_us=0, log2_slots=(12, 12, 12, 12), autogrow_permille=0,
                 max_log2_slots=(31, 31, 31, 31)):
        self.lib = _lib()
        self.h = self.lib.rls_create(int(local_cache), window_us, (C.c_uint32 * 4)(*log2_slots), autogrow_permille,
                                     (C.c_uint32 * 4)(*max_log2_slots))
        assert self.h, "HipRateLimitCache construction failed"

    def _ok(self, rc):
        if rc:
            raise hiprl.RedisError(self.lib.rls_error(self.h).decode())

    def do_limit(self, domain, key, value, rule, hits):
        """-> (code, remaining, throttle), (seq, pos)"""
        out, seq, pos = (C.c_uint32 * 3)(), C.c_uint64(), C.c_uint32()
        self._ok(self.lib.rls_do_limit(self.h, domain.encode(), key.encode(), value.encode(), rule, hits, out,
                                       C.byref(seq), C.byref(pos)))
        return tuple(out), (seq.value, pos.value)

    def peek(self, domain, key, value, rule):
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        self._ok(self.lib.rls_peek(self.h, domain.encode(), key.encode(), value.encode(), rule, out, C.byref(seq),
                                   C.byref(pos)))
        return dict(zip(NAMES, out)), (seq.value, pos.value)

    def set(self, domain, key, value, rule, keep_counter=False, keep_cache=False, **v):
        """-> the status before, (seq, pos)"""
        val = (C.c_uint32 * 5)(*[int(v.get(n, 0)) for n in NAMES])
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        self._ok(self.lib.rls_set(self.h, domain.encode(), key.encode(), value.encode(), rule, val, int(keep_counter),
                                  int(keep_cache), out, C.byref(seq), C.byref(pos)))
        return dict(zip(NAMES, out)), (seq.value, pos.value)

    def occupancy(self):
        out = (C.c_uint32 * 16)()
        self._ok(self.lib.rls_occupancy(self.h, out))
        return list(out[:8]), list(out[8:])

    def close(self):
        self.lib.rls_destroy(self.h)


def test_set_is_a_control_call_like_forget():
    m = Cache(True)
    rule = m.lib.rls_add_rule(m.h, 5, hiprl.MINUTE)
    ctl = m.lib.rls_trace_control()
    t = 1_700_000_007
    m.lib.rls_set_time(m.h, t)
    # a rule first seen by Set is registered as DoLimit registers it; the string is claimed
    before, (seq, pos) = m.set("s", "k", "v", rule, Found=1, Count=4, TtlSeconds=50)
    assert before == dict.fromkeys(NAMES, 0) and pos == ctl and seq != 2**64 - 1
    st, _ = m.peek("s", "k", "v", rule)
    assert st == dict(Found=1, LocalCached=0, Count=4, TtlSeconds=50, CachedSeconds=0)
    (code, rem, _), _ = m.do_limit("s", "k", "v", rule, 1)
    assert (code, rem) == (OK, 0)
    (code, rem, _), _ = m.do_limit("s", "k", "v", rule, 1)  # 6 > 5: over, and frozen
    assert (code, rem) == (OVER_LIMIT, 0)
    st, _ = m.peek("s", "k", "v", rule)
    assert (st["Count"], st["LocalCached"], st["CachedSeconds"]) == (6, 1, 60)
    # keep_counter: only the cache entry goes; the counter still says over
    before, _ = m.set("s", "k", "v", rule, keep_counter=True)
    assert before == st
    st2, _ = m.peek("s", "k", "v", rule)
    assert st2 == dict(st, LocalCached=0, CachedSeconds=0)
    # keep_cache: quota granted back, the (absent) cache entry untouched
    m.set("s", "k", "v", rule, keep_cache=True, Found=1, Count=2, TtlSeconds=30, LocalCached=1, CachedSeconds=9)
    st3, _ = m.peek("s", "k", "v", rule)
    assert st3 == dict(Found=1, LocalCached=0, Count=2, TtlSeconds=30, CachedSeconds=0)
    (code, rem, _), _ = m.do_limit("s", "k", "v", rule, 1)
    assert (code, rem) == (OK, 2)
    # a nil limit: nothing; a refusal of the engine arrives as RedisError
    assert m.set("s", "k", "v", -1, Found=1, Count=2, TtlSeconds=30)[0] == dict.fromkeys(NAMES, 0)
    with pytest.raises(hiprl.RedisError, match="ttl_s == 0"):
        m.set("s", "k", "v", rule, Found=1, Count=2)
    assert m.peek("s", "k", "v", rule)[0]["Count"] == 3
    m.close()


@pytest.mark.parametrize("mode", ["keep_cache", "keep_counter"])
def test_set_racing_concurrent_callers_has_one_place_in_the_serial_order(mode):
    """8 threads hit one key while the main thread sets it. Every call and every Set is traced; the
    serial order they report, replayed through the DoLimit rules of one key, gives every status.
    keep_cache: the Sets write the counter (to 5 below the limit); keep_counter: they drop the cache entry."""
    T, n, L = 8, 50, 60
    m = Cache(True, window_us=300)
    rule = m.lib.rls_add_rule(m.h, L, hiprl.HOUR)
    ctl = m.lib.rls_trace_control()
    m.lib.rls_set_time(m.h, 1_700_000_000)
    calls = [[] for _ in range(T)]

    def run(t):
        for i in range(n):
            hits = 1 + (t + i) % 3
            (code, rem, _), (seq, pos) = m.do_limit("race", "k", "shared", rule, hits)
            calls[t].append((seq, pos, "call", hits, code, rem))

    th = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    sets = []
    while any(x.is_alive() for x in th) and len(sets) < 150:
        if mode == "keep_cache":
            before, (seq, pos) = m.set("race", "k", "shared", rule, keep_cache=True, Found=1, Count=L - 5,
                                       TtlSeconds=3600)
        else:
            before, (seq, pos) = m.set("race", "k", "shared", rule, keep_counter=True)  # no cache entry
        assert pos == ctl and seq != 2**64 - 1
        sets.append((seq, -1, "set", before))  # before every call of batch `seq`
    for x in th:
        x.join()
    final, _ = m.peek("race", "k", "shared", rule)
    events = sorted([c for per in calls for c in per] + sets, key=lambda e: (e[0], e[1]))
    assert len({(e[0], e[1]) for e in events if e[2] == "call"}) == T * n
    count, frozen, mid, over = 0, False, 0, 0
    for e in events:
        if e[2] == "set":
            before = e[3]
            assert (before["Count"], bool(before["LocalCached"])) == (count, frozen), (e, count, frozen)
            mid += count > 0
            if mode == "keep_cache":
                count = L - 5
            else:
                frozen = False
            continue
        _, _, _, hits, code, rem = e
        if frozen:  # a local-cache hit: no INCRBY
            assert (code, rem) == (OVER_LIMIT, 0), (e, count)
            continue
        count += hits
        assert (code, rem) == ((OVER_LIMIT, 0) if count > L else (OK, L - count)), (e, count)
        if count > L:
            frozen = True
            over += 1
    assert (final["Count"], bool(final["LocalCached"])) == (count, frozen)
    assert mid > 0, "no Set landed among the callers' batches"
    assert over > 0, "guard: the key never went over its limit"
    m.close()


def test_set_over_the_watermark_is_followed_by_a_grow():
    m = Cache(False, log2_slots=(6, 6, 6, 6), autogrow_permille=500, max_log2_slots=(8, 8, 8, 8))
    rule = m.lib.rls_add_rule(m.h, 100, hiprl.HOUR)
    t = 1_700_000_007
    m.lib.rls_set_time(m.h, t)
    live0, slots0 = m.occupancy()
    assert slots0 == [64] * 8 and not any(live0) and m.lib.rls_resizes(m.h) == 0
    for i in range(40):
        m.set("grow", "k", f"v{i}", rule, Found=1, Count=i + 1, TtlSeconds=100)
        if i == 31:  # 32 live slots of 64: at the watermark, not over it
            assert m.lib.rls_resizes(m.h) == 0 and max(m.occupancy()[0]) == 32
        if i == 32:  # the Set that went over it was followed by the grow, before anything else ran
            assert m.lib.rls_resizes(m.h) == 1
    live, slots = m.occupancy()
    assert m.lib.rls_resizes(m.h) == 1 and sorted(slots) == [64] * 6 + [128] * 2 and max(live) == 40
    for i in range(40):
        st, _ = m.peek("grow", "k", f"v{i}", rule)
        assert (st["Found"], st["Count"], st["TtlSeconds"]) == (1, i + 1, 100), (i, st)
    m.close()
