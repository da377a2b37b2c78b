"""HipRateLimitCache::Adjust (rl_cache.hpp) through the batcher's queue (tests/cshim_adjust): an
Adjust between concurrent DoLimit callers sits at one place of the serial order, the place the
trace hook reports; a refund releases a frozen key; nothing is claimed, so auto-grow never follows
it; a call the engine refuses arrives as RedisError and the cache keeps serving."""
import ctypes as C
import threading
from pathlib import Path

import pytest

import hiprl

pytestmark = pytest.mark.gpu
SHIM = Path(__file__).resolve().parent / "cshim_adjust" / "librl_adjust_shim.so"
OK, OVER_LIMIT = 1, 2
NAMES = ["Found", "LocalCached", "Count", "TtlSeconds", "CachedSeconds"]


def _lib():
    if not SHIM.exists():
        raise RuntimeError(f"{SHIM} missing (built by __graft_entry__.build())")
    lib = C.CDLL(str(SHIM))
    vp, u32, u64, cp, pu32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint32)
    lib.rla_create.argtypes, lib.rla_create.restype = [C.c_int, u32, pu32, u32, pu32, u32], vp
    lib.rla_destroy.argtypes = [vp]
    lib.rla_set_time.argtypes = [vp, C.c_int64]
    lib.rla_add_rule.argtypes, lib.rla_add_rule.restype = [vp, u32, u32], C.c_int
    lib.rla_do_limit.argtypes = [vp, cp, cp, cp, C.c_int, u32, pu32, C.POINTER(u64), pu32]
    lib.rla_peek.argtypes = [vp, cp, cp, cp, C.c_int, pu32, C.POINTER(u64), pu32]
    lib.rla_adjust.argtypes = [vp, cp, cp, cp, C.c_int, C.POINTER(C.c_int32), u32, C.c_int, pu32, C.POINTER(u64), pu32]
    lib.rla_resizes.argtypes, lib.rla_resizes.restype = [vp], u64
    lib.rla_total_hits.argtypes, lib.rla_total_hits.restype = [vp, C.c_int], u64
    lib.rla_trace_control.restype = u32
    lib.rla_error.argtypes, lib.rla_error.restype = [vp], cp
    return lib


class Cache:
    def __init__(self, local_cache, window_us=0, log2_slots=(12, 12, 12, 12), autogrow_permille=0,
                 max_log2_slots=(31, 31, 31, 31), batch_limit=1 << 12):
        self.lib = _lib()
        self.h = self.lib.rla_create(int(local_cache), window_us, (C.c_uint32 * 4)(*log2_slots), autogrow_permille,
                                     (C.c_uint32 * 4)(*max_log2_slots), batch_limit)
        assert self.h, "HipRateLimitCache construction failed"

    def _ok(self, rc):
        if rc:
            raise hiprl.RedisError(self.lib.rla_error(self.h).decode())

    def do_limit(self, domain, key, value, rule, hits):
        """-> (code, remaining, throttle), (seq, pos)"""
        out, seq, pos = (C.c_uint32 * 3)(), C.c_uint64(), C.c_uint32()
        self._ok(self.lib.rla_do_limit(self.h, domain.encode(), key.encode(), value.encode(), rule, hits, out,
                                       C.byref(seq), C.byref(pos)))
        return tuple(out), (seq.value, pos.value)

    def peek(self, domain, key, value, rule):
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        self._ok(self.lib.rla_peek(self.h, domain.encode(), key.encode(), value.encode(), rule, out, C.byref(seq),
                                   C.byref(pos)))
        return dict(zip(NAMES, out)), (seq.value, pos.value)

    def adjust(self, domain, key, value, rule, deltas, keep_cache=False):
        """One descriptor per delta, all the same key -> the first one's status before, (seq, pos)"""
        deltas = [deltas] if isinstance(deltas, int) else list(deltas)
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        self._ok(self.lib.rla_adjust(self.h, domain.encode(), key.encode(), value.encode(), rule,
                                     (C.c_int32 * len(deltas))(*deltas), len(deltas), int(keep_cache), out,
                                     C.byref(seq), C.byref(pos)))
        return dict(zip(NAMES, out)), (seq.value, pos.value)

    def close(self):
        self.lib.rla_destroy(self.h)


def test_adjust_is_a_control_call_like_forget():
    m = Cache(True)
    rule = m.lib.rla_add_rule(m.h, 5, hiprl.MINUTE)
    ctl = m.lib.rla_trace_control()
    t = 1_700_000_007
    m.lib.rla_set_time(m.h, t)
    # a rule first seen by Adjust is registered as DoLimit registers it; an absent key stays absent
    before, (seq0, pos) = m.adjust("a", "k", "v", rule, 4)
    assert before == dict.fromkeys(NAMES, 0) and pos == ctl and seq0 != 2**64 - 1
    assert m.peek("a", "k", "v", rule)[0] == dict.fromkeys(NAMES, 0)
    (code, rem, _), (seq1, _) = m.do_limit("a", "k", "v", rule, 6)  # 6 > 5: over, and frozen
    assert (code, rem) == (OVER_LIMIT, 0)
    (code, rem, _), (seq2, _) = m.do_limit("a", "k", "v", rule, 1)  # a local-cache hit: no INCRBY
    assert (code, rem) == (OVER_LIMIT, 0) and seq2 > seq1 >= seq0
    st, _ = m.peek("a", "k", "v", rule)
    assert (st["Found"], st["Count"], st["LocalCached"], st["CachedSeconds"]) == (1, 6, 1, 60)
    hits = m.lib.rla_total_hits(m.h, rule)
    # keep_cache: the quota comes back, the key stays frozen until its deadline
    before, (seq3, pos) = m.adjust("a", "k", "v", rule, -1, keep_cache=True)
    assert before == st and pos == ctl and seq3 > seq2
    assert m.do_limit("a", "k", "v", rule, 1)[0][:2] == (OVER_LIMIT, 0)
    # the refund of a frozen key lets the next DoLimit through; two refunds of one key in one call add up
    before, (seq4, pos) = m.adjust("a", "k", "v", rule, [-1, -2])
    assert (before["Count"], before["LocalCached"]) == (5, 1) and pos == ctl
    st, _ = m.peek("a", "k", "v", rule)
    assert st == dict(Found=1, LocalCached=0, Count=2, TtlSeconds=before["TtlSeconds"], CachedSeconds=0)
    (code, rem, _), (seq5, pos5) = m.do_limit("a", "k", "v", rule, 1)
    # the control call is reported at the next batch to be gathered, in front of every call of it
    assert (code, rem) == (OK, 2) and seq5 == seq4 and pos5 != ctl
    assert m.lib.rla_total_hits(m.h, rule) == hits + 2  # the two DoLimits; no Adjust counts a hit
    # a nil limit: nothing
    assert m.adjust("a", "k", "v", -1, -3)[0] == dict.fromkeys(NAMES, 0)
    assert m.peek("a", "k", "v", rule)[0]["Count"] == 3
    # a call the engine refuses arrives as RedisError, and the cache keeps serving
    with pytest.raises(hiprl.RedisError, match="capacity"):
        m.adjust("a", "k", "v", rule, [-1] * ((1 << 12) + 4096 + 1))
    assert m.peek("a", "k", "v", rule)[0]["Count"] == 3
    assert m.do_limit("a", "k", "v", rule, 1)[0][:2] == (OK, 1)
    m.close()


def test_adjust_racing_concurrent_callers_has_one_place_in_the_serial_order():
    """8 threads hit one key while the main thread refunds it. Every call and every Adjust is
    traced; the serial order they report, replayed through the DoLimit rules of one key, gives every
    status: an Adjust sees the increments of the calls before it and is seen by those behind it."""
    T, n, L = 8, 50, 60
    m = Cache(True, window_us=300)
    rule = m.lib.rla_add_rule(m.h, L, hiprl.HOUR)
    ctl = m.lib.rla_trace_control()
    m.lib.rla_set_time(m.h, 1_700_000_000)
    calls = [[] for _ in range(T)]

    def run(t):
        for i in range(n):
            hits = 1 + (t + i) % 3
            (code, rem, _), (seq, pos) = m.do_limit("race", "k", "shared", rule, hits)
            calls[t].append((seq, pos, "call", hits, code, rem))

    refunds = []

    def refund(racing):
        # a small refund, a larger one after an Adjust that saw the key frozen (400 calls of 1..3
        # hits against at most 150 small refunds: the key does go over its limit)
        d = -10 if refunds and refunds[-1][3]["LocalCached"] else -1
        before, (seq, pos) = m.adjust("race", "k", "shared", rule, d)
        assert pos == ctl and seq != 2**64 - 1
        refunds.append((seq, -1, "adjust", before, d, racing))  # before every call of batch `seq`

    th = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    while any(x.is_alive() for x in th) and len(refunds) < 150:
        refund(True)
    for x in th:
        x.join()
    refund(False)
    refund(False)  # -10 if the one before saw the key frozen: 61..63 - 1 - 10 is under the limit
    final, _ = m.peek("race", "k", "shared", rule)
    events = sorted([c for per in calls for c in per] + refunds, key=lambda e: (e[0], e[1]))
    assert len({(e[0], e[1]) for e in events if e[2] == "call"}) == T * n
    count, exists, frozen, mid, over, released = 0, False, False, 0, 0, 0
    for e in events:
        if e[2] == "adjust":
            before, d, racing = e[3:]
            assert (bool(before["Found"]), before["Count"], bool(before["LocalCached"])) == (exists, count, frozen), e
            if exists:  # an absent counter is left alone
                mid += racing
                count = max(count + d, 0)
                if frozen and count <= L:
                    frozen, released = False, released + 1
            continue
        _, _, _, hits, code, rem = e
        if frozen:  # a local-cache hit: no INCRBY
            assert (code, rem) == (OVER_LIMIT, 0), (e, count)
            continue
        count += hits
        exists = True
        assert (code, rem) == ((OVER_LIMIT, 0) if count > L else (OK, L - count)), (e, count)
        if count > L:
            frozen = True
            over += 1
    assert (final["Count"], bool(final["LocalCached"])) == (count, frozen)
    assert mid > 0, "no Adjust landed among the callers' batches"
    assert over > 0, "guard: the key never went over its limit"
    assert released > 0, "guard: no refund released the frozen key"
    m.close()


def test_adjust_is_never_followed_by_a_grow():
    m = Cache(False, log2_slots=(6, 6, 6, 6), autogrow_permille=500, max_log2_slots=(8, 8, 8, 8))
    rule = m.lib.rla_add_rule(m.h, 100, hiprl.HOUR)
    m.lib.rla_set_time(m.h, 1_700_000_007)
    for i in range(32):  # 32 live slots of 64: at the watermark, not over it
        assert m.do_limit("grow", "k", f"v{i}", rule, 3)[0][:2] == (OK, 97)
    assert m.lib.rla_resizes(m.h) == 0
    for i in range(80):  # 48 of them absent: an Adjust claims nothing, so nothing grows
        before, _ = m.adjust("grow", "k", f"v{i}", rule, 2)
        assert (before["Found"], before["Count"]) == ((1, 3) if i < 32 else (0, 0))
    assert m.lib.rla_resizes(m.h) == 0
    assert m.peek("grow", "k", "v0", rule)[0]["Count"] == 5 and m.peek("grow", "k", "v40", rule)[0]["Found"] == 0
    assert m.do_limit("grow", "k", "v32", rule, 1)[0][:2] == (OK, 99)  # the 33rd slot: over the watermark
    assert m.peek("grow", "k", "v32", rule)[0]["Count"] == 1  # a control call: behind the batch's grow check
    assert m.lib.rla_resizes(m.h) == 1, "guard: auto-grow is on"
    m.close()
