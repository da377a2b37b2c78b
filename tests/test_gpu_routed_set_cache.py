"""HipRoutedRateLimitCache::Set (rl_cache.hpp) through two emulated ranks' batchers
(tests/cshim_routed_set): a control call agreed at the rule / stop agreement beside Peek and Forget.
A Set on one rank of a key the other rank owns is seen by a Peek from either rank and by the
owner's next DoLimit, it sits between the steps where the trace hook says it does, and both ranks'
Sets at the same agreements do not disturb each other."""
import ctypes as C
import threading
from pathlib import Path

import pytest

import hiprl
import oracle

pytestmark = pytest.mark.gpu
SHIM = Path(__file__).resolve().parent / "cshim_routed_set" / "librl_routed_set_shim.so"
SEED = 0x5EE7AB1E5EED  # HipSettings::hash_seed's default
NOW = 1_700_000_517
DOMAIN = "rs"
FIELDS = ["Found", "LocalCached", "Count", "TtlSeconds", "CachedSeconds"]
RULES = [(5, hiprl.MINUTE), (50, hiprl.HOUR)]


def _lib():
    if not SHIM.exists():
        raise RuntimeError(f"{SHIM} missing (built by __graft_entry__.build())")
    lib = C.CDLL(str(SHIM))
    vp, u32, u64, cp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p
    pu32, pu64 = C.POINTER(u32), C.POINTER(u64)
    lib.rls_create.argtypes, lib.rls_create.restype = [u32, u32, cp, C.c_int, u32, u32], vp
    lib.rls_destroy.argtypes = [vp]
    lib.rls_set_time.argtypes = [vp, C.c_int64]
    lib.rls_add_rule.argtypes, lib.rls_add_rule.restype = [vp, u32, u32], C.c_int
    lib.rls_do_limit.argtypes = [vp, cp, cp, cp, C.c_int, u32, pu32, pu64, pu32]
    lib.rls_peek.argtypes = [vp, cp, cp, cp, C.c_int, pu32, pu64, pu32]
    lib.rls_set.argtypes = [vp, cp, cp, cp, C.c_int, pu32, C.c_int, C.c_int, pu32, pu64, pu32]
    lib.rls_trace_control.restype = u32
    lib.rls_error.argtypes, lib.rls_error.restype = [vp], cp
    return lib


def _parallel(n, fn, timeout=120):
    errs = []

    def run(i):
        try:
            fn(i)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    ths = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(n)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout)
    assert not any(t.is_alive() for t in ths), "a caller or a rank hung"
    assert not errs, errs


class Rank:
    def __init__(self, lib, h):
        self.lib, self.h = lib, h

    def _fail(self):
        raise hiprl.RedisError(self.lib.rls_error(self.h).decode())

    def do_limit(self, value, rule, hits):
        out, seq, pos = (C.c_uint32 * 3)(), C.c_uint64(), C.c_uint32()
        if self.lib.rls_do_limit(self.h, DOMAIN.encode(), b"k", value.encode(), rule, hits, out, C.byref(seq),
                                 C.byref(pos)):
            self._fail()
        return tuple(out), (seq.value, pos.value)

    def peek(self, value, rule):
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        if self.lib.rls_peek(self.h, DOMAIN.encode(), b"k", value.encode(), rule, out, C.byref(seq), C.byref(pos)):
            self._fail()
        return dict(zip(FIELDS, out)), (seq.value, pos.value)

    def set(self, value, rule, keep_counter=False, keep_cache=False, **v):
        val = (C.c_uint32 * 5)(*[int(v.get(f, 0)) for f in FIELDS])
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        if self.lib.rls_set(self.h, DOMAIN.encode(), b"k", value.encode(), rule, val, int(keep_counter),
                            int(keep_cache), out, C.byref(seq), C.byref(pos)):
            self._fail()
        return dict(zip(FIELDS, out)), (seq.value, pos.value)


def owned_by(rank, G, tag):
    return next(f"{tag}{i}" for i in range(64) if oracle.route_owner(
        *oracle.prefix_lanes(hiprl.cache_key_prefix(DOMAIN, [("k", f"{tag}{i}")]), SEED), G) == rank)


def test_routed_cache_set_is_seen_from_both_ranks_where_the_trace_says():
    G = 2
    lib = _lib()
    ctl = lib.rls_trace_control()
    wid = hiprl.Router.emu_world(G)
    hs = [None] * G
    _parallel(G, lambda r: hs.__setitem__(r, lib.rls_create(G, r, wid, 1, 300, 4)))
    assert all(hs), hs
    ranks = [Rank(lib, h) for h in hs]
    for m in ranks:
        lib.rls_set_time(m.h, NOW)
        assert [lib.rls_add_rule(m.h, L, u) for L, u in RULES] == [0, 1]
    absent = dict.fromkeys(FIELDS, 0)

    # a key owned by rank 1, hit there, set from rank 0
    own1 = owned_by(1, G, "own")
    (code, rem, _), (seq_a, pos_a) = ranks[1].do_limit(own1, 1, 4)
    assert (code, rem) == (1, 46) and pos_a != ctl
    before, (seq_s, pos_s) = ranks[0].set(own1, 1, Found=1, Count=20, TtlSeconds=1000)
    assert (before["Found"], before["Count"], before["TtlSeconds"]) == (1, 4, 3600), before  # the state before the call
    assert pos_s == ctl and seq_s > seq_a  # after every call of the steps before its agreement
    want = dict(Found=1, LocalCached=0, Count=20, TtlSeconds=1000, CachedSeconds=0)
    for m in ranks:
        got, (seq_p, pos_p) = m.peek(own1, 1)
        assert got == want and pos_p == ctl and seq_p >= seq_s, (got, seq_p)
    (code, rem, _), (seq_b, _) = ranks[1].do_limit(own1, 1, 2)
    assert (code, rem) == (1, 50 - 22) and seq_b >= seq_s  # ... and before every call of the steps after it

    # a key owned by rank 0, never seen, set over its limit and frozen from rank 1: the owner's
    # DoLimit answers as the oracle that reached that state by requests
    own0 = owned_by(0, G, "cold")
    before, (_, pos) = ranks[1].set(own0, 0, Found=1, LocalCached=1, Count=9, TtlSeconds=60, CachedSeconds=40)
    assert before == absent and pos == ctl
    o = oracle.Oracle(local_cache=True)
    o.load_rules(RULES)
    o.submit(hiprl.build_batch([(DOMAIN, [[("k", own0)]], [0], 9, NOW)]))
    st, thr = o.submit(hiprl.build_batch([(DOMAIN, [[("k", own0)]], [0], 1, NOW)]))
    for m in ranks:
        got, _ = m.peek(own0, 0)
        assert (got["Found"], got["LocalCached"], got["Count"], got["CachedSeconds"]) == (1, 1, 9, 40), got
    res, _ = ranks[0].do_limit(own0, 0, 1)
    assert res == (int(st["code_flags"][0]) & 0xFF, int(st["limit_remaining"][0]), int(thr[0])) and res[0] == 2, res
    # KEEP bits: the counter alone, then nothing at all
    ranks[0].set(own0, 0, keep_cache=True, Found=1, Count=2, TtlSeconds=30)
    got, _ = ranks[1].peek(own0, 0)
    assert (got["Count"], got["TtlSeconds"], got["LocalCached"], got["CachedSeconds"]) == (2, 30, 1, 40), got
    same, _ = ranks[1].set(own0, 0, keep_counter=True, keep_cache=True, Found=1, Count=77, TtlSeconds=5)
    assert same == got and ranks[0].peek(own0, 0)[0] == got
    # a refused value fails the call, on the caller's rank, and writes nothing
    with pytest.raises(hiprl.RedisError):
        ranks[1].set(own0, 0, Found=1, Count=3, TtlSeconds=0)
    assert ranks[0].peek(own0, 0)[0] == got

    # both ranks' callers set their own keys over and over, at the same agreements
    def caller(i):
        r, m = i % G, ranks[i % G]
        key = f"mine{i}"
        last = absent
        for q in range(8):
            before, (_, pos) = m.set(key, 1, Found=1, Count=q + 1, TtlSeconds=100 + q)
            assert before == last and pos == ctl, (i, q, before, last)
            last = dict(Found=1, LocalCached=0, Count=q + 1, TtlSeconds=100 + q, CachedSeconds=0)
            assert ranks[1 - r].peek(key, 1)[0] == last, (i, q)
    _parallel(2 * G, caller)
    # destruction is the agreed stop, with the wider agreement words
    _parallel(G, lambda r: lib.rls_destroy(hs[r]))
