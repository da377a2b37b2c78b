"""HipRoutedRateLimitCache::Adjust (rl_cache.hpp) through two emulated ranks' batchers
(tests/cshim_routed_adjust): a control call agreed at the rule / stop agreement beside Peek, Forget
and Set. An Adjust on one rank of a key the other rank owns is seen by a Peek from either rank and
by the owner's next DoLimit; a refund releases a frozen key and keep_cache leaves it frozen; both
kinds pending at one agreement, on both ranks, run in the documented order (without keep_cache
first); and the trace hook places every call between the steps where the header says it goes."""
import ctypes as C
import threading
from pathlib import Path

import pytest

import hiprl
import oracle

pytestmark = pytest.mark.gpu
SHIM = Path(__file__).resolve().parent / "cshim_routed_adjust" / "librl_routed_adjust_shim.so"
SEED = 0x5EE7AB1E5EED  # HipSettings::hash_seed's default
NOW = 1_700_000_517
DOMAIN = "ra"
FIELDS = ["Found", "LocalCached", "Count", "TtlSeconds", "CachedSeconds"]
RULES = [(5, hiprl.MINUTE), (50, hiprl.HOUR)]
OK, OVER = 1, 2


def _lib():
    if not SHIM.exists():
        raise RuntimeError(f"{SHIM} missing (built by __graft_entry__.build())")
    lib = C.CDLL(str(SHIM))
    vp, u32, u64, cp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p
    pu32, pu64 = C.POINTER(u32), C.POINTER(u64)
    lib.rla_create.argtypes, lib.rla_create.restype = [u32, u32, cp, C.c_int, u32, u32], vp
    lib.rla_destroy.argtypes = [vp]
    lib.rla_set_time.argtypes = [vp, C.c_int64]
    lib.rla_add_rule.argtypes, lib.rla_add_rule.restype = [vp, u32, u32], C.c_int
    lib.rla_do_limit.argtypes = [vp, cp, cp, cp, C.c_int, u32, pu32, pu64, pu32]
    lib.rla_peek.argtypes = [vp, cp, cp, cp, C.c_int, pu32, pu64, pu32]
    lib.rla_adjust.argtypes = [vp, cp, cp, cp, C.c_int, C.c_int32, C.c_int, pu32, pu64, pu32]
    lib.rla_trace_control.restype = u32
    lib.rla_error.argtypes, lib.rla_error.restype = [vp], cp
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
        raise hiprl.RedisError(self.lib.rla_error(self.h).decode())

    def do_limit(self, value, rule, hits):
        out, seq, pos = (C.c_uint32 * 3)(), C.c_uint64(), C.c_uint32()
        if self.lib.rla_do_limit(self.h, DOMAIN.encode(), b"k", value.encode(), rule, hits, out, C.byref(seq),
                                 C.byref(pos)):
            self._fail()
        return tuple(out), (seq.value, pos.value)

    def peek(self, value, rule):
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        if self.lib.rla_peek(self.h, DOMAIN.encode(), b"k", value.encode(), rule, out, C.byref(seq), C.byref(pos)):
            self._fail()
        return dict(zip(FIELDS, out)), (seq.value, pos.value)

    def adjust(self, value, rule, delta, keep_cache=False):
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        if self.lib.rla_adjust(self.h, DOMAIN.encode(), b"k", value.encode(), rule, delta, int(keep_cache), out,
                               C.byref(seq), C.byref(pos)):
            self._fail()
        return dict(zip(FIELDS, out)), (seq.value, pos.value)


def owned_by(rank, G, tag):
    return next(f"{tag}{i}" for i in range(64) if oracle.route_owner(
        *oracle.prefix_lanes(hiprl.cache_key_prefix(DOMAIN, [("k", f"{tag}{i}")]), SEED), G) == rank)


def test_routed_cache_adjust_is_seen_from_both_ranks_where_the_trace_says():
    G = 2
    lib = _lib()
    ctl = lib.rla_trace_control()
    wid = hiprl.Router.emu_world(G)
    hs = [None] * G
    _parallel(G, lambda r: hs.__setitem__(r, lib.rla_create(G, r, wid, 1, 300, 4)))
    assert all(hs), hs
    ranks = [Rank(lib, h) for h in hs]
    for m in ranks:
        lib.rla_set_time(m.h, NOW)
        assert [lib.rla_add_rule(m.h, L, u) for L, u in RULES] == [0, 1]
    absent = dict.fromkeys(FIELDS, 0)

    # a key owned by rank 1, charged there, given back from rank 0
    own1 = owned_by(1, G, "own")
    (code, rem, _), (seq_a, pos_a) = ranks[1].do_limit(own1, 1, 9)
    assert (code, rem) == (OK, 41) and pos_a != ctl
    before, (seq_s, pos_s) = ranks[0].adjust(own1, 1, -4)
    assert (before["Found"], before["Count"], before["TtlSeconds"]) == (1, 9, 3600), before  # the state before the call
    assert pos_s == ctl and seq_s > seq_a  # after every call of the steps before its agreement
    want = dict(Found=1, LocalCached=0, Count=5, TtlSeconds=3600, CachedSeconds=0)
    for m in ranks:
        got, (seq_p, pos_p) = m.peek(own1, 1)
        assert got == want and pos_p == ctl and seq_p >= seq_s, (got, seq_p)
    (code, rem, _), (seq_b, _) = ranks[1].do_limit(own1, 1, 2)
    assert (code, rem) == (OK, 50 - 7) and seq_b >= seq_s  # ... and before every call of the steps after it
    # a counter that is absent is left alone: nothing is claimed
    gone = owned_by(1, G, "gone")
    assert ranks[0].adjust(gone, 1, 6)[0] == absent and ranks[1].peek(gone, 1)[0] == absent

    # a key owned by rank 0, charged over its limit there: frozen. keep_cache from rank 1 moves the
    # counter and leaves it frozen; the refund without it releases it, and the owner's next DoLimit
    # answers as the oracle that was charged what is left
    own0 = owned_by(0, G, "cold")
    (code, _, _), _ = ranks[0].do_limit(own0, 0, 8)
    assert code == OVER
    frozen, _ = ranks[1].peek(own0, 0)
    assert (frozen["Found"], frozen["LocalCached"], frozen["Count"]) == (1, 1, 8) and frozen["CachedSeconds"] > 0
    before, (_, pos) = ranks[1].adjust(own0, 0, -2, keep_cache=True)
    assert before == frozen and pos == ctl
    kept, _ = ranks[0].peek(own0, 0)
    assert kept == dict(frozen, Count=6)  # 6 > 5: over the limit, still frozen
    before, _ = ranks[1].adjust(own0, 0, -3, keep_cache=True)
    assert before == kept
    kept, _ = ranks[0].peek(own0, 0)
    assert kept == dict(frozen, Count=3)  # back under the limit, and keep_cache left the deadline
    assert ranks[0].do_limit(own0, 0, 1)[0][0] == OVER  # a local-cache hit: no INCRBY
    assert ranks[1].peek(own0, 0)[0] == kept
    before, _ = ranks[1].adjust(own0, 0, -1)
    assert before == kept
    free, _ = ranks[0].peek(own0, 0)
    assert free == dict(frozen, Count=2, LocalCached=0, CachedSeconds=0)
    o = oracle.Oracle(local_cache=True)
    o.load_rules(RULES)
    o.submit(hiprl.build_batch([(DOMAIN, [[("k", own0)]], [0], 2, NOW)]))
    st, thr = o.submit(hiprl.build_batch([(DOMAIN, [[("k", own0)]], [0], 1, NOW)]))
    res, _ = ranks[0].do_limit(own0, 0, 1)
    assert res == (int(st["code_flags"][0]) & 0xFF, int(st["limit_remaining"][0]), int(thr[0])) and res[0] == OK, res

    # both kinds pending at one agreement, on both ranks: the calls without keep_cache run first (one
    # rl_router_adjust), then those with it (a second one). Each caller's key is frozen at 8 under a
    # limit of 5; the kind that runs first reads 8, the other reads what the first left
    both = owned_by(1, G, "both")
    assert ranks[0].do_limit(both, 0, 8)[0][0] == OVER
    got = {}

    def caller(i):
        r, keep = i % G, i >= G  # ranks 0 and 1 without keep_cache, ranks 0 and 1 with it
        got[i] = ranks[r].adjust(both, 0, -2 if keep else -1, keep_cache=keep)
    for attempt in range(20):  # until the four calls meet at one agreement (they are enqueued within one step period)
        got.clear()
        _parallel(2 * G, caller)
        seqs = {seq for _, (seq, _) in got.values()}
        assert all(pos == ctl for _, (_, pos) in got.values())
        plain = [got[i][0]["Count"] for i in range(G)]
        keep = [got[i][0]["Count"] for i in range(G, 2 * G)]
        if len(seqs) == 1:
            # one agreement: both plain calls read the same state (summed, applied once), then both
            # keep calls read that state less 2
            assert plain[0] == plain[1] and keep[0] == keep[1] == plain[0] - 2, (plain, keep)
            break
        ranks[0].adjust(both, 0, 6)  # (what the attempt took: the counter is back at 8 and never reaches 0)
    else:
        pytest.fail("the four calls never met at one agreement")
    final, _ = ranks[0].peek(both, 0)
    assert final["Count"] == keep[0] - 4
    # destruction is the agreed stop, with the wider agreement words
    _parallel(G, lambda r: lib.rla_destroy(hs[r]))
