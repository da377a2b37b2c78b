"""HipRoutedRateLimitCache::Peek / Forget (rl_cache.hpp) through two emulated ranks' batchers
(tests/cshim_routed_peek): control calls agreed at the rule / stop agreement. Callers on both ranks
mix DoLimit, Peek and Forget on shared keys; replaying every call in the traced serial order —
(step, rank, position), each control call before the step the trace names, peeks before forgets
within one agreement — through one oracle reproduces every DoLimit response and every PeekStatus."""
import ctypes as C
import threading
from pathlib import Path

import numpy as np
import pytest

import hiprl
import oracle

pytestmark = pytest.mark.gpu
SHIM = Path(__file__).resolve().parent / "cshim_routed_peek" / "librl_routed_peek_shim.so"
SEED = 0x5EE7AB1E5EED  # HipSettings::hash_seed's default
NOW = 1_700_000_517
DOMAIN = "rp"
FIELDS = ["Found", "LocalCached", "Count", "TtlSeconds", "CachedSeconds"]


def _lib():
    if not SHIM.exists():
        raise RuntimeError(f"{SHIM} missing (built by __graft_entry__.build())")
    lib = C.CDLL(str(SHIM))
    vp, u32, u64, cp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p
    lib.rlr_create.argtypes, lib.rlr_create.restype = [u32, u32, cp, C.c_int, u32, u32], vp
    lib.rlr_destroy.argtypes = [vp]
    lib.rlr_set_time.argtypes = [vp, C.c_int64]
    lib.rlr_add_rule.argtypes, lib.rlr_add_rule.restype = [vp, u32, u32], C.c_int
    lib.rlr_do_limit.argtypes = [vp, cp, cp, cp, C.c_int, u32, C.POINTER(u32), C.POINTER(u64), C.POINTER(u32)]
    lib.rlr_peek.argtypes = [vp, C.c_int, cp, cp, cp, C.c_int, C.POINTER(u32), C.POINTER(u64), C.POINTER(u32)]
    lib.rlr_total_hits.argtypes, lib.rlr_total_hits.restype = [vp, C.c_int], u64
    lib.rlr_trace_control.restype = u32
    lib.rlr_routed_stats.argtypes = [vp, C.POINTER(u64)]
    lib.rlr_error.argtypes, lib.rlr_error.restype = [vp], cp
    return lib


def _parallel(n, fn, timeout=120):
    ths = [threading.Thread(target=fn, args=(i,), daemon=True) for i in range(n)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout)
    assert not any(t.is_alive() for t in ths), "a caller or a rank hung"


class Rank:
    def __init__(self, lib, h):
        self.lib, self.h = lib, h

    def do_limit(self, value, rule, hits):
        out, seq, pos = (C.c_uint32 * 3)(), C.c_uint64(), C.c_uint32()
        rc = self.lib.rlr_do_limit(self.h, DOMAIN.encode(), b"k", value.encode(), rule, hits, out, C.byref(seq),
                                   C.byref(pos))
        if rc:
            raise hiprl.RedisError(self.lib.rlr_error(self.h).decode())
        return tuple(out), (seq.value, pos.value)

    def peek(self, value, rule, forget=False):
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        rc = self.lib.rlr_peek(self.h, int(forget), DOMAIN.encode(), b"k", value.encode(), rule, out, C.byref(seq),
                               C.byref(pos))
        if rc:
            raise hiprl.RedisError(self.lib.rlr_error(self.h).decode())
        return dict(zip(FIELDS, out)), (seq.value, pos.value)


def test_routed_cache_peek_and_forget_in_the_traced_serial_order():
    G, T, n = 2, 3, 50
    rules = [(5, hiprl.MINUTE), (50, hiprl.HOUR), (9, hiprl.HOUR)]  # the last one: never used by a DoLimit
    lib = _lib()
    ctl = lib.rlr_trace_control()
    wid = hiprl.Router.emu_world(G)
    hs = [None] * G
    _parallel(G, lambda r: hs.__setitem__(r, lib.rlr_create(G, r, wid, 1, 300, 4)))
    assert all(hs), hs
    ranks = [Rank(lib, h) for h in hs]
    for m in ranks:
        lib.rlr_set_time(m.h, NOW)
        assert [lib.rlr_add_rule(m.h, L, u) for L, u in rules] == [0, 1, 2]
    # every caller's script, made up front: mostly DoLimit on 8 shared keys, every 7th call a Peek
    # or a Forget (both ranks make both); rank 0's first caller also peeks under the unused limit
    rng = np.random.default_rng(11)
    scripts = []
    for i in range(G * T):
        ops = []
        for q in range(n):
            value, rule = f"v{int(rng.integers(0, 8))}", int(rng.integers(0, 2))
            if q % 7 == 6:
                ops.append(("forget" if (q // 7 + i) % 3 == 0 else "peek", value, rule, 1))
            else:
                ops.append(("do", value, rule, int(rng.integers(0, 4))))
        scripts.append(ops)
    scripts[0][20] = ("peek", "v1", 2, 1)
    events = []  # (rank, kind, value, rule, hits, result, (seq, pos))
    lock = threading.Lock()

    def run_op(r, op):
        kind, value, rule, hits = op
        if kind == "do":
            res, place = ranks[r].do_limit(value, rule, hits)
        else:
            res, place = ranks[r].peek(value, rule, forget=kind == "forget")
        with lock:
            events.append((r, kind, value, rule, hits, res, place))
        return res

    def caller(i):
        for op in scripts[i]:
            run_op(i // T, op)
    _parallel(G * T, caller)
    # a key owned by rank 1, hit there, peeked and forgotten from rank 0
    own1 = next(f"own{i}" for i in range(64) if oracle.route_owner(
        *oracle.prefix_lanes(hiprl.cache_key_prefix(DOMAIN, [("k", f"own{i}")]), SEED), G) == 1)
    run_op(1, ("do", own1, 1, 4))
    run_op(1, ("do", own1, 1, 3))
    st = run_op(0, ("peek", own1, 1, 1))
    assert (st["Found"], st["Count"], st["LocalCached"]) == (1, 7, 0) and st["TtlSeconds"] == 3600, st
    assert run_op(0, ("forget", own1, 1, 1)) == st
    assert run_op(0, ("peek", own1, 1, 1)) == dict.fromkeys(FIELDS, 0)
    assert run_op(1, ("do", own1, 1, 2))[:2] == (1, 48)  # counts from 0 again
    hits_before = [lib.rlr_total_hits(m.h, 1) for m in ranks]
    run_op(0, ("peek", own1, 1, 1))
    assert [lib.rlr_total_hits(m.h, 1) for m in ranks] == hits_before  # a Peek adds no hits

    # ---- replay in the traced serial order ----
    for r, kind, *_, (seq, pos) in events:
        assert seq != 2 ** 64 - 1 and (pos == ctl) == (kind != "do"), (r, kind, seq, pos)
    assert len({e[6] + (e[0],) for e in events if e[1] == "do"}) == sum(e[1] == "do" for e in events)

    def order(e):
        r, kind, *_, (seq, pos) = e
        return (seq, 1, 0, r, pos) if kind == "do" else (seq, 0, kind == "forget", r, 0)
    events.sort(key=order)

    def fresh():
        o = oracle.Oracle(local_cache=True)
        o.load_rules(rules)
        return o

    def string_of(value, rule):
        return oracle.cache_key(hiprl.cache_key_prefix(DOMAIN, [("k", value)]), rules[rule][1], NOW)

    def want_peek(o, value, rule):
        k = string_of(value, rule)
        c, lc = o.counter(k, NOW), o.local_cached(k, NOW)
        return c >= 0, lc, max(c, 0)
    o = fresh()
    hist = []  # (key string, batch) of every DoLimit applied and not forgotten since
    seen = dict(peek_found=0, forget_found=0, cached=0)
    i = 0
    while i < len(events):
        r, kind, value, rule, hits, res, (seq, _) = events[i]
        if kind == "do":
            b = hiprl.build_batch([(DOMAIN, [[("k", value)]], [rule], hits, NOW)])
            st, thr = o.submit(b)
            want = (int(st["code_flags"][0]) & 0xFF, int(st["limit_remaining"][0]), int(thr[0]))
            assert res == want, (i, events[i], want)
            hist.append((string_of(value, rule), b))
            i += 1
            continue
        # the control calls of one kind of one agreement: all of them read the state before any clears
        j = i
        while j < len(events) and events[j][1] == kind and events[j][6][0] == seq:
            j += 1
        gone = set()
        for r2, _, value, rule, _, res, _ in events[i:j]:
            found, lc, count = want_peek(o, value, rule)
            assert (bool(res["Found"]), bool(res["LocalCached"]), res["Count"]) == (found, lc, count), (events[i], res)
            assert (res["TtlSeconds"] > 0) == found and (res["CachedSeconds"] > 0) == lc, res
            seen["peek_found" if kind == "peek" else "forget_found"] += found
            seen["cached"] += lc
            gone.add(string_of(value, rule))
        if kind == "forget":  # an oracle that never saw the forgotten strings
            hist = [h for h in hist if h[0] not in gone]
            o = fresh()
            for _, b in hist:
                o.submit(b)
        i = j
    # guards: the control calls met live, frozen and cleared state, from both ranks, at many agreements
    assert seen["peek_found"] >= 10 and seen["forget_found"] >= 5 and seen["cached"] >= 3, seen
    for kind in ("peek", "forget"):
        assert {e[0] for e in events if e[1] == kind} == {0, 1}
    assert len({e[6][0] for e in events if e[1] != "do"}) >= 5
    stats = (C.c_uint64 * 5)()
    lib.rlr_routed_stats(ranks[0].h, stats)
    assert stats[3] == 3  # the limit only a Peek used was agreed too
    # destruction is the agreed stop, with the wider agreement words
    _parallel(G, lambda r: lib.rlr_destroy(hs[r]))
