"""HipRateLimitCache with HIP_REFUND_REJECTED (rl_cache.hpp) through the batcher's queue
(tests/cshim_refund): every gather's decision batch is followed by one rl_refund_behind flight. Every
call's place in the serial order is the one the trace hook reports; replayed in that order through
RefundOracle (refund_model.py: the oracle's DoLimit, the model's refund behind every batch), it gives
every answer."""
import ctypes as C
import threading
from pathlib import Path

import numpy as np
import pytest

import hiprl
from refund_model import RefundOracle

pytestmark = pytest.mark.gpu
SHIM = Path(__file__).resolve().parent / "cshim_refund" / "librl_refund_shim.so"
OK, OVER_LIMIT = 1, 2
T0 = 1_700_000_000


def _lib():
    if not SHIM.exists():
        raise RuntimeError(f"{SHIM} missing (built by __graft_entry__.build())")
    lib = C.CDLL(str(SHIM))
    vp, u32, u64, cp, pu32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint32)
    lib.rlf_create.argtypes, lib.rlf_create.restype = [C.c_int, C.c_int, u32, pu32, u32], vp
    lib.rlf_destroy.argtypes = [vp]
    lib.rlf_set_time.argtypes = [vp, C.c_int64]
    lib.rlf_add_rule.argtypes, lib.rlf_add_rule.restype = [vp, u32, u32], C.c_int
    lib.rlf_do_limit.argtypes = [vp, cp, cp, C.c_int, cp, C.c_int, u32, pu32, C.POINTER(u64), pu32]
    lib.rlf_peek.argtypes = [vp, cp, cp, C.c_int, pu32]
    for f in (lib.rlf_refunds, lib.rlf_refund_failures, lib.rlf_batches, lib.rlf_compact_batches):
        f.argtypes, f.restype = [vp], u64
    lib.rlf_error.argtypes, lib.rlf_error.restype = [vp], cp
    return lib


class Cache:
    def __init__(self, local_cache, refund=True, window_us=0, log2_slots=(12, 12, 12, 12), batch_limit=1 << 12):
        self.lib = _lib()
        self.h = self.lib.rlf_create(int(local_cache), int(refund), window_us, (C.c_uint32 * 4)(*log2_slots), batch_limit)
        assert self.h, "HipRateLimitCache construction failed"

    def _ok(self, rc):
        if rc:
            raise hiprl.RedisError(self.lib.rlf_error(self.h).decode())

    def do_limit(self, k0, r0, k1, r1, hits):
        """-> (code0, remaining0, code1, remaining1, throttle), (seq, pos)"""
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        self._ok(self.lib.rlf_do_limit(self.h, b"q", k0.encode(), r0, k1.encode(), r1, hits, out, C.byref(seq),
                                       C.byref(pos)))
        return tuple(out), (seq.value, pos.value)

    def peek(self, key, rule):
        out = (C.c_uint32 * 3)()
        self._ok(self.lib.rlf_peek(self.h, b"q", key.encode(), rule, out))
        return tuple(out)

    def close(self):
        self.lib.rlf_destroy(self.h)


def test_the_cost_limiter_case_through_the_batcher():
    """9000 / 10000: a request of 1500 is rejected and gives its hits back on both descriptors; 100
    behind it passes. Without the option the reference's charge stands."""
    for refund in (True, False):
        m = Cache(False, refund)
        user, glob = m.lib.rlf_add_rule(m.h, 10000, hiprl.HOUR), m.lib.rlf_add_rule(m.h, 1 << 20, hiprl.HOUR)
        m.lib.rlf_set_time(m.h, T0)
        assert m.do_limit("u", user, "g", glob, 9000)[0][:2] == (OK, 1000)
        assert m.do_limit("u", user, "g", glob, 1500)[0][:3] == (OVER_LIMIT, 0, OK)
        assert m.peek("u", user) == (1, 0, 9000 if refund else 10500)
        assert m.peek("g", glob) == (1, 0, 9000 if refund else 10500)
        assert m.do_limit("u", user, "g", glob, 100)[0][:2] == ((OK, 900) if refund else (OVER_LIMIT, 0))
        assert m.lib.rlf_refunds(m.h) == (3 if refund else 0) and m.lib.rlf_refund_failures(m.h) == 0
        # with the option no batch goes in the compact format: its statuses would not be on the device
        assert (m.lib.rlf_compact_batches(m.h) == 0) == refund
        m.close()


@pytest.mark.parametrize("local_cache", [False, True])
def test_callers_replay_in_the_traced_order(local_cache):
    """Eight threads call DoLimit on 16 shared keys, each request with a per-key and a shared
    descriptor."""
    TD, n, K = 8, 150, 16
    rules = [(40, hiprl.HOUR), (600, hiprl.HOUR)]
    m = Cache(local_cache, window_us=200)
    ids = [m.lib.rlf_add_rule(m.h, L, u) for L, u in rules]
    m.lib.rlf_set_time(m.h, T0)
    # one call before the race, so that registering the rules is not part of it
    first = m.do_limit("warm", ids[0], "warm2", ids[1], 1)
    events = [[first + (("warm", "warm2", 1),)]] + [[] for _ in range(TD)]

    def caller(t):
        rng = np.random.default_rng(t)
        for i in range(n):
            k0, k1, hits = f"s{int(rng.integers(0, K))}", f"g{int(rng.integers(0, 2))}", int(rng.integers(0, 4))
            events[1 + t].append(m.do_limit(k0, ids[0], k1, ids[1], hits) + ((k0, k1, hits),))

    th = [threading.Thread(target=caller, args=(t,)) for t in range(TD)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    ev = sorted((e for per in events for e in per), key=lambda e: e[1])
    assert len({e[1] for e in ev}) == TD * n + 1, "every call has a place of its own"
    o = RefundOracle(rules, local_cache=local_cache)
    rejected = batches = i = 0
    while i < len(ev):
        j = i
        while j < len(ev) and ev[j][1][0] == ev[i][1][0]:
            j += 1
        hb = hiprl.build_batch([("q", [[("k", k0)], [("k", k1)]], [0, 1], hits, T0) for _, _, (k0, k1, hits) in ev[i:j]])
        st, thr = o.submit(hb)
        _, rep = o.refund(hb, st)
        rejected += rep["rejected_req"]
        batches += 1
        for r, (got, _, call) in enumerate(ev[i:j]):
            want = tuple(int(st[2 * r + d][f]) & msk for d in (0, 1) for f, msk in (("code_flags", 0xFF), ("limit_remaining", -1)))
            assert got == want + (int(thr[r]),), (call, got, want)
        i = j
    assert m.lib.rlf_refunds(m.h) == batches and m.lib.rlf_refund_failures(m.h) == 0
    assert rejected > TD * n // 4 and batches > 10, (rejected, batches)
    for k in range(K):
        key, store = o._key(hiprl.build_batch([("q", [[("k", f"s{k}")]], [0], 1, T0)]), 0)
        count, _, _, flags = o.peek(key, store, T0)
        assert m.peek(f"s{k}", ids[0]) == (int(bool(flags & hiprl.PEEK_FOUND)), int(bool(flags & hiprl.PEEK_LOCAL_CACHED)), count)
    m.close()
