"""HIP_REFUND_REJECTED on HipRoutedRateLimitCache (rl_cache.hpp) through two emulated ranks' batchers
(tests/cshim_routed_refund). A request a step rejects is queued by its rank's batcher and given back
at the next agreement by one rl_router_refund, at the owner of each of its keys; the trace hook
reports the refund as a control call with a null request. The counters peeked from both ranks behind
that agreement equal RoutedRefundOracle (routed_refund_model.py) with the refund placed where the
trace says; with the option off the same stream leaves the reference's counters, charged in full."""
import ctypes as C
import threading
from pathlib import Path

import pytest

import hiprl
import oracle
from routed_refund_model import RoutedRefundOracle

pytestmark = pytest.mark.gpu
SHIM = Path(__file__).resolve().parent / "cshim_routed_refund" / "librl_routed_refund_shim.so"
SEED = 0x5EE7AB1E5EED  # HipSettings::hash_seed's default
NOW = 1_700_000_517
DOMAIN = "rr"
FIELDS = ["Found", "LocalCached", "Count", "TtlSeconds", "CachedSeconds"]
RULES = [(10000, hiprl.MINUTE), (10000, hiprl.HOUR)]  # a cost limiter: units per window
OK, OVER = 1, 2
F, LC = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED


def _lib():
    if not SHIM.exists():
        raise RuntimeError(f"{SHIM} missing (built by __graft_entry__.build())")
    lib = C.CDLL(str(SHIM))
    vp, u32, u64, cp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p
    pu32, pu64 = C.POINTER(u32), C.POINTER(u64)
    lib.rlr_create.argtypes, lib.rlr_create.restype = [u32, u32, cp, C.c_int, C.c_int, u32, u32], vp
    lib.rlr_destroy.argtypes = [vp]
    lib.rlr_set_time.argtypes = [vp, C.c_int64]
    lib.rlr_add_rule.argtypes, lib.rlr_add_rule.restype = [vp, u32, u32], C.c_int
    lib.rlr_do_limit.argtypes = [vp, cp, cp, u32, C.POINTER(cp), C.POINTER(C.c_int), u32, pu32, pu64, pu32]
    lib.rlr_peek.argtypes = [vp, cp, cp, cp, C.c_int, pu32, pu64, pu32]
    lib.rlr_refund_flights.argtypes, lib.rlr_refund_flights.restype = [vp], u64
    lib.rlr_refund_failures.argtypes, lib.rlr_refund_failures.restype = [vp], u64
    lib.rlr_refund_seqs.argtypes, lib.rlr_refund_seqs.restype = [vp, pu64, u32], u32
    lib.rlr_trace_control.restype = u32
    lib.rlr_error.argtypes, lib.rlr_error.restype = [vp], cp
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
        raise hiprl.RedisError(self.lib.rlr_error(self.h).decode())

    def do_limit(self, values, rules, hits):
        n = len(values)
        out, seq, pos = (C.c_uint32 * (2 * n))(), C.c_uint64(), C.c_uint32()
        vs = (C.c_char_p * n)(*[v.encode() for v in values])
        rs = (C.c_int * n)(*rules)
        if self.lib.rlr_do_limit(self.h, DOMAIN.encode(), b"k", n, vs, rs, hits, out, C.byref(seq), C.byref(pos)):
            self._fail()
        return [(out[2 * i], out[2 * i + 1]) for i in range(n)], (seq.value, pos.value)

    def peek(self, value, rule):
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        if self.lib.rlr_peek(self.h, DOMAIN.encode(), b"k", value.encode(), rule, out, C.byref(seq), C.byref(pos)):
            self._fail()
        return dict(zip(FIELDS, out)), (seq.value, pos.value)

    def refund_seqs(self):
        buf = (C.c_uint64 * 64)()
        n = self.lib.rlr_refund_seqs(self.h, buf, 64)
        return list(buf[:min(n, 64)])


def owned_by(rank, G, tag):
    return next(f"{tag}{i}" for i in range(64) if oracle.route_owner(
        *oracle.prefix_lanes(hiprl.cache_key_prefix(DOMAIN, [("k", f"{tag}{i}")]), SEED), G) == rank)


def request(values, rules, hits):
    return hiprl.build_batch([(DOMAIN, [[("k", v)] for v in values], rules, hits, NOW)])


def model_peek(m, value, rule):
    b = request([value], [rule], 1)
    count, ttl, cached, flags = m.peek(*m._key(b, 0), NOW)
    return dict(Found=int(bool(flags & F)), LocalCached=int(bool(flags & LC)), Count=count, TtlSeconds=ttl,
                CachedSeconds=cached)


def model_do_limit(m, values, rules, hits):
    b = request(values, rules, hits)
    st, _ = m.submit(b)
    return b, st, [(int(c) & 0xFF, int(r)) for c, r in zip(st["code_flags"], st["limit_remaining"])]


@pytest.mark.parametrize("refund", [True, False])
def test_rejected_requests_are_given_back_at_the_next_agreement(refund):
    G = 2
    lib = _lib()
    ctl = lib.rlr_trace_control()
    wid = hiprl.Router.emu_world(G)
    hs = [None] * G
    _parallel(G, lambda r: hs.__setitem__(r, lib.rlr_create(G, r, wid, 1, int(refund), 300, 4)))
    assert all(hs), hs
    ranks = [Rank(lib, h) for h in hs]
    for rk in ranks:
        lib.rlr_set_time(rk.h, NOW)
        assert [lib.rlr_add_rule(rk.h, L, u) for L, u in RULES] == [0, 1]
    m = RoutedRefundOracle(RULES, local_cache=True)
    glob, user = owned_by(1, G, "glob"), owned_by(0, G, "user")  # the verdict is seen on rank 0; "glob" lives on rank 1

    # 9000 of 10000 spent; a request of cost 1500 on the global key and on a per-user key is rejected
    # by the global one, and both descriptors were charged
    got, (seq_a, _) = ranks[1].do_limit([glob], [0], 9000)
    assert got == model_do_limit(m, [glob], [0], 9000)[2] == [(OK, 1000)]
    got, (seq_b, pos_b) = ranks[0].do_limit([glob, user], [0, 1], 1500)
    b, st, want = model_do_limit(m, [glob, user], [0, 1], 1500)
    assert got == want and [c for c, _ in got] == [OVER, OK] and pos_b != ctl and seq_b >= seq_a
    empty = request([], [], 1)
    if refund:  # where the trace says: at the agreement behind the step, in front of that agreement's Peeks
        amounts, _, origin, owner = m.refund_routed([b, empty], [st, st[:0]])
        assert amounts == [[1500, 1500], []] and owner == dict(absent=0, refunded=2, floored=0, unfrozen=1)
    peeks = [(rk.peek(glob, 0), rk.peek(user, 1)) for rk in ranks]
    for (pg, (seq_g, pos_g)), (pu, (seq_u, pos_u)) in peeks:
        assert pos_g == pos_u == ctl and seq_g > seq_b
        assert pg == model_peek(m, glob, 0) and pu == model_peek(m, user, 1), (pg, pu)
    # refunded: 9000 again, not frozen, and the user's quota is back; charged in full otherwise
    assert (peeks[0][0][0]["Count"], peeks[0][0][0]["LocalCached"], peeks[0][1][0]["Count"]) == \
        ((9000, 0, 0) if refund else (10500, 1, 1500))
    seqs = ranks[0].refund_seqs()
    if refund:
        assert len(seqs) == 1 and seq_b < seqs[0] <= peeks[0][0][1][0], (seq_b, seqs, peeks[0][0][1])
        assert ranks[1].refund_seqs() == [] and lib.rlr_refund_flights(ranks[0].h) == 1
    else:
        assert seqs == [] and lib.rlr_refund_flights(ranks[0].h) == 0
    assert lib.rlr_refund_flights(ranks[1].h) == 0
    assert [lib.rlr_refund_failures(rk.h) for rk in ranks] == [0, 0]
    # the owner's next decision: 100 more fit behind the refund, and are refused without it
    got, _ = ranks[1].do_limit([glob], [0], 100)
    assert got == model_do_limit(m, [glob], [0], 100)[2] == ([(OK, 900)] if refund else [(OVER, 0)])
    _parallel(G, lambda r: lib.rlr_destroy(hs[r]))
