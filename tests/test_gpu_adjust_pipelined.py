"""Adjust in flight (rl_hip.h "Adjust in flight") on the GPU: rl_adjust_pipelined, rl_adjust_submit and
rl_wait_adjust between batches in flight. The reference is the engine itself run one call at a
time (rl_submit_device, rl_wait, the synchronous rl_adjust, pinned by test_gpu_adjust.py) and the
dict model of adjust_model.py. Every comparison is of exact integers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hiprl
import router
import streams
from adjust_model import adjust_model, string_of
from streams import RULES

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = -1, -4, -5
NIL = hiprl.NIL_RULE
F, NILF, BAD = hiprl.PEEK_FOUND, hiprl.PEEK_NIL, hiprl.PEEK_BAD
MAXD = 1 << 14


def dev():
    return torch.device("cuda", 0)


def engine(local_cache=False, rules=RULES, **kw):
    kw.setdefault("max_batch_desc", MAXD)
    kw.setdefault("pipeline", "v4")
    e = hiprl.Engine(near_limit_ratio=0.8, local_cache=local_cache, **kw)
    e.load_rules(rules)
    return e


def key_batch(items):
    """[(prefix bytes, rule id, now)] -> a batch of one request per descriptor (times must not matter
    to the order: req_of is the descriptor index)."""
    off = np.concatenate([[0], np.cumsum([len(p) for p, _, _ in items])]).astype(np.uint32)
    blob = np.frombuffer(b"".join(p for p, _, _ in items), np.uint8).copy()
    n = len(items)
    return hiprl.Batch(blob, off, np.array([r for _, r, _ in items], np.uint32), np.arange(n, dtype=np.uint32),
                       np.array([t for _, _, t in items], np.int64), np.ones(n, np.uint32))


def pfx(name):
    return hiprl.cache_key_prefix("adjp", [("k", str(name))])


def strings_of(b, rules):
    return [None if int(b.rule[i]) == NIL else
            string_of(b.prefix(i), rules[int(b.rule[i])][1], int(b.now[b.req_of[i]])) for i in range(b.n_desc)]


def recs(e):
    return sorted(r.tobytes() for r in e.snapshot_records()[1])


class DevBatch:
    """A decision batch on the device with its outputs."""

    def __init__(self, hb):
        self.hb = hb
        self.db = router.DeviceBatch.from_host(hb, dev())
        self.out = torch.zeros(max(1, hb.n_desc) * 20, dtype=torch.uint8, device=dev())
        self.thr = torch.zeros(max(1, hb.n_req), dtype=torch.int32, device=dev())

    def submit(self, e, pipelined=True):
        db = self.db
        f = e.submit_pipelined if pipelined else e.submit_device_async
        f(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), self.out.data_ptr(), self.thr.data_ptr())

    def result(self):
        return (self.out[:self.hb.n_desc * 20].cpu().numpy().view(hiprl.STATUS_DTYPE),
                self.thr[:self.hb.n_req].cpu().numpy().view(np.uint32))


class DevAdjust:
    """An adjust on the device: its batch, deltas and reply array."""

    def __init__(self, hb, deltas):
        self.hb, self.deltas = hb, np.ascontiguousarray(deltas, np.int32)
        self.db = router.DeviceBatch.from_host(hb, dev())
        self.delta = torch.from_numpy(self.deltas.copy() if hb.n_desc else np.zeros(1, np.int32)).to(dev())
        self.rep = torch.full((max(1, hb.n_desc) * 16,), 0xAB, dtype=torch.uint8, device=dev())

    def submit(self, e, keep=False, want=True):
        db = self.db
        e.adjust_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), self.delta.data_ptr(), keep,
                           self.rep.data_ptr() if want else 0)

    def replies(self):
        return self.rep[:self.hb.n_desc * 16].cpu().numpy().view(hiprl.PEEK_DTYPE)


def run_flights(e, flights, depth, keep=False):
    """flights: DevBatch / DevAdjust in order, at most `depth` in flight. -> the adjusts' reports."""
    reports, q = [], []

    def wait_oldest():
        f = q.pop(0)
        if isinstance(f, DevAdjust):
            out, rep = e.wait_adjust()
            assert out is None, "the device form keeps no host replies"
            reports.append(rep)
        else:
            e.wait()

    for f in flights:
        if isinstance(f, DevAdjust):
            f.submit(e, keep)
        else:
            f.submit(e)
        q.append(f)
        if len(q) == depth:
            wait_oldest()
    while q:
        wait_oldest()
    torch.cuda.synchronize()
    return reports


def run_serial(e, batches, adjusts, rules, local_cache, keep, model=True):
    """Engine S: batch, rl_wait, rl_adjust, ... one call at a time; each adjust also held against the
    dict model. -> (statuses, throttles, replies, reports) per call."""
    res, outs, reps = [], [], []
    for k, hb in enumerate(batches):
        b = DevBatch(hb)
        torch.cuda.synchronize()
        b.submit(e, pipelined=False)
        e.wait()
        torch.cuda.synchronize()
        res.append(b.result())
        for ab, deltas in adjusts[k]:
            before = e.peek(ab) if model else None
            out, rep = e.adjust(ab, np.array(deltas, np.int64), keep_cache=keep)
            if model:
                limits = [0 if int(r) == NIL else rules[int(r)][0] for r in ab.rule]
                want, want_rep = adjust_model(strings_of(ab, rules), before, deltas, limits, local_cache, keep)
                assert np.array_equal(out, before), "a reply is the state before the call"
                assert np.array_equal(e.peek(ab), want), "the state after the call is the model's"
                # (the model sees deadlines only through LOCAL_CACHED: with expired deadlines about,
                # its unfrozen is a lower bound)
                assert {**rep, "unfrozen": 0} == {**want_rep, "unfrozen": 0} and rep["unfrozen"] >= want_rep["unfrozen"]
            outs.append(out)
            reps.append(rep)
    return res, outs, reps


def stream_adjust(hb, k, rng, n_rules):
    """The adjust behind batch k: every third descriptor of it, 50 strings never charged, a few nil
    rules, and duplicates of one key; deltas in [-4, 4]."""
    items = [(hb.prefix(i), int(hb.rule[i]), int(hb.now[hb.req_of[i]])) for i in range(0, hb.n_desc, 3)]
    t = int(hb.now[0])
    items += [(pfx(f"never{k}_{j}"), int(rng.integers(0, n_rules)), t) for j in range(50)]
    items += [(pfx(f"nil{k}_{j}"), NIL, t) for j in range(3)]
    first = next(it for it in items if it[1] != NIL)
    items += [first] * 4
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    deltas = rng.integers(-4, 5, len(items))
    assert (deltas == 0).any() and deltas.min() == -4 and deltas.max() == 4
    return key_batch(items), deltas


# ---- 1. serial equivalence ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream_of(seed):
    """test_pipelined_differential_stream's batches, and the adjust behind each."""
    rng = np.random.default_rng(100 + seed)
    reqs = streams.make_stream(seed, 6000, 1_700_000_000 + 1000 * seed)
    sizes = streams.batch_sizes(reqs, rng, 900)
    hbs, i = [], 0
    for bs in sizes:
        hbs.append(hiprl.build_batch(reqs[i:i + bs]))
        i += bs
    return hbs, [[stream_adjust(hb, k, rng, len(RULES))] for k, hb in enumerate(hbs)]


@functools.lru_cache(maxsize=None)
def serial_reference(seed, local_cache, keep):
    """Engine S over the stream, once for both depths: the results, its stats and its records."""
    hbs, adjusts = stream_of(seed)
    S = engine(local_cache)
    res, outs, reps = run_serial(S, hbs, adjusts, RULES, local_cache, keep)
    got = res, outs, reps, S.stats(), recs(S)
    S.close()
    return got


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_serial_equivalence(seed, local_cache, keep, depth):
    hbs, adjusts = stream_of(seed)
    res, outs, reps, s_stats, s_recs = serial_reference(seed, local_cache, keep)
    P = engine(local_cache)
    flights = []
    for k, hb in enumerate(hbs):
        flights.append(DevBatch(hb))
        flights += [DevAdjust(ab, d) for ab, d in adjusts[k]]
    torch.cuda.synchronize()
    reports = run_flights(P, flights, depth, keep)
    pb = [f for f in flights if isinstance(f, DevBatch)]
    pa = [f for f in flights if isinstance(f, DevAdjust)]
    for k, b in enumerate(pb):
        streams.assert_same(*res[k], *b.result(), f"batch {k} seed={seed} local={local_cache} keep={keep} depth={depth}")
    assert sum(r["applied"] for r in reps) > 100 and sum(r["absent"] for r in reps) >= 50 * len(hbs)
    assert not local_cache or keep or sum(r["unfrozen"] for r in reps) > 0, "guard: the cache part ran"
    for k, a in enumerate(pa):
        got = a.replies()
        bad = np.nonzero(got != outs[k])[0]
        assert not bad.size, (k, int(bad[0]), got[bad[0]], outs[k][bad[0]])
        assert reports[k] == reps[k], (k, reports[k], reps[k])
    assert P.stats() == s_stats
    assert recs(P) == s_recs
    P.close()


# ---- 2. the poison chain -----------------------------------------------------------------------------
def poison_batches():
    """test_pipelined_fallbacks_first_and_middle's batch 0 (1500 descriptors of one key, no hot set
    yet: refused and rerun) and a batch 1."""
    rng = np.random.default_rng(7)
    now = 1_700_000_200
    out = []
    for k in range(2):
        batch = []
        for i in range(4000):
            x = rng.random()
            rule = int(rng.integers(0, 3))
            if k == 0 and i < 1500:
                key, rule = "big0", 2
            elif x < 0.3:
                h = int(rng.integers(0, 4))
                key, rule = f"hot{h}", h % 3
            else:
                key = f"k{int(rng.integers(0, 5000))}"
            batch.append(("pl", [[("k", key)]], [rule], int(rng.integers(0, 4)), now))
        out.append(batch)
    return out, now


@pytest.mark.parametrize("depth,n_adj", [(3, 1), (3, 2)])
@pytest.mark.parametrize("local_cache", [False, True])
def test_poison_chain(local_cache, depth, n_adj):
    """In flight behind the refused batch 0: one adjust and batch 1 (n_adj == 1), or two adjusts back
    to back (n_adj == 2, batch 1 behind them once batch 0 has completed). The keys exist only after
    batch 0's rerun: an adjust that ignored the poison would report them all absent."""
    (r0, r1), now = poison_batches()
    hb0, hb1 = hiprl.build_batch(r0), hiprl.build_batch(r1)
    first = {}
    for dom, descs, rules, _, _ in r0:
        first.setdefault(descs[0][0][1], rules[0])
    others = [k for k in first if k.startswith("k")][:200]
    assert len(others) == 200 and "big0" in first
    prefix = lambda key: hiprl.cache_key_prefix("pl", [("k", key)])
    items = [(prefix(k), first[k], now) for k in ["big0"] + others] + [(pfx("nil"), NIL, now)] * 2
    rng = np.random.default_rng(3)
    adjs = [(key_batch(items), rng.integers(-4, 5, len(items))) for _ in range(n_adj)]
    P, S = engine(local_cache), engine(local_cache)
    flights = [DevBatch(hb0)] + [DevAdjust(ab, d) for ab, d in adjs] + [DevBatch(hb1)]
    torch.cuda.synchronize()
    reports = run_flights(P, flights, depth)
    for rep in reports:
        assert rep["applied"] == len(items) - 2 and rep["absent"] == 0 and rep["nil"] == 2, rep
    res, outs, reps = run_serial(S, [hb0, hb1], [adjs, []], RULES, local_cache, False)
    assert P.stats()["batches"] == 2 and S.stats()["lsd_fallbacks"] == 1, "guard: batch 0 alone is refused"
    if n_adj == 1:
        # batch 0 and, poisoned behind the adjust, batch 1
        assert P.stats()["lsd_fallbacks"] >= 2, P.stats()
    else:
        # with three flights batch 1 is submitted only once batch 0 has completed, so it is never
        # poisoned: one fallback, and the two refused adjusts are not counted as such
        assert P.stats()["lsd_fallbacks"] == 1, P.stats()
    streams.assert_same(*res[0], *flights[0].result(), "refused batch 0")
    streams.assert_same(*res[1], *flights[-1].result(), "batch 1 behind the adjust")
    for k in range(n_adj):
        assert np.array_equal(flights[1 + k].replies(), outs[k]) and reports[k] == reps[k]
    assert recs(P) == recs(S)
    P.close()
    S.close()


def test_poison_chain_depth_2():
    """Depth 2: the adjust alone is in flight behind the refused batch."""
    (r0, r1), now = poison_batches()
    hb0, hb1 = hiprl.build_batch(r0), hiprl.build_batch(r1)
    items = [(hiprl.cache_key_prefix("pl", [("k", "big0")]), 2, now)]
    adjs = [(key_batch(items), np.array([-3]))]
    P, S = engine(), engine()
    flights = [DevBatch(hb0), DevAdjust(*adjs[0]), DevBatch(hb1)]
    torch.cuda.synchronize()
    reports = run_flights(P, flights, 2)
    assert reports[0]["applied"] == 1 and reports[0]["absent"] == 0
    assert P.stats()["lsd_fallbacks"] >= 1
    res, outs, reps = run_serial(S, [hb0, hb1], [adjs, []], RULES, False, False)
    streams.assert_same(*res[1], *flights[-1].result(), "batch 1")
    assert np.array_equal(flights[1].replies(), outs[0]) and reports == reps and recs(P) == recs(S)
    P.close()
    S.close()


# ---- 3. gates ------------------------------------------------------------------------------------------
def small_flights(t=1_700_000_007, n=100):
    reqs = [("adjp", [[("k", str(i % 7))]], [1 + i % 3], 1, t) for i in range(n)]
    hb = hiprl.build_batch(reqs)
    ab = key_batch([(pfx(i), 1 + i % 3, t) for i in range(7)])
    return hb, ab


def code_of(f, *a, **kw):
    with pytest.raises(hiprl.RedisError) as ei:
        f(*a, **kw)
    return ei.value.code


def test_gates():
    t = 1_700_000_007
    hb, ab = small_flights(t)
    e = engine(max_batch_desc=1 << 10, rule_stats=True, cache_stats=True, local_cache=True)
    b0 = DevBatch(hb)
    torch.cuda.synchronize()
    b0.submit(e, pipelined=False)
    e.wait()
    hdr, snap = e.snapshot_records()
    a = DevAdjust(ab, [-1] * 7)
    torch.cuda.synchronize()
    a.submit(e)
    # everything that needs the engine quiet, one by one; the flight stays
    quiet = [
        (e.peek, ab), (e.forget, ab), (e.adjust, ab, [0] * 7), (e.set, ab, np.zeros(7, hiprl.PEEK_DTYPE)),
        (e.snapshot_begin,), (e.restore_begin, hdr), (e.merge_chunk, hdr, snap, t), (e.resize, [9, 9, 9, 9]),
        (e.census, t), (e.rule_stats,), (e.cache_stats,), (e.set_stream, 0), (e.set_routed_plan, 0, 0, 0),
        (e.adjust_routed_plan, 0, 0),
        # the waits of the other kinds complete nothing
        (e.wait_into, 7, 7), (e.wait_view, 7, 7), (e.wait_raw_view, 7), (e.wait_raw_into, 7),
    ]
    for call in quiet:
        assert code_of(*call) == ESTATE, call[0].__name__
        # the flight is still there: rl_query answers (without a flight it is RL_ESTATE itself)
        assert isinstance(e.query(), bool), call[0].__name__
    # a fourth flight is refused, of either kind and form
    b1, b2 = DevBatch(hb), DevBatch(hb)
    a2 = DevAdjust(ab, [1] * 7)
    torch.cuda.synchronize()
    b1.submit(e)
    a2.submit(e)
    assert code_of(DevAdjust(ab, [1] * 7).submit, e) == ESTATE
    assert code_of(e.adjust_submit, ab, [1] * 7) == ESTATE
    assert code_of(b2.submit, e) == ESTATE
    # flights complete in order: adjust, batch, adjust; rl_wait_adjust refuses the batch
    out, rep = e.wait_adjust()
    assert out is None and rep["applied"] == 7
    assert code_of(e.wait_adjust) == ESTATE
    e.wait()
    e.wait()  # rl_wait completes an adjust flight and discards its report
    assert code_of(e.wait) == ESTATE and code_of(e.wait_adjust) == ESTATE
    torch.cuda.synchronize()
    assert (a.replies()["flags"] & F).all() and (a2.replies()["flags"] & F).all()
    # a restore or a routed plan open: both submit forms are refused, nothing is in flight
    hdr, snap = e.snapshot_records()
    for opener, closer in ((lambda: e.set_routed_plan(0, 0, 0), lambda: e.set_routed_commit(False)),
                          (lambda: e.adjust_routed_plan(0, 0), lambda: e.adjust_routed_commit(False)),
                          (lambda: e.restore_begin(hdr), lambda: (e.restore_put(snap), e.restore_end()))):
        opener()
        assert code_of(a.submit, e) == ESTATE and code_of(e.adjust_submit, ab, [1] * 7) == ESTATE
        closer()
        assert code_of(e.wait) == ESTATE
    # argument refusals: immediate, no flight
    s = hiprl._batch_struct(ab)
    d = np.ones(7, np.int32)
    big = key_batch([(pfx(i), 1, t) for i in range((1 << 10) + 1)])
    sb = hiprl._batch_struct(big)
    for fn, tail in ((e.lib.rl_adjust_pipelined, (None,)), (e.lib.rl_adjust_submit, (1,))):
        assert fn(e.h, C.byref(s), None, 0, *tail) == EINVAL  # null delta
        assert fn(e.h, C.byref(s), d.ctypes.data, 2, *tail) == EINVAL  # an unknown flag bit
        assert fn(e.h, C.byref(sb), d.ctypes.data, 0, *tail) == ECAPACITY
        s.reserved = 1
        assert fn(e.h, C.byref(s), d.ctypes.data, 0, *tail) == EINVAL
        s.reserved = 0
    assert code_of(e.wait) == ESTATE
    e.close()


def test_gate_lsd_only():
    hb, ab = small_flights()
    e = engine(max_batch_desc=1 << 10, pipeline="lsd")
    b0, a = DevBatch(hb), DevAdjust(ab, [-1] * 7)
    torch.cuda.synchronize()
    b0.submit(e, pipelined=False)
    assert code_of(a.submit, e) == ESTATE and code_of(e.adjust_submit, ab, [-1] * 7) == ESTATE
    e.wait()
    a.submit(e)  # alone it is legal
    assert e.wait_adjust()[1]["applied"] == 7
    e.adjust_submit(ab, [-1] * 7)
    out, rep = e.wait_adjust()
    assert rep["applied"] == 7 and np.array_equal(out["count"] + 1, a.replies()["count"])
    e.close()


# ---- 4. a malformed device descriptor --------------------------------------------------------------
@pytest.mark.parametrize("case", ["rule", "time", "req_of"])
def test_malformed_device_descriptor(case):
    t = 1_700_000_007
    hb, _ = small_flights(t)
    e = engine(max_batch_desc=1 << 10)
    b0 = DevBatch(hb)
    torch.cuda.synchronize()
    b0.submit(e, pipelined=False)
    e.wait()
    items = [(pfx(i % 7), 1 + i % 3, t) for i in range(70)]
    ab = key_batch(items)
    bad = 33
    if case == "rule":
        ab.rule[bad] = len(RULES)
    elif case == "time":
        ab.now[bad] = 0xFFFD0001
    else:
        ab.req_of[bad] = bad - 2  # decreases (and is below n_req)
    a = DevAdjust(ab, [-1] * 70)
    torch.cuda.synchronize()
    r0 = recs(e)
    a.submit(e)
    assert code_of(e.wait_adjust) == EINVAL
    assert code_of(e.wait) == ESTATE, "the failed flight is gone"
    torch.cuda.synchronize()
    rep = a.replies()
    assert int(rep[bad]["flags"]) == BAD
    good = [i for i in range(70) if i != bad]
    assert (rep["flags"][good] & F).all() and (rep["count"][good] > 0).all(), "the state before the call"
    assert recs(e) == r0, "nothing written"
    # the next flight works
    ok = DevAdjust(key_batch(items), [-1] * 70)
    torch.cuda.synchronize()
    ok.submit(e)
    _, report = e.wait_adjust()
    assert report["applied"] == 70 and recs(e) != r0
    e.close()


# ---- 5. the host form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("acquired", [False, True])
def test_host_form(acquired):
    t = 1_700_000_007
    hb, _ = small_flights(t)
    P, S = engine(True, max_batch_desc=1 << 10), engine(True, max_batch_desc=1 << 10)
    P.submit(hb)
    for _ in range(2):  # (P's adjust goes behind its second batch)
        S.submit(hb)
    items = [(pfx(i % 9), 1 + i % 3, t) for i in range(40)] + [(pfx("nil"), NIL, t)]
    ab = key_batch(items)
    deltas = np.random.default_rng(5).integers(-4, 5, ab.n_desc)
    want_out, want_rep = S.adjust(ab, deltas)
    b1 = DevBatch(hb)
    torch.cuda.synchronize()
    b1.submit(P)
    if acquired:
        slot = P.host_acquire()
        n = ab.n_desc
        slot["blob"][:ab.blob.shape[0]] = ab.blob
        slot["off"][:n + 1] = ab.off
        slot["rule"][:n] = ab.rule
        slot["req_of"][:n] = ab.req_of
        slot["now"][:n] = ab.now
        s = hiprl.RlBatch()
        s.n_desc, s.n_req, s.blob_bytes, s.reserved = n, n, int(ab.off[-1]), 0
        hiprl._set_ptrs(s, [slot[k].ctypes.data for k in ("blob", "off", "rule", "req_of", "now", "hits")])
        d = np.ascontiguousarray(deltas, np.int32)
        assert P.lib.rl_adjust_submit(P.h, C.byref(s), d.ctypes.data, 0, 1) == 0
    else:
        P.adjust_submit(ab, deltas)
    P.wait()
    out, rep = P.wait_adjust()
    assert np.array_equal(out, want_out) and rep == want_rep
    # want_out == False keeps none; n_desc == 0 is an empty flight with a zero report
    P.adjust_submit(ab, np.zeros(ab.n_desc, np.int64), want_out=False)
    out, rep = P.wait_adjust()
    assert out is None and rep["applied"] == want_rep["applied"]
    P.adjust_submit(key_batch([]), np.zeros(0, np.int64))
    out, rep = P.wait_adjust()
    assert out is None and rep == dict.fromkeys(hiprl.ADJUST_REPORT_FIELDS, 0)
    # host refusals add no flight: a batch's contents (rl_adjust's list)
    for field, i, v in (("rule", 3, len(RULES)), ("now", 3, 0xFFFD0001), ("req_of", 3, 1), ("off", 3, 1 << 20)):
        bad = key_batch(items)
        getattr(bad, field)[i] = v
        assert code_of(P.adjust_submit, bad, deltas) == EINVAL, field
        assert code_of(P.wait) == ESTATE
    # a wait of another kind on the flight is refused and writes nothing to its buffer (a host-form
    # flight cannot be made to fail on the device: its contents were checked before it was staged)
    P.adjust_submit(ab, deltas)
    buf = np.full(ab.n_desc * 16, 0xAB, np.uint8)
    assert P.lib.rl_wait_into(P.h, buf.ctypes.data, None) == ESTATE and (buf == 0xAB).all()
    P.wait()
    S.adjust(ab, deltas)
    assert recs(P) == recs(S)
    P.close()
    S.close()


# ---- 6. flags and timing --------------------------------------------------------------------------------
def test_stat_flags_and_timing():
    t = 1_700_000_007
    hb, ab = small_flights(t)
    res = []
    for timing in (False, True):
        e = engine(True, max_batch_desc=1 << 10, rule_stats=True, cache_stats=True)
        e.set_timing(timing)
        fl = [DevBatch(hb), DevAdjust(ab, [-1, 0, 1, 2, -2, 3, -3]), DevBatch(hb), DevAdjust(ab, [1] * 7), DevBatch(hb)]
        torch.cuda.synchronize()
        reports = run_flights(e, fl, 3)
        s = e.stats()
        assert (s["batches"], s["descriptors"]) == (3, 3 * hb.n_desc)
        rs, cs = e.rule_stats(), e.cache_stats()
        res.append(([f.result() if isinstance(f, DevBatch) else f.replies() for f in fl], reports, rs.tobytes(), cs,
                    recs(e)))
        if timing:
            kt = e.kernel_times()
            assert kt["k_adjust_index"][1] == 2 and kt["k_adjust_apply"][1] == 2, kt
        # The adjusts move counters, so the batches behind them decide otherwise than without them:
        # the rows are those of the same sequence run one call at a time with the synchronous
        # rl_adjust, which is pinned to leave every stat alone (test_gpu_adjust.py) ...
        ref = engine(True, max_batch_desc=1 << 10, rule_stats=True, cache_stats=True)
        for f in fl:
            if isinstance(f, DevBatch):
                ref.submit(hb)
            else:
                ref.adjust(ab, f.deltas)
        assert np.array_equal(rs, ref.rule_stats()) and int(rs["total_hits"].sum()) > 0 and int(rs["over_limit"].sum()) > 0
        assert cs == ref.cache_stats() and cs["lookups"] > 0 and cs["hits"] > 0, (cs, ref.cache_stats())
        ref.close()
        e.close()
        # ... and with adjusts that move nothing (every delta 0, found and absent keys), the rows of an
        # engine that ran the three batches and no adjust at all
        e, ref = (engine(True, max_batch_desc=1 << 10, rule_stats=True, cache_stats=True) for _ in range(2))
        e.set_timing(timing)
        zero = key_batch([(pfx(i), 1 + i % 3, t) for i in range(12)])
        fl0 = [DevBatch(hb), DevAdjust(zero, [0] * 12), DevBatch(hb), DevAdjust(zero, [0] * 12), DevBatch(hb)]
        torch.cuda.synchronize()
        rep0 = run_flights(e, fl0, 3)
        assert [r["applied"] for r in rep0] == [7, 7] and [r["absent"] for r in rep0] == [5, 5]
        for _ in range(3):
            ref.submit(hb)
        assert np.array_equal(e.rule_stats(), ref.rule_stats()) and e.cache_stats() == ref.cache_stats()
        ref.close()
        e.close()
    (r0, rep0, rs0, cs0, rec0), (r1, rep1, rs1, cs1, rec1) = res
    for x, y in zip(r0, r1):
        if isinstance(x, tuple):
            streams.assert_same(*x, *y, "timing on / off")
        else:
            assert np.array_equal(x, y)
    assert rep0 == rep1 and rec0 == rec1 and rs0 == rs1 and cs0 == cs1
