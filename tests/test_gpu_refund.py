"""Refund (rl_hip.h "Refund") on the GPU, through the C ABI: rl_refund_pipelined, rl_refund_behind
and rl_wait_refund. The reference is RefundOracle (refund_model.py): the oracle's DoLimit with the
model's refund applied behind every batch; test_refund_cpu.py pins it to the C++ oracle. Every
comparison is of exact integers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hiprl
import router
import streams
from refund_model import RefundOracle

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC, ECAPACITY, ESTATE = -1, -3, -4, -5
NIL = hiprl.NIL_RULE
MAXD = 1 << 12
T0 = 1_700_000_000
S, M, H, D = hiprl.SECOND, hiprl.MINUTE, hiprl.HOUR, hiprl.DAY
# rule 5 is shadowed: over its limit it rejects nothing
RULES = [(4, S), (12, M), (30, H), (60, D), (1 << 30, H), (2, M, True)]


def dev():
    return torch.device("cuda", 0)


def engine(local_cache=False, split=False, rules=RULES, **kw):
    kw.setdefault("max_batch_desc", MAXD)
    kw.setdefault("pipeline", "v4")
    e = hiprl.Engine(near_limit_ratio=0.8, local_cache=local_cache, per_second_split=split, **kw)
    e.load_rules(rules)
    return e


def recs(e):
    return sorted(r.tobytes() for r in e.snapshot_records()[1])


def code_of(f, *a, **kw):
    with pytest.raises(hiprl.RedisError) as ei:
        f(*a, **kw)
    return ei.value.code


class DevBatch:
    """A decision batch on the device with its outputs and its refund's amounts."""

    def __init__(self, hb):
        self.hb = hb
        self.db = router.DeviceBatch.from_host(hb, dev())
        self.out = torch.zeros(max(1, hb.n_desc) * 20, dtype=torch.uint8, device=dev())
        self.thr = torch.zeros(max(1, hb.n_req), dtype=torch.int32, device=dev())
        self.amt = torch.full((max(1, hb.n_desc),), -1, dtype=torch.int32, device=dev())

    def args(self):
        db = self.db
        return db.n_desc, db.n_req, db.blob_bytes(), db.ptrs()

    def submit(self, e, pipelined=True):
        (e.submit_pipelined if pipelined else e.submit_device_async)(*self.args(), self.out.data_ptr(), self.thr.data_ptr())

    def refund(self, e, keep=False, behind=False):
        if behind:
            e.refund_behind(keep)
        else:
            e.refund_pipelined(*self.args(), self.out.data_ptr(), keep, self.amt.data_ptr())

    def result(self):
        return (self.out[:self.hb.n_desc * 20].cpu().numpy().view(hiprl.STATUS_DTYPE),
                self.thr[:self.hb.n_req].cpu().numpy().view(np.uint32))

    def amounts(self):
        return self.amt[:self.hb.n_desc].cpu().numpy().view(np.uint32).tolist()


def model_peeks(m, hb):
    """What rl_peek answers for every descriptor of hb, from the model's state."""
    rows = []
    for i in range(hb.n_desc):
        key, store = m._key(hb, i)
        rows.append((0, 0, 0, hiprl.PEEK_NIL) if key is None else m.peek(key, store, int(hb.now[hb.req_of[i]])))
    return np.array(rows, hiprl.PEEK_DTYPE).reshape(len(rows))


def assert_peeks(e, m, hb, ctx):
    got, want = e.peek(hb), model_peeks(m, hb)
    bad = np.nonzero(got != want)[0]
    assert not bad.size, (ctx, int(bad[0]), got[bad[0]], want[bad[0]])


def run_flights(e, batches, depth, keep=False, behind=False, quiet=None, quiet_every=1):
    """B0 R0 B1 R1 ... with at most `depth` flights in flight; quiet(k) runs with nothing in flight
    behind refund k, for every quiet_every-th k: the flights are completed there, and between two
    such boundaries the pipeline stays `depth` deep. -> the reports."""
    reports, q = [], []

    def wait_oldest():
        if q.pop(0) == "r":
            reports.append(e.wait_refund())
        else:
            e.wait()

    for k, b in enumerate(batches):
        for kind in "br":
            if kind == "b":
                b.submit(e)
            else:
                b.refund(e, keep, behind)
            q.append(kind)
            if len(q) == depth:
                wait_oldest()
        if quiet and k % quiet_every == quiet_every - 1:
            while q:
                wait_oldest()
            torch.cuda.synchronize()
            quiet(k)
    while q:
        wait_oldest()
    torch.cuda.synchronize()
    return reports


# ---- 1. stream parity --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream():
    """10 batches of 300-3000 descriptors, 1-4 descriptors per request, on a few hundred keys under
    small limits; the time moves a second per batch, so the per-second windows turn over."""
    rng = np.random.default_rng(11)
    hbs = []
    for k in range(10):
        n_desc, reqs, n = int(rng.integers(300, 3001)), [], 0
        while n < n_desc:
            nd = int(rng.integers(1, 5))
            descs, rules = [], []
            for _ in range(nd):
                rule = int(rng.choice([0, 1, 2, 3, 4, 5, NIL], p=[.2, .2, .2, .15, .15, .05, .05]))
                span = 1500 if rule in (0, 4) else 700
                descs.append([("k", str(int(span * rng.random() ** 2)))])
                rules.append(rule)
            reqs.append(("rf", descs, rules, int(rng.integers(0, 4)), T0 + k + int(rng.integers(0, 2))))
            n += nd
        reqs.sort(key=lambda r: r[4])
        hbs.append(hiprl.build_batch(reqs))
    return hbs


@functools.lru_cache(maxsize=None)
def stream_reference(local_cache, split):
    """The model over the stream, once for both depths: per batch the statuses, throttles, amounts,
    report and the peeks of the batch's keys behind its refund."""
    m = RefundOracle(RULES, local_cache=local_cache, per_second_split=split)
    ref = []
    for hb in stream():
        st, thr = m.submit(hb)
        amounts, rep = m.refund(hb, st)
        ref.append((st, thr, amounts, rep, model_peeks(m, hb)))
    rejected = sum(r[3]["rejected_req"] for r in ref) / sum(hb.n_req for hb in stream())
    assert 0.10 <= rejected <= 0.40, rejected
    assert sum(r[3]["refunded"] for r in ref) > 1000
    assert not local_cache or sum(r[3]["unfrozen"] for r in ref) > 0, "guard: the cache part ran"
    return ref


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("local_cache", [False, True])
def test_stream_parity(local_cache, split, depth):
    """Depth 2 is quiet at every boundary: there every key of the batch is peeked. Depth 3 keeps the
    next batch in flight over a boundary, so rl_peek (which needs nothing in flight) cannot run
    there without emptying the pipeline: the flights are completed and the keys peeked behind every
    third batch, three flights deep in between, and the boundaries between are held by the statuses
    of every batch (they show the counters the refunds left), the amounts and the reports."""
    hbs, ref = stream(), stream_reference(local_cache, split)
    e = engine(local_cache, split)
    batches = [DevBatch(hb) for hb in hbs]
    torch.cuda.synchronize()

    def boundary(k):
        got, want = e.peek(hbs[k]), ref[k][4]
        bad = np.nonzero(got != want)[0]
        assert not bad.size, (k, int(bad[0]), got[bad[0]], want[bad[0]])

    reports = run_flights(e, batches, depth, quiet=boundary, quiet_every=1 if depth == 2 else 3)
    for k, b in enumerate(batches):
        ctx = f"batch {k} local={local_cache} split={split} depth={depth}"
        streams.assert_same(ref[k][0], ref[k][1], *b.result(), ctx)
        assert b.amounts() == ref[k][2], ctx
        assert reports[k] == ref[k][3], (ctx, reports[k], ref[k][3])
    boundary(len(hbs) - 1)
    assert e.stats()["batches"] == len(hbs), "a refund is no batch"
    e.close()


# ---- 2. shapes where the kernels can go wrong -------------------------------------------------------------
def run_case(reqs_per_batch, local_cache=False, behind=False, rules=RULES, keep=False):
    """Every batch with a refund behind it, against the model: statuses, amounts, report, peeks."""
    m = RefundOracle(rules, local_cache=local_cache)
    e = engine(local_cache, rules=rules)
    reports = []
    for reqs in reqs_per_batch:
        hb = hiprl.build_batch(reqs)
        b = DevBatch(hb)
        torch.cuda.synchronize()
        got = run_flights(e, [b], 2, keep=keep, behind=behind)[0]
        st, thr = m.submit(hb)
        amounts, rep = m.refund(hb, st, keep)
        streams.assert_same(st, thr, *b.result(), "statuses")
        assert behind or b.amounts() == amounts
        assert got == rep, (got, rep)
        assert_peeks(e, m, hb, "peeks behind the refund")
        reports.append(rep)
    e.close()
    return reports


def req(keys, rules, hits, t=T0 + 7):
    return ("rf", [[("k", str(k))] for k in keys], rules, hits, t)


@pytest.mark.parametrize("behind", [False, True])
def test_mark_reaches_back_over_blocks(behind):
    """A request of 700 descriptors whose only over-limit descriptor is its last."""
    first = req(["last"], [0], 4)
    big = req([f"a{i}" for i in range(699)] + ["last"], [4] * 699 + [0], 1)
    rep = run_case([[first, big, req(["z"], [4], 1)]], behind=behind)[0]
    assert rep["rejected_req"] == 1 and rep["refunded"] == 700 and rep["skipped"] == 2


def test_request_boundaries_at_wave_and_block_edges():
    """Requests end at descriptors 63 and 255: a rejected request must not leak over the edge."""
    pre = [req(["x"], [0], 4)]  # descriptor 0
    a = req([f"a{i}" for i in range(62)] + ["x"], [4] * 62 + [0], 1)  # 1..63, rejected by its last
    b = req([f"b{i}" for i in range(192)], [4] * 192, 1)  # 64..255, not rejected
    c = req(["x"] + [f"c{i}" for i in range(9)], [0] + [4] * 9, 1)  # 256.., rejected by its first
    d = req([f"d{i}" for i in range(5)], [4] * 5, 2)
    rep = run_case([pre + [a, b, c, d]])[0]
    assert rep["rejected_req"] == 2 and rep["refunded"] == 63 + 10 and rep["skipped"] == 1 + 192 + 5


@pytest.mark.parametrize("local_cache", [False, True])
def test_one_key_inside_waves_and_over_blocks(local_cache):
    """200 rejected requests of one key side by side (whole waves of one pair: the combined path),
    and the same spread over five blocks among keys of their own (one lane per pair and wave: the
    uncombined path). The 64-bit sums agree with the model either way."""
    side = [req(["hot"], [1], 7) for _ in range(202)]
    spread = []
    for i in range(230):
        spread.append(req(["hot"], [1], 7))
        spread.append(req([f"s{i}_{j}" for j in range(3)] + [f"t{i}"], [4] * 3 + [2], 1))
        spread.append(req([f"u{i}"], [3], 2))
    assert sum(len(r[1]) for r in spread) > 5 * 256
    r0, r1 = run_case([side, spread], local_cache)
    # 12 per minute at 7 a request: one passes; with the local cache the frozen key is not counted
    assert r0["rejected_req"] == 201 and r0["refunded"] == (201 if not local_cache else 1)
    assert r1["rejected_req"] >= 199


@pytest.mark.parametrize("behind", [False, True])
def test_keep_cache_leaves_the_key_frozen(behind):
    """RL_REFUND_KEEP_CACHE: the counters come back, the deadline stays, so the next request on the
    key is a local-cache hit; without the flag the key counts again."""
    batches = [[req(["f"], [1], 7), req(["f", "o"], [1, 4], 7)], [req(["f", "o"], [1, 4], 1)]]
    kept = run_case(batches, True, behind, keep=True)
    assert kept[0]["refunded"] == 2 and kept[0]["unfrozen"] == 0
    assert kept[1]["rejected_req"] == 1 and kept[1]["refunded"] == 1, "the hit itself is owed nothing"
    freed = run_case(batches, True, behind)
    assert freed[0]["unfrozen"] == 1 and freed[1]["rejected_req"] == 0


def test_hits_addend_edges():
    """hits_addend in {0, 1, 7, 2^31 - 1, 2^31, 2^32 - 1}: the amount is the full uint32."""
    reqs = []
    for h in (0, 1, 7):
        reqs.append(req([f"e{h}"], [0], 4))  # at its limit: the next is rejected
        reqs.append(req([f"e{h}", f"g{h}"], [0, 4], h))
    for h in (2**31 - 1, 2**31, 2**32 - 1):
        reqs.append(req([f"e{h}", f"g{h}"], [0, 4], h))
    # two of one key in one wave: a sum no int32 delta holds (the counter itself stays below 2^32)
    reqs += [req(["w"], [0], 2**31 - 1), req(["w"], [0], 2**31 - 1)]
    rep = run_case([reqs])[0]
    assert rep["rejected_req"] == 8 and rep["refunded"] == 14 and rep["floored"] == 0


@pytest.mark.parametrize("n_desc", [1, 63, 64, 65, 257])
def test_batch_sizes(n_desc):
    pre = [req([k], [0], 4) for k in range(3)]
    rep = run_case([pre, [req([i % 5], [0], 1) for i in range(n_desc)]])[1]
    assert rep["descriptors"] == n_desc and rep["rejected_req"] > 0


# ---- 3. nothing rejected -----------------------------------------------------------------------------
def test_nothing_rejected():
    hb = hiprl.build_batch([req([f"n{i}", f"m{i % 9}"], [4, 4], 1 + i % 3) for i in range(500)])
    e = engine(True)
    b = DevBatch(hb)
    torch.cuda.synchronize()
    b.submit(e, pipelined=False)
    e.wait()
    before = recs(e)
    b.refund(e)
    rep = e.wait_refund()
    torch.cuda.synchronize()
    assert rep == dict(descriptors=1000, rejected_req=0, skipped=1000, absent=0, refunded=0, floored=0, unfrozen=0)
    assert recs(e) == before and b.amounts() == [0] * 1000
    # an empty batch is an empty flight with a zero report
    z = DevBatch(hiprl.build_batch([]))
    z.refund(e)
    assert e.wait_refund() == dict.fromkeys(hiprl.REFUND_REPORT_FIELDS, 0)
    e.close()


# ---- 4. behind a refused batch ---------------------------------------------------------------------------
def poison_batches():
    """test_gpu_adjust_pipelined.py's: batch 0 holds 1500 descriptors of one key with no hot set yet,
    so the bucketed pipeline refuses it and the wait reruns it; most of those requests are rejected."""
    rng = np.random.default_rng(7)
    out = []
    for k in range(2):
        batch = []
        for i in range(4000):
            rule = int(rng.integers(0, 3))
            if k == 0 and i < 1500:
                key, rule = "big0", 2
            elif rng.random() < 0.3:
                h = int(rng.integers(0, 4))
                key, rule = f"hot{h}", h % 3
            else:
                key = f"k{int(rng.integers(0, 5000))}"
            batch.append(("pl", [[("k", key)]], [rule], int(rng.integers(0, 4)), T0 + 200))
        out.append(hiprl.build_batch(batch))
    return out


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("local_cache", [False, True])
def test_refund_behind_a_refused_batch_equals_the_serial_run(local_cache, depth):
    hbs = poison_batches()
    P, Q = engine(local_cache, rules=streams.RULES), engine(local_cache, rules=streams.RULES)
    pb, qb = [DevBatch(hb) for hb in hbs], [DevBatch(hb) for hb in hbs]
    torch.cuda.synchronize()
    p_rep = run_flights(P, pb, depth)
    q_rep = []
    for b in qb:  # one call at a time
        b.submit(Q, pipelined=False)
        Q.wait()
        b.refund(Q)
        q_rep.append(Q.wait_refund())
    torch.cuda.synchronize()
    assert Q.stats()["lsd_fallbacks"] == 1 and P.stats()["lsd_fallbacks"] >= 1, "guard: batch 0 is refused"
    assert q_rep[0]["rejected_req"] > 1000 and q_rep[0]["refunded"] > (0 if local_cache else 1000)
    for k in range(2):
        streams.assert_same(*qb[k].result(), *pb[k].result(), f"batch {k}")
        assert pb[k].amounts() == qb[k].amounts() and p_rep[k] == q_rep[k], (k, p_rep[k], q_rep[k])
    assert recs(P) == recs(Q)
    # ... and the serial run is the model's
    m = RefundOracle(streams.RULES, local_cache=local_cache)
    for k, hb in enumerate(hbs):
        st, thr = m.submit(hb)
        amounts, rep = m.refund(hb, st)
        streams.assert_same(st, thr, *qb[k].result(), f"model, batch {k}")
        assert amounts == qb[k].amounts() and rep == q_rep[k]
    P.close()
    Q.close()


# ---- 4b. behind a batch that fails -------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pipelined", "behind", "host"])
def test_refund_behind_a_failed_batch_writes_nothing(form):
    """A batch the device refuses with RL_ENOSPC writes no statuses: its status array still holds an
    earlier batch's, all OVER_LIMIT here. A refund queued behind it must not act on those."""
    batch = lambda ids, h: hiprl.build_batch([req([i], [0], h) for i in ids])
    full, refused = batch(range(500), 5), batch(range(400), 1)  # 500 live + 400 descriptors > 768
    e = engine(log2_slots=(10, 10, 10, 10), max_load_permille=750)
    if form == "host":
        st, _ = e.submit(full)  # host slot 0
        for _ in range(2):  # slots 1 and 2: the next batch meets slot 0's statuses again
            e.submit(batch([0], 1))
    else:
        b = DevBatch(full)
        torch.cuda.synchronize()
        b.submit(e, pipelined=False)
        e.wait()
        st = b.result()[0]
    assert ((st["code_flags"] & 0xFF) == 2).all(), "guard: the stale statuses are all rejected"
    before, peeks = recs(e), e.peek(refused)
    assert (peeks["count"] >= 5).all()
    if form == "host":
        e.submit_host_async(refused)
        e.refund_behind()
    else:
        r = DevBatch(refused)
        r.out = b.out  # the caller's status array, used again
        torch.cuda.synchronize()
        r.submit(e)
        r.refund(e, behind=form == "behind")
    assert code_of(e.wait) == ENOSPC
    assert code_of(e.wait_refund) == ESTATE, "the refund reports its batch's failure"
    assert code_of(e.wait) == ESTATE, "both flights are gone"
    torch.cuda.synchronize()
    assert recs(e) == before and np.array_equal(e.peek(refused), peeks), "nothing written"
    # the engine goes on: a batch that fits, refunded
    ok = DevBatch(batch(range(100), 1))
    torch.cuda.synchronize()
    ok.submit(e)
    ok.refund(e, behind=form != "pipelined")
    e.wait()
    rep = e.wait_refund()
    assert rep["rejected_req"] == 100 and rep["refunded"] == 100
    assert (e.peek(batch(range(100), 1))["count"] == peeks["count"][:100]).all()
    e.close()


# ---- 5. rl_refund_behind of a host batch --------------------------------------------------------------
def test_refund_behind_host_batches():
    """Host batches with a refund behind each, three flights deep, so that a staging slot comes up
    for its next batch while the refund of its previous one may still be in flight."""
    hbs = stream()[:7]
    ref = stream_reference(False, False)
    e = engine()
    q = []

    def wait_oldest(got):
        kind, k = q.pop(0)
        if kind == "r":
            got[k] = (got[k], e.wait_refund())
        else:
            got[k] = e.wait_into(hbs[k].n_desc, hbs[k].n_req)

    got = {}
    for k, hb in enumerate(hbs):
        e.submit_host_async(hb)
        q.append(("b", k))
        e.refund_behind()
        q.append(("r", k))
        while len(q) > 1:
            wait_oldest(got)
    while q:
        wait_oldest(got)
    for k in range(len(hbs)):
        (st, thr), rep = got[k]
        streams.assert_same(ref[k][0], ref[k][1], st, thr, f"host batch {k}")
        assert rep == ref[k][3]
    e.close()


def test_host_slot_is_held_for_its_refund():
    """B0 R0 B1 B2 ...: B2 takes B0's staging slot while R0, which reads that slot's device arrays
    and statuses, has not been waited for. Equal to the same calls made one at a time."""
    hbs = stream()[:6]
    order = [("b", 0), ("r", 0), ("b", 1), ("b", 2), ("r", 2), ("b", 3), ("b", 4), ("r", 4), ("b", 5)]
    res = []
    for depth in (2, 3):
        e, q, got = engine(), [], {}
        for kind, k in order:
            while len(q) >= depth:
                kk, k0 = q.pop(0)
                got[kk, k0] = e.wait_refund() if kk == "r" else e.wait_into(hbs[k0].n_desc, hbs[k0].n_req)
            if kind == "b":
                e.submit_host_async(hbs[k])
            else:
                e.refund_behind()
            q.append((kind, k))
        while q:
            kk, k0 = q.pop(0)
            got[kk, k0] = e.wait_refund() if kk == "r" else e.wait_into(hbs[k0].n_desc, hbs[k0].n_req)
        res.append((got, recs(e)))
        e.close()
    (g1, r1), (g3, r3) = res
    for key in g1:
        if key[0] == "r":
            assert g1[key] == g3[key] and g1[key]["refunded"] > 0, key
        else:
            streams.assert_same(*g1[key], *g3[key], str(key))
    assert r1 == r3


# ---- 6. gates ------------------------------------------------------------------------------------------
def small():
    return hiprl.build_batch([req([i % 7], [0], 1) for i in range(100)])


def test_gates():
    hb = small()
    e = engine(True, max_batch_desc=1 << 10)
    b = DevBatch(hb)
    torch.cuda.synchronize()
    assert code_of(e.refund_behind) == ESTATE, "nothing in flight"
    assert code_of(e.wait_refund) == ESTATE
    b.submit(e)
    assert code_of(e.wait_refund) == ESTATE, "the oldest flight is a batch"
    e.refund_behind()
    assert code_of(e.refund_behind) == ESTATE, "behind a refund"
    e.wait()
    # on a refund, the waits of the other kinds complete nothing
    for call in ((e.wait_adjust,), (e.wait_into, 7, 7), (e.wait_view, 7, 7), (e.wait_raw_view, 7), (e.wait_raw_into, 7),
                 (e.peek, hb), (e.snapshot_begin,)):
        assert code_of(*call) == ESTATE, call[0].__name__
        assert isinstance(e.query(), bool)
    rep = e.wait_refund()
    assert rep["descriptors"] == 100 and rep["rejected_req"] > 0
    # behind an adjust, and behind a compact batch
    ab = hiprl.build_batch([req([i], [0], 1) for i in range(7)])
    e.adjust_submit(ab, [0] * 7)
    assert code_of(e.refund_behind) == ESTATE, "behind an adjust"
    assert code_of(e.wait_refund) == ESTATE, "the oldest flight is an adjust"
    e.wait()
    e.submit_c(hiprl.compact_batch(hb))
    assert code_of(e.refund_behind) == ESTATE, "behind a compact batch"
    e.wait_raw_into(hb.n_desc)
    # a fourth flight is refused; rl_wait completes a refund and drops its report
    b.submit(e)
    b.refund(e)
    b2 = DevBatch(hb)
    torch.cuda.synchronize()
    b2.submit(e)
    assert code_of(b2.refund, e) == ESTATE and code_of(e.refund_behind) == ESTATE
    for _ in range(3):
        e.wait()
    assert code_of(e.wait) == ESTATE
    # a restore or a routed plan open
    hdr, snap = e.snapshot_records()
    for opener, closer in ((lambda: e.set_routed_plan(0, 0, 0), lambda: e.set_routed_commit(False)),
                          (lambda: e.adjust_routed_plan(0, 0), lambda: e.adjust_routed_commit(False)),
                          (lambda: e.restore_begin(hdr), lambda: (e.restore_put(snap), e.restore_end()))):
        opener()
        assert code_of(b.refund, e) == ESTATE
        closer()
        assert code_of(e.wait) == ESTATE
    # argument refusals: immediate, no flight
    s = hiprl.RlBatch()
    s.n_desc, s.n_req, s.blob_bytes, s.reserved = b.args()[0], b.args()[1], b.args()[2], 0
    hiprl._set_ptrs(s, b.args()[3])
    fn = e.lib.rl_refund_pipelined
    assert fn(e.h, C.byref(s), None, 0, None) == EINVAL  # null statuses
    assert fn(e.h, C.byref(s), b.out.data_ptr(), 2, None) == EINVAL  # an unknown flag bit
    s.reserved = 1
    assert fn(e.h, C.byref(s), b.out.data_ptr(), 0, None) == EINVAL
    s.reserved = 0
    s.n_desc = (1 << 10) + 1
    assert fn(e.h, C.byref(s), b.out.data_ptr(), 0, None) == ECAPACITY
    s.n_desc = 100
    ptrs = list(b.args()[3])
    ptrs[5] = 0
    hiprl._set_ptrs(s, ptrs)
    assert fn(e.h, C.byref(s), b.out.data_ptr(), 0, None) == EINVAL  # null hits_addend
    assert code_of(e.wait) == ESTATE
    e.close()


def test_gate_lsd_only():
    hb = small()
    e = engine(max_batch_desc=1 << 10, pipeline="lsd")
    b = DevBatch(hb)
    torch.cuda.synchronize()
    b.submit(e, pipelined=False)
    assert code_of(b.refund, e) == ESTATE and code_of(e.refund_behind) == ESTATE
    e.wait()
    b.refund(e)  # alone it is legal
    assert e.wait_refund()["rejected_req"] > 0
    e.close()


@pytest.mark.parametrize("case", ["rule", "time", "req_of"])
def test_malformed_device_descriptor(case):
    hb = small()
    e = engine(max_batch_desc=1 << 10)
    b = DevBatch(hb)
    torch.cuda.synchronize()
    b.submit(e, pipelined=False)
    e.wait()
    torch.cuda.synchronize()
    r0 = recs(e)
    bad = 33
    if case == "rule":
        b.db.rule[bad] = len(RULES)
    elif case == "time":
        b.db.now[bad] = 0xFFFD0001
    else:
        b.db.req_of[bad] = bad - 2  # decreases (and is below n_req)
    torch.cuda.synchronize()
    b.refund(e)
    assert code_of(e.wait_refund) == EINVAL
    assert code_of(e.wait) == ESTATE, "the failed flight is gone"
    assert recs(e) == r0, "nothing written"
    e.close()
