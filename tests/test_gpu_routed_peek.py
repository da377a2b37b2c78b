"""Routed peek / forget (rl_hip.h "Routed peek / forget") on the GPU.

Engine level: rl_peek_routed over host-built records answers byte for byte what Engine.peek (the
lone engine's path, pinned to the oracle by test_gpu_peek.py) answers for the same keys and times.
Router level, local transport and emulated collectives: every origin's peek equals the oracle's
Redis GET / freecache Get of the serial stream wherever the key lives, peeks change nothing, a
forget reports the state before the call (duplicates across origins included) and is DEL plus
dropping the local-cache entry at the owner, and a refused batch on one origin leaves every
owner untouched. Every plan (batches, key pools, guards) is made on the CPU from the oracle alone.
"""
import functools

import numpy as np
import pytest
import torch

import hiprl
import oracle
import routing
import streams
from streams import RULES
from test_gpu_combining import Bufs
from test_gpu_emulated_router import parallel
from test_gpu_router import stream_batches

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 0x5EE7AB1E5EED
EINVAL, ECAPACITY, ESTATE, EPEER = -1, -4, -5, -7
NIL = hiprl.NIL_RULE
T0 = 1_700_000_000
MAXD = 2048  # the routers' max_desc
F, LC, NILF, PS, BAD = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND, hiprl.PEEK_BAD
SIZES = [257, 0, 256, 1]  # descriptors per origin, rotated over origins and rounds


# ---- helpers (key_batch, key_string, check_against_oracle, nil_where: as in test_gpu_peek.py) ----
def make_oracle(local_cache=False, **kw):
    o = oracle.Oracle(local_cache=local_cache, **kw)
    o.load_rules(RULES)
    return o


def key_batch(items, now):
    """[(prefix bytes, rule id)] -> one request at `now` (or one request per descriptor when `now`
    is a sequence), prefixes packed back to back."""
    lens = [len(p) for p, _ in items]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    blob = np.frombuffer(b"".join(p for p, _ in items), np.uint8).copy()
    rule = np.array([r for _, r in items], np.uint32)
    if np.ndim(now) == 0:
        return hiprl.Batch(blob, off, rule, np.zeros(len(items), np.uint32), np.array([now], np.int64),
                           np.ones(1, np.uint32))
    return hiprl.Batch(blob, off, rule, np.arange(len(items), dtype=np.uint32), np.array(now, np.int64),
                       np.ones(len(items), np.uint32))


def key_string(b, i, rules=RULES):
    now = int(b.now[b.req_of[i]])
    return oracle.cache_key(b.prefix(i), rules[int(b.rule[i])][1], now), now


def check_against_oracle(rep, b, o, rules=RULES, split=False, ctx=""):
    """Every reply of a peek of b against the oracle's GET / freecache Get. Returns (found,
    absent, cached) counts over the non-nil descriptors."""
    assert rep.shape[0] == b.n_desc
    found = absent = cached = 0
    for i in range(b.n_desc):
        r = rep[i]
        fl = int(r["flags"])
        if int(b.rule[i]) == NIL:
            assert (fl, int(r["count"]), int(r["ttl_s"]), int(r["cached_s"])) == (NILF, 0, 0, 0), (ctx, i, r)
            continue
        k, now = key_string(b, i, rules)
        ps = split and rules[int(b.rule[i])][1] == hiprl.SECOND
        c = o.counter(k, now, per_second=ps)
        lc = o.local_cached(k, now)
        assert bool(fl & F) == (c >= 0), (ctx, i, k, r, c)
        assert int(r["count"]) == max(c, 0), (ctx, i, k, r, c)
        assert bool(fl & LC) == lc, (ctx, i, k, r, lc)
        assert bool(fl & PS) == ps and not fl & (NILF | BAD), (ctx, i, r)
        assert (int(r["cached_s"]) > 0) == lc, (ctx, i, r)
        assert (int(r["ttl_s"]) > 0) == (c >= 0 and not ps), (ctx, i, r)
        found += c >= 0
        absent += c < 0
        cached += lc
    return found, absent, cached


def nil_where(b, strings, rules=RULES):
    """b with every descriptor whose key string is in `strings` turned into a nil limit."""
    rule = b.rule.copy()
    for i in range(b.n_desc):
        if int(rule[i]) != NIL and key_string(b, i, rules)[0] in strings:
            rule[i] = NIL
    return hiprl.Batch(b.blob, b.off, rule, b.req_of, b.now, b.hits, b.jit)


def distinct_keys(batches):
    seen = {}
    for b in batches:
        for i in range(b.n_desc):
            if int(b.rule[i]) != NIL:
                seen.setdefault((b.prefix(i), int(b.rule[i])))
    return list(seen)


def unseen_keys(n, tag):
    return [(hiprl.cache_key_prefix("unseen", [("u", f"{tag}.{i}")]), i % len(RULES)) for i in range(n)]


def owner_of(item, G):
    return oracle.route_owner(*oracle.prefix_lanes(item[0], SEED), G)


def state_of(o, item, t):
    """(counter or -1, locally cached) of a (prefix, rule) at time t per the oracle."""
    k = oracle.cache_key(item[0], RULES[item[1]][1], t)
    return o.counter(k, t), o.local_cached(k, t)


@functools.lru_cache(maxsize=None)
def steps_of(G, n_steps, seed):
    """stream_batches rows (never modified): 300 requests per origin and step, step s at T0 + s."""
    return stream_batches(G, n_steps, 300, seed)


def check_step(o, row, got, ctx):
    est, ethr = o.submit(routing.concat_batches(row))
    d0 = r0 = 0
    for g, (b, (st, thr)) in enumerate(zip(row, got)):
        streams.assert_same(est[d0:d0 + b.n_desc], ethr[r0:r0 + b.n_req], st, thr, f"{ctx} origin={g}")
        d0 += b.n_desc
        r0 += b.n_req


def new_engines(G, local_cache):
    es = []
    for _ in range(G):
        e = hiprl.Engine(local_cache=local_cache, max_batch_desc=MAXD * G)
        e.load_rules(RULES)
        es.append(e)
    return es


class LocalWorld:
    """G engines behind one local-transport router (no host staging: the peek allocates its own)."""

    def __init__(self, G, local_cache):
        self.G = G
        self.engines = new_engines(G, local_cache)
        self.router = hiprl.Router(self.engines, max_desc=MAXD)

    def step(self, row):
        bf = Bufs(row)
        torch.cuda.synchronize()
        self.router.step(*bf.args())
        return bf.results()

    def ask(self, what, batches):
        """-> (one reply array per origin or None, the code per origin: one call, one code)."""
        try:
            return getattr(self.router, what)(batches), [None] * self.G
        except hiprl.RedisError as e:
            return None, [e.code] * self.G

    def step_with_calls_in_flight(self, row, batches):
        bf = Bufs(row)
        torch.cuda.synchronize()
        self.router.submit(*bf.args())
        codes = [self.ask(w, batches)[1] for w in ("peek", "forget")]
        self.router.wait()
        return bf.results(), codes

    def close(self):
        self.router.close()


class EmuWorld:
    """G emulated ranks, one thread each (test_gpu_emulated_router.py), with host staging."""

    def __init__(self, G, local_cache):
        self.G = G
        wid = hiprl.Router.emu_world(G)
        self.engines = new_engines(G, local_cache)
        self.routers = [None] * G

        def mk(r):
            self.routers[r] = hiprl.Router([self.engines[r]], max_desc=MAXD, n_shards=G, rank=r, rccl_id=wid,
                                           emulated=True, host=True)
        parallel(G, mk)
        assert all(r is not None for r in self.routers)

    def step(self, row):
        bf = Bufs(row)
        bs, outs, thrs = bf.args()
        torch.cuda.synchronize()

        def worker(r):
            self.routers[r].step([bs[r]], [outs[r]], [thrs[r]])
        parallel(self.G, worker)
        return bf.results()

    def ask(self, what, batches):
        reps, codes = [None] * self.G, [None] * self.G

        def worker(r):
            try:
                reps[r] = getattr(self.routers[r], what)([batches[r]])[0]
            except hiprl.RedisError as e:
                codes[r] = e.code
        parallel(self.G, worker)
        return (reps if all(c is None for c in codes) else None), codes

    def step_with_calls_in_flight(self, row, batches):
        bf = Bufs(row)
        bs, outs, thrs = bf.args()
        torch.cuda.synchronize()
        codes = [[None] * self.G, [None] * self.G]

        def worker(r):
            R = self.routers[r]
            R.submit([bs[r]], [outs[r]], [thrs[r]])
            for w, what in enumerate(("peek", "forget")):
                try:
                    getattr(R, what)([batches[r]])
                except hiprl.RedisError as e:
                    codes[w][r] = e.code
            R.wait()
        parallel(self.G, worker)
        return bf.results(), codes

    def close(self):
        parallel(self.G, lambda r: self.routers[r].close())


def world(transport, G, local_cache):
    return LocalWorld(G, local_cache) if transport == "local" else EmuWorld(G, local_cache)


# ---- 1. engine level: records against Engine.peek --------------------------------------------------
@functools.lru_cache(maxsize=None)
def engine_plan(local_cache, split):
    """A short stream in batches, the oracle after it, and the key pool: the stream's distinct
    (prefix, rule) pairs and as many strings never seen, interleaved. Guards from the oracle."""
    seed = 5
    reqs = streams.make_stream(seed, 600, t0=T0 - 30)
    sizes = streams.batch_sizes(reqs, np.random.default_rng(seed), 200)
    batches, i = [], 0
    for bs in sizes:
        batches.append(hiprl.build_batch(reqs[i:i + bs]))
        i += bs
    o = make_oracle(local_cache, per_second_split=split)
    for b in batches:
        o.submit(b)
    t = int(batches[-1].now[-1])
    seen = distinct_keys(batches)
    pool = [x for pair in zip(seen, unseen_keys(len(seen), "e")) for x in pair]
    found = absent = cached = 0
    for it in pool:
        k = oracle.cache_key(it[0], RULES[it[1]][1], t)
        c = o.counter(k, t, per_second=split and RULES[it[1]][1] == hiprl.SECOND)
        found += c >= 0
        absent += c < 0
        cached += o.local_cached(k, t)
    assert found >= 30 and absent >= 30 and (not local_cache or cached >= 20), (found, absent, cached)
    return batches, t, pool


def records_of(b):
    """The batch's routed records (routing.REC_DTYPE) as an origin's pack writes them."""
    rec = np.zeros(b.n_desc, routing.REC_DTYPE)
    for i in range(b.n_desc):
        a, bb = oracle.prefix_lanes(b.prefix(i), SEED)
        q = int(b.req_of[i])
        rec[i] = (a, bb, int(b.now[q]), int(b.rule[i]), 1, q)
    return rec


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("local_cache", [False, True])
def test_engine_records_equal_engine_peek(local_cache, split):
    batches, t, pool = engine_plan(local_cache, split)
    e = hiprl.Engine(local_cache=local_cache, per_second_split=split, max_batch_desc=1 << 12)
    e.load_rules(RULES)
    for b in batches:
        e.submit(b)
    for n in (1, 255, 256, 257, 3001):
        items = [pool[(7 * n + i) % len(pool)] for i in range(n)]
        pb = key_batch(items, [t - (i % 3 == 0) for i in range(n)])  # two request times
        want = e.peek(pb)
        rec = records_of(pb)
        bad = []
        if n > 300:  # malformed records between answered neighbours
            rec["rule"][5] = len(RULES)
            rec["rule"][100] = 0xFFFE
            rec["rule"][101] = NIL
            rec["now"][257] = 0xFFFD0001
            bad = [5, 100, 101, 257]
            rec["rule"][7] |= 9 << 16  # (a record's EXPIRE jitter rides in the rule word's upper half)
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
        d_rep = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        e.peek_routed(d_rec.data_ptr(), n, d_rep.data_ptr())
        torch.cuda.synchronize()
        got = d_rep.cpu().numpy().view(hiprl.PEEK_DTYPE)
        for i in bad:
            assert got[i].tobytes() == np.array([(0, 0, 0, BAD)], hiprl.PEEK_DTYPE).tobytes(), (n, i, got[i])
            want[i] = got[i]
        assert got.tobytes() == want.tobytes(), (n, np.flatnonzero(got != want)[:5])
    # n == 0 launches nothing; unknown flags are refused
    e.peek_routed(0, 0, 0)
    assert e.lib.rl_peek_routed(e.h, None, 0, None, 2) == EINVAL
    e.close()


# ---- 2. routed peek equals the oracle and the lone engine ------------------------------------------
def peek_rounds(G, pool, t):
    """Per round one batch per origin: a different slice of the pool each, sizes rotating through
    SIZES (so one origin of every round passes an empty batch)."""
    rounds = []
    for r in range(len(SIZES)):
        row = []
        for g in range(G):
            n = SIZES[(g + r) % len(SIZES)]
            start = (g * 97 + r * 131) % len(pool)
            row.append(key_batch([pool[(start + i) % len(pool)] for i in range(n)], t))
        rounds.append(row)
    return rounds


@functools.lru_cache(maxsize=None)
def peek_plan(G, local_cache):
    seed = 60 + G
    steps = steps_of(G, 4, seed)
    o = make_oracle(local_cache)
    for row in steps[:3]:
        o.submit(routing.concat_batches(row))
    t = T0 + 3
    seen = distinct_keys([b for row in steps[:3] for b in row])
    pool = []
    for i, (s, u) in enumerate(zip(seen, unseen_keys(len(seen), f"p{G}"))):
        pool += [s, u] + ([(b"", NIL)] if i % 16 == 0 else [])
    rounds = peek_rounds(G, pool, t)
    if G == 3:  # origin 1's keys all belong to owner 2: owners 0 and 1 receive nothing from it
        only2 = [it for it in pool if it[1] != NIL and owner_of(it, G) == 2][:40]
        assert len(only2) == 40
        rounds.append([rounds[0][0], key_batch(only2, t), rounds[0][2]])
    # guards
    sizes = {b.n_desc for row in rounds for b in row}
    assert {0, 1, 256, 257} <= sizes
    owners_with_live = set()
    reaches_all = False
    for row in rounds:
        for b in row:
            own = routing.owners_of(b, RULES, G, SEED)
            reaches_all |= set(range(G)) <= set(own.tolist())
            for i in range(b.n_desc):
                if own[i] >= 0 and o.counter(key_string(b, i)[0], t) >= 0:
                    owners_with_live.add(int(own[i]))
    assert owners_with_live == set(range(G)) and reaches_all
    if G == 3:
        assert set(routing.owners_of(rounds[-1][1], RULES, G, SEED).tolist()) == {2}
    return steps, rounds


@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("transport,G", [("local", 1), ("local", 3), ("local", 4), ("emulated", 2), ("emulated", 4)])
def test_routed_peek_equals_oracle(transport, G, local_cache):
    steps, rounds = peek_plan(G, local_cache)
    ctx = f"{transport} G={G} local={local_cache}"
    w = world(transport, G, local_cache)
    o = make_oracle(local_cache)
    for s, row in enumerate(steps[:3]):
        check_step(o, row, w.step(row), f"{ctx} step={s}")
    found = cached = 0
    for r, row in enumerate(rounds):
        reps, codes = w.ask("peek", row)
        assert reps is not None, (ctx, r, codes)
        for g, (b, rep) in enumerate(zip(row, reps)):
            f, _, c = check_against_oracle(rep, b, o, ctx=f"{ctx} round={r} origin={g}")
            found, cached = found + f, cached + c
    assert found >= 30 and (not local_cache or cached >= 10), (found, cached)
    # peeks changed nothing: the fourth step is the oracle's
    check_step(o, steps[3], w.step(steps[3]), f"{ctx} step=3")
    w.close()


# ---- 3. routed forget ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forget_plan(G):
    seed = 80 + G
    steps = steps_of(G, 4, seed)
    o = make_oracle(True)
    for row in steps[:2]:
        o.submit(routing.concat_batches(row))
    t = T0 + 2
    seen = distinct_keys([b for row in steps[:2] for b in row])
    st = {it: state_of(o, it, t) for it in seen}
    cached = [it for it in seen if st[it][1]]
    live = [it for it in seen if st[it][0] >= 0 and not st[it][1]]
    gone = [it for it in seen if st[it][0] < 0 and not st[it][1]] + unseen_keys(8, f"f{G}")
    both = cached[:12] + live[:12]
    only_a, only_b = live[12:26], cached[12:18] + live[26:36]
    a = both + only_a + gone[:6] + both[:3] + [(b"", NIL)]  # (duplicates inside one origin too)
    b = only_b + both[::-1] + gone[6:12]
    batches = [key_batch(a, t), key_batch(b, t)] + [key_batch([], t)] * (G - 2)
    sa, sb = set(a) - {(b"", NIL)}, set(b)
    n_cached = sum(1 for it in sa | sb if st.get(it, (-1, False))[1])
    n_absent = sum(1 for it in sa | sb if st.get(it, (-1, False)) == (-1, False))
    assert len(sa & sb) >= 10 and len(sa - sb) >= 10 and len(sb - sa) >= 10 and n_cached >= 10 and n_absent >= 5, (
        len(sa & sb), len(sa - sb), len(sb - sa), n_cached, n_absent)
    forgotten = {key_string(pb, i)[0] for pb in batches for i in range(pb.n_desc) if int(pb.rule[i]) != NIL}
    return steps, batches, forgotten


@pytest.mark.parametrize("transport,G", [("local", 3), ("emulated", 2)])
def test_routed_forget(transport, G):
    steps, batches, forgotten = forget_plan(G)
    ctx = f"forget {transport} G={G}"
    w = world(transport, G, True)
    o = make_oracle(True)
    for s, row in enumerate(steps[:2]):
        check_step(o, row, w.step(row), f"{ctx} step={s}")
    before = [(e.occupancy(), e.stats()["live_keys"]) for e in w.engines]
    reps, codes = w.ask("forget", batches)
    assert reps is not None, (ctx, codes)
    for g, (b, rep) in enumerate(zip(batches, reps)):  # the state before the call, for every duplicate
        check_against_oracle(rep, b, o, ctx=f"{ctx} origin={g}")
    assert [(e.occupancy(), e.stats()["live_keys"]) for e in w.engines] == before
    reps, codes = w.ask("peek", batches)
    assert reps is not None, (ctx, codes)
    for b, rep in zip(batches, reps):
        assert not np.any(rep["flags"] & (F | LC)) and not np.any(rep["count"]) and not np.any(rep["ttl_s"]), ctx
        assert not np.any(rep["cached_s"]), ctx
    # the oracle that never saw the forgotten strings
    o2 = make_oracle(True)
    for row in steps[:2]:
        o2.submit(nil_where(routing.concat_batches(row), forgotten))
    differ = 0
    for s, row in enumerate(steps[2:], 2):
        got = w.step(row)
        kept = o.submit(routing.concat_batches(row))[0]
        check_step(o2, row, got, f"{ctx} step={s}")
        differ += int((np.concatenate([st for st, _ in got]) != kept).sum())
    assert differ >= 5, "guard: the forget changes too few decisions"
    w.close()


# ---- 4. refusals change nothing anywhere -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refusal_plan():
    G = 3
    steps = steps_of(G, 3, 91)
    o = make_oracle(True)
    o.submit(routing.concat_batches(steps[0]))
    t = T0 + 1
    live = [it for it in distinct_keys(steps[0]) if state_of(o, it, t)[0] >= 0]
    assert len(live) >= 110
    good0, good2, mid = live[:40], live[40:80], live[80:110]
    bad = {}
    b = key_batch(mid, t)
    rule = b.rule.copy()
    rule[3] = 99
    bad["rule"] = (hiprl.Batch(b.blob, b.off, rule, b.req_of, b.now, b.hits), EINVAL)
    b = key_batch(mid, [t] * len(mid))
    req_of = b.req_of.copy()
    req_of[5] = 0
    bad["req_of"] = (hiprl.Batch(b.blob, b.off, b.rule, req_of, b.now, b.hits), EINVAL)
    bad["capacity"] = (key_batch([live[i % len(live)] for i in range(MAXD + 1)], t), ECAPACITY)
    return steps, key_batch(good0, t), key_batch(good2, t), bad, key_batch([], t)


@pytest.mark.parametrize("case", ["rule", "req_of", "capacity"])
@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_refusals_change_nothing(transport, case):
    steps, good0, good2, bad, empty = refusal_plan()
    G = 3
    ctx = f"refusal {transport} {case}"
    w = world(transport, G, True)
    o = make_oracle(True)
    check_step(o, steps[0], w.step(steps[0]), f"{ctx} step=0")
    bad_batch, code = bad[case]
    reps, codes = w.ask("forget", [good0, bad_batch, good2])
    assert reps is None
    assert codes == ([code] * 3 if transport == "local" else [EPEER, code, EPEER]), (ctx, codes)
    reps, codes = w.ask("peek", [good0, empty, good2])
    assert reps is not None, (ctx, codes)
    for g, b in ((0, good0), (2, good2)):
        f, a, _ = check_against_oracle(reps[g], b, o, ctx=f"{ctx} origin={g}")
        assert (f, a) == (b.n_desc, 0) and np.all(reps[g]["flags"] & F), ctx  # every key still present
    assert reps[1].shape[0] == 0
    check_step(o, steps[1], w.step(steps[1]), f"{ctx} step=1")
    if case == "rule":  # with a step submitted and not waited for
        got, codes = w.step_with_calls_in_flight(steps[2], [good0, empty, good2])
        assert codes == [[ESTATE] * 3, [ESTATE] * 3], (ctx, codes)
        check_step(o, steps[2], got, f"{ctx} step=2")
        reps, codes = w.ask("peek", [good0, empty, good2])  # and the calls work again
        assert reps is not None, (ctx, codes)
        check_against_oracle(reps[0], good0, o, ctx=f"{ctx} after the step")
    w.close()


# ---- 5. one-rank RCCL communicator -----------------------------------------------------------------
def test_rccl_one_rank_round_trip(monkeypatch):
    monkeypatch.setenv("NCCL_SOCKET_IFNAME", "lo")
    steps = steps_of(1, 3, 17)
    es = new_engines(1, True)
    r = hiprl.Router(es, max_desc=MAXD, n_shards=1, rank=0, rccl_id=hiprl.Router.unique_id())

    def step(row):
        bf = Bufs(row)
        torch.cuda.synchronize()
        r.step(*bf.args())
        return bf.results()
    o = make_oracle(True)
    for s, row in enumerate(steps[:2]):
        check_step(o, row, step(row), f"rccl step={s}")
    t = T0 + 2
    seen = distinct_keys([b for row in steps[:2] for b in row])
    pool = [x for pair in zip(seen, unseen_keys(len(seen), "r")) for x in pair]
    pb = key_batch(pool[:257] + [(b"", NIL)], t)
    f, a, c = check_against_oracle(r.peek([pb])[0], pb, o, ctx="rccl peek")
    assert f >= 30 and a >= 30 and c >= 5, (f, a, c)
    fb = key_batch(pool[:80:2] + pool[:10:2], t)
    check_against_oracle(r.forget([fb])[0], fb, o, ctx="rccl forget")
    after = r.peek([fb])[0]
    assert not np.any(after["flags"] & (F | LC)) and not np.any(after["count"])
    forgotten = {key_string(fb, i)[0] for i in range(fb.n_desc)}
    o2 = make_oracle(True)
    for row in steps[:2]:
        o2.submit(nil_where(routing.concat_batches(row), forgotten))
    check_step(o2, steps[2], step(steps[2]), "rccl step=2")
    r.close()
