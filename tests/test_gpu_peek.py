"""rl_peek / rl_peek_device / rl_forget (rl_hip.h "Peek / forget") on the GPU: what they report
equals the oracle's Redis GET and freecache Get at every batch boundary of the parity streams,
peeks change nothing, and a forget is DEL plus dropping the local-cache entry — the rest of the
stream is decided as by an oracle that never saw the forgotten strings."""
import functools

import numpy as np
import pytest
import torch

import hiprl
import oracle
import router
import streams
from streams import RULES, batch_sizes, make_stream

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = -1, -4, -5
NIL = hiprl.NIL_RULE
MAX_DESC = 1 << 14
MAX_NOW = 0xFFFD0000
F, LC, NILF, PS, BAD = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND, hiprl.PEEK_BAD


def engine(local_cache=False, pipeline="v4", log2_slots=(16, 16, 16, 14), rules=RULES, **kw):
    kw.setdefault("max_batch_desc", MAX_DESC)
    e = hiprl.Engine(local_cache=local_cache, pipeline=pipeline, log2_slots=log2_slots, **kw)
    e.load_rules(rules)
    return e


def make_oracle(local_cache=False, rules=RULES, **kw):
    o = oracle.Oracle(local_cache=local_cache, **kw)
    o.load_rules(rules)
    return o


def run(backend, batches):
    out = [backend.submit(b) for b in batches]
    return np.concatenate([s for s, _ in out]), np.concatenate([t for _, t in out])


@functools.lru_cache(maxsize=None)
def stream(seed):
    """The snapshot suite's stream of a seed as batches (6000 requests, batches <= 1500), and the
    cut: the batch boundary nearest the middle request."""
    reqs = make_stream(seed, 6000, t0=1_700_000_000 - 7 + seed * 86400 - 130)
    sizes = batch_sizes(reqs, np.random.default_rng(seed + 100), 1500)
    cut = int(np.argmin(np.abs(np.cumsum(sizes) - 3000))) + 1
    batches, i = [], 0
    for bs in sizes:
        batches.append(hiprl.build_batch(reqs[i:i + bs]))
        i += bs
    assert 0 < cut < len(batches)
    return batches, cut


@functools.lru_cache(maxsize=None)
def expected(seed, local_cache):
    """One oracle over the whole stream: per-batch outputs (never modified)."""
    o = make_oracle(local_cache)
    return [o.submit(b) for b in stream(seed)[0]]


def cat(outs):
    return np.concatenate([s for s, _ in outs]), np.concatenate([t for _, t in outs])


def retimed(b, t):
    """The batch with every request at time t."""
    return hiprl.Batch(b.blob, b.off, b.rule, b.req_of, np.full(b.n_req, t, np.int64), b.hits)


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


def key_string(b, i, rules):
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


def peek_chunks(e, b_items, now, chunk=8192):
    out = []
    for i in range(0, len(b_items), chunk):
        pb = key_batch(b_items[i:i + chunk], now)
        out.append((pb, e.peek(pb)))
    return out


# ---- 1. parity with the oracle at every batch boundary ------------------------------------------
@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_peek_parity_at_every_batch_boundary(seed, local_cache, pipeline):
    batches, _ = stream(seed)
    ctx = f"seed={seed} local={local_cache} pipeline={pipeline}"
    e = engine(local_cache, pipeline)
    o = make_oracle(local_cache)
    outs = []
    for j, b in enumerate(batches):
        outs.append(e.submit(b))
        o.submit(b)
        t_next = int(batches[j + 1].now[0]) if j + 1 < len(batches) else int(b.now[-1])
        pb = retimed(b, t_next)
        check_against_oracle(e.peek(pb), pb, o, ctx=f"{ctx} after batch {j}")
    # every distinct (prefix, rule) of the stream, at the stream's last time
    seen = {}
    for b in batches:
        for i in range(b.n_desc):
            if int(b.rule[i]) != NIL:
                seen.setdefault((b.prefix(i), int(b.rule[i])))
    t_end = int(batches[-1].now[-1])
    found = absent = cached = 0
    for pb, rep in peek_chunks(e, list(seen), t_end):
        f, a, c = check_against_oracle(rep, pb, o, ctx=f"{ctx} at the end")
        found, absent, cached = found + f, absent + a, cached + c
    # guard (the oracle's own figures): the end state holds live, expired and frozen strings
    assert found >= 30 and absent >= 30 and (not local_cache or cached >= 20), (found, absent, cached)
    # peeks changed nothing: the whole stream is the oracle's
    streams.assert_same(*cat(expected(seed, local_cache)), *cat(outs), ctx)
    e.close()


# ---- 2. TTL ------------------------------------------------------------------------------------
def test_ttl_and_expiry_inside_the_window():
    big = 1 << 30
    rules = [(big, hiprl.MINUTE), (big, hiprl.HOUR)]
    t0 = 1_700_000_000  # second 20 of its minute
    assert t0 % 60 == 20
    e = engine(rules=rules)
    o = make_oracle(rules=rules)
    keys = [("k0", 0), ("k1", 0), ("k2", 1), ("k3", 1), ("k4", 0)]
    touches = [  # (time, [(key index, jitter)])
        (t0, [(0, 0), (1, 7), (2, 300), (3, 0), (4, 300)]),
        (t0 + 5, [(1, 0), (2, 7), (4, 7)]),
        (t0 + 9, [(4, 0), (3, 300)]),
    ]
    last = {}
    for t, items in touches:
        reqs = [("ttl", [[("k", keys[k][0])]], [keys[k][1]], 1, t) for k, _ in items]
        b = hiprl.build_batch(reqs, jit=[j for _, j in items])
        streams.assert_same(*o.submit(b), *e.submit(b), f"ttl touches at {t}")
        for k, j in items:
            last[k] = (t, j)
    now = t0 + 12
    pb = key_batch([(hiprl.cache_key_prefix("ttl", [("k", n)]), r) for n, r in keys], now)
    rep = e.peek(pb)
    check_against_oracle(rep, pb, o, rules)
    for k, (n, r) in enumerate(keys):
        t_last, jit = last[k]
        div = hiprl.UNIT_DIVIDER[rules[r][1]]
        assert int(rep[k]["flags"]) == F and int(rep[k]["ttl_s"]) == t_last + div + jit - now, (k, rep[k])
    assert [int(c) for c in rep["count"]] == [1, 2, 2, 2, 3]
    # jitter 0, MINUTE: in the next window the string is another one
    nxt = t0 - 20 + 60
    pb = key_batch([(hiprl.cache_key_prefix("ttl", [("k", "k0")]), 0)], nxt)
    rep = e.peek(pb)
    check_against_oracle(rep, pb, o, rules)
    assert int(rep[0]["flags"]) == 0 and int(rep[0]["count"]) == 0
    # now >= exp inside the string's window: a MINUTE touch of the string of an hour's first
    # minute expires after 60 s, and the HOUR rule reads the same string for the whole hour
    th = (t0 // 3600 + 1) * 3600
    b = hiprl.build_batch([("ttl", [[("k", "shared")]], [0], 4, th + 5)])
    streams.assert_same(*o.submit(b), *e.submit(b), "shared string touch")
    pfx = hiprl.cache_key_prefix("ttl", [("k", "shared")])
    pb = key_batch([(pfx, 1), (pfx, 1), (pfx, 0)], [th + 64, th + 65, th + 59])
    rep = e.peek(pb)
    check_against_oracle(rep, pb, o, rules)
    assert [int(x) for x in rep["flags"]] == [F, 0, F]
    assert [int(x) for x in rep["ttl_s"]] == [1, 0, 6] and [int(x) for x in rep["count"]] == [4, 0, 4]


# ---- 3. forget ---------------------------------------------------------------------------------
def nil_where(b, strings, rules):
    """b with every descriptor whose key string is in `strings` turned into a nil limit."""
    rule = b.rule.copy()
    for i in range(b.n_desc):
        if int(rule[i]) != NIL and key_string(b, i, rules)[0] in strings:
            rule[i] = NIL
    return hiprl.Batch(b.blob, b.off, rule, b.req_of, b.now, b.hits, b.jit)


@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_forget_is_del_plus_cache_drop(seed, local_cache):
    batches, cut = stream(seed)
    ctx = f"seed={seed} local={local_cache}"
    e = engine(local_cache)
    first = run(e, batches[:cut])
    t_cut = int(batches[cut].now[0])
    lb = batches[cut - 1]
    fb = key_batch([(lb.prefix(i), int(lb.rule[i])) for i in range(lb.n_desc) if int(lb.rule[i]) != NIL], t_cut)
    forgotten = {key_string(fb, i, RULES)[0] for i in range(fb.n_desc)}
    before = e.peek(fb)
    occ, live, ins = e.occupancy(), e.stats()["live_keys"], e.stats()["inserted_keys"]
    assert np.array_equal(e.forget(fb), before), ctx
    after = e.peek(fb)
    assert not np.any(after["flags"] & (F | LC)) and not np.any(after["count"]) and not np.any(after["ttl_s"]), ctx
    assert e.occupancy() == occ and e.stats()["live_keys"] == live and e.stats()["inserted_keys"] == ins
    rest = run(e, batches[cut:])
    # the oracle that never saw the forgotten strings before the cut
    o2 = make_oracle(local_cache)
    for b in batches[:cut]:
        o2.submit(nil_where(b, forgotten, RULES))
    want = run(o2, batches[cut:])
    kept = cat(expected(seed, local_cache)[cut:])
    assert (want[0] != kept[0]).sum() >= 50, "guard: the forget changes too few decisions"
    streams.assert_same(*want, *rest, f"{ctx}: after the forget")
    streams.assert_same(*cat(expected(seed, local_cache)[:cut]), *first, f"{ctx}: before the forget")
    e.close()


# ---- 4. tight region ---------------------------------------------------------------------------
def test_tight_region_with_probe_wrap():
    """180 keys of one HOUR window in a 256-slot region (load limit 192): long probe chains, some
    past the region's end; 40 absent keys end their walks at a free slot."""
    t = 1_700_000_000
    assert oracle.place(t // 3600 * 3600)[0] == 4  # an HOUR-home region
    rules = [(3, hiprl.HOUR)]
    batches = [hiprl.build_batch([("tight", [[("k", str(i))]], [0], 2, t) for i in range(j, j + 10)])
               for j in range(0, 180, 10)]
    o = make_oracle(True, rules)
    e = engine(True, rules=rules, max_batch_desc=256, log2_slots=(8, 8, 8, 8))
    streams.assert_same(*run(o, batches), *run(e, batches), "tight: first pass")
    occ = e.occupancy()
    assert occ["live"][4] == 180 and occ["slots"][4] == 256
    pfx = lambda i: hiprl.cache_key_prefix("tight", [("k", str(i))])
    pb = key_batch([(pfx(i), 0) for i in range(220)], t + 1)
    rep = e.peek(pb)
    assert check_against_oracle(rep, pb, o, rules)[:2] == (180, 40)
    assert np.all(rep["flags"][:180] == F) and np.all(rep["count"][:180] == 2) and not np.any(rep["flags"][180:])
    fb = key_batch([(pfx(i), 0) for i in range(0, 180, 2)], t + 1)
    e.forget(fb)
    rep = e.peek(pb)
    assert int((rep["flags"] & F != 0).sum()) == 90
    assert np.all(rep["flags"][1:180:2] == F) and not np.any(rep["flags"][0:180:2])
    assert e.occupancy() == occ
    forgotten = {key_string(fb, i, rules)[0] for i in range(fb.n_desc)}
    o2 = make_oracle(True, rules)
    for b in batches:
        o2.submit(nil_where(b, forgotten, rules))
    streams.assert_same(*run(o2, batches), *run(e, batches), "tight: second pass")
    assert e.occupancy()["live"][4] == 180 and e.stats()["inserted_keys"] == 180  # every key kept its slot


# ---- 5. shapes and edges -----------------------------------------------------------------------
LENS = [0, 1, 7, 8, 9, 23, 24, 25, 33, 70]


@functools.lru_cache(maxsize=None)
def shape_engine():
    rules = [(1 << 30, hiprl.MINUTE)]
    return engine(rules=rules), make_oracle(rules=rules), rules


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_shapes_and_prefix_lengths(n):
    """Prefixes of every length class packed back to back: unaligned offsets, and lengths on both
    sides of the 24 bytes the preload covers."""
    e, o, rules = shape_engine()
    t = 1_700_003_000 + 60 * n  # a minute of its own per n (the engine is shared)
    items = []
    for i in range(n):
        ln = LENS[(i + n) % len(LENS)]
        items.append(((f"{n}.{i}." * 24).encode()[:ln], 0))
    sb = key_batch(items, [t] * n)
    sb.hits[:] = 1 + np.arange(n) % 3
    streams.assert_same(*o.submit(sb), *e.submit(sb), f"shapes n={n}")
    pb = key_batch(items, t + 1)
    rep = e.peek(pb)
    assert rep.shape[0] == n
    found, absent, _ = check_against_oracle(rep, pb, o, rules, ctx=f"shapes n={n}")
    assert (found, absent) == (n, 0)
    assert np.all(rep["ttl_s"] == 59)
    # the same strings with every offset moved by three bytes
    if n:
        shifted = hiprl.Batch(np.concatenate([np.frombuffer(b"xyz", np.uint8), pb.blob]), pb.off + np.uint32(3), pb.rule,
                              pb.req_of, pb.now, pb.hits)
        assert np.array_equal(e.peek(shifted), rep)
    assert e.forget(key_batch(items, t + 1)).shape[0] == n


def test_colliding_entry_splits_are_one_string():
    e, o, rules = shape_engine()
    t = 1_700_004_000
    b = hiprl.build_batch([("dom", [[("a_b", "c")]], [0], 3, t), ("dom", [[("a", "b_c")]], [0], 4, t)])
    streams.assert_same(*o.submit(b), *e.submit(b), "colliding splits")
    rep = e.peek(hiprl.build_batch([("dom", [[("a", "b_c")], [("a_b", "c")]], [0, 0], 1, t + 2)]))
    assert [int(x) for x in rep["count"]] == [7, 7] and np.all(rep["flags"] == F)


@pytest.mark.parametrize("unit", [hiprl.SECOND, hiprl.MINUTE])
def test_window_rollover(unit):
    rules = [(9, unit)]
    e = engine(True, rules=rules)
    o = make_oracle(True, rules)
    div = hiprl.UNIT_DIVIDER[unit]
    t = 1_700_000_040 // div * div + div - 1  # the window's last second
    b = hiprl.build_batch([("roll", [[("k", str(i % 7))]], [0], 4, t) for i in range(30)])
    streams.assert_same(*o.submit(b), *e.submit(b), "rollover touch")
    items = [(hiprl.cache_key_prefix("roll", [("k", str(i))]), 0) for i in range(7)]
    pb = key_batch(items, t)
    assert check_against_oracle(e.peek(pb), pb, o, rules)[0] == 7
    for now in (t + 1, t + div, t + 1 + div, t + 2 * div):  # windows w + 1 and w + 2
        pb = key_batch(items, now)
        rep = e.peek(pb)
        check_against_oracle(rep, pb, o, rules, ctx=f"now={now}")
        assert not np.any(rep["flags"]) and not np.any(rep["count"]), now


def test_per_second_split_stores():
    """A SECOND and a MINUTE rule on one prefix at a minute's first second: one string, one slot,
    two counters. Each is reported and forgotten on its own."""
    rules = [(100, hiprl.SECOND), (100, hiprl.MINUTE)]
    t = 1_700_000_040 // 60 * 60
    e = engine(rules=rules, per_second_split=True)
    o = make_oracle(rules=rules, per_second_split=True)
    names = ["p1", "p2", "p3", "p4", "p5"]
    touch = hiprl.build_batch([("ps", [[("k", n)]], [r], h, t) for n in names for r, h in ((0, 3), (1, 5))])
    streams.assert_same(*o.submit(touch), *e.submit(touch), "split touch")
    pfx = {n: hiprl.cache_key_prefix("ps", [("k", n)]) for n in names}
    both = key_batch([(pfx[n], r) for n in names for r in (0, 1)], t)
    rep = e.peek(both)
    check_against_oracle(rep, both, o, rules, split=True)
    assert [int(x) for x in rep["count"]] == [3, 5] * 5
    assert [int(x) for x in rep["flags"]] == [F | PS, F] * 5 and [int(x) for x in rep["ttl_s"]] == [0, 60] * 5
    # one call: p1 loses its SECOND counter, p2 its MINUTE counter, p3 and p4 both (in both orders)
    fb = key_batch([(pfx["p1"], 0), (pfx["p2"], 1), (pfx["p3"], 0), (pfx["p3"], 1), (pfx["p4"], 1), (pfx["p4"], 0)], t)
    frep = e.forget(fb)
    assert [int(x) for x in frep["count"]] == [3, 5, 3, 5, 5, 3]
    rep = e.peek(both)
    assert [int(x) for x in rep["count"]] == [0, 5, 3, 0, 0, 0, 0, 0, 3, 5]
    assert [int(x) for x in rep["flags"]] == [PS, F, F | PS, 0, PS, 0, PS, 0, F | PS, F]
    # the next INCRBY of a forgotten store starts from 0, the other store goes on
    forgotten = {(key_string(fb, i, rules)[0], int(fb.rule[i])) for i in range(fb.n_desc)}
    rule = touch.rule.copy()
    for i in range(touch.n_desc):
        if (key_string(touch, i, rules)[0], int(rule[i])) in forgotten:
            rule[i] = NIL
    o2 = make_oracle(rules=rules, per_second_split=True)
    o2.submit(hiprl.Batch(touch.blob, touch.off, rule, touch.req_of, touch.now, touch.hits))
    streams.assert_same(*o2.submit(touch), *e.submit(touch), "split: after the forget")
    rep = e.peek(both)
    check_against_oracle(rep, both, o2, rules, split=True)
    assert [int(x) for x in rep["count"]] == [3, 10, 6, 5, 3, 5, 3, 5, 6, 10]


def test_lag_window_keeps_the_previous_second():
    rules = [(50, hiprl.SECOND)]
    t = 1_700_000_001
    e = engine(rules=rules, lag_window=True, log2_slots=(8, 8, 8, 8), max_batch_desc=4096)
    o = make_oracle(rules=rules)
    late = hiprl.build_batch([("lag", [[("a", str(i))]], [0], 1 + i % 3, t) for i in range(30)])
    newest = hiprl.build_batch([("lag", [[("b", str(i))]], [0], 2, t + 2) for i in range(60)])
    for b in (late, newest):
        streams.assert_same(*o.submit(b), *e.submit(b), "lag touches")
    assert e.occupancy()["gen"][t % 2] == t + 3  # the table has seen t + 2
    pb = key_batch([(hiprl.cache_key_prefix("lag", [("a", str(i))]), 0) for i in range(30)], t)
    rep = e.peek(pb)
    assert np.all(rep["flags"] == F) and [int(x) for x in rep["count"]] == [1 + i % 3 for i in range(30)]
    pb2 = key_batch([(hiprl.cache_key_prefix("lag", [("b", str(i))]), 0) for i in range(60)], t + 2)
    assert np.all(e.peek(pb2)["flags"] == F)
    e.forget(pb)
    assert not np.any(e.peek(pb)["flags"]) and np.all(e.peek(pb2)["count"] == 2)


def test_duplicates_in_one_forget():
    e, o, rules = shape_engine()
    t = 1_700_005_000
    b = hiprl.build_batch([("dup", [[("k", "x")]], [0], 6, t), ("dup", [[("k", "y")]], [0], 2, t)])
    streams.assert_same(*o.submit(b), *e.submit(b), "dup touch")
    px, py = (hiprl.cache_key_prefix("dup", [("k", v)]) for v in "xy")
    fb = key_batch([(px, 0)] * 70 + [(py, 0)] + [(px, 0)] * 3, t + 1)
    rep = e.forget(fb)
    assert [int(x) for x in rep["count"]] == [6] * 70 + [2] + [6] * 3  # every duplicate: the state before the call
    assert np.all(rep["flags"] == F)
    assert not np.any(e.peek(fb)["flags"])
    st, _ = e.submit(b)
    assert [int(x) for x in st["limit_remaining"]] == [(1 << 30) - 6, (1 << 30) - 2]


# ---- 6. errors ---------------------------------------------------------------------------------
def raises(code, fn, *a):
    with pytest.raises(hiprl.RedisError) as ei:
        fn(*a)
    assert ei.value.code == code, ei.value


def device_peek(e, b, dev):
    db = router.DeviceBatch.from_host(b, dev)
    out = torch.zeros(max(1, b.n_desc) * 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    e.peek_device(db.n_desc, db.n_req, int(b.blob.shape[0]), db.ptrs(), out.data_ptr())
    torch.cuda.synchronize()
    return out[:b.n_desc * 16].cpu().numpy().view(hiprl.PEEK_DTYPE)


def test_refused_while_a_batch_is_in_flight_or_a_restore_is_open():
    dev = torch.device("cuda", 0)
    batches, _ = stream(1)
    e = engine(True)
    o = make_oracle(True)
    want0, want1 = o.submit(batches[0]), o.submit(batches[1])
    streams.assert_same(*want0, *e.submit(batches[0]), "batch 0")
    b = batches[1]
    db = router.DeviceBatch.from_host(b, dev)
    out = torch.zeros(b.n_desc * 20, dtype=torch.uint8, device=dev)
    thr = torch.zeros(b.n_req, dtype=torch.int32, device=dev)
    rep = torch.zeros(b.n_desc * 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    e.submit_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), out.data_ptr(), thr.data_ptr())
    raises(ESTATE, e.peek, b)
    raises(ESTATE, e.forget, b)
    raises(ESTATE, e.peek_device, db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), rep.data_ptr())
    e.wait()
    torch.cuda.synchronize()
    streams.assert_same(*want1, out.cpu().numpy().view(hiprl.STATUS_DTYPE), thr.cpu().numpy().view(np.uint32),
                        "the batch in flight")
    pb = retimed(b, int(b.now[-1]))
    check_against_oracle(e.peek(pb), pb, o)
    # an open snapshot does not block a peek; an open restore does
    h = e.snapshot_begin()
    check_against_oracle(e.peek(pb), pb, o)
    recs = []
    while True:
        part = e.snapshot_next(4096)
        if not part.shape[0]:
            break
        recs.append(part)
    e.snapshot_end()
    e.restore_begin(h)
    raises(ESTATE, e.peek, b)
    raises(ESTATE, e.forget, b)
    raises(ESTATE, e.peek_device, db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), rep.data_ptr())
    e.restore_put(np.concatenate(recs))
    e.restore_end()
    check_against_oracle(e.peek(pb), pb, o)
    e.close()


def test_malformed_batches():
    dev = torch.device("cuda", 0)
    rules = [(5, hiprl.MINUTE), (5, hiprl.HOUR)]
    t = 1_700_000_000
    e = engine(True, rules=rules, max_batch_desc=64)
    o = make_oracle(True, rules)
    b = hiprl.build_batch([("bad", [[("k", str(i % 9))], [("j", str(i % 4))]], [0, 1], 2, t) for i in range(30)])
    streams.assert_same(*o.submit(b), *e.submit(b), "touch")
    good = retimed(b, t + 1)
    base = e.peek(good)
    assert check_against_oracle(base, good, o, rules)[2] > 0  # some strings are frozen

    def variant(rule=None, now=None, req_of=None):
        return hiprl.Batch(good.blob, good.off, good.rule if rule is None else rule,
                           good.req_of if req_of is None else req_of, good.now if now is None else now, good.hits)

    bad_rule = good.rule.copy()
    bad_rule[[3, 40]] = len(rules)
    neg = good.now.copy()
    neg[7] = -1
    late = good.now.copy()
    late[29] = MAX_NOW + 1
    edge = good.now.copy()
    edge[:] = MAX_NOW
    dec = good.req_of.copy()
    dec[10] = 9
    for fn in (e.peek, e.forget):
        raises(EINVAL, fn, variant(rule=bad_rule))
        raises(EINVAL, fn, variant(now=neg))
        raises(EINVAL, fn, variant(now=late))
        raises(EINVAL, fn, variant(req_of=dec))
        big = hiprl.build_batch([("bad", [[("k", str(i))]], [0], 1, t) for i in range(65)])
        raises(ECAPACITY, fn, big)
    assert not np.any(e.peek(variant(now=edge))["flags"])  # the last admissible time
    assert np.array_equal(e.peek(good), base)  # the refused forgets changed nothing
    # the device form answers what it can: RL_PEEK_BAD on exactly the malformed descriptors
    both = good.now.copy()
    both[7], both[29] = -1, MAX_NOW + 1
    rep = device_peek(e, variant(rule=bad_rule, now=both), dev)
    is_bad = np.isin(np.arange(good.n_desc), [3, 40]) | np.isin(good.req_of, [7, 29])
    assert is_bad.sum() == 6
    assert np.all(rep["flags"][is_bad] == BAD) and not np.any(rep["count"][is_bad] | rep["ttl_s"][is_bad]
                                                              | rep["cached_s"][is_bad])
    assert np.array_equal(rep[~is_bad], base[~is_bad])
    streams.assert_same(*o.submit(b), *e.submit(b), "after the refusals")
    e.close()


# ---- 7. device form ----------------------------------------------------------------------------
@pytest.mark.parametrize("local_cache", [False, True])
def test_device_form_equals_host_form(local_cache):
    dev = torch.device("cuda", 0)
    batches, cut = stream(2)
    e = engine(local_cache)
    run(e, batches[:cut])
    pb = retimed(batches[cut - 1], int(batches[cut].now[0]))
    host = e.peek(pb)
    assert np.any(host["flags"] & F) and np.any(host["flags"] == NILF) and np.any(host["flags"] == 0)
    assert np.array_equal(device_peek(e, pb, dev), host)
    assert device_peek(e, key_batch([], 0), dev).shape[0] == 0
    e.close()
