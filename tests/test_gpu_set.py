"""rl_set (rl_hip.h "Set") on the GPU: the write that completes peek / forget. The oracle has no
setter, so every expected state is reached by requests: an engine whose counters were set from
another engine's peek, from hand-built values or from a Redis dump decides the rest of a stream
exactly as the oracle that ran the whole stream."""
import functools

import numpy as np
import pytest
import torch

import hiprl
import oracle
import resp
import router
import streams
from streams import RULES, batch_sizes, make_stream

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC, ECAPACITY, ESTATE = -1, -3, -4, -5
NIL = hiprl.NIL_RULE
MAX_NOW = 0xFFFD0000
F, LC, PS = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_PER_SECOND
KC, KF = hiprl.SET_KEEP_COUNTER, hiprl.SET_KEEP_CACHE
SMALL = (8, 8, 7, 6)  # slots per home unit: probe chains wrap, and a resize has somewhere to go
# the parity streams hold a few thousand strings per home unit: tables that take them (a batch
# must fit its region with every descriptor counted as a claim), two geometries
BIG_A, BIG_B = (11, 12, 12, 12), (12, 13, 13, 11)
DIV = hiprl.UNIT_DIVIDER
H0 = (1_700_000_000 // 3600 + 1) * 3600  # an hour's first second (not a day's)
assert H0 % 86400 and H0 % 3600 == 0


def engine(local_cache=False, log2_slots=SMALL, rules=RULES, **kw):
    kw.setdefault("max_batch_desc", 1 << 13)
    e = hiprl.Engine(local_cache=local_cache, log2_slots=log2_slots, **kw)
    e.load_rules(rules)
    return e


def make_oracle(local_cache=False, rules=RULES, **kw):
    o = oracle.Oracle(local_cache=local_cache, **kw)
    o.load_rules(rules)
    return o


def run(backend, batches):
    out = [backend.submit(b) for b in batches]
    return np.concatenate([s for s, _ in out]), np.concatenate([t for _, t in out])


def key_batch(items, now):
    """[(prefix bytes, rule id)] -> one request at `now`, or one request per descriptor when `now`
    is a sequence."""
    lens = [len(p) for p, _ in items]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    blob = np.frombuffer(b"".join(p for p, _ in items), np.uint8).copy()
    rule = np.array([r for _, r in items], np.uint32)
    if np.ndim(now) == 0:
        return hiprl.Batch(blob, off, rule, np.zeros(len(items), np.uint32), np.array([now], np.int64),
                           np.ones(1, np.uint32))
    return hiprl.Batch(blob, off, rule, np.arange(len(items), dtype=np.uint32), np.array(now, np.int64),
                       np.ones(len(items), np.uint32))


def vals(rows):
    """[(count, ttl_s, cached_s, flags)] -> PEEK_DTYPE."""
    return np.array([tuple(r) for r in rows], hiprl.PEEK_DTYPE).reshape(len(rows))


def pfx(name, dom="set"):
    return hiprl.cache_key_prefix(dom, [("k", str(name))])


def state(e, now):
    """Everything a refused or empty call must leave alone."""
    c = e.census(now)
    return e.occupancy(), e.stats()["inserted_keys"], e.stats()["live_keys"], {k: v.tolist() for k, v in c.items()}


def rec_set(e):
    return {r.tobytes() for r in e.snapshot_records()[1]}


# ---- 1. transplant -----------------------------------------------------------------------------
SHARED = [("sh", "x")]


@functools.lru_cache(maxsize=None)
def transplant_stream(seed):
    """A parity stream across an hour's first second, with one prefix asked under a MINUTE and an
    HOUR rule (one string in the hour's first minute), as batches; and the cut: the first batch
    boundary at or after second 10 of the hour."""
    reqs = make_stream(seed, 3600, t0=H0 - 40)
    for j in range(0, len(reqs), 7):
        dom, descs, rules, ha, t = reqs[j]
        reqs[j] = (dom, descs + [SHARED], rules + [4 + 2 if j % 14 else 8 + 1], ha, t)  # (10, MINUTE) / (3, HOUR)
    sizes = batch_sizes(reqs, np.random.default_rng(seed + 7), 700)
    batches, i, cut = [], 0, None
    for bs in sizes:
        if cut is None and reqs[i][4] >= H0 + 10:
            cut = len(batches)
        batches.append(hiprl.build_batch(reqs[i:i + bs]))
        i += bs
    assert cut and cut < len(batches) - 2 and reqs[-1][4] > H0 + 20
    return batches, cut


def seen_items(batches):
    seen = {}
    for b in batches:
        for i in range(b.n_desc):
            if int(b.rule[i]) != NIL:
                seen.setdefault((b.prefix(i), RULES[int(b.rule[i])][1]), int(b.rule[i]))
    return [(p, r) for (p, _), r in seen.items()]


@pytest.mark.parametrize("local_cache,split,lag", [(False, False, False), (True, False, False), (False, True, False),
                                                   (True, True, False), (True, False, True)])
def test_transplant(local_cache, split, lag):
    batches, cut = transplant_stream(3)
    batches = list(batches)
    t = int(batches[cut].now[0])
    if lag:  # a batch one second behind the one before it
        late = batches[cut + 1]
        late = hiprl.Batch(late.blob, late.off, late.rule, late.req_of,
                           np.full(late.n_req, int(batches[cut].now[-1]) - 1, np.int64), late.hits)
        batches.insert(cut + 1, late)
    o = make_oracle(local_cache, per_second_split=split)
    a = engine(local_cache, log2_slots=BIG_A, per_second_split=split, lag_window=lag)
    streams.assert_same(*run(o, batches[:cut]), *run(a, batches[:cut]), "first half")
    items = seen_items(batches[:cut])
    times = [t] * len(items)
    if lag:  # the strings of the second before, which the late batch asks for
        extra = [(p, r) for p, r in items if RULES[r][1] == hiprl.SECOND]
        items, times = items + extra, times + [t - 1] * len(extra)
    pb = key_batch(items, times)
    v = a.peek(pb)
    assert (v["flags"] & F).sum() >= 40 and (not local_cache or (v["flags"] & LC).sum() >= 10), "guard"
    assert (v["count"] > 1).sum() >= 20 and (not split or (v["flags"] & PS).any())
    b = engine(local_cache, log2_slots=BIG_B, per_second_split=split, lag_window=lag)
    before = b.set(pb, v)
    assert not (before["flags"] & (F | LC)).any()  # a fresh engine: nothing found
    assert np.array_equal(b.peek(pb), v)
    streams.assert_same(*run(o, batches[cut:]), *run(b, batches[cut:]), f"second half {local_cache} {split} {lag}")
    a.close()
    b.close()


# ---- 2. set equals requests ----------------------------------------------------------------------
@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("t,unit", [(1_700_000_007, hiprl.MINUTE), (MAX_NOW, hiprl.DAY)])
def test_set_equals_requests(local_cache, t, unit):
    L = 10
    rules = [(L, unit)]
    div = DIV[unit]
    cs = [1, L - 1, L, L + 1, 2**32 - 2]
    items = [(pfx(f"c{c}"), 0) for c in cs]
    o = make_oracle(local_cache, rules=rules)
    o.submit(hiprl.build_batch([("set", [[("k", f"c{c}")]], [0], c, t) for c in cs]))
    e = engine(local_cache, rules=rules)
    e.set(key_batch(items, t), vals([(c, div, div if local_cache and c > L else 0,
                                      F | (LC if local_cache and c > L else 0)) for c in cs]))
    t2 = min(t + 1, MAX_NOW)
    for now, h in [(t, 1), (t, 1), (t2, 2)]:
        nb = hiprl.build_batch([("set", [[("k", f"c{c}")]], [0], 3 if c == cs[-1] else h, now) for c in cs])
        streams.assert_same(*o.submit(nb), *e.submit(nb), f"after set, now={now} h={h}")
    # the last key wrapped at its first request, as the numeric-edge suite pins it: 2^32 - 2 + 3 -> 1
    rep = e.peek(key_batch(items[-1:], t2))
    assert local_cache or int(rep[0]["count"]) == (2**32 - 2 + 3 * 3) % 2**32
    e.close()


# ---- 3. duplicates and out -----------------------------------------------------------------------
def test_duplicates_last_wins_and_out_is_the_state_before():
    t = H0 + 120
    assert t % 60 == 0
    rules = [(1 << 30, hiprl.SECOND), (1 << 30, hiprl.MINUTE)]
    e = engine(True, rules=rules, per_second_split=True, log2_slots=(8, 11, 7, 6))  # 1021 strings of one minute
    e.submit(hiprl.build_batch([("set", [[("k", "dup")], [("k", "two")], [("k", "two")]], [1, 0, 1], 5, t)]))
    n = 1025
    items = [(pfx(f"f{i}"), 1) for i in range(n)]
    dup_at = [0, 63, 64, n - 1]
    rows = [(i + 1, 30, 0, F) for i in range(n)]
    for k, i in enumerate(dup_at):
        items[i] = (pfx("dup"), 1)
        rows[i] = (1000 + k, 40 + k, 7 + k if k != 2 else 0, F | (LC if k != 2 else 0))
    items[500], rows[500] = (pfx("two"), 0), (77, 0, 0, F)   # SECOND rule: the per-second store
    items[700], rows[700] = (pfx("two"), 1), (88, 33, 0, F)  # MINUTE rule: the main store, same string
    pb, v = key_batch(items, t), vals(rows)
    before = e.peek(pb)
    assert [int(before[i]["count"]) for i in dup_at] == [5] * 4 and int(before[500]["count"]) == 5
    out = e.set(pb, v)
    assert np.array_equal(out, before)
    rep = e.peek(pb)
    last = v[dup_at[-1]]
    for i in dup_at:
        assert rep[i] == last, (i, rep[i], last)
    assert (int(rep[500]["count"]), int(rep[500]["flags"])) == (77, F | PS)
    assert (int(rep[700]["count"]), int(rep[700]["ttl_s"]), int(rep[700]["flags"])) == (88, 33, F)
    others = np.array([i for i in range(n) if i not in dup_at + [500, 700]])
    assert np.array_equal(rep[others], v[others])
    # the cache part: the last descriptor of the string that writes it, here with KEEP_COUNTER
    v2 = v.copy()
    v2[dup_at[-1]] = (0, 0, 99, LC | KC)
    recs = rec_set(e)
    e.set(pb, v, want_out=False)
    assert rec_set(e) == recs, "the same call twice gives the same table"
    e.set(pb, v2)
    rep = e.peek(pb)
    assert (int(rep[0]["count"]), int(rep[0]["ttl_s"]), int(rep[0]["cached_s"])) == (1002, 42, 99)
    e.close()


@pytest.mark.parametrize("n", [1, 65, 257, 1025, 3001])
def test_sizes_with_duplicates_in_one_wave_in_other_waves_and_in_other_blocks(n):
    """n descriptors over 2n/3 + 1 strings: key j recurs at j + distinct, so its duplicate sits in
    the same wave, another wave or another block depending on n. The last value wins, the claims
    are the distinct strings, and the same call again changes nothing."""
    t = 1_700_000_007
    distinct = 2 * n // 3 + 1
    e = engine(True, rules=[(9, hiprl.HOUR)], log2_slots=(4, 4, 12, 4), max_batch_desc=3001)
    pb = key_batch([(pfx(f"z{j % distinct}"), 0) for j in range(n)], t)
    v = vals([(j + 1, 100 + j % 50, (j % 7) * 10, F | (LC if j % 7 else 0)) for j in range(n)])
    ins0 = e.stats()["inserted_keys"]
    assert not e.set(pb, v)["flags"].any()
    want = v[[max(k for k in (j % distinct, j % distinct + distinct) if k < n) for j in range(n)]]
    rep = e.peek(pb)
    assert np.array_equal(rep, want), n
    assert e.stats()["inserted_keys"] - ins0 == distinct == sum(e.occupancy()["live"])
    recs = rec_set(e)
    assert np.array_equal(e.set(pb, v), want) and rec_set(e) == recs
    assert e.stats()["inserted_keys"] - ins0 == distinct
    e.close()


# ---- 4. KEEP bits --------------------------------------------------------------------------------
def test_keep_bits():
    t = 1_700_000_007
    rules = [(3, hiprl.MINUTE)]
    e = engine(True, rules=rules)
    e.submit(hiprl.build_batch([("set", [[("k", "a")], [("k", "b")]], [0, 0], 5, t)]))  # both over: cached
    pb = key_batch([(pfx("a"), 0), (pfx("b"), 0), (pfx("absent"), 0)], t + 1)
    p0 = e.peek(pb)
    assert [int(x) for x in p0["flags"]] == [F | LC, F | LC, 0]
    s0 = state(e, t + 1)
    # both bits: a peek
    out = e.set(pb, vals([(9, 9, 9, F | LC | KC | KF)] * 3))
    assert np.array_equal(out, p0) and np.array_equal(e.peek(pb), p0) and state(e, t + 1) == s0
    # a pure DEL on an absent string claims nothing
    e.set(key_batch([(pfx("absent"), 0)], t + 1), vals([(0, 0, 0, 0)]))
    assert state(e, t + 1) == s0
    # counter only / cache only
    e.set(pb, vals([(2, 50, 0, F | KF), (0, 0, 0, KC), (0, 0, 0, KC | KF)]))
    rep = e.peek(pb)
    assert rep[0] == np.array((2, 50, p0[0]["cached_s"], F | LC), hiprl.PEEK_DTYPE)
    assert rep[1] == np.array((5, p0[1]["ttl_s"], 0, F), hiprl.PEEK_DTYPE)
    assert rep[2] == p0[2] and state(e, t + 1)[:3] == s0[:3]
    # unfrozen, "b" counts again; "a" is still frozen
    st, _ = e.submit(hiprl.build_batch([("set", [[("k", "a")], [("k", "b")]], [0, 0], 1, t + 1)]))
    fl = [int(s["code_flags"]) >> 8 for s in st]
    assert fl[0] & hiprl.FLAG_LOCAL_CACHE_HIT and not fl[1] & hiprl.FLAG_LOCAL_CACHE_HIT
    assert int(e.peek(pb)[1]["count"]) == 6
    e.close()


def test_python_mirror_set():
    t = 1_700_000_007
    c = hiprl.HipRateLimitCache(lambda: t, local_cache=True, log2_slots=SMALL, max_batch_desc=256)
    lim = hiprl.NewRateLimit(5, hiprl.MINUTE, "k", hiprl.StatsStore())
    req = hiprl.NewRateLimitRequest("set", [[("k", "m")], [("k", "nil")]], 1)
    before = c.set(req, [lim, None], vals([(4, 50, 0, F), (9, 9, 9, F)]))
    assert [int(x) for x in before["flags"]] == [0, hiprl.PEEK_NIL] and lim.Stats.TotalHits.Value() == 0
    r = c.DoLimit(req, [lim, None])
    assert (r.DescriptorStatuses[0].Code, r.DescriptorStatuses[0].LimitRemaining) == (hiprl.CODE_OK, 0)
    assert c.DoLimit(req, [lim, None]).DescriptorStatuses[0].Code == hiprl.CODE_OVER_LIMIT  # 6 > 5, and frozen
    before = c.set(req, [lim, None], vals([(0, 0, 0, 0), (0, 0, 0, 0)]), keep_counter=True)  # unfreeze only
    assert (int(before[0]["count"]), int(before[0]["flags"])) == (6, F | LC)
    before = c.set(req, [lim, None], vals([(1, 20, 0, F), (0, 0, 0, 0)]), keep_cache=True)
    assert (int(before[0]["count"]), int(before[0]["flags"])) == (6, F)
    r = c.DoLimit(req, [lim, None])
    assert (r.DescriptorStatuses[0].Code, r.DescriptorStatuses[0].LimitRemaining) == (hiprl.CODE_OK, 3)
    c.engine.close()


# ---- 5. occupancy --------------------------------------------------------------------------------
def home_items(tag, per=9):
    """`per` strings in each of the eight regions: (prefix, rule id, time)."""
    t = 1_700_000_021
    m, h, d = t // 60 * 60, t // 3600 * 3600, t // 86400 * 86400
    out = []
    for u, pair in enumerate([(t, t + 1), (m + 60, m + 120), (h + 3600, h + 4 * 3600), (d + 86400, d + 2 * 86400)]):
        for now in pair:
            out += [(pfx(f"{tag}{u}_{now}_{k}"), u * 4, now + (0 if u == 0 else 1)) for k in range(per)]
    return out


def check_occupancy(e, now):
    occ, c = e.occupancy(), e.census(now)
    assert occ["live"] == c["live"].tolist() and not c["prev"].any(), (occ, c["live"], c["prev"])
    assert e.stats()["live_keys"] == int(c["live"].sum())
    return occ, c


@pytest.mark.parametrize("prefilled", [False, True])
@pytest.mark.parametrize("local_cache,split", [(False, False), (True, True)])
def test_occupancy_and_census(local_cache, split, prefilled):
    e = engine(local_cache, per_second_split=split)
    its = home_items("o")
    n = len(its)
    regions = [oracle.place(t // DIV[RULES[r][1]] * DIV[RULES[r][1]])[0] for _, r, t in its]
    assert sorted(set(regions)) == list(range(8)) and all(regions.count(r) == 9 for r in range(8))
    k = np.arange(n)
    existed = (k % 2 == 0) & prefilled
    if prefilled:  # every other string exists already, by requests (limit 1, one hit: not over)
        for now in sorted({t for _, _, t in its}):
            sel = [(p, r) for j, (p, r, t) in enumerate(its) if t == now and existed[j]]
            e.submit(key_batch(sel, now))
    ins0, now = e.stats()["inserted_keys"], min(t for _, _, t in its)  # every deadline below is ahead of `now`
    occ0, _ = check_occupancy(e, now)
    assert sum(occ0["live"]) == int(existed.sum())
    pb = key_batch([(p, r) for p, r, _ in its], [t for _, _, t in its])
    # thirds: a counter, a cache entry with the counter deleted, a pure DEL
    long = 3 * 86400
    rows = [((j + 1, long, 0, F), (0, 0, long, LC), (0, 0, 0, 0))[j % 3] for j in range(n)]
    before = e.set(pb, vals(rows))
    assert np.array_equal((before["flags"] & F) != 0, existed)
    gets = (k % 3 == 0) | ((k % 3 == 1) & local_cache)
    claims = int((gets & ~existed).sum())
    occ, c = check_occupancy(e, now)
    assert e.stats()["inserted_keys"] - ins0 == claims and sum(occ["live"]) - sum(occ0["live"]) == claims
    for r in range(8):
        in_r = np.array(regions) == r
        assert occ["live"][r] - occ0["live"][r] == int((gets & ~existed & in_r).sum())
        assert occ["gen"][r] == oracle.place(its[int(np.nonzero(in_r)[0][0])][2] // DIV[RULES[r // 2 * 4][1]]
                                             * DIV[RULES[r // 2 * 4][1]])[1]
    rep = e.peek(pb)
    ps = (rep["flags"] & PS) != 0
    found = (rep["flags"] & F) != 0
    assert np.array_equal(found, k % 3 == 0)
    assert np.array_equal((rep["flags"] & LC) != 0, (k % 3 == 1) & local_cache)
    assert ps.any() == split
    assert int(c["keys_main"].sum()) == int((found & ~ps).sum())
    assert int(c["keys_per_second"].sum()) == int((found & ps).sum())
    assert int(c["cached"].sum()) == int(((k % 3 == 1) & local_cache).sum())
    # the result snapshots, restores and resizes like any table
    hdr, recs = e.snapshot_records()
    e2 = engine(local_cache, log2_slots=(9, 9, 9, 9), per_second_split=split)
    e2.restore_records(hdr, recs)
    assert np.array_equal(e2.peek(pb), rep)
    e.resize((9, 9, 8, 7))
    assert np.array_equal(e.peek(pb), rep)
    check_occupancy(e, now)
    e.close()
    e2.close()


# ---- 6. refusals are atomic ----------------------------------------------------------------------
def test_refusals_change_nothing():
    t = 1_700_000_007
    rules = [(5, hiprl.MINUTE), (5, hiprl.SECOND), (5, hiprl.HOUR)]
    # MINUTE-home regions of 16 slots, load limit 12
    e = engine(True, log2_slots=(6, 4, 6, 6), rules=rules, max_load_permille=750, max_batch_desc=64, max_batch_req=64)
    assert e.occupancy()["limit"][2:4] == [12, 12]
    e.submit(hiprl.build_batch([("set", [[("k", "old")], [("k", "sec")]], [2, 1], 9, t)]))  # over: cached too
    watch = key_batch([(pfx("old"), 2), (pfx("sec"), 1)] + [(pfx(f"n{i}"), 0) for i in range(13)], t)
    p0, s0 = e.peek(watch), state(e, t)

    def refused(code, b, v, **kw):
        with pytest.raises(hiprl.RedisError) as ei:
            e.set(b, v, **kw)
        assert ei.value.code == code, ei.value
        assert np.array_equal(e.peek(watch), p0) and state(e, t) == s0, code

    one = key_batch([(pfx("n0"), 0)], t)
    ok = vals([(3, 30, 0, F)])
    refused(EINVAL, one, vals([(3, 0, 0, F)]))                      # FOUND main value without a TTL
    refused(EINVAL, one, vals([(3, 30, 0, F | LC)]))                # LOCAL_CACHED without a deadline
    refused(EINVAL, key_batch([(pfx("n0"), 0)], MAX_NOW), vals([(3, 0x30000, 0, F)]))  # t + ttl_s >= 2^32
    refused(EINVAL, key_batch([(pfx("n0"), 0)], MAX_NOW), vals([(3, 30, 0x30000, F | LC)]))
    refused(EINVAL, key_batch([(pfx("n0"), 0)], MAX_NOW + 1), ok)  # rl_peek's list: the time
    refused(EINVAL, key_batch([(pfx("n0"), 7)], t), ok)            # ... an unknown rule
    refused(EINVAL, key_batch([(pfx("n0"), 0), (pfx("n1"), 0)], [t, t + 120]), vals([ok[0], ok[0]]))  # two generations
    refused(ECAPACITY, key_batch([(pfx(f"x{i}"), 0) for i in range(65)], t), vals([ok[0]] * 65))
    with pytest.raises(hiprl.RedisError) as ei:
        s = hiprl._batch_struct(one)
        e._check(e.lib.rl_set(e.h, hiprl.C.byref(s), None, None), "rl_set")
    assert ei.value.code == EINVAL and state(e, t) == s0
    # a value whose ignored part is malformed is fine: KEEP bits, and the per-second store's TTL
    e.set(one, vals([(3, 0, 0, F | KC | KF)]))
    assert state(e, t) == s0
    # RL_ENOSPC: 13 distinct new strings pass the empty region's limit of 12; 13 descriptors of 12 fit
    new13 = [(pfx(f"n{i}"), 0) for i in range(13)]
    refused(ENOSPC, key_batch(new13, t), vals([ok[0]] * 13))
    out = e.set(key_batch(new13[:12] + new13[:1], t), vals([ok[0]] * 13))
    assert not out["flags"].any() and e.occupancy()["live"][oracle.place(t // 60 * 60)[0]] == 12
    p0, s0 = e.peek(watch), state(e, t)
    assert int((p0["flags"] & F).sum()) == 2 + 12
    refused(ENOSPC, key_batch(new13[12:], t), ok)
    refused(EINVAL, key_batch([(pfx("n0"), 0)], t - 120), ok)  # a window that is over: the region is two on
    e.set(key_batch(new13[12:] + new13[:2], t), vals([(0, 0, 0, 0), (8, 20, 0, F), (0, 0, 0, 0)]))  # no claim: fits
    rep = e.peek(watch)
    assert [int(x) for x in rep["count"][2:5]] == [8, 0, 3] and state(e, t)[:3] == s0[:3]
    # an open snapshot does not block the call; an open restore and a batch in flight do
    p0, s0 = e.peek(watch), state(e, t)
    h = e.snapshot_begin()
    e.set(one, vals([(4, 30, 0, F)]))
    recs = e.snapshot_next(4096)
    e.snapshot_end()
    e.restore_begin(h)
    with pytest.raises(hiprl.RedisError) as ei:
        e.set(one, ok)
    assert ei.value.code == ESTATE
    e.restore_put(recs)
    e.restore_end()
    assert np.array_equal(e.peek(watch), p0)  # the snapshot was the state at its begin
    dev = torch.device("cuda", 0)
    b = hiprl.build_batch([("set", [[("k", "old")]], [2], 1, t)])
    db = router.DeviceBatch.from_host(b, dev)
    d_out = torch.zeros(b.n_desc * 20, dtype=torch.uint8, device=dev)
    d_thr = torch.zeros(b.n_req, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.submit_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), d_out.data_ptr(), d_thr.data_ptr())
    with pytest.raises(hiprl.RedisError) as ei:
        e.set(one, ok)
    assert ei.value.code == ESTATE
    e.wait()
    torch.cuda.synchronize()
    e.close()


# ---- 7. a live engine with a learned hot set -----------------------------------------------------
def test_live_engine_with_hot_set():
    t0 = 1_700_000_007
    L = 40
    rules = [(L, hiprl.MINUTE), (1000, hiprl.HOUR)]
    rng = np.random.default_rng(5)

    def batch(t, n=700):
        reqs = []
        for _ in range(n):
            k = "hot" if rng.random() < 0.6 else f"c{int(rng.integers(0, 50))}"
            reqs.append(("set", [[("k", k)]], [1 if k == "hot" else 0], int(rng.integers(1, 3)), t))
        return hiprl.build_batch(reqs)

    batches = [batch(t0 + j) for j in range(7)]
    o, e = make_oracle(True, rules=rules), engine(True, rules=rules, log2_slots=(8, 10, 10, 6))
    cut = 3
    streams.assert_same(*run(o, batches[:cut]), *run(e, batches[:cut]), "before")
    assert e.stats()["hot_keys"] >= 1, "guard: the dominant key is in the hot set"
    t = t0 + cut
    items = [(pfx("hot"), 1)] + [(pfx(f"c{i}"), 0) for i in range(50)]
    pb = key_batch(items, t)
    v = e.peek(pb)
    assert int(v[0]["count"]) > 500 and (v["flags"] & LC).any()
    assert np.array_equal(e.forget(pb), v) and not e.peek(pb)["flags"].any()
    assert not e.set(pb, v)["flags"].any() and np.array_equal(e.peek(pb), v)
    streams.assert_same(*run(o, batches[cut:cut + 2]), *run(e, batches[cut:cut + 2]), "after forget + set")
    # only the hot key: the rest of the stream is an oracle's whose hot key got c in one request
    t, c = t0 + cut + 2, 990
    e.set(key_batch(items[:1], t), vals([(c, 3000, 0, F)]))  # and out of the local cache
    o2 = make_oracle(True, rules=rules)
    o2.submit(hiprl.build_batch([("set", [[("k", "hot")]], [1], c, t)]))
    hot_only = [hiprl.build_batch([("set", [[("k", "hot")]], [1], 1 + j % 2, t + j // 300) for j in range(600)])]
    st_e, thr_e = run(e, hot_only)
    streams.assert_same(*run(o2, hot_only), st_e, thr_e, "hot key after a counter-only set")
    assert (st_e["code_flags"] & 0xFF == hiprl.CODE_OVER_LIMIT).sum() > 100 and (st_e["code_flags"] & 0xFF == hiprl.CODE_OK).sum() > 5
    e.close()


# ---- 8. import -----------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_import_from_a_redis_dump(split):
    reqs = make_stream(11, 3000, t0=H0 - 30, dt_max=1)
    times = sorted({r[4] for r in reqs})
    batches = []  # single-time batches, two per second
    for t in times:
        at = [r for r in reqs if r[4] == t]
        batches += [hiprl.build_batch(at[:len(at) // 2 + 1]), hiprl.build_batch(at[len(at) // 2 + 1:])]
    batches = [b for b in batches if b.n_req]
    cut = next(j for j in range(len(batches) // 2, len(batches)) if batches[j - 1].now[0] == batches[j].now[0])
    o = make_oracle(False, per_second_split=split)
    clock = {"t": 0}
    main, ps = resp.RespStore(lambda: clock["t"]), resp.RespStore(lambda: clock["t"])
    first = []
    for b in batches[:cut]:
        clock["t"] = int(b.now[0])
        st, thr = o.submit(b)
        resp.replay_local(main, ps, b, RULES, st, split)
        first.append((st, thr))
    t = int(batches[cut].now[0])
    unit_rule = {u: k * 4 for k, u in enumerate(streams.UNITS)}
    e = engine(False, per_second_split=split, log2_slots=BIG_B)
    n_set = 0
    for store, is_ps in ((main, False), (ps, True)):
        ib, iv, skipped = resp.import_batch(store.dump(t), t, unit_rule, per_second=is_ps)
        assert is_ps or ib.n_desc >= 50
        assert (ib.n_desc > 0) == (not is_ps or split)
        if ib.n_desc:
            e.set(ib, iv)
            rep = e.peek(ib)
            assert np.array_equal(rep["count"], iv["count"]) and bool(((rep["flags"] & PS) != 0).all()) == is_ps
        n_set += ib.n_desc
    assert e.stats()["inserted_keys"] <= n_set
    streams.assert_same(*run(o, batches[cut:]), *run(e, batches[cut:]), f"after the import, split={split}")
    e.close()
