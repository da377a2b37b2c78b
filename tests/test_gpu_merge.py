"""rl_merge (rl_hip.h "Merge") on the GPU: the records of a snapshot folded into a live table.
Consolidating a routed deployment's per-rank snapshots, and merging a second engine's counters of
the same keys, continue a request stream bit-exactly as one oracle that saw the whole history;
every word of the table afterwards equals a dict model of the fold (tests/merge_model.py); every
refusal leaves the engine byte-identical."""
import functools

import numpy as np
import pytest
import torch

import hiprl
import oracle
import router
import routing
import streams
from merge_model import FIELDS, TableModel, ident, sorted_set
from streams import RULES
from test_gpu_peek import check_against_oracle, key_batch, retimed
from test_gpu_snapshot import cat, expected, run, stream

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC, ECAPACITY, ESTATE = -1, -3, -4, -5
MAX_DESC = 1 << 14
MAX_NOW = 0xFFFD0000
M32 = 0xFFFFFFFF
DEV = torch.device("cuda", 0)
T0 = 1_700_000_000  # an HOUR window holds it well inside: T0 % 3600 == 800
OLD = T0 - 7200      # two HOUR windows earlier: the same HOUR-home region (neither window starts a day)


def engine(local_cache=False, pipeline="v4", log2_slots=(16, 16, 16, 14), rules=RULES, **kw):
    kw.setdefault("max_batch_desc", MAX_DESC)
    e = hiprl.Engine(local_cache=local_cache, pipeline=pipeline, log2_slots=log2_slots, **kw)
    e.load_rules(rules)
    return e


def add(total, rep):
    for f in FIELDS:
        total[f] = total.get(f, 0) + rep[f]
    return total


def frozen(e):
    """Everything a refusal must leave as it was: the records, the header, occupancy, stats."""
    h, recs = e.snapshot_records()
    return sorted_set(recs).tobytes(), bytes(h), e.occupancy(), e.stats()


def check_table(e, model, now, ctx):
    """Every word: the engine's live records equal the model's; the census, the occupancy and a
    snapshot header agree on the live and previous-generation counts."""
    h, recs = e.snapshot_records()
    want = model.records()
    got = sorted_set(recs)
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    assert np.array_equal(got, want), (ctx, got[got != want][:3], want[got != want][:3])
    live, prev = model.counts()
    occ = e.occupancy()
    cen = e.census(now)
    assert list(h.gen) == occ["gen"] == model.gen, (ctx, list(h.gen), occ["gen"], model.gen)
    assert list(h.live) == live and list(h.prev) == prev, (ctx, list(h.live), live, list(h.prev), prev)
    assert occ["live"] == live, (ctx, occ["live"], live)  # times only move forward here: the mirror is exact
    assert [int(x) for x in cen["live"]] == live and [int(x) for x in cen["prev"]] == prev, (ctx, cen)
    assert e.stats()["live_keys"] == sum(live)


def merged(e, model, h, recs, now, chunk, ctx):
    """merge_records on the engine and the model, chunk by chunk; the summed report, which must be
    the model's and account for every record."""
    rep = e.merge_records(h, recs, now, chunk=chunk)
    want = {}
    for i in range(0, max(1, recs.shape[0]), chunk):
        add(want, model.merge(recs[i:i + chunk], now))
    assert rep == want, (ctx, rep, want)
    assert rep["records"] == recs.shape[0] == sum(rep[f] for f in FIELDS[1:]), (ctx, rep)
    return rep


def key_reqs(keys, rule, hits, t, dom="mrg"):
    return [(dom, [[("k", k)]], [rule], hits, t) for k in keys]


def keys_engine(keys, t, rules, hits=2, **kw):
    """An engine that has counted `keys` once each at time t (in batches of at most 64)."""
    e = engine(rules=rules, **kw)
    for j in range(0, len(keys), 64):
        e.submit(hiprl.build_batch(key_reqs(keys[j:j + 64], 0, hits, t)))
    return e


# ---- 1. consolidation of a routed deployment -------------------------------------------------
@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_consolidation_of_three_shards(seed, local_cache):
    """Three lag-window engines behind an emulated router decide the first half; their snapshots
    go into one fresh lone engine, which decides the second half as the whole-stream oracle."""
    batches, cut = stream(seed)
    want = cat(expected(seed, local_cache)[cut:])
    G = 3
    shards = []
    for g in range(G):
        e = engine(local_cache, lag_window=True)
        shards.append(router.EngineShard(e, g, G, DEV, MAX_DESC))
    empty = hiprl.build_batch([])
    for i, b in enumerate(batches[:cut]):
        row = [empty] * G
        row[i % G] = b  # rank order is arrival order: one origin per step
        routing.exchange_local(shards, [router.DeviceBatch.from_host(x, DEV) for x in row])
    torch.cuda.synchronize()
    now = int(batches[cut].now[0])
    target = engine(local_cache)
    model = TableModel(lag=False, local_cache=local_cache)
    total, n_recs, idents = {}, 0, set()
    for g, sh in enumerate(shards):
        h, recs = sh.eng.snapshot_records()
        assert h.flags & hiprl.SNAP_LAG and recs.shape[0] > 100
        idents |= {(int(c), int(k)) for c, k in zip(recs["ctrl"], recs["key"])}
        n_recs += recs.shape[0]
        add(total, merged(target, model, h, recs, now, 1000, f"seed={seed} shard={g}"))
    assert len(idents) == n_recs  # the owners' key sets are disjoint
    assert total["records"] == n_recs and total["folded"] == 0 and total["claimed"] > 300, total
    assert target.stats()["inserted_keys"] == total["claimed"]
    check_table(target, model, now, f"seed={seed} local={local_cache}")
    got = run(target, batches[cut:])
    streams.assert_same(want[0], want[1], got[0], got[1], f"consolidated seed={seed} local={local_cache}")


# ---- 2. the same keys on both sides -----------------------------------------------------------
def last_touch(batches):
    """(prefix, window start) -> time of the last INCRBY, over the non-nil descriptors."""
    last = {}
    for b in batches:
        for i in range(b.n_desc):
            r = int(b.rule[i])
            if r == hiprl.NIL_RULE:
                continue
            t = int(b.now[b.req_of[i]])
            div = hiprl.UNIT_DIVIDER[RULES[r][1]]
            k = (b.prefix(i), t // div * div)
            last[k] = max(last.get(k, 0), t)
    return last


@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
@pytest.mark.parametrize("split", [False, True])
def test_same_keys_on_both_sides(split, pipeline):
    """make_stream counts every string under one unit, without jitter: the sum is exact. A and B
    take the even and odd batches of the first half; B merged into A answers every peek as the
    oracle's GET and decides the second half as the whole-stream oracle."""
    seed = 1
    batches, cut = stream(seed)
    o = oracle.Oracle(per_second_split=split)
    o.load_rules(RULES)
    for b in batches[:cut]:
        o.submit(b)
    a, bb = (engine(pipeline=pipeline, per_second_split=split) for _ in range(2))
    for i, b in enumerate(batches[:cut]):
        (a if i % 2 == 0 else bb).submit(b)
    now = int(batches[cut].now[0])
    model = TableModel.of(a)
    h, recs = bb.snapshot_records()
    assert bool(h.flags & hiprl.SNAP_SPLIT) == split
    rep = merged(a, model, h, recs, now, MAX_DESC, f"split={split}")
    assert rep["folded"] > 50 and rep["claimed"] > 50, rep
    check_table(a, model, now, f"same keys split={split} {pipeline}")
    last = last_touch(batches[:cut])
    found = exact = 0
    for b in batches[:cut]:
        pb = retimed(b, now)
        got = a.peek(pb)
        found += check_against_oracle(got, pb, o, split=split, ctx=f"peek split={split}")[0]
        for i in range(pb.n_desc):  # the TTL too: no jitter, so EXPIRE of the last INCRBY on either side
            r = int(pb.rule[i])
            if r == hiprl.NIL_RULE or not int(got[i]["flags"]) & hiprl.PEEK_FOUND:
                continue
            unit = RULES[r][1]
            if split and unit == hiprl.SECOND:
                continue
            div = hiprl.UNIT_DIVIDER[unit]
            assert int(got[i]["ttl_s"]) == last[(pb.prefix(i), now // div * div)] + div - now, (i, got[i])
            exact += 1
    assert found > 500 and exact > 300, (found, exact)
    want = [o.submit(b) for b in batches[cut:]]
    f = oracle.Oracle(per_second_split=split)
    f.load_rules(RULES)
    fresh = run(f, batches[cut:])
    assert (fresh[0] != cat(want)[0]).sum() > 100, "the cut carries no state"
    got = run(a, batches[cut:])
    streams.assert_same(*cat(want), *got, f"merged split={split} {pipeline}")


# ---- 4. online ----------------------------------------------------------------------------------
def test_online_merge_between_batches():
    """B's records arrive a chunk after each of A's second-half batches, at that batch's last
    time: after every chunk the table equals the model of the fold at that time, and the final
    peeks answer from it."""
    batches, cut = stream(2)
    a, bb = engine(True), engine(True)
    for i, b in enumerate(batches[:cut]):
        (a if i % 2 == 0 else bb).submit(b)
    h, recs = bb.snapshot_records()
    rest = batches[cut:]
    per = -(-recs.shape[0] // len(rest))
    total, now = {}, 0
    for j, b in enumerate(rest):
        a.submit(b)
        now = int(b.now[-1])
        part = recs[j * per:(j + 1) * per]
        model = TableModel.of(a, local_cache=True)
        add(total, merged(a, model, h, part, now, MAX_DESC, f"chunk {j}"))
        check_table(a, model, now, f"online chunk {j}")
    assert total["records"] == recs.shape[0] and total["folded"] > 20 and total["claimed"] > 20, total
    model = TableModel.of(a, local_cache=True)
    seen = 0
    for b in rest[-2:]:
        pb = retimed(b, now)
        got = a.peek(pb)
        for i in range(pb.n_desc):
            r = int(pb.rule[i])
            if r == hiprl.NIL_RULE:
                continue
            st = model.slots.get(ident(pb.prefix(i), RULES[r][1], now), [0, 0, 0, 0])
            alive, cached = now < st[1], now < st[3]
            want = (st[0] if alive else 0, st[1] - now if alive else 0, st[3] - now if cached else 0,
                    (hiprl.PEEK_FOUND if alive else 0) | (hiprl.PEEK_LOCAL_CACHED if cached else 0))
            assert tuple(int(x) for x in got[i]) == want, (i, got[i], want)
            seen += alive
    assert seen > 100


def test_merge_needs_an_idle_engine():
    src = keys_engine([f"s{i}" for i in range(40)], T0, [(5, hiprl.HOUR)])
    h, recs = src.snapshot_records()
    e = keys_engine([f"s{i}" for i in range(20, 70)], T0, [(5, hiprl.HOUR)])
    before = frozen(e)

    def refused():
        with pytest.raises(hiprl.RedisError) as ei:
            e.merge_chunk(h, recs, T0)
        assert ei.value.code == ESTATE, ei.value

    nil = hiprl.build_batch([("mrg", [[("k", "x")]], [hiprl.NIL_RULE], 1, T0)])  # decides without the table
    e.submit_host_async(nil)
    refused()
    e.wait_into(nil.n_desc, nil.n_req)
    after = frozen(e)
    assert after[:3] == before[:3] and after[3]["inserted_keys"] == before[3]["inserted_keys"]
    e.set_routed_plan(0, 0, 0)  # an empty plan is open
    refused()
    e.set_routed_commit(False)
    assert frozen(e) == after
    e.snapshot_begin()  # an open snapshot does not block
    rep = e.merge_chunk(h, recs, T0)
    e.snapshot_end()
    assert (rep["folded"], rep["claimed"]) == (20, 20), rep
    other = engine(rules=[(5, hiprl.HOUR)])
    other.restore_begin(h)
    with pytest.raises(hiprl.RedisError) as ei:
        other.merge_chunk(h, recs, T0)
    assert ei.value.code == ESTATE, ei.value
    other.restore_put(recs)
    other.restore_end()
    assert np.array_equal(sorted_set(other.snapshot_records()[1]), sorted_set(recs))


# ---- 5. exact capacity ---------------------------------------------------------------------------
def test_capacity_is_counted_exactly():
    """Regions of 256 slots (limit 192). 100 keys held, 100 merged of which 50 are present: 150
    live, where a count of every record as a claim would have refused. 50 more are refused with
    nothing changed, and fit after a resize."""
    rules = [(3, hiprl.HOUR)]
    assert oracle.place(T0 // 3600 * 3600)[0] == 4
    small = dict(log2_slots=(8, 8, 8, 8), max_batch_desc=256)
    t = keys_engine([f"k{i}" for i in range(100)], T0, rules, **small)
    s1 = keys_engine([f"k{i}" for i in range(50, 150)], T0 + 5, rules, hits=1)
    s2 = keys_engine([f"k{i}" for i in range(150, 200)], T0 + 9, rules)
    model = TableModel.of(t)
    rep = merged(t, model, *s1.snapshot_records(), T0 + 10, 256, "k50..k149")
    assert (rep["folded"], rep["claimed"]) == (50, 50), rep
    occ = t.occupancy()
    assert occ["live"][4] == 150 and occ["limit"][4] == 192 and occ["slots"][4] == 256, occ
    check_table(t, model, T0 + 10, "150 live")
    h2, r2 = s2.snapshot_records()
    before = frozen(t)
    with pytest.raises(hiprl.RedisError) as ei:
        t.merge_chunk(h2, r2, T0 + 10)
    assert ei.value.code == ENOSPC, ei.value
    assert frozen(t) == before
    with pytest.raises(hiprl.MergeRefused) as ei:  # the chunked form says how far it came: 180 fit, 200 do not
        t.merge_records(h2, r2, T0 + 10, chunk=30)
    assert ei.value.code == ENOSPC and ei.value.merged == 30 and ei.value.report["claimed"] == 30, ei.value
    model.merge(r2[:30], T0 + 10)
    check_table(t, model, T0 + 10, "30 of the refused set")
    t.resize((0, 0, 9, 0))
    rep = merged(t, model, h2, r2[30:], T0 + 10, 256, "k180..k199 after the resize")
    assert rep["claimed"] == 20 and t.occupancy()["live"][4] == 200
    check_table(t, model, T0 + 10, "after the resize")
    # the merged table decides on as one oracle that saw all three histories
    o = oracle.Oracle()
    o.load_rules(rules)
    for keys, tm, hits in ((range(100), T0, 2), (range(50, 150), T0 + 5, 1), (range(150, 200), T0 + 9, 2)):
        o.submit(hiprl.build_batch(key_reqs([f"k{i}" for i in keys], 0, hits, tm)))
    nxt = [hiprl.build_batch(key_reqs([f"k{i}" for i in range(j, j + 50)], 0, 1, T0 + 11)) for j in range(0, 200, 50)]
    streams.assert_same(*run(o, nxt), *run(t, nxt), "after the merges")


def test_tight_region_with_probe_wrap():
    """180 records into a 256-slot region: long probe chains, some past the region's end."""
    rules = [(3, hiprl.HOUR)]
    keys = [f"w{i}" for i in range(180)]
    src = keys_engine(keys, T0, rules)
    h, recs = src.snapshot_records()
    assert recs.shape[0] == 180
    t = engine(rules=rules, log2_slots=(8, 8, 8, 8), max_batch_desc=256)
    model = TableModel()
    rep = merged(t, model, h, recs, T0, 256, "tight")
    assert rep["claimed"] == 180
    check_table(t, model, T0, "tight")
    # (a batch's capacity check counts every descriptor as a possible claim: 180 + 10 <= 192)
    batches = [hiprl.build_batch(key_reqs(keys[j:j + 10], 0, 2, T0 + 1)) for j in range(0, 180, 10)]
    streams.assert_same(*run(src, batches), *run(t, batches), "tight: decided on")
    assert t.stats()["inserted_keys"] == 180  # every key found its merged slot


# ---- 6. generations ------------------------------------------------------------------------------
def test_newer_snapshot_advances_the_region():
    rules = [(5, hiprl.HOUR)]
    old = [f"a{i}" for i in range(30)]
    new = [f"b{i}" for i in range(20)] + old[:5]
    t = keys_engine(old, OLD, rules)
    src = keys_engine(new, T0, rules)
    h, recs = src.snapshot_records()
    model = TableModel.of(t)
    now = T0
    rep = merged(t, model, h, recs, now, 256, "newer")
    assert rep["claimed"] == 25 and rep["folded"] == 0, rep
    region, gen = oracle.place(now // 3600 * 3600)
    occ = t.occupancy()
    assert region == 4 and occ["gen"][4] == gen and occ["live"][4] == 25, occ
    cen = t.census(now)
    assert int(cen["stale"][4]) == 30 and int(cen["live"][4]) == 25, cen
    check_table(t, model, now, "newer")
    o = oracle.Oracle()
    o.load_rules(rules)
    o.submit(hiprl.build_batch(key_reqs(new, 0, 2, now)))
    nxt = [hiprl.build_batch(key_reqs(new + old, 0, 2, now + 1))]
    streams.assert_same(*run(o, nxt), *run(t, nxt), "after the advance")


def test_older_snapshot_is_dropped():
    rules = [(5, hiprl.HOUR)]
    t = keys_engine([f"b{i}" for i in range(20)], T0, rules)
    src = keys_engine([f"a{i}" for i in range(30)] + ["b1"], OLD, rules)
    h, recs = src.snapshot_records()
    before = frozen(t)
    rep = t.merge_chunk(h, recs, T0)
    assert rep == dict(records=31, folded=0, claimed=0, dropped_over=31, dropped_empty=0)
    assert frozen(t) == before


def lag_source():
    """SECOND keys at t (30) and t + 2 (60) in a lag-window engine: newest and previous generation."""
    t = T0 + 1
    rules = [(5, hiprl.SECOND)]
    src = engine(rules=rules, lag_window=True, log2_slots=(8, 8, 8, 8), max_batch_desc=256)
    src.submit(hiprl.build_batch(key_reqs([f"a{i}" for i in range(30)], 0, 1, t)))
    src.submit(hiprl.build_batch(key_reqs([f"b{i}" for i in range(60)], 0, 2, t + 2)))
    h, recs = src.snapshot_records()
    r = t % 2
    assert list(h.live)[r] == 60 and list(h.prev)[r] == 30 and recs.shape[0] == 90
    return rules, t, r, h, recs


def test_lag_window_classes():
    rules, t, r, h, recs = lag_source()
    # both generations still hold something at t (a SECOND counter lives one second)
    lagged = engine(rules=rules, lag_window=True, log2_slots=(9, 8, 8, 8), max_batch_desc=256)
    model = TableModel(lag=True)
    rep = merged(lagged, model, h, recs, t, 256, "lag into lag")
    assert rep["claimed"] == 90, rep
    h2, _ = lagged.snapshot_records()
    assert list(h2.live) == list(h.live) and list(h2.prev) == list(h.prev) and list(h2.gen) == list(h.gen)
    check_table(lagged, model, t, "lag into lag")
    # in two calls, the previous generation after the newest: it lands behind the region's generation
    twice = engine(rules=rules, lag_window=True, log2_slots=(8, 8, 8, 8), max_batch_desc=256)
    model = TableModel(lag=True)
    newest = (recs["ctrl"] & np.uint64(M32)) == np.uint64(list(h.gen)[r])
    assert merged(twice, model, h, recs[newest], t, 256, "newest")["claimed"] == 60
    assert merged(twice, model, h, recs[~newest], t, 256, "previous")["claimed"] == 30
    check_table(twice, model, t, "lag in two calls")
    lone = engine(rules=rules, log2_slots=(8, 8, 8, 8), max_batch_desc=256)
    model = TableModel(lag=False)
    rep = merged(lone, model, h, recs, t, 256, "lag into lone")
    assert (rep["claimed"], rep["dropped_over"]) == (60, 30), rep
    check_table(lone, model, t, "lag into lone")


def test_untouched_engine_claims_everything():
    batches, cut = stream(3)
    src = engine(True)
    run(src, batches[:cut])
    h, recs = src.snapshot_records()
    now = int(batches[0].now[0])  # the stream's first second: every counter of it is still alive
    t = engine(True, log2_slots=(15, 14, 15, 14))
    assert t.occupancy()["gen"] == [0] * 8
    model = TableModel(local_cache=True)
    rep = merged(t, model, h, recs, now, 777, "untouched")
    assert rep["claimed"] == recs.shape[0] > 300, rep
    check_table(t, model, now, "untouched")


def test_dead_records_are_dropped_empty():
    rules = [(5, hiprl.HOUR)]
    keys = [f"d{i}" for i in range(40)]
    src = keys_engine(keys, T0, rules, local_cache=True)
    h, recs = src.snapshot_records()
    assert int(recs["exp"].max()) == T0 + 3600 and int(recs["pcount"].max()) == 0
    dead = T0 + 3600  # every counter has expired and nothing is cached (5 is not passed by 2 hits)
    present = keys_engine(keys[:25] + ["other"], T0, rules, local_cache=True)
    before = frozen(present)
    rep = present.merge_chunk(h, recs, dead)
    assert rep == dict(records=40, folded=0, claimed=0, dropped_over=0, dropped_empty=40), rep
    assert frozen(present) == before
    rep = present.merge_chunk(h, recs, dead - 1)  # one second earlier they all count
    assert (rep["folded"], rep["claimed"]) == (25, 15), rep


# ---- 7. shapes -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_source():
    rules = [(5, hiprl.MINUTE), (5, hiprl.HOUR), (5, hiprl.DAY)]
    e = engine(rules=rules)
    reqs = [("shape", [[("k", str(i))]], [i % 3], 1 + i % 4, T0 + 17) for i in range(1100)]
    e.submit(hiprl.build_batch(reqs))
    h, recs = e.snapshot_records()
    assert recs.shape[0] == 1100
    return rules, h, recs


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_every_prefix_length(n):
    rules, h, recs = shape_source()
    t = engine(rules=rules, log2_slots=(12, 12, 12, 12), max_batch_desc=2048)
    model = TableModel()
    rep = merged(t, model, h, recs[:n], T0 + 20, 2048, f"n={n}")
    assert rep["claimed"] == n
    check_table(t, model, T0 + 20, f"n={n}")


# ---- 8. refusals ---------------------------------------------------------------------------------
def clone(h):
    return hiprl.RlSnapshotHeader.from_buffer_copy(bytes(h))


def test_refusals_change_nothing():
    rules = [(5, hiprl.HOUR)]
    src = keys_engine([f"r{i}" for i in range(60)], T0, rules)
    h, recs = src.snapshot_records()
    t = keys_engine([f"r{i}" for i in range(30, 90)], T0, rules, max_batch_desc=256)
    before = frozen(t)

    def refused(code, hdr, r, now=T0 + 1):
        with pytest.raises(hiprl.RedisError) as ei:
            t.merge_chunk(hdr, r, now)
        assert ei.value.code == code, ei.value
        assert frozen(t) == before, ei.value

    bad = clone(h)
    bad.magic[7] = ord("2")
    refused(EINVAL, bad, recs)
    for field, v in (("header_bytes", 128), ("record_bytes", 64), ("reserved0", 1)):
        bad = clone(h)
        setattr(bad, field, v)
        refused(EINVAL, bad, recs)
    bad = clone(h)
    bad.reserved[21] = 7
    refused(EINVAL, bad, recs)
    bad = clone(h)
    bad.seed_check ^= 1  # a foreign seed
    refused(EINVAL, bad, recs)
    bad = clone(h)
    bad.flags ^= hiprl.SNAP_SPLIT
    refused(EINVAL, bad, recs)
    refused(EINVAL, bad, recs[:0])  # the header is validated with n == 0 too
    r = recs.copy()
    r["ctrl"][7] &= np.uint64(~M32 & 0xFFFFFFFFFFFFFFFF)  # generation 0
    refused(EINVAL, h, r)
    r = recs.copy()
    r["ctrl"][59] += np.uint64(1)  # the generation's parity is the other region's
    refused(EINVAL, h, r)
    r = recs.copy()
    g = 60 * 472222 + 1  # a MINUTE-home region, but this window start is an hour boundary: an HOUR-home string
    assert (g - 1) * 60 % 3600 == 0 and oracle.place((g - 1) * 60)[0] >= 4
    r["ctrl"][0] = np.uint64(g | (0xABCD << 32))
    r["key"][0] = np.uint64((2 << 61) | (int(r["key"][0]) & ((1 << 61) - 1)))
    refused(EINVAL, h, r)
    refused(EINVAL, h, recs, now=-1)
    refused(EINVAL, h, recs, now=MAX_NOW + 1)
    many = np.tile(recs, 5)[:257]
    refused(ECAPACITY, h, many)
    r = recs.copy()
    r[41] = r[3]  # one identity twice in a call
    refused(EINVAL, h, r)
    r = recs.copy()
    r[1] = r[0]  # neighbours in one wave
    refused(EINVAL, h, r[:2])
    # the empty call with a good header is fine and reports zeros
    assert t.merge_chunk(h, recs[:0], T0 + 1) == dict.fromkeys(FIELDS, 0)
    assert frozen(t) == before
    # the same chunk in two calls adds twice: a caller must not repeat an applied chunk
    model = TableModel.of(t)
    assert merged(t, model, h, recs, T0 + 1, 256, "once")["folded"] == 30
    assert merged(t, model, h, recs, T0 + 1, 256, "twice")["folded"] == 60
    check_table(t, model, T0 + 1, "twice")
    pk = t.peek(key_batch([(hiprl.cache_key_prefix("mrg", [("k", "r40")]), 0)], T0 + 1))
    assert int(pk[0]["count"]) == 2 + 2 + 2
