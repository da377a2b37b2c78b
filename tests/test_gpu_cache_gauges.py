"""The table census (rl_census) and the local-cache lookup counters (rl_cache_stats_*) on the GPU
(rl_hip.h "Local-cache gauges and the table census").

Census: the expected report is made by enumerating every key string a stream produced
(rlo_cache_key), placing it (rlo_place) and asking the oracle about it at `now`:
  keys_main        rlo_counter(string, now) >= 0 on the main store
  count_log2       the bit length of that counter mod 2^32
  cached           rlo_local_cached(string, now)
  live             the strings of a region's newest window generation by rlo_place (lag regions:
                   prev = the generation two before it), also against rl_snapshot_begin's header
  keys_per_second  the table keeps no TTL for the per-second store, and the census counts slots
                   with a non-zero per-second counter (rl_peek's predicate): the expected value
                   is rlo_counter(string, per-second store, expiry ignored) >= 0 over the strings
                   that are live by rlo_place
  cache_expired    strings live by rlo_place that the oracle's cache holds (rlo_local_cached at
                   time 0) and that are no longer cached at `now`
Lookup counters: numpy over synthetic statuses; the reference-pinned hitCount / missCount of
tests/golden/local_cache_gauges.json on the integration stream; the oracle's statuses."""
import ctypes as C
import functools
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import hiprl
import oracle
import router
import routing
import streams
from streams import RULES, batch_sizes, make_stream

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC, ESTATE = -1, -3, -5
NIL = hiprl.NIL_RULE
DEV = torch.device("cuda", 0)
ROOT = Path(__file__).resolve().parents[1]
OFFSETS = (0, 1, 61, 3601)
PER_REGION = hiprl.CENSUS_REGION_FIELDS[1:]


def raises(code, fn, *a, **kw):
    with pytest.raises(hiprl.RedisError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value


# ---- the expected census ------------------------------------------------------------------------
def key_strings(reqs, rules):
    """{key string: window start} of every descriptor with a limit."""
    out = {}
    for dom, descs, rids, _, now in reqs:
        for entries, rid in zip(descs, rids):
            if rid == NIL:
                continue
            unit = rules[rid][1]
            div = hiprl.UNIT_DIVIDER[unit]
            out[oracle.cache_key(hiprl.cache_key_prefix(dom, entries), unit, now)] = now // div * div
    return out


def expected_census(o, strings, now, log2_slots, local_cache, split, lag=False):
    """(report, edges): the report the census must give, and whether a main-store expiry and a
    local-cache deadline fall exactly on `now`."""
    rep = {f: np.zeros(8, np.uint64) for f in hiprl.CENSUS_REGION_FIELDS}
    rep["count_log2"] = np.zeros(hiprl.CENSUS_LOG2_BINS, np.uint64)
    for r in range(8):
        rep["slots"][r] = 1 << log2_slots[r // 2]
    placed = {s: oracle.place(ws) for s, ws in strings.items()}
    newest = [0] * 8
    for r, g in placed.values():
        newest[r] = max(newest[r], g)
    older = np.zeros(8, np.uint64)
    exp_edge = frz_edge = False
    for s, (r, g) in placed.items():
        cls = 0 if g == newest[r] else 1 if lag and r < 2 and g + 2 == newest[r] else 2
        if cls == 2:
            older[r] += 1
        else:
            rep["live" if cls == 0 else "prev"][r] += 1
        c = o.counter(s, now)
        if c >= 0:
            assert cls < 2, ("a key Redis still holds sits in a superseded slot (the documented limit)", s, now)
            rep["keys_main"][r] += 1
            rep["count_log2"][int(c % (1 << 32)).bit_length()] += 1
        elif now > 0 and o.counter(s, now - 1) >= 0:
            exp_edge = True
        if split and cls < 2 and o.counter(s, None, per_second=True) >= 0:
            rep["keys_per_second"][r] += 1
        if local_cache:
            if o.local_cached(s, now):
                assert cls < 2, (s, now)
                rep["cached"][r] += 1
            elif cls < 2 and o.local_cached(s, 0):
                rep["cache_expired"][r] += 1
                frz_edge = frz_edge or o.local_cached(s, now - 1)
    return rep, older, (exp_edge, frz_edge)


def assert_report(got, want, older, ctx):
    for f in ("slots", "live", "prev", "keys_main", "keys_per_second", "cached", "cache_expired", "count_log2"):
        assert np.array_equal(got[f], want[f]), (ctx, f, got[f].tolist(), want[f].tolist())
    # claimed and not live: superseded strings' slots, less the ones a newer string took over
    assert np.all(got["stale"] <= older), (ctx, got["stale"].tolist(), older.tolist())
    assert np.all(got["live"] + got["prev"] + got["stale"] <= got["slots"]), ctx
    assert int(got["count_log2"].sum()) == int(got["keys_main"].sum()), ctx


def assert_matches_header(e, rep, ctx):
    h = e.snapshot_begin()
    e.snapshot_end()
    assert rep["live"].tolist() == list(h.live) and rep["prev"].tolist() == list(h.prev), (ctx, rep["live"], list(h.live))


def same_reports(a, b):
    return all(np.array_equal(a[f], b[f]) for f in a)


@functools.lru_cache(maxsize=None)
def big_stream():
    """4000 requests from 65 s before an hour boundary: the batches cross SECOND, MINUTE and HOUR
    rollovers. The last batch is kept back: it is submitted after the censuses."""
    t0 = 472_222 * 3600 - 65
    reqs = make_stream(21, 4000, t0=t0)
    times = [r[4] for r in reqs]
    assert times == sorted(times) and times[0] // 3600 != times[-1] // 3600 and times[-1] - times[0] > 70
    sizes = batch_sizes(reqs, np.random.default_rng(3), 1000)
    cuts = np.cumsum([0] + sizes)
    return reqs, [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


def tiny_stream():
    """Eight keys, two per unit, limits 1 and 3, from 2 s before an hour boundary to 2 s past it:
    at most four strings per table region and generation (a 16-slot region's load limit is 12)."""
    t0 = 472_300 * 3600 - 2
    reqs = []
    for t in range(t0, t0 + 5):
        for j in range(8):
            reqs.append(("tiny", [[("k", str(j))]], [(j % 4) * 4 + (1 if j >= 4 else 0)], 1 + j % 2, t))
        reqs.append(("tiny", [[("k", "0")], [("n", "il")]], [0, NIL], 2, t))
    return reqs


def check_census(reqs, cuts, log2_slots, local_cache, split, lag=False, rules=RULES, need_exp_edge=True):
    """Submit all batches but the last, take the census at the four times against the oracle, then
    submit the last batch: bit-exact against the oracle, the census changed nothing."""
    e = hiprl.Engine(local_cache=local_cache, per_second_split=split, log2_slots=log2_slots, lag_window=lag,
                     max_batch_desc=1 << 13)
    o = oracle.Oracle(local_cache=local_cache, per_second_split=split)
    for x in (e, o):
        x.load_rules(rules)
    for a, b in cuts[:-1]:
        hb = hiprl.build_batch(reqs[a:b])
        streams.assert_same(*e.submit(hb), *o.submit(hb), ctx="before the census")
    done = reqs[:cuts[-2][1]]
    newest = done[-1][4]
    strings = key_strings(done, rules)
    ctx = f"log2={log2_slots} cache={local_cache} split={split} lag={lag}"
    before = (e.occupancy(), e.stats())
    edges = [False, False]
    reports = []
    for off in OFFSETS:
        want, older, ed = expected_census(o, strings, newest + off, log2_slots, local_cache, split, lag)
        got = e.census(newest + off)
        assert_report(got, want, older, f"{ctx} now=newest+{off}")
        edges = [edges[0] or ed[0], edges[1] or ed[1]]
        reports.append(got)
    assert edges[0] or not need_exp_edge, "no main-store expiry fell on a census time (now == exp)"
    assert edges[1] or not local_cache, "no local-cache deadline fell on a census time (now == frz)"
    assert_matches_header(e, reports[0], ctx)
    assert int(reports[0]["keys_main"].sum()) > int(reports[-1]["keys_main"].sum())  # guard: keys expired
    assert (int(reports[0]["cached"].sum()) > 0) == local_cache
    assert (int(reports[0]["keys_per_second"].sum()) > 0) == split
    assert (int(reports[0]["prev"].sum()) > 0) == lag
    assert (e.occupancy(), e.stats()) == before
    hb = hiprl.build_batch(reqs[cuts[-1][0]:cuts[-1][1]])
    streams.assert_same(*e.submit(hb), *o.submit(hb), ctx="after the census")
    return e, o, strings, newest


# ---- 1. census against the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("local_cache", [False, True])
def test_census_equals_the_oracle_on_the_default_table(local_cache, split):
    reqs, cuts = big_stream()
    e, *_ = check_census(reqs, cuts, (16, 16, 16, 14), local_cache, split)
    e.close()


def test_census_with_a_lag_window_reports_the_previous_generation():
    reqs, cuts = big_stream()
    e, *_ = check_census(reqs, cuts, (16, 16, 16, 14), True, False, lag=True)
    e.close()


@pytest.mark.parametrize("log2_slots", [(4, 4, 4, 4), (4, 13, 12, 5)])
@pytest.mark.parametrize("split", [False, True])
def test_census_small_tables(log2_slots, split):
    """128 slots: all eight regions in one tile; (4,13,12,5): region borders inside tiles and
    waves, the table ends mid-tile."""
    reqs = tiny_stream()
    cuts = [(a, min(a + 9, len(reqs))) for a in range(0, len(reqs), 9)]  # one second per batch
    # (with the split the 4-s stream's main store holds MINUTE keys and longer: none expires at +1)
    e, *_ = check_census(reqs, cuts, log2_slots, True, split, need_exp_edge=not split)
    e.close()


def test_census_grid_caps_equal_the_uncapped_report(monkeypatch):
    """104 tiles: one block, three blocks (the grid stride) and one tile per block."""
    reqs, cuts = big_stream()
    newest = reqs[cuts[-2][1] - 1][4]
    reports = []
    for cap in (None, 1, 3):
        if cap is None:
            monkeypatch.delenv("RL_DIAG_CENSUS_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("RL_DIAG_CENSUS_BLOCKS", str(cap))
        e = hiprl.Engine(local_cache=True, max_batch_desc=1 << 13)
        e.load_rules(RULES)
        for a, b in cuts[:-1]:
            e.submit(hiprl.build_batch(reqs[a:b]))
        reports.append([e.census(newest + off) for off in OFFSETS])
        e.close()
    assert int(reports[0][0]["keys_main"].sum()) > 100 and int(reports[0][0]["cached"].sum()) > 10
    for capped in reports[1:]:
        for a, b in zip(reports[0], capped):
            assert same_reports(a, b)


def test_census_after_reset_and_forget():
    reqs, cuts = big_stream()
    e, o, strings, newest = check_census(reqs, cuts, (16, 16, 16, 14), True, False)
    # a frozen string of the last batch: forget it
    last = reqs[cuts[-1][0]:cuts[-1][1]]
    now = last[-1][4]
    pick = None
    for dom, descs, rids, _, t in reversed(last):
        for entries, rid in zip(descs, rids):
            if rid != NIL and t == now and o.local_cached(oracle.cache_key(hiprl.cache_key_prefix(dom, entries), RULES[rid][1], t), now):
                pick = (dom, [entries], [rid], 1, now)
    assert pick is not None
    before = e.census(now)
    rep = e.forget(hiprl.build_batch([pick]))
    assert int(rep["flags"][0]) & hiprl.PEEK_FOUND and int(rep["flags"][0]) & hiprl.PEEK_LOCAL_CACHED
    after = e.census(now)
    assert int(before["cached"].sum()) - int(after["cached"].sum()) == 1
    assert int(before["keys_main"].sum()) - int(after["keys_main"].sum()) == 1
    assert np.array_equal(before["live"], after["live"])  # the slot stays claimed
    e.reset()
    z = e.census(now)
    for f in PER_REGION + ("count_log2",):
        assert not np.any(z[f]), f
    assert z["slots"].tolist() == [1 << 16] * 6 + [1 << 14] * 2
    e.close()


def test_census_refusals():
    e = hiprl.Engine(local_cache=True)
    e.load_rules(RULES)
    t = 1_700_000_000
    b = hiprl.build_batch([("r", [[("k", str(i % 9))]], [i % 16], 1, t) for i in range(200)])
    e.submit(b)
    raises(EINVAL, e.census, 0xFFFD0001)
    raises(EINVAL, e.census, -1)
    assert int(e.census(0xFFFD0000)["live"].sum()) > 0
    rep = hiprl.RlCensusReport()
    rep.struct_size = C.sizeof(hiprl.RlCensusReport) - 8
    assert e.lib.rl_census(e.h, t, C.byref(rep)) == EINVAL
    e.submit_host_async(b)
    raises(ESTATE, e.census, t)  # a batch is in flight
    e.wait_into(b.n_desc, b.n_req)
    h, recs = e.snapshot_records()
    h2 = e.snapshot_begin()  # an open snapshot does not block it
    assert int(e.census(t)["live"].sum()) == int(h2.n_records) == recs.shape[0]
    e.snapshot_end()
    e.restore_begin(h)
    raises(ESTATE, e.census, t)  # a restore is open
    e.reset()
    assert int(e.census(t)["live"].sum()) == 0
    e.close()


# ---- 2. lookup counters, explicit form ----------------------------------------------------------
N_RULES = 100


def synthetic(n, rule, seed, nil_every=7):
    """test_gpu_rule_stats.py's helper: n statuses with every flag combination, deltas and hits of
    any size, several descriptors per request, nil rules mixed in."""
    rng = np.random.default_rng(seed)
    rule = np.asarray(rule, np.uint32).copy()
    if nil_every:
        rule[rng.integers(0, nil_every, n) == 0] = NIL
    n_req = max(1, (n + 2) // 3)
    req_of = np.sort(rng.integers(0, n_req, n)).astype(np.uint32)
    hits = rng.integers(0, 5, n_req).astype(np.uint32)
    st = np.zeros(n, hiprl.STATUS_DTYPE)
    flags = np.arange(n, dtype=np.uint32) % 8  # HAS_LIMIT | LOCAL_CACHE_HIT | SHADOW: all eight
    rng.shuffle(flags)
    st["code_flags"] = rng.integers(0, 3, n).astype(np.uint32) | (flags << 8)
    st["limit_remaining"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    st["reset_s"] = rng.integers(0, 86400, n).astype(np.uint32)
    st["over_limit_delta"] = rng.integers(0, 50, n).astype(np.uint32)
    st["near_limit_delta"] = rng.integers(0, 50, n).astype(np.uint32)
    return rule, req_of, hits, st


def reduce_cache(n_rules, rule, st):
    ok = np.asarray(rule, np.uint32) < n_rules  # NIL is 0xFFFFFFFF: never below n_rules
    hits = int((ok & (((st["code_flags"] >> 8) & hiprl.FLAG_LOCAL_CACHE_HIT) != 0)).sum())
    return {"hits": hits, "misses": int(ok.sum()) - hits, "lookups": int(ok.sum())}


def add_counts(a, b):
    return {k: a[k] + b[k] for k in a}


def add_device(e, rule, st):
    """One rl_cache_stats_add_device of host arrays (uploaded); only rule_id is set in the batch."""
    d_rule = torch.from_numpy(np.ascontiguousarray(rule).view(np.int32)).to(DEV)
    d_st = torch.from_numpy(np.ascontiguousarray(st).view(np.uint8)).to(DEV)
    torch.cuda.synchronize()
    e.cache_stats_add_device(len(rule), 0, 0, [0, 0, d_rule.data_ptr(), 0, 0, 0, 0], d_st.data_ptr())
    return d_rule, d_st  # alive until the caller has read the counters


def explicit_engine(local_cache=True):
    e = hiprl.Engine(local_cache=local_cache, max_batch_desc=1 << 13)
    e.load_rules([(10 + i % 7, 1 + i % 4) for i in range(N_RULES)])
    return e


@functools.lru_cache(maxsize=None)
def shared_engine():
    return explicit_engine()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
def test_explicit_counts_on_synthetic_statuses(n):
    e = shared_engine()
    e.cache_stats(clear=True)
    ids = np.arange(n) % (N_RULES + 20)  # ids at and above n_rules mixed in: they add nothing
    rule, _, _, st = synthetic(n, ids, seed=n)
    keep = add_device(e, rule, st)
    want = reduce_cache(N_RULES, rule, st)
    assert e.cache_stats() == want, n
    rule2, _, _, st2 = synthetic(n, ids, seed=n + 99, nil_every=0)
    keep2 = add_device(e, rule2, st2)  # noqa: F841
    want = add_counts(want, reduce_cache(N_RULES, rule2, st2))
    assert e.cache_stats() == want, (n, "second add")
    assert e.cache_stats(clear=True) == want and e.cache_stats() == {"hits": 0, "misses": 0, "lookups": 0}
    del keep


def test_explicit_counts_all_nil_all_hit_and_the_block_cap(monkeypatch):
    monkeypatch.setenv("RL_DIAG_CACHE_STATS_BLOCKS", "2")
    e = explicit_engine()
    monkeypatch.delenv("RL_DIAG_CACHE_STATS_BLOCKS")
    n = 5 * 2048 + 17  # three passes of two blocks, the last one partial
    rule, _, _, st = synthetic(n, np.arange(n) % (N_RULES + 20), seed=4)
    keep = [add_device(e, rule, st)]
    want = reduce_cache(N_RULES, rule, st)
    assert 0 < want["hits"] < want["lookups"] < n
    assert e.cache_stats() == want
    nil = np.full(n, NIL, np.uint32)
    keep.append(add_device(e, nil, st))
    assert e.cache_stats() == want, "all nil"
    hit = np.zeros(n, hiprl.STATUS_DTYPE)
    hit["code_flags"] = hiprl.CODE_OVER_LIMIT | ((hiprl.FLAG_HAS_LIMIT | hiprl.FLAG_LOCAL_CACHE_HIT) << 8)
    keep.append(add_device(e, np.full(n, 5, np.uint32), hit))
    want = add_counts(want, {"hits": n, "misses": 0, "lookups": n})
    assert e.cache_stats() == want, "all hit"
    raises(EINVAL, e.cache_stats_add_device, 5, 0, 0, [0] * 7, keep[0][1].data_ptr())  # null rule_id
    assert e.lib.rl_cache_stats_read(e.h, None, 0) == EINVAL
    cs = hiprl.RlCacheStats()
    assert e.lib.rl_cache_stats_read(e.h, C.byref(cs), 2) == EINVAL  # unknown flag
    e.close()


def test_an_engine_without_the_cache_counts_nothing():
    e = explicit_engine(local_cache=False)
    e.set_timing(True)
    rule, _, _, st = synthetic(500, np.arange(500) % N_RULES, seed=1)
    keep = add_device(e, rule, st)  # noqa: F841
    assert e.cache_stats() == {"hits": 0, "misses": 0, "lookups": 0}
    assert e.kernel_times()["k_cache_stats"][1] == 0
    e.close()
    e = hiprl.Engine(local_cache=False, cache_stats=True)  # the flag alone launches nothing either
    e.load_rules(RULES)
    e.set_timing(True)
    e.submit(hiprl.build_batch([("off", [[("k", str(i % 9))]], [i % 3], 1, 1_700_000_000) for i in range(300)]))
    assert e.kernel_times()["k_cache_stats"][1] == 0 and e.cache_stats()["lookups"] == 0
    e.close()


# ---- 3. lookup counters, automatic --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gauges():
    return json.loads((ROOT / "tests" / "golden" / "local_cache_gauges.json").read_text())["streams"]


def local1(golden):
    s = next(x for x in golden["streams"] if x["name"] == "integration_basic_local1")
    return s, streams.fixture_requests(s), gauges()[s["name"]]


def as_counts(pair):
    return {"hits": pair[0], "misses": pair[1], "lookups": pair[0] + pair[1]}


def random_cuts(n, seed, max_bs):
    rng, cuts, i = np.random.default_rng(seed), [], 0
    while i < n:
        j = min(n, i + int(rng.integers(1, max_bs + 1)))
        cuts.append((i, j))
        i = j
    return cuts


@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
@pytest.mark.parametrize("cuts", ["one", "random"])
def test_automatic_counts_equal_the_fixture_through_submit(golden, cuts, pipeline):
    s, reqs, want = local1(golden)
    e = hiprl.Engine(local_cache=True, cache_stats=True, pipeline=pipeline)
    e.load_rules([tuple(x) for x in s["rules"]])
    for a, b in ([(k, k + 1) for k in range(len(reqs))] if cuts == "one" else random_cuts(len(reqs), 9, 6)):
        e.submit(hiprl.build_batch(reqs[a:b]))
        assert e.cache_stats() == as_counts(want[b - 1]), (s["name"], b - 1)
    assert e.cache_stats(clear=True) == {"hits": 8, "misses": 48, "lookups": 56}
    assert e.cache_stats() == {"hits": 0, "misses": 0, "lookups": 0}
    e.close()


@pytest.mark.parametrize("rule_stats", [False, True])
def test_automatic_counts_through_submit_pipelined_three_in_flight(golden, rule_stats):
    s, reqs, want = local1(golden)
    e = hiprl.Engine(local_cache=True, cache_stats=True, rule_stats=rule_stats)
    e.load_rules([tuple(x) for x in s["rules"]])
    cuts = random_cuts(len(reqs), 5, 4)
    hbs = [hiprl.build_batch(reqs[a:b]) for a, b in cuts]
    dbs = [router.DeviceBatch.from_host(hb, DEV) for hb in hbs]
    outs = [torch.zeros(db.n_desc * 20, dtype=torch.uint8, device=DEV) for db in dbs]
    thrs = [torch.zeros(db.n_req, dtype=torch.int32, device=DEV) for db in dbs]
    torch.cuda.synchronize()
    pending = 0
    for k, db in enumerate(dbs):
        e.submit_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), outs[k].data_ptr(), thrs[k].data_ptr())
        pending += 1
        if pending == 3 or k == len(dbs) - 1:
            raises(ESTATE, e.cache_stats)  # batches are in flight
            while pending:
                e.wait()
                pending -= 1
            assert e.cache_stats() == as_counts(want[cuts[k][1] - 1]), k
    if rule_stats:  # both sets of counters: the reference-pinned per-rule totals of the last request
        rows = e.rule_stats()
        for name, st in s["expect"][-1]["stats"].items():
            r = s["stat_keys"].index(name)
            for f, v in st.items():
                assert int(rows[f][r]) == v, (name, f)
        assert int(rows["total_hits"].sum()) > 0
    e.close()


@pytest.mark.parametrize("rule_stats", [False, True])
def test_a_refused_batch_adds_nothing_and_its_rerun_adds_once(rule_stats):
    t = 1_700_000_021
    rules = [(3, hiprl.SECOND), (5, hiprl.SECOND)]
    e = hiprl.Engine(local_cache=True, cache_stats=True, rule_stats=rule_stats, log2_slots=(4, 4, 4, 4),
                     max_batch_desc=4096)  # 16-slot regions: load limit 12
    e.load_rules(rules)
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)
    # the capacity check counts a batch's descriptors, not its new keys: 0 live + 6 fit, 3 live + 10 do not
    ok = hiprl.build_batch([("cap", [[("k", str(i % 3))]], [0], 4, t) for i in range(6)])
    refused = hiprl.build_batch([("cap", [[("k", str(i))]], [i % 2], 1, t) for i in [0] + list(range(5, 14))])
    e.submit(ok)
    want = reduce_cache(len(rules), ok.rule, o.submit(ok)[0])
    assert want == {"hits": 3, "misses": 3, "lookups": 6} and e.cache_stats() == want
    with pytest.raises(hiprl.RedisError, match="RL_ENOSPC"):
        e.submit(refused)
    assert e.cache_stats() == want, "after RL_ENOSPC"
    e.resize((8, 0, 0, 0))
    e.submit(refused)
    want = add_counts(want, reduce_cache(len(rules), refused.rule, o.submit(refused)[0]))
    assert want == {"hits": 4, "misses": 12, "lookups": 16} and e.cache_stats() == want, "the rerun after the resize"
    if rule_stats:
        assert int(e.rule_stats()["total_hits"].sum()) == 4 * 6 + 10
    e.close()


# ---- 4. routed origin ---------------------------------------------------------------------------
def test_routed_origins_add_their_own_statuses():
    """Local transport, two shards, one rl_router_step; each origin then adds the statuses
    rl_route_unpack left in device memory. The engines' counters sum to the oracle's."""
    per, G = 1200, 2
    es = []
    for _ in range(G):
        e = hiprl.Engine(local_cache=True, max_batch_desc=4 * per * G)
        e.load_rules(RULES)
        es.append(e)
    r = hiprl.Router(es, max_desc=4 * per)
    batches = []
    for g in range(G):
        reqs = make_stream(70 + g, per, t0=1_700_000_300, keyspace=30, dt_max=1)
        batches.append(hiprl.build_batch([(d, de, ru, h, 1_700_000_300) for d, de, ru, h, _ in reqs]))
    dbs = [router.DeviceBatch.from_host(b, DEV) for b in batches]
    outs = [torch.zeros(b.n_desc * 20, dtype=torch.uint8, device=DEV) for b in batches]
    thrs = [torch.zeros(b.n_req, dtype=torch.int32, device=DEV) for b in batches]
    torch.cuda.synchronize()
    r.step([hiprl.Engine.device_batch(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs()) for db in dbs],
           [x.data_ptr() for x in outs], [x.data_ptr() for x in thrs])
    for e, db, out in zip(es, dbs, outs):
        e.cache_stats_add_device(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), out.data_ptr())
    o = oracle.Oracle(local_cache=True)
    o.load_rules(RULES)
    whole = routing.concat_batches(batches)
    est, _ = o.submit(whole)
    got, d0 = {"hits": 0, "misses": 0, "lookups": 0}, 0
    for e, b in zip(es, batches):
        mine = e.cache_stats()
        assert mine == reduce_cache(len(RULES), b.rule, est[d0:d0 + b.n_desc]), "one origin"
        got = add_counts(got, mine)
        d0 += b.n_desc
    ost = o.local_cache_stats()
    assert got == {"hits": ost["hit"], "misses": ost["miss"], "lookups": ost["lookup"]}
    assert got["hits"] > 100
    r.close()
