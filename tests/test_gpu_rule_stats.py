"""Per-rule stat counters summed on the device (rl_hip.h "Rule stats") on the GPU.

The expected rows are always a numpy uint64 reduction of statuses by the contribution rule of
the header: total_hits += max(1, hits_addend) for every descriptor with a rule, and for a status
with HAS_LIMIT over_limit / near_limit += its deltas, over_limit_with_local_cache += the over
delta on a local-cache hit, shadow_mode += 1 on a shadow decision. In automatic mode
(RL_CFG_RULE_STATS) the statuses reduced are the oracle's, never the device's own."""
import functools

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
FIELDS = hiprl.RULE_STAT_FIELDS
LDS_K = 1024  # k_rule_stats sums rule ids below it in LDS (rl_rule_stats.hip RS_K): a power of two


def reduce_stats(n_rules, rule, req_of, hits, st, n_req=None):
    """The contribution rule, descriptor by descriptor group, in uint64 (wraps like the device)."""
    rows = np.zeros(n_rules, hiprl.RULE_STAT_DTYPE)
    rule = np.asarray(rule, np.uint32)
    req_of = np.asarray(req_of, np.uint32)
    n_req = len(hits) if n_req is None else n_req
    ok = (rule < n_rules) & (req_of < n_req)  # NIL is 0xFFFFFFFF: never below n_rules
    r = rule[ok].astype(np.int64)
    h = np.maximum(np.asarray(hits, np.uint32)[req_of[ok]], 1).astype(np.uint64)
    fl = st["code_flags"][ok] >> 8
    lim = (fl & hiprl.FLAG_HAS_LIMIT) != 0
    over = np.where(lim, st["over_limit_delta"][ok], 0).astype(np.uint64)
    near = np.where(lim, st["near_limit_delta"][ok], 0).astype(np.uint64)
    olc = np.where(lim & ((fl & hiprl.FLAG_LOCAL_CACHE_HIT) != 0), st["over_limit_delta"][ok], 0).astype(np.uint64)
    shadow = (lim & ((fl & hiprl.FLAG_SHADOW) != 0)).astype(np.uint64)
    for f, v in zip(FIELDS, (h, over, near, olc, shadow)):
        np.add.at(rows[f], r, v)
    return rows


def add_rows(a, b):
    out = a.copy()
    for f in FIELDS:
        out[f] = a[f] + b[f]
    return out


def assert_rows(got, want, ctx=""):
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    assert not np.any(got["reserved"]), ctx
    for f in FIELDS:
        if not np.array_equal(got[f], want[f]):
            i = int(np.nonzero(got[f] != want[f])[0][0])
            raise AssertionError(f"{ctx}: {f} differs at rule {i}: device {int(got[f][i])}, expected {int(want[f][i])}")


def raises(code, fn, *a, **kw):
    with pytest.raises(hiprl.RedisError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value


def batch_reduction(b, st, n_rules):
    return reduce_stats(n_rules, b.rule, b.req_of, b.hits, st)


# ---- 1. synthetic statuses through rule_stats_add_device ----------------------------------------
N_BIG = 70_000


@functools.lru_cache(maxsize=None)
def big_engine():
    """An engine without the flag and with 70,000 rules (rows on both sides of every LDS bound)."""
    e = hiprl.Engine(max_batch_desc=1 << 13)
    e.load_rules([(10 + i % 7, 1 + i % 4) for i in range(N_BIG)])
    return e


def synthetic(n, rule, seed, nil_every=7):
    """n statuses with every flag combination, deltas and hits of any size, several descriptors
    per request, hits_addend 0, nil rules and statuses without HAS_LIMIT mixed in."""
    rng = np.random.default_rng(seed)
    rule = np.asarray(rule, np.uint32).copy()
    if nil_every:
        rule[rng.integers(0, nil_every, n) == 0] = NIL
    n_req = max(1, (n + 2) // 3)
    req_of = np.sort(rng.integers(0, n_req, n)).astype(np.uint32)
    hits = rng.integers(0, 5, n_req).astype(np.uint32)  # 0 means 1
    st = np.zeros(n, hiprl.STATUS_DTYPE)
    flags = np.arange(n, dtype=np.uint32) % 8  # HAS_LIMIT | LOCAL_CACHE_HIT | SHADOW: all eight
    rng.shuffle(flags)
    st["code_flags"] = rng.integers(0, 3, n).astype(np.uint32) | (flags << 8)
    st["limit_remaining"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    st["reset_s"] = rng.integers(0, 86400, n).astype(np.uint32)
    st["over_limit_delta"] = rng.integers(0, 50, n).astype(np.uint32)
    st["near_limit_delta"] = rng.integers(0, 50, n).astype(np.uint32)
    return rule, req_of, hits, st


def add_device(e, rule, req_of, hits, st, n_req=None):
    """One rl_rule_stats_add_device of host arrays (uploaded); only rule, req_of and hits are set."""
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV) if len(a) else torch.zeros(1, dtype=torch.int32, device=DEV)
    d_rule, d_req, d_hits = t(rule, np.int32), t(req_of, np.int32), t(hits, np.int32)
    d_st = t(st.view(np.uint8), np.uint8) if len(st) else torch.zeros(20, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    e.rule_stats_add_device(len(rule), len(hits) if n_req is None else n_req, 0,
                            [0, 0, d_rule.data_ptr(), d_req.data_ptr(), 0, d_hits.data_ptr(), 0], d_st.data_ptr())
    return d_rule, d_req, d_hits, d_st  # alive until the caller has read the rows


PATTERNS = {"one": lambda i: np.full(i.shape, 5), "mod2": lambda i: i % 2, "mod64": lambda i: i % 64,
            "mod65": lambda i: i % 65}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_synthetic_shapes_and_rule_patterns(n, pattern):
    e = big_engine()
    e.rule_stats(0, N_BIG, clear=True)
    rule, req_of, hits, st = synthetic(n, PATTERNS[pattern](np.arange(n)), seed=n + len(pattern))
    keep = add_device(e, rule, req_of, hits, st)
    want = reduce_stats(N_BIG, rule, req_of, hits, st)
    assert_rows(e.rule_stats(0, N_BIG), want, f"n={n} {pattern}")
    # a wave of one rule only (no nil rules): the in-wave sum
    rule, req_of, hits, st = synthetic(n, PATTERNS[pattern](np.arange(n)), seed=n + 99, nil_every=0)
    keep = add_device(e, rule, req_of, hits, st)  # noqa: F841
    want = add_rows(want, reduce_stats(N_BIG, rule, req_of, hits, st))
    assert_rows(e.rule_stats(0, N_BIG), want, f"n={n} {pattern}, second add")
    if n > 1:
        assert want["total_hits"].sum() > n  # guard: both adds counted


def test_ids_around_every_power_of_two_and_the_last_rule():
    """Ids k-1, k, k+1 for every power of two k from 2^6 to 2^16, id 0 and the last loaded rule:
    crosses the LDS bound (1024) and any other power-of-two one."""
    assert LDS_K & (LDS_K - 1) == 0 and 64 <= LDS_K <= 65536
    e = big_engine()
    e.rule_stats(0, N_BIG, clear=True)
    ids = sorted({0, N_BIG - 1} | {k + d for p in range(6, 17) for k in [1 << p] for d in (-1, 0, 1)})
    assert len(ids) == 35 and max(ids) == N_BIG - 1 and LDS_K - 1 in ids and LDS_K in ids
    rule = np.array([ids[(i * 11) % len(ids)] for i in range(35 * 40)], np.uint32)
    rule, req_of, hits, st = synthetic(len(rule), rule, seed=5)
    keep = add_device(e, rule, req_of, hits, st)  # noqa: F841
    want = reduce_stats(N_BIG, rule, req_of, hits, st)
    got = e.rule_stats(0, N_BIG)
    assert_rows(got, want, "power-of-two ids")
    assert set(np.nonzero(got["total_hits"])[0]) == set(ids)


def test_sums_pass_32_bits_and_bad_indices_are_ignored():
    e = big_engine()
    e.rule_stats(0, N_BIG, clear=True)
    n, n_req = 200, 50
    rule = (np.arange(n) % 3 + 1000).astype(np.uint32)  # rule 1000: below the LDS bound; 1024..: above
    rule[np.arange(n) % 3 == 2] = 2000
    req_of = (np.arange(n) // 4).astype(np.uint32)
    hits = np.full(n_req, 3, np.uint32)
    hits[:8] = 0xFFFFFFFF
    st = np.zeros(n, hiprl.STATUS_DTYPE)
    st["code_flags"] = hiprl.CODE_OVER_LIMIT | ((hiprl.FLAG_HAS_LIMIT | hiprl.FLAG_LOCAL_CACHE_HIT) << 8)
    st["over_limit_delta"][:40] = 0xFFFFFFFF
    st["near_limit_delta"][:40] = 0xFFFFFFFF
    rule[100], req_of[101] = N_BIG, n_req  # one unknown rule id, one request index past n_req: ignored
    keep = add_device(e, rule, req_of, hits, st, n_req=n_req)  # noqa: F841
    want = reduce_stats(N_BIG, rule, req_of, hits, st, n_req=n_req)
    for r in (1000, 1001, 2000):
        for f in FIELDS[:4]:
            assert int(want[f][r]) > 3 * 0xFFFFFFFF, (r, f)  # guard: >= 3 descriptors of 2^32 - 1
    got = e.rule_stats(0, N_BIG)
    assert_rows(got, want, "large deltas")
    assert int(got["total_hits"].sum()) == int(want["total_hits"].sum()) < int(np.maximum(hits, 1).astype(np.uint64)[req_of[req_of < n_req]].sum())
    # whole waves of one rule: the in-wave sum passes 2^32 too
    m = 130
    st2 = np.zeros(m, hiprl.STATUS_DTYPE)
    st2["code_flags"] = hiprl.CODE_OK | ((hiprl.FLAG_HAS_LIMIT | hiprl.FLAG_SHADOW) << 8)
    st2["over_limit_delta"] = st2["near_limit_delta"] = 0xFFFFFFFF
    one = (np.full(m, 7, np.uint32), np.arange(m, dtype=np.uint32), np.full(m, 0xFFFFFFFF, np.uint32), st2)
    keep = add_device(e, *one)  # noqa: F841
    want = add_rows(want, reduce_stats(N_BIG, *one))
    assert int(want["near_limit"][7]) == m * 0xFFFFFFFF and int(want["shadow_mode"][7]) == m
    assert_rows(e.rule_stats(0, N_BIG), want, "large deltas, one rule per wave")


def test_read_with_clear_zeroes_only_its_range():
    e = big_engine()
    e.rule_stats(0, N_BIG, clear=True)
    n = 3000
    rule, req_of, hits, st = synthetic(n, np.arange(n) % 300 + 900, seed=8, nil_every=0)
    keep = add_device(e, rule, req_of, hits, st)  # noqa: F841
    want = reduce_stats(N_BIG, rule, req_of, hits, st)
    part = e.rule_stats(1000, 100, clear=True)
    assert_rows(part, want[1000:1100], "the cleared range, as read")
    want[1000:1100] = np.zeros(100, hiprl.RULE_STAT_DTYPE)
    got = e.rule_stats(0, N_BIG)
    assert_rows(got, want, "after the clear")
    assert np.all(got["total_hits"][900:1000] > 0) and np.all(got["total_hits"][1100:1200] > 0)
    # argument errors
    raises(EINVAL, e.rule_stats, N_BIG - 1, 2)
    raises(EINVAL, e.rule_stats, N_BIG + 1, 0)
    assert e.rule_stats(N_BIG, 0).shape == (0,)
    assert e.rule_stats(N_BIG - 1, 1).shape == (1,)


def test_flag_off_launches_no_kernel():
    b = hiprl.build_batch([("off", [[("k", str(i % 9))]], [i % 3], 1, 1_700_000_000) for i in range(300)])
    for flag in (False, True):
        e = hiprl.Engine(rule_stats=flag)
        e.load_rules(RULES)
        e.set_timing(True)
        e.submit(b)
        assert (e.kernel_times()["k_rule_stats"][1] > 0) == flag
        assert bool(e.rule_stats()["total_hits"].sum()) == flag
        e.close()


# ---- 2. automatic mode on the parity streams ----------------------------------------------------
SHADOW_RULES = [(L, u, i % 3 == 0) for i, (L, u) in enumerate(RULES)]


@functools.lru_cache(maxsize=None)
def stream(seed):
    """test_gpu_peek's stream of a seed: 6000 requests in batches <= 1500."""
    reqs = make_stream(seed, 6000, t0=1_700_000_000 - 7 + seed * 86400 - 130)
    sizes = batch_sizes(reqs, np.random.default_rng(seed + 100), 1500)
    batches, i = [], 0
    for bs in sizes:
        batches.append(hiprl.build_batch(reqs[i:i + bs]))
        i += bs
    return batches


@functools.lru_cache(maxsize=None)
def expected_rows(seed, local_cache, shadow=False):
    """The oracle's statuses reduced, cumulative after every batch (never modified)."""
    rules = SHADOW_RULES if shadow else RULES
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(rules)
    out, acc = [], np.zeros(len(rules), hiprl.RULE_STAT_DTYPE)
    for b in stream(seed):
        acc = add_rows(acc, batch_reduction(b, o.submit(b)[0], len(rules)))
        out.append(acc)
    return out


def check_stream_auto(seed, local_cache, pipeline, shadow=False):
    rules = SHADOW_RULES if shadow else RULES
    e = hiprl.Engine(local_cache=local_cache, pipeline=pipeline, max_batch_desc=1 << 14, rule_stats=True)
    e.load_rules(rules)
    want = expected_rows(seed, local_cache, shadow)
    for j, b in enumerate(stream(seed)):
        e.submit(b)
        assert_rows(e.rule_stats(), want[j], f"seed={seed} local={local_cache} {pipeline} after batch {j}")
    e.close()
    return want[-1]


@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_automatic_mode_on_the_parity_streams(seed, local_cache, pipeline):
    last = check_stream_auto(seed, local_cache, pipeline)
    assert last["over_limit"].sum() > 100 and last["near_limit"].sum() > 10  # guard (the oracle's own figures)
    assert (last["over_limit_with_local_cache"].sum() > 100) == local_cache


@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
def test_automatic_mode_with_shadow_rules(pipeline):
    last = check_stream_auto(2, True, pipeline, shadow=True)
    assert last["shadow_mode"].sum() > 100
    assert not np.any(last["shadow_mode"][[i for i in range(len(RULES)) if i % 3]])


# ---- 3. the reference's own counters -------------------------------------------------------------
def test_golden_integration_streams(golden):
    """Both integration streams, one request per batch: after every request the device rows equal
    the reference-pinned cumulative stats (expect[i].stats), mapped through stat_keys."""
    checked = 0
    for s in golden["streams"]:
        e = hiprl.Engine(local_cache=s["local_cache"], rule_stats=True)
        e.load_rules([tuple(x) for x in s["rules"]])
        for req, exp in zip(streams.fixture_requests(s), s["expect"]):
            e.submit(hiprl.build_batch([req]))
            rows = e.rule_stats()
            for name, want in exp["stats"].items():
                r = s["stat_keys"].index(name)
                for k, v in want.items():
                    assert int(rows[k][r]) == v, (s["name"], exp["src"], name, k, int(rows[k][r]), v)
                    checked += 1
        e.close()
    assert checked >= 100


# ---- 4. counted once ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fallback_stream():
    """The stream of test_gpu_pipelined.py::test_pipelined_fallbacks_first_and_middle: batch 0 is
    refused (an MSD bucket over BUCKET_CAP), batch 1 poisoned behind it, batch 4 refused with
    batch 5 in flight. With the oracle's reduction over the whole stream (local cache on)."""
    rng = np.random.default_rng(7)
    now = 1_700_000_200
    hbs = []
    for k in range(10):
        t = now + k // 3
        batch = []
        for i in range(4000):
            x = rng.random()
            rule = int(rng.integers(0, 3))
            if k == 0 and i < 1500:
                key, rule = "big0", 2
            elif k == 4 and i % 2 == 0 and i < 3000:
                key, rule = "big4", 2
            elif x < 0.3:
                h = int(rng.integers(0, 4))
                key, rule = f"hot{h}", h % 3
            else:
                key = f"k{int(rng.integers(0, 5000))}"
            batch.append(("pl", [[("k", key)]], [rule], int(rng.integers(0, 4)), t))
        hbs.append(hiprl.build_batch(batch))
    o = oracle.Oracle(local_cache=True)
    o.load_rules(RULES)
    want = np.zeros(len(RULES), hiprl.RULE_STAT_DTYPE)
    for hb in hbs:
        want = add_rows(want, batch_reduction(hb, o.submit(hb)[0], len(RULES)))
    return hbs, want


@pytest.mark.parametrize("depth", [2, 3])
def test_fallbacks_and_poisoned_batches_count_once(depth):
    hbs, want = fallback_stream()
    e = hiprl.Engine(local_cache=True, max_batch_desc=1 << 14, pipeline="v4", rule_stats=True)
    e.load_rules(RULES)
    dbs = [router.DeviceBatch.from_host(hb, DEV) for hb in hbs]
    outs = [torch.zeros(db.n_desc * 20, dtype=torch.uint8, device=DEV) for db in dbs]
    thrs = [torch.zeros(db.n_req, dtype=torch.int32, device=DEV) for db in dbs]
    torch.cuda.synchronize()
    pending = 0
    for k, db in enumerate(dbs):
        e.submit_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), outs[k].data_ptr(), thrs[k].data_ptr())
        pending += 1
        if k == 2:
            raises(ESTATE, e.rule_stats)  # a batch is in flight
        if pending == depth:
            e.wait()
            pending -= 1
    for _ in range(pending):
        e.wait()
    s = e.stats()
    assert s["lsd_fallbacks"] >= 3 and s["batches"] == len(hbs), s
    assert_rows(e.rule_stats(), want, f"fallback stream depth={depth}")
    e.close()


def test_resorted_batches_count_once():
    """The sort_bits=8, lsd_only stream of test_gpu_parity.py::test_sort_prefix_widths_and_resort."""
    reqs = make_stream(11, 4000, t0=1_600_000_000, keyspace=400)
    sizes = batch_sizes(reqs, np.random.default_rng(5), 2000)
    o = oracle.Oracle(local_cache=True)
    o.load_rules(RULES)
    e = hiprl.Engine(local_cache=True, sort_bits=8, max_batch_desc=1 << 17, lsd_only=True, rule_stats=True)
    e.load_rules(RULES)
    want, i = np.zeros(len(RULES), hiprl.RULE_STAT_DTYPE), 0
    for bs in sizes:
        b = hiprl.build_batch(reqs[i:i + bs])
        i += bs
        want = add_rows(want, batch_reduction(b, o.submit(b)[0], len(RULES)))
        e.submit(b)
    assert e.stats()["resorts"] > 0
    assert_rows(e.rule_stats(), want, "re-sorted stream")
    e.close()


# ---- 5. counted never ---------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
def test_refused_batches_count_nothing(pipeline):
    """test_gpu_configs.py::test_capacity_refusal_changes_nothing's small table: a batch refused
    with RL_ENOSPC, then one with an unknown rule id (RL_EINVAL); the good batches around them count."""
    rules = [(3, hiprl.SECOND), (5, hiprl.SECOND)]
    t = 1_700_000_021

    def batch(ids, h=1, rule=0):
        return hiprl.build_batch([("cap", [[("k", str(i))]], [rule if i % 2 else 0], h, t) for i in ids])

    e = hiprl.Engine(local_cache=True, max_batch_desc=4096, log2_slots=(10, 10, 10, 10), max_blob_bytes=64 * 4096,
                     pipeline=pipeline, rule_stats=True)  # limit 768 slots
    e.load_rules(rules)
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)
    ok1, refused, ok2 = batch(range(500), rule=1), batch(range(500, 900), 2), batch(range(300, 550), 4, rule=1)
    unknown = batch(range(40), rule=len(rules))
    e.submit(ok1)
    want = batch_reduction(ok1, o.submit(ok1)[0], len(rules))
    assert_rows(e.rule_stats(), want, "first")
    with pytest.raises(hiprl.RedisError, match="RL_ENOSPC"):
        e.submit(refused)
    assert_rows(e.rule_stats(), want, "after RL_ENOSPC")
    with pytest.raises(hiprl.RedisError, match="RL_EINVAL"):
        e.submit(unknown)
    assert_rows(e.rule_stats(), want, "after RL_EINVAL")
    e.submit(ok2)
    want = add_rows(want, batch_reduction(ok2, o.submit(ok2)[0], len(rules)))
    assert_rows(e.rule_stats(), want, "after the refusals")
    assert want["over_limit"].sum() > 0
    e.close()


# ---- 6. lifetime --------------------------------------------------------------------------------
def test_rows_survive_reset_resize_and_rule_growth():
    t = 1_700_000_100
    rules = list(RULES)
    e = hiprl.Engine(local_cache=True, rule_stats=True, max_batch_desc=4096)
    e.load_rules(rules)
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)
    b = hiprl.build_batch([("life", [[("k", str(i % 50))]], [i % len(rules)], i % 4, t) for i in range(2000)])
    e.submit(b)
    want = batch_reduction(b, o.submit(b)[0], len(rules))
    assert want["over_limit"].sum() > 0
    e.reset()
    assert_rows(e.rule_stats(), want, "after reset")
    e.resize((15, 0, 17, 0))
    assert_rows(e.rule_stats(), want, "after resize")
    # past the rule table's first allocation: it is reallocated, the rows follow with their contents
    n_more = 40_000
    more = rules + [(7, hiprl.MINUTE)] * (n_more - len(rules))
    e.load_rules(more)
    grown = np.zeros(n_more, hiprl.RULE_STAT_DTYPE)
    grown[:len(rules)] = want
    assert_rows(e.rule_stats(), grown, "after the rule table grew")  # appended ids start at 0
    o2 = oracle.Oracle(local_cache=True)  # (the engine was reset: a fresh oracle)
    o2.load_rules(more)
    b2 = hiprl.build_batch([("life2", [[("k", str(i % 20))]], [[3, n_more - 1, 20_000][i % 3]], 2, t + 1)
                            for i in range(600)])
    e.submit(b2)
    grown = add_rows(grown, batch_reduction(b2, o2.submit(b2)[0], n_more))
    assert_rows(e.rule_stats(), grown, "a batch on appended ids")
    assert grown["total_hits"][n_more - 1] == 400 and grown["over_limit"][n_more - 1] > 0
    e.close()


# ---- 7. routed origin ---------------------------------------------------------------------------
def test_routed_origins_add_their_own_statuses():
    """Local transport, two shards, one rl_router_step; each origin then adds the statuses
    rl_route_unpack left in device memory. The engines' rows sum to the oracle's reduction."""
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
        e.rule_stats_add_device(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), out.data_ptr())
    o = oracle.Oracle(local_cache=True)
    o.load_rules(RULES)
    whole = routing.concat_batches(batches)
    est, _ = o.submit(whole)
    want = batch_reduction(whole, est, len(RULES))
    got = np.zeros(len(RULES), hiprl.RULE_STAT_DTYPE)
    d0 = 0
    for e, b in zip(es, batches):
        rows = e.rule_stats()
        assert_rows(rows, batch_reduction(b, est[d0:d0 + b.n_desc], len(RULES)), "one origin")
        got = add_rows(got, rows)
        d0 += b.n_desc
    assert_rows(got, want, "sum over the origins")
    assert want["over_limit"].sum() > 0 and want["over_limit_with_local_cache"].sum() > 0
    r.close()
