"""Numeric-range edges on every decision path of the device, bit-exact against the oracle
(which test_numeric_edges_cpu.py pins to an independent model in this regime).

Limits up to 2^32 - 1, hits_addend up to 2^32 - 1, INCRBY replies that wrap at 2^32, near
thresholds where float32(L) is inexact, times up to MAX_NOW and across a day boundary. Per case
the width-dependent code it reaches:
  1  k4_group / LSD leader, cold keys: the u64 INCRBY prefix of a key's list, the freeze search
     (binary while base + P < 2^32, linear past it), the u32 counter left in the table
  2  a reply landing exactly on 2^32: OVER, then OK with 40..0 remaining, then OVER again
  3  the same in a block's global scratch (a key with 950 records)
  4  hot keys: k4_hist's 52-bit sums per (tile, bucket) with their 12-bit counts (a whole tile of
     one key at 2^32 - 1 hits), k4_scan's u64 prefix over tiles, k4_place's atomicMax on the
     counter, deferred descriptors, the fallback to the LSD pipeline when a hot counter would pass
     2^32 under the local cache (sums of exactly 2^32 and 2^42)
  5  the exact sequential path (one string under a SECOND and a MINUTE rule)
  6  the compact wire format's 24-bit hits whose sum passes 2^32, raw replies decided on the host
  7  DevRule.near (float32 product) and the decision's u32 arithmetic, on the decide grid
  8  times: now_mod in MRec.rn, the multiply-high divisions, the DAY regions' parity flip,
     exp = t + div + jitter near 2^32, the refusal past MAX_NOW
A case that is meant to wrap proves it from the oracle's output alone (edge_model.wrapped): a test
that stopped wrapping fails.
"""
import functools

import numpy as np
import pytest

import edge_model as em
import hiprl
import oracle
import streams
import workload
from test_gpu_peek import EINVAL, check_against_oracle, key_batch

pytestmark = pytest.mark.gpu

M32 = em.M32
RULES = em.EDGE_RULES
R_MAX, R_F0, R_40, R_0, R_M24, R_H31, R_DAY, R_MMAX = range(8)
P = em.PALETTE
NOW = 1_700_000_100  # the first second of a minute
MAX_DESC = 1 << 13


def pair(local_cache=False, pipeline="v4", rules=RULES, ratio=0.8, **kw):
    o = oracle.Oracle(near_limit_ratio=ratio, local_cache=local_cache)
    o.load_rules(rules)
    e = hiprl.Engine(near_limit_ratio=ratio, local_cache=local_cache, pipeline=pipeline, max_batch_desc=MAX_DESC, **kw)
    e.load_rules(rules)
    return o, e


def both(o, e, b, ctx, compact=False):
    """The batch through the oracle and the engine, compared bit for bit; returns the oracle's output."""
    want = o.submit(b)
    got = e.submit_compact(b) if compact else e.submit(b)
    streams.assert_same(*want, *got, ctx)
    return want


def counters(b, rules):
    """Per descriptor the name of its counter: (prefix, window start)."""
    return [None if int(r) == em.NIL else (b.prefix(i), int(b.now[b.req_of[i]]) // em.DIV[rules[int(r)][1]])
            for i, r in enumerate(b.rule)]


def assert_wrapped(outs, batches, rules, ctx):
    st = np.concatenate([s for s, _ in outs])
    rid = [int(r) for b in batches for r in b.rule]
    keys = [k for b in batches for k in counters(b, rules)]
    assert em.wrapped(st, rules, rid, keys), f"{ctx}: no counter under L = 2^32 - 1 wrapped in the reference"


def req(key, rule, hits, now=NOW, dom="ne"):
    return (dom, [[("k", key)]], [rule], hits, now)


class U32Counters:
    """The oracle for check_against_oracle, its Redis counters (int64) as the uint32 a reply carries."""

    def __init__(self, o):
        self.o = o

    def counter(self, key, now=None, per_second=False):
        c = self.o.counter(key, now, per_second)
        return c if c < 0 else c & M32

    def local_cached(self, key, now):
        return self.o.local_cached(key, now)


def peek_found(e, o, pb, rules, ctx=""):
    """A peek of pb checked against the oracle; returns the replies and how many keys were found."""
    rep = e.peek(pb)
    return rep, check_against_oracle(rep, pb, U32Counters(o), rules, ctx=ctx)[0]


def fallbacks(e):
    return e.stats()["lsd_fallbacks"]


# ---- 1. cold keys in k4_group and the LSD leader -------------------------------------------------
@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("n", [2, 65, 257, 896])
def test_cold_key_with_palette_hits(n, local_cache, pipeline):
    """One key of n records per batch under L = 2^32 - 1, 2^32 - 16 and 40, hits from the palette;
    then the three keys interleaved in one batch on top of the counters left in the table. Under
    L = 2^32 - 1 and 40 the palette starts at 2^32 - 1, so two records already wrap. Under
    L = 2^32 - 16 it starts at 0: the replies run 1, 2, 2^31 + 1, 1 (wrapped, not over), 2^32 - 15
    (over): the freezing record lies behind the wrap, where a search that takes base + P for
    monotone finds the record before it."""
    ctx = f"cold n={n} local={local_cache} {pipeline}"
    o, e = pair(local_cache, pipeline)
    hits = {r: [P[(i + rot) % len(P)] for i in range(n)] for r, rot in ((R_MAX, 5), (R_F0, 0), (R_40, 5))}
    batches = [hiprl.build_batch([req(f"c{r}", r, h) for h in hits[r]]) for r in (R_MAX, R_F0, R_40)]
    batches.append(hiprl.build_batch([req(f"c{r}", r, hits[r][n - 1 - i]) for i in range(n) for r in (R_MAX, R_F0, R_40)]))
    outs = [both(o, e, b, f"{ctx} batch {k}") for k, b in enumerate(batches)]
    assert_wrapped(outs, batches, RULES, ctx)
    if local_cache and n >= 5:  # (the oracle's own output) the L = 2^32 - 16 key froze at its fifth record
        hit = (outs[1][0]["code_flags"] >> 8) & em.LOCAL_HIT != 0
        assert not hit[:5].any() and hit[5:].all(), hit[:8]
    if pipeline == "v4":
        assert fallbacks(e) == 0, e.stats()
    pb = key_batch([(hiprl.cache_key_prefix("ne", [("k", f"c{r}")]), r) for r in (R_MAX, R_F0, R_40)], NOW)
    assert peek_found(e, o, pb, RULES, ctx)[1] == 3
    e.close()


# ---- 2. landing exactly on the wrap --------------------------------------------------------------
@pytest.mark.parametrize("local_cache", [False, True])
def test_reply_lands_exactly_on_two_to_the_32(local_cache):
    ctx = f"landing local={local_cache}"
    o, e = pair(local_cache)
    b1 = hiprl.build_batch([req("land", R_40, 0xFFFFFFCE), req("wide", R_MAX, 0xFFFFFFCE)])
    b2 = hiprl.build_batch([req(k, r, 1) for _ in range(100) for k, r in (("land", R_40), ("wide", R_MAX))])
    outs = [both(o, e, b1, f"{ctx} batch 1"), both(o, e, b2, f"{ctx} batch 2")]
    assert_wrapped(outs, [b1, b2], RULES, ctx)
    st = outs[1][0][0::2]  # the L = 40 key's 100 records
    code, flags = st["code_flags"] & 0xFF, st["code_flags"] >> 8
    if local_cache:  # frozen by batch 1's reply of 2^32 - 50
        assert np.all(code == em.OVER) and np.all(flags & em.LOCAL_HIT)
    else:  # replies 2^32 - 49 .. 2^32 - 1, 0 .. 40, 41 .. 50
        assert [int(c) for c in code] == [em.OVER] * 49 + [em.OK] * 41 + [em.OVER] * 10
        assert [int(x) for x in st["limit_remaining"][49:90]] == list(range(40, -1, -1))
        assert not np.any(flags & em.LOCAL_HIT)
    assert fallbacks(e) == 0, e.stats()
    e.close()


# ---- 3. global-scratch range ---------------------------------------------------------------------
@pytest.mark.parametrize("big_rule,late", [(R_MAX, False), (R_F0, False), (R_F0, True)])
@pytest.mark.parametrize("local_cache", [False, True])
def test_global_scratch_key_with_wrapping_hits(local_cache, big_rule, late):
    """test_gpu_group_layout.test_global_scratch_beside_lds_ranges's shape: 950 records of one key
    (grouped in a block's global scratch) beside 3 000 cold ones. Under L = 2^32 - 1 the big key
    adds 2^32 - 1 each, and so it does under L = 2^32 - 16: the replies run 2^32 - 1 downwards, the
    first record is over the limit (and freezes the key, base + P >= 2^32 from the second record
    on), and without the cache 15 records are over before the replies are OK from 0 remaining
    upwards. late: under L = 2^32 - 16 it adds 2^31 each instead, so its replies alternate 2^31 and
    0 and never pass the limit, until record 900 adds 2^31 - 8 and record 901 lands on 2^32 - 8:
    the freezing record lies 450 wraps into the list."""
    ctx = f"global scratch local={local_cache} rule={big_rule} late={late}"
    rng = np.random.default_rng(23)
    seq = np.concatenate([np.full(950, 1_000_000), np.full(3, 2_000_000), rng.integers(0, 1000, size=3000)])
    rng.shuffle(seq)
    big_hits = [0x80000000] * 900 + [0x7FFFFFF8] + [0x80000000] * 49 if late else [M32] * 950
    reqs, j = [], 0
    for i, k in enumerate(int(x) for x in seq):
        if k == 1_000_000:
            reqs.append(req(str(k), big_rule, big_hits[j]))
            j += 1
        else:
            reqs.append(req(str(k), R_MAX, M32) if k == 2_000_000 else req(str(k), R_40, 1 + i % 3))
    o, e = pair(local_cache)
    b = hiprl.build_batch(reqs)
    out = both(o, e, b, ctx)
    assert_wrapped([out], [b], RULES, ctx)
    big = out[0][seq == 1_000_000]
    over = big["code_flags"] & 0xFF == em.OVER
    local = (big["code_flags"] >> 8) & em.LOCAL_HIT != 0
    if big_rule == R_F0 and not late:  # (the oracle's own output) replies 2^32 - 1, 2^32 - 2, ...
        if local_cache:  # the first record freezes the key
            assert over.all() and not local[0] and local[1:].all()
        else:  # 2^32 - 1 .. 2^32 - 15 are over; 2^32 - 16 = L leaves 0, the next ones 1, 2, ...
            assert over[:15].all() and not over[15:].any() and not local.any()
            assert [int(x) for x in big["limit_remaining"][15:]] == list(range(950 - 15))
    if late:  # (the oracle's own output) first over the limit at record 901
        assert not over[:901].any() and over[901]
        # frozen from there, or the replies go on alternating 2^31 - 8 and 2^32 - 8
        assert over[902:].all() if local_cache else (over[901::2].all() and not over[902::2].any())
    assert fallbacks(e) == 0, e.stats()
    e.close()


# ---- 4. hot path ---------------------------------------------------------------------------------
HOT_RULES = (R_MAX, R_F0, R_40, R_DAY)  # of hot ids 0..3
TILE = 2048


def hot_batch(ids, nows, per_req, hits):
    """Key "hp_k_<id>_": hot ids 0..3 under HOT_RULES, every other id under L = 40 per second or
    2^24 + 1 per minute; per_req descriptors per request; hits: per request."""
    ids = np.asarray(ids, np.uint64)
    n = len(ids)
    req_of = (np.arange(n) // per_req).astype(np.uint32)
    n_req = int(req_of[-1]) + 1
    blob, off = workload.prefix_blob([b"hp_k_", ids, b"_"])
    rule = np.where(ids < 4, np.array(HOT_RULES + (0,) * 4, np.uint32)[np.minimum(ids, 7).astype(np.int64)],
                    np.where(ids % 2 == 0, R_40, R_M24)).astype(np.uint32)
    now = np.asarray(nows, np.int64)[np.arange(n_req) * per_req]
    return hiprl.Batch(blob, off, rule, req_of, now, np.asarray(hits, np.uint32)[:n_req])


@functools.lru_cache(maxsize=None)
def hot_stream(n, wrap):
    """Two teaching batches (test_gpu_hist_entry._teach: 300-600 descriptors per hot key), batch A
    of n descriptors, about half of them hot, three per request, hits from the palette (wrap) or
    <= 3 (the control), over two seconds; batch B in A's last second and batch C a second later,
    hits <= 3."""
    rng = np.random.default_rng(n)
    out = []
    for _ in range(2):
        ids = np.concatenate([np.full(300 + 100 * h, h) for h in range(4)] + [1000 + rng.integers(0, 8000, 3000)])
        rng.shuffle(ids)
        out.append(hot_batch(ids, np.full(len(ids), NOW - 1), 1, 1 + np.arange(len(ids)) % 3))
    pos = np.arange(n)
    hot = (pos % TILE < 64) | (rng.random(n) < 0.45)
    ids = np.where(hot, pos % 4, 1000 + rng.integers(0, 3 * n + 10, n))
    small = np.arange(n) % 4
    out.append(hot_batch(ids, NOW + (pos >= n // 2), 3, np.array(P, np.uint32)[np.arange(n) % len(P)] if wrap else small))
    for t in (NOW + 1, NOW + 2):
        ids = np.where(rng.random(600) < 0.5, np.arange(600) % 4, 1000 + rng.integers(0, 3 * n + 10, 600))
        out.append(hot_batch(ids, np.full(600, t), 3, small))
    return out


def run_hot(n, local_cache, wrap):
    ctx = f"hot n={n} local={local_cache} wrap={wrap}"
    o, e = pair(local_cache)
    batches = hot_stream(n, wrap)
    outs, fb, hk = [], [], []
    for k, b in enumerate(batches):
        outs.append(both(o, e, b, f"{ctx} batch {k}"))
        fb.append(fallbacks(e))
        hk.append(e.stats()["hot_keys"])
    # hot_keys is the size of the hot set uploaded for the last batch submitted: the teaching batches
    # ran with none (the set is built from their candidates), batch A with all four. (A batch rerun
    # on the LSD pipeline rebuilds the set from that run's segments, so B and C are the callers' to check.)
    assert hk[:3] == [0, 0, 4], hk
    pb = key_batch([(b"hp_k_%d_" % h, HOT_RULES[h]) for h in range(4)], NOW + 2)
    assert peek_found(e, o, pb, RULES, ctx)[1] == 4
    s = e.stats()
    e.close()
    return outs, batches, fb, s


@pytest.mark.parametrize("n", [700, 2 * TILE + 77])
def test_hot_keys_with_palette_hits(n):
    outs, batches, fb, s = run_hot(n, False, True)
    assert_wrapped(outs[2:3], batches[2:3], RULES, f"hot n={n} batch A")
    assert fb[-1] == 0 and s["hot_keys"] == 4, s


def test_hot_tile_of_one_key_with_the_largest_hits():
    """The largest per-(tile, hot bucket) word there is: a whole tile of 2048 descriptors of one hot
    key (the 12-bit count field's largest value) adding 2^32 - 1 each (a sum of 2^43 - 2^11, the
    most the 52-bit field ever holds); a second tile splits the rest between two hot keys, so
    k4_scan's prefix over tiles starts from that sum."""
    ctx = "hot full tile"
    o, e = pair(False)
    for k, b in enumerate(hot_stream(700, True)[:2]):
        both(o, e, b, f"{ctx} teaching batch {k}")
    ids = np.concatenate([np.zeros(TILE, np.int64), np.arange(TILE) % 2 * 3])  # tile 1: ids 0 and 3
    b = hot_batch(ids, np.full(len(ids), NOW), 1, np.full(len(ids), M32, np.uint32))
    assert_wrapped([both(o, e, b, ctx)], [b], RULES, ctx)
    small = hot_batch(np.arange(600) % 4, np.full(600, NOW), 3, np.arange(600) % 4)
    both(o, e, small, f"{ctx}: on top of the counters left")
    s = e.stats()
    assert s["lsd_fallbacks"] == 0 and s["hot_keys"] == 4, s
    pb = key_batch([(b"hp_k_%d_" % h, HOT_RULES[h]) for h in range(4)], NOW)
    assert peek_found(e, o, pb, RULES, ctx)[1] == 4
    e.close()


@pytest.mark.parametrize("n", [700, 2 * TILE + 77])
def test_hot_keys_with_palette_hits_local_cache(n):
    """With the local cache on, the batch in which a hot counter would pass 2^32 is rerun on the
    LSD pipeline (the freeze search of the hot path needs a monotone sequence); the same stream
    with hits <= 3 stays on v4."""
    outs, batches, fb, s = run_hot(n, True, True)
    assert_wrapped(outs[2:3], batches[2:3], RULES, f"hot n={n} batch A")
    assert fb[1] == 0 and fb[2] > fb[1], (fb, s)
    _, _, fb0, s0 = run_hot(n, True, False)
    assert fb0[-1] == 0 and s0["hot_keys"] == 4, (fb0, s0)


@pytest.mark.parametrize("shape", ["2^42 in one tile", "2^32 over two tiles"])
def test_hot_sum_on_a_power_of_two_local_cache(shape):
    """The sums' high bits decide one thing only, whether a hot counter would pass 2^32 under the
    local cache (then the batch goes to the LSD pipeline); the replies themselves are mod 2^32.
    A sum whose low bits are all zero is where a narrower sum would say "no": 1024 x (2^32 - 1) +
    1024 = 2^42 in one tile's word, and 2^31 + 2^31 = 2^32 (the smallest that passes) from two
    tiles through k4_scan's prefix. The key is new in its second, so the counter starts at 0."""
    ctx = f"hot sum {shape}"
    o, e = pair(True)
    for k, b in enumerate(hot_stream(700, True)[:2]):
        both(o, e, b, f"{ctx} teaching batch {k}")
    cold = 5000 + np.arange(TILE + 200)
    if shape == "2^42 in one tile":
        ids = np.concatenate([np.zeros(1025, np.int64), cold[:1500]])
        hits = np.concatenate([np.full(1024, M32), [1024], 1 + np.arange(1500) % 3])
    else:
        ids = np.concatenate([[0], cold[:TILE - 1], [0], cold[TILE:]])
        hits = np.where(ids == 0, 0x80000000, 1 + np.arange(len(ids)) % 3)
    fb = fallbacks(e)
    b = hot_batch(ids, np.full(len(ids), NOW), 1, hits.astype(np.uint32))
    assert int(b.hits[ids == 0].astype(np.uint64).sum()) in (2 ** 42, 2 ** 32)
    out = both(o, e, b, ctx)
    # one fallback, and the batch that wrapped ran with the four-key hot set (hot_keys: the set
    # uploaded for the last batch submitted)
    assert fb == 0 and fallbacks(e) == 1 and e.stats()["hot_keys"] == 4, e.stats()
    last = out[0][np.nonzero(ids == 0)[0][-1]]  # (the oracle's own output) the key's last reply is 0 mod 2^32
    assert int(last["code_flags"]) & 0xFF == em.OK and int(last["limit_remaining"]) == M32
    both(o, e, hot_batch(np.arange(600) % 4, np.full(600, NOW), 3, np.arange(600) % 4), f"{ctx}: the batch behind it")
    e.close()


# ---- 5. exact sequential path --------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
@pytest.mark.parametrize("local_cache", [False, True])
def test_one_string_under_a_second_and_a_minute_rule(local_cache, pipeline):
    """NOW starts a minute, so "ne_k_mix_<NOW>" is one string for both rules (L = 2^32 - 1): units
    mixed in one key's list, 600 records, hits from the palette."""
    ctx = f"mixed units local={local_cache} {pipeline}"
    assert NOW % 60 == 0
    o, e = pair(local_cache, pipeline)
    b = hiprl.build_batch([req("mix", (R_MAX, R_MMAX)[(i // 3) % 2], P[(i + 5) % len(P)]) for i in range(600)])
    out = both(o, e, b, ctx)
    # one counter (the rules differ, the string does not): the proof reads it under both rules
    st = out[0]
    after = M32 - st["limit_remaining"].astype(np.int64)
    assert np.all(st["code_flags"] & 0xFF == em.OK) and np.any(np.diff(after) < 0), f"{ctx}: no wrap in the reference"
    b2 = hiprl.build_batch([req("mix", R_MMAX, 2, NOW + 1), req("mix", R_MAX, 2, NOW + 1)])
    both(o, e, b2, f"{ctx} a second later")
    if pipeline == "v4":
        assert fallbacks(e) == 0, e.stats()
    e.close()


# ---- 6. compact format and raw replies -----------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
@pytest.mark.parametrize("local_cache", [False, True])
def test_compact_hits_sum_past_two_to_the_32(local_cache, pipeline):
    """300 records of 2^24 - 1 hits per key: no single h passes 24 bits, the sum passes 2^32."""
    ctx = f"compact local={local_cache} {pipeline}"
    assert 300 * 0xFFFFFF > 2 ** 32
    o, e = pair(local_cache, pipeline)
    b = hiprl.build_batch([req(f"z{r}", r, 0xFFFFFF) for _ in range(300) for r in (R_MAX, R_F0, R_40)])
    outs = [both(o, e, b, ctx, compact=True)]
    outs.append(both(o, e, b, f"{ctx} again", compact=True))  # on top of the wrapped counters
    assert_wrapped(outs, [b, b], RULES, ctx)
    if pipeline == "v4":
        assert fallbacks(e) == 0, e.stats()
    e.close()


# ---- 7. limits and ratios on the device ----------------------------------------------------------
def grid_streams(ratio):
    """The decide vectors of a ratio as requests on fresh keys: a warm-up request that brings the
    counter to after - hits (mod 2^32), then the checked one; a local-cache-hit vector by a
    warm-up of L + 1 (unreachable for L = 2^32 - 1). -> (rules, {local_hit: {now: [(vector,
    requests)]}})."""
    rules, rid, by = [], {}, {False: {}, True: {}}
    for k, v in enumerate(em.grid([ratio])):
        r = rid.setdefault((v["L"], v["unit"]), len(rid))
        if r == len(rules):
            rules.append((v["L"], v["unit"]))
        pre = v["L"] + 1 if v["local_hit"] else (v["after"] - v["hits"]) & M32
        if pre > M32:
            continue
        reqs = [req(f"g{k}", r, pre, v["now"], "grid")] if pre else []
        reqs.append(req(f"g{k}", r, v["hits"], v["now"], "grid"))
        by[v["local_hit"]].setdefault(v["now"], []).append((v, reqs))
    return rules, by


@pytest.mark.parametrize("ratio", [0.0, 0.8, 1.0])
def test_decide_grid_on_the_device(ratio):
    """One batch per request time, in time order: a batch may straddle one window boundary of a
    region, no more (ERR_WINDOW_SPAN), and the grid's times lie decades apart, so
    all vectors of a ratio cannot share a batch. A time's vectors are split only at max_batch_desc."""
    rules, by = grid_streams(ratio)
    checked = 0
    for local_hit, by_now in by.items():
        o, e = pair(local_hit, rules=rules, ratio=ratio)
        for now in sorted(by_now):
            items = by_now[now]
            for c0 in range(0, len(items), MAX_DESC // 2):
                chunk = items[c0:c0 + MAX_DESC // 2]
                b = hiprl.build_batch([q for _, reqs in chunk for q in reqs])
                st, thr = both(o, e, b, f"grid ratio={ratio} local_hit={local_hit} now={now}")
                i = -1
                for v, reqs in chunk:
                    i += len(reqs)
                    want = em.decide(v["L"], v["unit"], np.float32(ratio), now, v["hits"], v["after"], local_hit)
                    assert tuple(int(x) for x in st[i]) + (int(thr[i]),) == want, (v, st[i], thr[i])
                    checked += 1
        assert fallbacks(e) == 0, e.stats()
        e.close()
    assert checked > 3000, checked


# ---- 8. times ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
@pytest.mark.parametrize("local_cache", [False, True])
def test_single_time_batches_at_edge_times(local_cache, pipeline):
    rules, batches = em.time_batches()
    o, e = pair(local_cache, pipeline, rules=rules)
    for reqs in batches:
        both(o, e, hiprl.build_batch(reqs), f"edge time {reqs[0][4]} local={local_cache} {pipeline}")
    if pipeline == "v4":  # no batch was handed to the LSD pipeline: the v4 kernels decided at every time
        assert fallbacks(e) == 0, e.stats()
    e.close()


@pytest.mark.parametrize("n_rules", [1 << 15, 0xFFFF])
def test_largest_rule_id_in_the_last_second_of_a_day(n_rules):
    """MRec.rn = rule | now_mod << 15 with every bit set: rule 32767 (the most the v4 pipeline
    takes) under a DAY rule at now_mod 86399. And rule id 0xFFFE, the largest the compact format's
    16 bits carry beside the nil id 0xFFFF; with that many rules the engine runs the LSD pipeline."""
    ctx = f"{n_rules} rules"
    rules = [(3 + i % 5, 1 + i % 4) for i in range(n_rules)]
    top = n_rules - 1
    rules[top], rules[top - 1] = (M32, hiprl.DAY), (40, hiprl.DAY)
    t = 86400 * 19676 + 86399
    o, e = pair(True, rules=rules)
    small = [1, 0xFFFFFF, 0, 7]  # what the compact format's 24 bits carry
    batches = [hiprl.build_batch([("rid", [[("k", "cw"[i % 2] + str(i % 7))], [("j", str(i % 3))]],
                                  [top - (i + 1) % 2, (i * 4099) % n_rules], hits[i % len(hits)], t) for i in range(300)])
               for hits in (P, small)]
    outs = [both(o, e, batches[0], f"{ctx} batch 0"), both(o, e, batches[1], f"{ctx} compact", compact=True)]
    assert_wrapped(outs, batches, rules, ctx)
    assert int(batches[0].rule.max()) == top
    if n_rules <= 1 << 15:
        assert fallbacks(e) == 0, e.stats()
    e.close()


@functools.lru_cache(maxsize=None)
def day_boundary_stream():
    reqs = streams.make_stream(41, 3000, t0=86400 * 19676 - 5)
    assert reqs[0][4] // 86400 + 1 == reqs[-1][4] // 86400
    return reqs, streams.batch_sizes(reqs, np.random.default_rng(42), 700)


@functools.lru_cache(maxsize=None)
def day_boundary_expected(local_cache):
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(streams.RULES)
    return streams.replay(o, *day_boundary_stream())


@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
@pytest.mark.parametrize("local_cache", [False, True])
def test_stream_across_a_day_boundary(local_cache, pipeline):
    reqs, sizes = day_boundary_stream()
    e = hiprl.Engine(local_cache=local_cache, pipeline=pipeline, max_batch_desc=MAX_DESC)
    e.load_rules(streams.RULES)
    streams.assert_same(*day_boundary_expected(local_cache), *streams.replay(e, reqs, sizes),
                        f"day boundary local={local_cache} {pipeline}")
    if pipeline == "v4":
        assert fallbacks(e) == 0, e.stats()
    e.close()


@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
def test_largest_jitter_on_a_day_rule_at_max_now(pipeline):
    rules, batches, jits = em.jitter_stream()
    o, e = pair(False, pipeline, rules=rules)
    for k, (reqs, j) in enumerate(zip(batches, jits)):
        both(o, e, hiprl.build_batch(reqs, jit=j), f"jitter batch {k} {pipeline}")
    pb = key_batch([(b"j_k_d_", 0), (b"j_k_m_", 2)], em.MAX_NOW)
    rep, found = peek_found(e, o, pb, rules)
    assert found == 2
    assert int(rep[0]["count"]) == 4 and int(rep[0]["ttl_s"]) == 86400 + 65535  # EXPIRE of the batch at MAX_NOW
    if pipeline == "v4":
        assert fallbacks(e) == 0, e.stats()
    e.close()


@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
def test_a_request_past_max_now_is_refused(pipeline):
    o, e = pair(True, pipeline)
    t = em.MAX_NOW
    good = hiprl.build_batch([req(str(i % 4), (R_40, R_DAY, R_M24, R_H31)[i % 4], 30, t) for i in range(12)])
    both(o, e, good, f"at MAX_NOW {pipeline}")
    pb = key_batch([(good.prefix(i), int(good.rule[i])) for i in range(4)], t)
    base, found = peek_found(e, o, pb, RULES)
    assert found == 4
    bad = hiprl.build_batch([req(str(i % 4), (R_40, R_DAY, R_M24, R_H31)[i % 4], 30, t + (i == 11)) for i in range(12)])
    with pytest.raises(hiprl.RedisError) as ei:
        e.submit(bad)
    assert ei.value.code == EINVAL, ei.value
    assert np.array_equal(e.peek(pb), base)
    both(o, e, good, f"after the refusal {pipeline}")
    if pipeline == "v4":  # the refusal is no fallback either
        assert fallbacks(e) == 0, e.stats()
    e.close()
