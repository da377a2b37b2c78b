"""The hot set at capacity, in churn and under tag-table clustering, bit-exact against the oracle.

Small batches that reach what the 2..8 hot prefixes of the other GPU tests leave unrun: hot
indices 8..255 (k4_scan's hot blocks 1..31, k4_group's second EXPIRE block, the last block's
frozen-key pass over all 512 buckets), the set's maintenance (HOT_MAX, more qualifying prefixes
than fit, more candidates than CAND_MAX, the join / stay thresholds at their edges, the batches on
which the set is resampled, a set that shrinks and refills with batches in flight), and hot sets
that are one probe chain of the LDS tag table (hot_cases.py). Every status field and request
throttle goes through streams.assert_same; the table is read back with rl_peek.
"""
import functools

import numpy as np
import pytest
import torch

import hiprl
import hot_cases as hc
import oracle
import router
import streams
from hot_cases import HOT_CAND_MIN, HOT_MAX, HOT_MIN_SEG, T
from test_gpu_peek import F, LC, check_against_oracle, key_batch

pytestmark = pytest.mark.gpu

N_COLD = 300


# The capacity check ahead of a batch counts a region's descriptors, not its keys (k4_scan
# capacity_ok on FP_CNT): the two tests whose batches put more descriptors on one unit than the
# default DAY region holds (2^14 slots) run on a larger table.
BIG_TABLE = (18, 18, 18, 18)


def pair(local_cache, log2_slots=(16, 16, 16, 14)):
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(hc.RULES)
    e = hiprl.Engine(local_cache=local_cache, max_batch_desc=1 << 18, log2_slots=log2_slots)
    e.load_rules(hc.RULES)
    return o, e


def family_keys(family, K):
    """The family's K keys, then the cold tail: plain cold keys, and for a clustered family
    non-members that start their probe at the family's home (same home / other tag, and
    chain-mates with the family's own home and tag)."""
    hot = hc.FAMILIES[family](K)
    tail = hc.cold(N_COLD)
    if family != "spread":
        home, tag = hc.home_tag(hot[0])
        tail += list(hc.same_home_other_tag(home, tag, 8)) + hc.chain_mates(hot, 40)
    return hc.keys_of(hot + tail)


def sweep_case(family, K, local_cache, jitter=False, extra=None):
    """teach, then one checked batch at T - 1 -> T. Returns (o, e, keys, batch)."""
    keys = family_keys(family, K)
    o, e = pair(local_cache)
    fb = hc.teach(o, e, keys, T - 4, n_hot=K)
    frozen = hc.frozen_before(o, keys, K, T - 1)
    b = hc.checked_batch(keys, K, jitter=jitter, extra=extra)
    ctx = f"{family} K={K} local={local_cache}"
    f = hc.figures(hc.submit_checked(o, e, b, ctx)[0])
    s = e.stats()
    assert s["hot_keys"] == min(K, HOT_MAX) and s["lsd_fallbacks"] == fb, (ctx, s)
    assert s["inserted_keys"] == o.num_strings(), (ctx, s, o.num_strings())
    # guards, from the oracle alone: decisions on both sides of a limit, and with the local cache
    # hits and keys frozen before the batch (tiny-limit MINUTE / HOUR / DAY keys)
    assert f["over"] >= K and f["ok"] >= K, (ctx, f)
    if local_cache:
        assert f["local_hits"] >= K // 4 and frozen >= sum(hc.is_tiny(i) and i % 4 != 0 for i in range(K)), (ctx, f, frozen)
        assert K < 8 or frozen > 0
    return o, e, keys, b


def check_write_back(o, e, keys, K, b, local_cache, ctx):
    """rl_peek of every hot key string of both windows after the checked batch."""
    items = [(keys.prefixes[i], int(keys.rules[i])) for i in range(K)]
    pb = key_batch(items + items, [T - 1] * K + [T] * K)
    rep = e.peek(pb)
    found, absent, cached = check_against_oracle(rep, pb, o, hc.RULES, ctx=ctx)
    assert found == 2 * K and absent == 0, (ctx, found, absent)
    if not local_cache:
        # every descriptor did its INCRBY and EXPIRE: the string's TTL is that of its last one
        last = hc.last_touch(b)
        for i in range(2 * K):
            now = int(pb.now[i])
            div = hiprl.UNIT_DIVIDER[hc.RULES[items[i % K][1]][1]]
            t_last, jit, _ = last[(items[i % K][0], now // div * div)]
            assert int(rep[i]["flags"]) == F and int(rep[i]["ttl_s"]) == t_last + div + jit - now, (ctx, i, rep[i])
        return
    assert cached >= K // 3, (ctx, cached)  # tiny and small limits freeze in both windows
    for i in range(2 * K):
        if not int(rep[i]["flags"]) & LC:
            continue
        now = int(pb.now[i])
        k = oracle.cache_key(items[i % K][0], hc.RULES[items[i % K][1]][1], now)
        c = int(rep[i]["cached_s"])
        assert o.local_cached(k, now + c - 1) and not o.local_cached(k, now + c), (ctx, i, rep[i])


# ---- index sweep -------------------------------------------------------------------------------
@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("K", [8, 9, 16, 17, 128, 129, 255, 256])
def test_index_sweep(K, local_cache):
    """K spread hot keys of all four units in both window parities: with K = 256 all 512 hot
    buckets are live. 8 | 9 and 16 | 17: k4_scan's hot blocks own 8 hot indices each; 128 | 129:
    k4_group's two EXPIRE blocks."""
    _, e, _, _ = sweep_case("spread", K, local_cache)
    e.close()


# ---- table write-back --------------------------------------------------------------------------
@pytest.mark.parametrize("local_cache", [False, True])
def test_table_write_back(local_cache):
    o, e, keys, b = sweep_case("spread", 256, local_cache, jitter=not local_cache)
    check_write_back(o, e, keys, 256, b, local_cache, f"write-back local={local_cache}")
    e.close()


# ---- more candidates than fit --------------------------------------------------------------------
@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("K", [257, 300])
def test_more_qualifying_prefixes_than_fit(K, local_cache):
    """The set stays at HOT_MAX; the prefixes left out are decided on the MSD path, >= 128
    descriptors each, in the same batches."""
    _, e, _, _ = sweep_case("spread", K, local_cache)
    e.close()


def test_more_candidates_than_cand_max():
    """1100 prefixes x 128 descriptors in one batch: 1100 candidates for CAND_MAX = 1024 places.
    That batch's sample is applied behind the next submit and uploaded by the one after."""
    keys = hc.keys_of(hc.spread(1100) + hc.cold(100))
    o, e = pair(False, BIG_TABLE)
    counts = np.full(len(keys), 2)
    counts[:1100] = HOT_MIN_SEG
    big = hc.make_batch(keys, hc.mix(counts, np.random.default_rng(5)), T - 4)
    assert big.n_desc > hc.CAND_MAX * HOT_MIN_SEG
    hc.submit_checked(o, e, big, "1100 candidates")
    assert e.stats()["lsd_fallbacks"] == 0, e.stats()
    for j in range(2):
        hc.submit_checked(o, e, hc.teaching_batch(keys, 300, T - 3 + j, j), f"behind the big batch {j}")
    assert e.stats()["hot_keys"] == HOT_MAX, e.stats()
    hc.submit_checked(o, e, hc.checked_batch(keys, 300), "checked")
    s = e.stats()
    assert s["hot_keys"] == HOT_MAX and s["lsd_fallbacks"] == 0 and s["inserted_keys"] == o.num_strings(), s
    e.close()


# ---- thresholds and the batches that are sampled ------------------------------------------------
@pytest.mark.parametrize("local_cache", [False, True])
def test_thresholds_and_sampled_batches(local_cache):
    """Keys J0..J19 and N0..N19, each batch at one time of its own (a key is one segment). The set
    is sampled while it is empty, after a fallback and when (batches & 7) == 0; a sample is applied
    behind the next submit and uploaded (hot_keys) by the one after.

      batch  sampled because   counts                                   hot_keys after it
      0, 1   set empty         J 128, N 127                             0, 0
      2      -                 J 128, N 127                             20  (only the 128s joined)
      3..7   -                 all 10 (nobody looks)                    20
      8      batches == 8      J0..9 63, J10..19 64, N 127              20
      9      -                 all 10                                   20
      10     -                 all 10                                   10  (the 63s left)
      11     falls back        J0..9 100, J10..19 64, J10 once under a second rule,
                               N0..4 128, N5..9 127                     10
      12     -                 all 10                                   14  (J11..19 stay, N0..4 join;
                                                                             J10 had two rules)
      13..15 -                 all 10                                   14
      16     batches == 16     all 10                                   14
      17     -                 all 10                                   14
      18     set empty         J 128                                    0
      19     set empty         J 128                                    0
      20     -                 J 128                                    20
    """
    J, N = 20, 20
    keys = hc.keys_of([b"hs_j_%d_tail_" % i for i in range(J)] + [b"hs_n_%d_tail_" % i for i in range(N)] + hc.cold(200))
    # J10 under its unit's next limit class: the same key string, a second rule
    alt = hc.Keys([keys.prefixes[10]], [int(keys.rules[10]) // 3 * 3 + (int(keys.rules[10]) + 1) % 3])
    allk = keys + alt
    ALT = len(keys)

    def counts(j):
        c = np.full(len(allk), 2)
        c[ALT] = 0
        c[:J + N] = 10
        if j in (0, 1, 2):
            c[:J], c[J:J + N] = HOT_MIN_SEG, HOT_MIN_SEG - 1
        elif j == 8:
            c[:10], c[10:J], c[J:J + N] = HOT_CAND_MIN - 1, HOT_CAND_MIN, HOT_MIN_SEG - 1
        elif j == 11:
            c[:10], c[10:J] = 100, HOT_CAND_MIN
            c[10] -= 1
            c[ALT] = 1
            c[J:J + 5], c[J + 5:J + 10] = HOT_MIN_SEG, HOT_MIN_SEG - 1
        elif j >= 18:
            c[:J] = HOT_MIN_SEG
        return c

    want = {0: 0, 1: 0, 2: 20, 7: 20, 8: 20, 9: 20, 10: 10, 11: 10, 12: 14, 15: 14, 16: 14, 17: 14, 18: 0, 19: 0, 20: 20}
    o, e = pair(local_cache)
    got = {}
    for j in range(21):
        b = hc.make_batch(allk, hc.mix(counts(j), np.random.default_rng(j)), T + 100 + j)
        hc.submit_checked(o, e, b, f"thresholds local={local_cache} batch {j}")
        s = e.stats()
        got[j] = s["hot_keys"]
        assert s["lsd_fallbacks"] == (1 if j >= 11 else 0), (j, s)
    assert {j: got[j] for j in want} == want, got
    assert e.stats()["inserted_keys"] == o.num_strings()
    e.close()


# ---- churn with batches in flight ----------------------------------------------------------------
CHURN_N = 32


@functools.lru_cache(maxsize=None)
def churn_batches():
    """Populations A and B of 200 keys. A is hot at first; B rises while A stays just above the
    stay threshold (the set fills: 200 + 56), then A falls away (B takes the set: 200), then A
    returns (full again). Two batches per second."""
    A = B = 200
    keys = hc.keys_of([b"hs_a_%d_tail_" % i for i in range(A)] + [b"hs_b_%d_tail_" % i for i in range(B)] + hc.cold(200))
    out = []
    for j in range(CHURN_N):
        c = np.full(len(keys), 2)
        a, b = ((HOT_MIN_SEG, 0) if j < 6 else (HOT_CAND_MIN + 6, HOT_MIN_SEG) if j < 12 else
                (8, HOT_MIN_SEG) if j < 20 else (HOT_MIN_SEG, HOT_MIN_SEG))
        c[:A], c[A:A + B] = a, b
        out.append(hc.make_batch(keys, hc.mix(c, np.random.default_rng(300 + j)), T + 200 + j // 2))
    return out


@functools.lru_cache(maxsize=None)
def churn_reference(local_cache):
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(hc.RULES)
    return [o.submit(b) for b in churn_batches()], o.num_strings()


@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("depth", [2, 3])
def test_churn_with_batches_in_flight(depth, local_cache):
    """The set shrinks and refills, so hot indices shift, while `depth` device batches are in
    flight on the three versioned hot tables."""
    dev = torch.device("cuda", 0)
    hbs = churn_batches()
    ref, n_strings = churn_reference(local_cache)
    _, e = pair(local_cache, BIG_TABLE)
    dbs = [router.DeviceBatch.from_host(hb, dev) for hb in hbs]
    outs = [torch.zeros(db.n_desc * 20, dtype=torch.uint8, device=dev) for db in dbs]
    thrs = [torch.zeros(db.n_req, dtype=torch.int32, device=dev) for db in dbs]
    torch.cuda.synchronize()
    traj, pending = [], 0
    for k, db in enumerate(dbs):
        e.submit_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), outs[k].data_ptr(), thrs[k].data_ptr())
        pending += 1
        if pending == depth:
            e.wait()
            traj.append(e.stats()["hot_keys"])
            pending -= 1
    for _ in range(pending):
        e.wait()
        traj.append(e.stats()["hot_keys"])
    torch.cuda.synchronize()
    for k, hb in enumerate(hbs):
        streams.assert_same(*ref[k], outs[k].cpu().numpy().view(hiprl.STATUS_DTYPE),
                            thrs[k].cpu().numpy().view(np.uint32), f"churn depth={depth} local={local_cache} batch {k}")
    s = e.stats()
    print(f"churn depth={depth} local={local_cache}: hot_keys {traj}, fallbacks {s['lsd_fallbacks']}")
    assert s["batches"] == CHURN_N and s["inserted_keys"] == n_strings and s["lsd_fallbacks"] == 0, s
    full = traj.index(HOT_MAX) if HOT_MAX in traj else -1
    assert full >= 0 and any(0 < x < HOT_MAX for x in traj[full:]), traj
    changes = sum(1 for x, y in zip(traj, traj[1:]) if x != y)
    assert changes >= 3, traj
    e.close()


# ---- clustering --------------------------------------------------------------------------------
@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("family", ["clustered", "wrapping", "two_lane"])
def test_clustered_hot_set(family, local_cache):
    """The index sweep's K = 256 case and the write-back on a set that is one probe chain (or 16):
    every lookup is settled by the (a, b) confirmation. The cold tail holds non-members that
    start at the family's home, chain-mates among them, which walk the whole chain."""
    o, e, keys, b = sweep_case(family, 256, local_cache, jitter=not local_cache)
    check_write_back(o, e, keys, 256, b, local_cache, f"{family} local={local_cache}")
    e.close()


@pytest.mark.parametrize("family", ["clustered", "wrapping"])
def test_unused_byte_values_walk_the_chain(family):
    """199 of the family's 256 byte values are hot; one batch carries every other value: each
    misses behind 199 equal tag words."""
    K = 199
    hot = hc.FAMILIES[family](K)
    unused = hc.unused_values(hot)
    assert len(unused) == 256 - K and len({hc.home_tag(p) for p in hot + unused}) == 1
    keys = hc.keys_of(hot + unused + hc.cold(N_COLD))
    o, e = pair(True)
    fb = hc.teach(o, e, keys, T - 4, n_hot=K)
    b = hc.checked_batch(keys, K, extra=np.arange(K, 256))
    blob = b.blob.tobytes()
    assert set(unused) <= {blob[int(b.off[i]):int(b.off[i + 1])] for i in range(b.n_desc)}
    hc.submit_checked(o, e, b, f"{family} unused values")
    s = e.stats()
    assert s["hot_keys"] == K and s["lsd_fallbacks"] == fb and s["inserted_keys"] == o.num_strings(), s
    e.close()
