"""k4_group's hand-off from k4_scan and its last-block epilogue, against the oracle.

The v4 pipeline sums every block's key count and new-slot counts into sharded counters of the
batch's control block; the last k4_group block reads them, updates the occupancy and writes
the host's summary. These streams pin what travels that way (unique keys per batch, inserted
keys, live slots per region) next to the usual bit-exact statuses. The batch shapes are those
at which k4_group's gather of a range's records from the tiles' bucket-start columns takes
another path: one tile and the sizes around it, more than 512 tiles (a second chunk of tiles)
with 64 ranges per group, nearly empty groups, split and whole ranges in one group; then
batches in flight around a refused one, and a candidate-sampling batch.
"""

import numpy as np
import pytest
import torch

import hiprl
import oracle
import router
import streams
import workload
from streams import RULES
from test_gpu_parity import _bucket_keys, hot_stream

pytestmark = pytest.mark.gpu

NOW = 1_700_000_100


def _pair(local_cache=False, rules=RULES, **kw):
    o = oracle.Oracle(near_limit_ratio=0.8, local_cache=local_cache)
    o.load_rules(rules)
    kw.setdefault("max_batch_desc", 1 << 14)
    e = hiprl.Engine(near_limit_ratio=0.8, local_cache=local_cache, pipeline="v4", **kw)
    e.load_rules(rules)
    return o, e


def _strings(b, rules=RULES):
    """The batch's distinct key strings as (prefix bytes, window start) pairs."""
    div = np.array([hiprl.UNIT_DIVIDER[u] for _, u in rules], np.int64)[b.rule]
    ws = b.now[b.req_of] // div * div
    blob = b.blob.tobytes()
    return {(blob[int(b.off[i]):int(b.off[i + 1])], int(ws[i])) for i in range(b.n_desc)}


def _live(strings):
    """Live slots per region after `strings` arrived in time order on a lone engine: the
    strings of each region's newest window generation (rl_common.h occ_advance)."""
    gen = [0] * 8
    cnt = {}
    for ws in {w for _, w in strings}:
        r, g = oracle.place(ws)
        gen[r] = max(gen[r], g)
    for _, ws in strings:
        p = oracle.place(ws)
        cnt[p] = cnt.get(p, 0) + 1
    return [cnt.get((r, gen[r]), 0) for r in range(8)], gen


def _check_counts(e, o, strings):
    s = e.stats()
    assert s["inserted_keys"] == o.num_strings() == len(strings), (s, o.num_strings(), len(strings))
    occ = e.occupancy()
    live, gen = _live(strings)
    assert occ["live"] == live, (occ, live)
    assert [g for g, n in zip(occ["gen"], live) if n] == [g for g, n in zip(gen, live) if n], (occ, gen)


def _unit_rule(i):
    return (i % 4) * 4 + (i // 4) % 4  # every unit, every limit


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 3 * 2048 + 5])
def test_tile_count_edges(n):
    """One cold batch of n distinct keys: one tile, the sizes around the tile and a few tiles."""
    reqs = [("tc", [[("k", str(i))]], [_unit_rule(i)], 1 + i % 3, NOW) for i in range(n)]
    b = hiprl.build_batch(reqs)
    o, e = _pair()
    streams.assert_same(*o.submit(b), *e.submit(b), f"n={n}")
    strings = _strings(b)
    assert len(strings) == n
    assert e.last_batch_info()["unique_keys"] == n
    assert e.stats()["lsd_fallbacks"] == 0, e.stats()
    _check_counts(e, o, strings)
    assert sum(e.occupancy()["live"]) == n


def test_many_tiles_many_ranges():
    """513 tiles and 3 descriptors over ~1.5e6 uniform keys: buckets average 513 records, so
    every range is one bucket, each group has 64 ranges (a block takes a third and later
    range) and the gather needs its second chunk of tiles."""
    d = 513 * 2048 + 3
    b = workload.config2_batch(0, d=d, N=1_500_000)
    o, e = _pair(rules=workload.CONFIG2_RULES, log2_slots=(23, 12, 12, 12), max_batch_desc=d, max_batch_req=d,
                 max_blob_bytes=int(b.blob.shape[0]) + 64)
    streams.assert_same(*o.submit(b, threads=8), *e.submit(b), "513 tiles")
    s = e.stats()
    assert s["lsd_fallbacks"] == 0, s
    u = o.num_strings()  # one cold batch: every distinct key is a new string
    assert e.last_batch_info()["unique_keys"] == u and s["inserted_keys"] == u, (s, u, e.last_batch_info())
    assert sum(e.occupancy()["live"]) == u


def test_nearly_empty_groups():
    """Two batches of 300 descriptors over 5 keys: most runs are empty, most groups have no range."""
    o, e = _pair()
    strings = set()
    for k in range(2):
        reqs = [("ne", [[("k", str(i % 5))]], [_unit_rule(i % 5)], 1 + i % 2, NOW) for i in range(300)]
        b = hiprl.build_batch(reqs)
        streams.assert_same(*o.submit(b), *e.submit(b), f"batch {k}")
        assert e.last_batch_info()["unique_keys"] == 5
        strings |= _strings(b)
    assert e.stats()["lsd_fallbacks"] == 0, e.stats()
    _check_counts(e, o, strings)


@pytest.mark.parametrize("local_cache", [False, True])
def test_split_and_whole_ranges_in_one_group(local_cache):
    """Keys a and b (~480 descriptors each) share one MSD bucket in different fingerprint
    halves, so the bucket is split into two half ranges; key c fills most of another bucket;
    cold keys of the same 64-bucket group give that group whole-bucket ranges as well."""
    a, b_, bkt = _bucket_keys("sp", NOW)
    c = next(i for i in range(len(bkt)) if bkt[i] != bkt[a])
    mates = [i for i in range(len(bkt)) if bkt[i] >> np.uint64(6) == bkt[a] >> np.uint64(6) and bkt[i] != bkt[a]
             and i != c]
    assert len(mates) >= 64, len(mates)
    rng = np.random.default_rng(11)
    reqs = []
    for i in range(8000):
        x = rng.random()
        if x < 0.06:
            k = a
        elif x < 0.12:
            k = b_
        elif x < 0.22:
            k = c
        elif x < 0.45:
            k = mates[int(rng.integers(0, len(mates)))]
        else:
            k = 20000 + int(rng.integers(0, 3000))
        reqs.append(("sp", [[("k", str(k))]], [2], int(rng.integers(0, 3)), NOW))  # SECOND L=10
    b = hiprl.build_batch(reqs)
    o, e = _pair(local_cache)
    streams.assert_same(*o.submit(b), *e.submit(b), f"split + whole local={local_cache}")
    assert e.stats()["lsd_fallbacks"] == 0, e.stats()
    strings = _strings(b)
    assert e.last_batch_info()["unique_keys"] == len(strings)
    _check_counts(e, o, strings)


@pytest.mark.parametrize("depth", [2, 3])
def test_counters_across_batches_in_flight(depth):
    """Six batches, `depth` in flight, the SECOND window rolling over after every second one
    (the last two advance the generation of the first two's region). Batch 2
    carries a key with 1500 descriptors and no hot set: it is refused, the batch behind it is
    poisoned, and both are rerun on the LSD pipeline (fallbacks are expected here). Every
    batch's unique keys, and in the end the inserted keys and the live slots per region, are
    the oracle's: nothing is counted twice on a rerun or left over from a batch in flight."""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    hbs = []
    for k in range(6):
        t = NOW + k // 2
        reqs = []
        for i in range(3000):
            if k == 2 and i < 1500:
                key, rule = "big", 2
            else:
                kid = int(rng.integers(0, 4000))
                key, rule = f"k{kid}", _unit_rule(kid)
            reqs.append(("cf", [[("k", key)]], [rule], int(rng.integers(0, 4)), t))
        hbs.append(hiprl.build_batch(reqs))
    o, e = _pair()
    ref = [o.submit(hb) for hb in hbs]
    dbs = [router.DeviceBatch.from_host(hb, dev) for hb in hbs]
    outs = [torch.zeros(db.n_desc * 20, dtype=torch.uint8, device=dev) for db in dbs]
    thrs = [torch.zeros(db.n_req, dtype=torch.int32, device=dev) for db in dbs]
    torch.cuda.synchronize()
    unique, pending = [], 0
    for k, db in enumerate(dbs):
        e.submit_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), outs[k].data_ptr(), thrs[k].data_ptr())
        pending += 1
        if pending == depth:
            e.wait()
            unique.append(e.last_batch_info()["unique_keys"])
            pending -= 1
    for _ in range(pending):
        e.wait()
        unique.append(e.last_batch_info()["unique_keys"])
    torch.cuda.synchronize()
    strings = set()
    for k, hb in enumerate(hbs):
        streams.assert_same(*ref[k], outs[k].cpu().numpy().view(hiprl.STATUS_DTYPE),
                            thrs[k].cpu().numpy().view(np.uint32), f"depth={depth} batch {k}")
        strings |= _strings(hb)
    assert unique == [len(_strings(hb)) for hb in hbs], unique
    s = e.stats()
    assert s["lsd_fallbacks"] >= 1 and s["batches"] == 6, s
    _check_counts(e, o, strings)


@pytest.mark.parametrize("local_cache", [False, True])
def test_hot_set_through_candidate_batch(local_cache):
    """Ten batches of a stream with two steady hot keys: the set is learned from the first
    batch, so the ninth is the next one whose candidates are sampled, with a hot set in place."""
    reqs, sizes = hot_stream(10, 2000, t0=NOW - 3, seed=3 + local_cache)
    o, e = _pair(local_cache)
    streams.assert_same(*streams.replay(o, reqs, sizes), *streams.replay(e, reqs, sizes), f"local={local_cache}")
    s = e.stats()
    assert s["hot_keys"] >= 2 and s["lsd_fallbacks"] == 0, s
    assert s["inserted_keys"] == o.num_strings(), s
