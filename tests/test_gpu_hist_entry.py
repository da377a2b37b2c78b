"""k4_hist's entry, against the oracle.

A tile issues its descriptor loads first and copies the hot table into LDS, and zeroes its
LDS counters and its share of the request throttles, under their latency; the barrier that
publishes the table is passed while the second load level is in flight. These batches read the
table right behind that barrier in every tile: hot descriptors of both window parities at the
head of each tile, in one tile, a partial tile and a few tiles, with requests of several
descriptors (the throttle words every tile zeroes) and the local cache on and off.
"""

import numpy as np
import pytest

import hiprl
import oracle
import streams
import workload

pytestmark = pytest.mark.gpu

NOW = 1_700_000_100  # the first second of a minute: NOW - 1 lies in the minute before
TILE = 2048          # V4_TILE
RULES = [(10, hiprl.SECOND), (600, hiprl.MINUTE), (36000, hiprl.HOUR)]
HOT_IDS = (0, 1, 2, 3)  # rule = id % 2: ids 0 and 2 are SECOND keys, 1 and 3 MINUTE keys


def _batch(ids, nows, per_req):
    """Key "he_k_<id>_" under rule id % 2, `per_req` descriptors per request (the last request
    takes the rest), request times as given (non-decreasing)."""
    ids = np.asarray(ids, np.uint64)
    n = len(ids)
    req_of = (np.arange(n) // per_req).astype(np.uint32)
    n_req = int(req_of[-1]) + 1
    blob, off = workload.prefix_blob([b"he_k_", ids, b"_"])
    now = np.asarray(nows, np.int64)[np.arange(n_req) * per_req]
    return hiprl.Batch(blob, off, (ids % np.uint64(2)).astype(np.uint32), req_of, now,
                       (1 + np.arange(n_req) % 3).astype(np.uint32))


def _teach(o, e, rng, t):
    """Two batches that make HOT_IDS the hot set (300-600 descriptors each: at least HOT_MIN_SEG,
    no MSD bucket over BUCKET_CAP). The first batch's candidates become the set after the second
    one's submit, so the batch after these two is the first that finds hot prefixes."""
    for k in range(2):
        ids = np.concatenate([np.full(300 + 100 * h, h) for h in HOT_IDS] + [1000 + 2 * rng.integers(0, 4000, 3000)])
        rng.shuffle(ids)
        b = _batch(ids, np.full(len(ids), t), 1)
        streams.assert_same(*o.submit(b), *e.submit(b), f"teaching batch {k}")


@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("n", [1, 700, TILE, TILE + 1, 4 * TILE + 77])
def test_hot_lookups_at_tile_heads(n, local_cache):
    rng = np.random.default_rng(n)
    o = oracle.Oracle(near_limit_ratio=0.8, local_cache=local_cache)
    o.load_rules(RULES)
    e = hiprl.Engine(near_limit_ratio=0.8, local_cache=local_cache, pipeline="v4", max_batch_desc=1 << 14)
    e.load_rules(RULES)
    _teach(o, e, rng, NOW - 1)
    pos = np.arange(n)
    # the first 64 descriptors of every tile (wave 0's first loads) and a quarter of the rest
    hot = (pos % TILE < 64) | (rng.random(n) < 0.25)
    ids = np.where(hot, pos % 4, 1000 + 2 * rng.integers(0, 3 * n + 10, n))
    b = _batch(ids, NOW + (pos >= n // 2), 3)
    streams.assert_same(*o.submit(b), *e.submit(b), f"n={n} local={local_cache}")
    s = e.stats()
    assert s["hot_keys"] == len(HOT_IDS) and s["lsd_fallbacks"] == 0, s
    assert s["inserted_keys"] == o.num_strings(), (s, o.num_strings())
