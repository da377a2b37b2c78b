"""k4_group's key lists laid out by all four waves, against the oracle.

A staged range of m records is cut into four parts of whole 64-position chunks
(64 * ceil(m / 256) positions each, the last ones short or empty); every wave lays out its own
part, and one packed word per hash slot carries the key's records per part, its total and the
mixed-rule flags. A key's list must still hold its positions in arrival order: the INCRBY
prefix, the local cache's freeze search and the freezing request's last INCRBY all read it.
The cases put one key, or a few keys of one range, on every part and chunk boundary, send the
flags and the freeze through the packed word, and run a dense stream in which every group
holds ranges of several hundred records. Every case is bit-exact against the oracle and
checks that the batch stayed on the v4 pipeline (lsd_fallbacks == 0).
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
from test_gpu_group_runs import _check_counts, _strings

pytestmark = pytest.mark.gpu

NOW = 1_700_000_100  # a multiple of 60: the SECOND and the MINUTE window start there
SEED = 0x5EE7AB1E5EED  # the engine's default hash seed
S10 = 2  # RULES[2] = (10, SECOND)
# rules of the flag and freeze cases
XRULES = [(10, hiprl.SECOND), (40, hiprl.SECOND), (10, hiprl.MINUTE), (600, hiprl.SECOND), (510, hiprl.SECOND),
          (3, hiprl.SECOND), (100000, hiprl.SECOND), (90000, hiprl.SECOND), (100000, hiprl.MINUTE)]
X_S10, X_S40, X_M10, X_S600, X_S510, X_S3, X_BIG, X_BIG2, X_MBIG = range(9)


def _pair(local_cache=False, rules=RULES, **kw):
    o = oracle.Oracle(near_limit_ratio=0.8, local_cache=local_cache)
    o.load_rules(rules)
    kw.setdefault("max_batch_desc", 1 << 12)
    kw.setdefault("log2_slots", (16, 16, 12, 12))  # NOW starts a minute: its strings live in the MINUTE regions
    e = hiprl.Engine(near_limit_ratio=0.8, local_cache=local_cache, pipeline="v4", **kw)
    e.load_rules(rules)
    return o, e


_BKT = {}


def _buckets(dom, n=20000):
    """MSD bucket (fingerprint bits 63..53) of the key strings dom_k_<id>_ at window start NOW,
    ids 0..n-1, computed once per domain."""
    if dom not in _BKT:
        ids = np.arange(n, dtype=np.uint64)
        blob, off = workload.prefix_blob([dom.encode() + b"_k_", ids, b"_"])
        hi, _ = oracle.fingerprints(blob, off, NOW, SEED)
        bkt = (hi >> np.uint64(53)).astype(np.int64)
        bkt.setflags(write=False)
        _BKT[dom] = bkt
    return _BKT[dom]


def _same_bucket(dom, k):
    """k key ids of one MSD bucket."""
    bkt = _buckets(dom)
    vals, cnt = np.unique(bkt, return_counts=True)
    b = int(vals[np.nonzero(cnt >= k)[0][0]])
    return [int(i) for i in np.nonzero(bkt == b)[0][:k]]


def _adjacent_buckets(dom):
    """Two key ids in adjacent MSD buckets of one 64-bucket group, lower bucket first."""
    bkt = _buckets(dom)
    first = {}
    for i, b in enumerate(bkt.tolist()):
        first.setdefault(b, i)
    for b, i in sorted(first.items()):
        if b % 64 != 63 and b + 1 in first:
            return i, first[b + 1]
    raise AssertionError("no adjacent buckets")


def _req(dom, key, rule, hits, now=NOW, n_desc=1):
    return (dom, [[("k", str(key))]] * n_desc, [rule] * n_desc, hits, now)


def _run_one(reqs, ctx, local_cache=False, rules=RULES, **kw):
    b = hiprl.build_batch(reqs)
    o, e = _pair(local_cache, rules, **kw)
    streams.assert_same(*o.submit(b), *e.submit(b), ctx)
    assert e.stats()["lsd_fallbacks"] == 0, e.stats()
    return b, o, e


# 1. one key, n records: m = n in one range ------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768,
                               769, 895, 896])
def test_one_key_n_records(n):
    """Every part and chunk boundary of the split: parts of 64, 128, 192 and 256 positions. The
    limit is never reached, so every descriptor's limit_remaining shows its own INCRBY reply,
    that is its place in the key's list."""
    reqs = [_req("one", 7, X_BIG, 1 + i % 3) for i in range(n)]
    b, o, e = _run_one(reqs, f"one key n={n}", rules=XRULES)
    assert e.last_batch_info()["unique_keys"] == 1


@pytest.mark.parametrize("local_cache", [False, True])
def test_one_key_896_wrapping_addends(local_cache):
    """896 records of 2^32 - 1 hits each: the 64-bit prefix across the parts, the u32 counter wraps."""
    reqs = [_req("one", 7, S10, 0xFFFFFFFF) for _ in range(896)]
    _run_one(reqs, f"wrap local={local_cache}", local_cache)


# 2. two and three keys of one range ---------------------------------------------------------

def _pattern_keys(name, keys):
    """896 positions -> key per position."""
    a, b, c = (list(keys) + [keys[0]])[:3]
    out = []
    for p in range(896):
        lane, part = p % 64, p // 256
        if name == "alternating":
            out.append(keys[p % len(keys)])
        elif name == "first_last":  # A only in the first and the last part, B at lane 0 and 63 of every chunk
            out.append(b if lane in (0, 63) else a if part in (0, 3) else c)
        else:
            raise AssertionError(name)
    return out


@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("nkeys,pattern", [(2, "alternating"), (3, "alternating"), (3, "first_last")])
def test_keys_of_one_bucket(nkeys, pattern, local_cache):
    """Keys of one MSD bucket interleaved in one range of exactly 896 records (limit never reached)."""
    keys = _same_bucket("kb", nkeys)
    reqs = [_req("kb", k, X_BIG, 1 + i % 3) for i, k in enumerate(_pattern_keys(pattern, keys))]
    b, o, e = _run_one(reqs, f"{nkeys} keys {pattern} local={local_cache}", local_cache, XRULES)
    assert e.last_batch_info()["unique_keys"] == nkeys


@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("na", [1, 64, 255, 256, 257, 448, 895])
def test_keys_of_adjacent_buckets(na, local_cache):
    """Two keys in adjacent buckets of one group, 896 records together: k4_scan packs both
    buckets into one range, key A's na records in front of key B's (bucket order), so B's list
    starts anywhere in a part. The keys alternate in arrival order."""
    a, b_ = _adjacent_buckets("ab")
    seq = []
    ca, cb = na, 896 - na
    while ca or cb:
        if ca and (ca >= cb or not cb):
            seq.append(a)
            ca -= 1
        if cb and (cb >= ca or not ca):
            seq.append(b_)
            cb -= 1
    assert len(seq) == 896 and seq.count(a) == na
    reqs = [_req("ab", k, X_BIG, 1 + i % 3) for i, k in enumerate(seq)]
    b, o, e = _run_one(reqs, f"adjacent na={na} local={local_cache}", local_cache, XRULES)
    assert e.last_batch_info()["unique_keys"] == 2


# 3. flags through the packed word -----------------------------------------------------------

@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("first_rule,second_rule", [(X_S10, X_S40), (X_S10, X_M10), (X_BIG, X_BIG2), (X_BIG, X_MBIG)],
                         ids=["mixed", "mixed_unit", "mixed_big", "mixed_unit_big"])
@pytest.mark.parametrize("where", ["half", "last", "first"])
def test_mixed_rules_across_parts(where, first_rule, second_rule, local_cache):
    """One key string under two rules: of one unit (the mixed flag: per-record limits), or of
    two units whose windows start together (the mixed-unit flag: the exact sequential pass).
    600 records (parts of 192): the second rule on the later half, on the last record alone
    (fourth part) or on the first record alone. Limits of 10 and 40 are crossed early; the
    big ones never, so that every reply shows its record's own limit and place in the list."""
    n = 600
    other = {"half": lambda i: i >= n // 2, "last": lambda i: i == n - 1, "first": lambda i: i == 0}[where]
    reqs = [_req("mx", 3, second_rule if other(i) else first_rule, 1 + i % 2) for i in range(n)]
    _run_one(reqs, f"flags {where} rule={second_rule} local={local_cache}", local_cache, XRULES)


# 4. the local cache's freeze over list order ---------------------------------------------

def test_freeze_in_third_part():
    """800 records of one hit, limit 600: record 600 (third part of 256) crosses it; the
    freeze search runs over the list in arrival order."""
    reqs = [_req("fz", 5, X_S600, 1) for _ in range(800)]
    _run_one(reqs, "freeze third part", True, XRULES)


@pytest.mark.parametrize("lead", [509, 507, 253])
def test_freezing_request_straddles_parts(lead):
    """`lead` one-descriptor requests, then one request with six descriptors of the key whose
    positions straddle a part boundary (256 or 512) and which crosses the limit of 510 or is
    far below it, then the rest up to 800: the INCRBYs of the freezing request still happen."""
    reqs = [_req("fz", 5, X_S510, 1) for _ in range(lead)]
    reqs.append(_req("fz", 5, X_S510, 1, n_desc=6))
    reqs += [_req("fz", 5, X_S510, 1) for _ in range(800 - lead - 6)]
    _run_one(reqs, f"freezing request lead={lead}", True, XRULES)


def test_key_frozen_before_batch():
    """Batch 1 freezes key F (100 records, limit 3: below the hot-set threshold). Batch 2, same
    second: F's 100 records spread over a range that it shares with 600 records of a bucket
    mate, so the frozen key's list runs through every part."""
    f, mate = _same_bucket("fb", 2)
    o, e = _pair(True, XRULES)
    b1 = hiprl.build_batch([_req("fb", f, X_S3, 1) for _ in range(100)])
    streams.assert_same(*o.submit(b1), *e.submit(b1), "freezing batch")
    reqs = [_req("fb", f if i % 7 == 0 else mate, X_S3 if i % 7 == 0 else X_BIG, 1 + i % 2) for i in range(700)]
    b2 = hiprl.build_batch(reqs)
    st, thr = e.submit(b2)
    streams.assert_same(*o.submit(b2), st, thr, "frozen before")
    hit = (st["code_flags"] >> 8) & hiprl.FLAG_LOCAL_CACHE_HIT
    assert int(hit.astype(bool).sum()) == 100  # every descriptor of F is a local-cache hit
    assert e.stats()["lsd_fallbacks"] == 0, e.stats()


# 5. a dense stream --------------------------------------------------------------------------

@pytest.mark.parametrize("local_cache", [False, True])
def test_dense_stream_two_in_flight(local_cache):
    """Four batches of ~20 000 descriptors over ~1 500 keys, multiplicities 1..127 (no key
    turns hot), two in flight, the second pair one second later: all 32 groups hold ranges of
    several hundred records."""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17)
    hbs = []
    for k in range(4):
        t = NOW + k // 2
        mult = 1 + (127 * rng.random(1500) ** 8).astype(np.int64)  # 1..127, mean ~15
        keys = rng.choice(3000, size=1500, replace=False)
        seq = np.repeat(keys, mult)
        rng.shuffle(seq)
        reqs = [("ds", [[("k", str(int(x)))]], [int(x) % 4], 1 + i % 3, t) for i, x in enumerate(seq)]  # SECOND, L by key
        hbs.append(hiprl.build_batch(reqs))
    o, e = _pair(local_cache, max_batch_desc=1 << 15)
    ref = [o.submit(hb) for hb in hbs]
    dbs = [router.DeviceBatch.from_host(hb, dev) for hb in hbs]
    outs = [torch.zeros(db.n_desc * 20, dtype=torch.uint8, device=dev) for db in dbs]
    thrs = [torch.zeros(db.n_req, dtype=torch.int32, device=dev) for db in dbs]
    torch.cuda.synchronize()
    unique, pending = [], 0
    for k, db in enumerate(dbs):
        e.submit_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), outs[k].data_ptr(), thrs[k].data_ptr())
        pending += 1
        if pending == 2:
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
                            thrs[k].cpu().numpy().view(np.uint32), f"dense local={local_cache} batch {k}")
        strings |= _strings(hb)
    assert unique == [len(_strings(hb)) for hb in hbs], unique
    assert min(hb.n_desc for hb in hbs) >= 15000
    assert e.stats()["lsd_fallbacks"] == 0, e.stats()
    _check_counts(e, o, strings)


# 6. both storage paths in one batch -------------------------------------------------------

@pytest.mark.parametrize("local_cache", [False, True])
def test_global_scratch_beside_lds_ranges(local_cache):
    """Key C has 950 records: its bucket is over the LDS stage and so is its fingerprint half,
    so it is grouped in the block's global scratch (the one-wave layout), in one batch with
    ordinary ranges (3 000 records over 1 000 keys, up to 9 a key)."""
    rng = np.random.default_rng(23)
    seq = np.concatenate([np.full(950, 1_000_000), rng.integers(0, 1000, size=3000)])
    rng.shuffle(seq)
    reqs = [_req("gs", int(k), S10, 1 + i % 3) for i, k in enumerate(seq)]
    b, o, e = _run_one(reqs, f"global + LDS local={local_cache}", local_cache)
    strings = _strings(b)
    assert e.last_batch_info()["unique_keys"] == len(strings)
    _check_counts(e, o, strings)
