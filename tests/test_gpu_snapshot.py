"""Snapshot / restore of the counter table (rl_hip.h "Snapshot / restore") on the GPU: an engine
that saves and a new one that loads — of the same or another geometry — continue a request
stream bit-exactly as one oracle that never stopped decides it."""
import functools

import numpy as np
import pytest

import hiprl
import oracle
import streams
from streams import RULES, batch_sizes, make_stream

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC, ESTATE = -1, -3, -5
MAX_DESC = 1 << 14


def engine(local_cache=False, pipeline="v4", log2_slots=(16, 16, 16, 14), rules=RULES, **kw):
    kw.setdefault("max_batch_desc", MAX_DESC)
    e = hiprl.Engine(local_cache=local_cache, pipeline=pipeline, log2_slots=log2_slots, **kw)
    e.load_rules(rules)
    return e


def run(backend, batches):
    out = [backend.submit(b) for b in batches]
    return np.concatenate([s for s, _ in out]), np.concatenate([t for _, t in out])


def cat(outs):
    return np.concatenate([s for s, _ in outs]), np.concatenate([t for _, t in outs])


def sorted_set(recs):
    return np.sort(recs, order=["key", "ctrl"])


@functools.lru_cache(maxsize=None)
def stream(seed):
    """The parity suite's stream of a seed as batches, and the cut: the batch boundary nearest
    the middle request."""
    reqs = make_stream(seed, 6000, t0=1_700_000_000 - 7 + seed * 86400 - 130)
    sizes = batch_sizes(reqs, np.random.default_rng(seed + 100), 1500)
    ends = np.cumsum(sizes)
    cut = int(np.argmin(np.abs(ends - 3000))) + 1  # batches [0, cut) | [cut, ...)
    batches, i = [], 0
    for bs in sizes:
        batches.append(hiprl.build_batch(reqs[i:i + bs]))
        i += bs
    assert 0 < cut < len(batches)
    return batches, cut


@functools.lru_cache(maxsize=None)
def expected(seed, local_cache):
    """One oracle over the whole stream: per-batch outputs. Guards the tests that use it: a fresh
    oracle on the second half must decide it differently, so the cut always carries state."""
    batches, cut = stream(seed)
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(RULES)
    outs = [o.submit(b) for b in batches]
    f = oracle.Oracle(local_cache=local_cache)
    f.load_rules(RULES)
    fst, fthr = run(f, batches[cut:])
    cst, cthr = cat(outs[cut:])
    assert (fst != cst).sum() > 100 and (fthr != cthr).sum() > 10, "the cut carries no state"
    return outs


def continue_on(seed, local_cache, pipeline, tmp_path, log2_b=(16, 16, 16, 14)):
    batches, cut = stream(seed)
    want = cat(expected(seed, local_cache))
    a = engine(local_cache, pipeline)
    first = run(a, batches[:cut])
    path = tmp_path / "table.rlsnap"
    ha = a.save(path)
    live_a = a.stats()["live_keys"]
    a.close()
    b = engine(local_cache, pipeline, log2_slots=log2_b)
    hb = b.load(path)
    assert bytes(hb) == bytes(ha) and hb.n_records > 0
    assert b.stats()["live_keys"] == live_a
    rest = run(b, batches[cut:])
    got = np.concatenate([first[0], rest[0]]), np.concatenate([first[1], rest[1]])
    streams.assert_same(want[0], want[1], got[0], got[1],
                        f"seed={seed} local={local_cache} pipeline={pipeline} B={log2_b}")
    b.close()


@pytest.mark.parametrize("pipeline", ["v4", "lsd"])
@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_continuation_parity(seed, local_cache, pipeline, tmp_path):
    continue_on(seed, local_cache, pipeline, tmp_path)


@pytest.mark.parametrize("log2_b", [(14, 15, 17, 15), (18, 14, 14, 14)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_resize(seed, log2_b, tmp_path):
    """The loading engine's table differs in every region: records are placed by the key's top
    bits under the new region sizes."""
    continue_on(seed, True, "v4", tmp_path, log2_b=log2_b)


def test_tight_region_with_probe_wrap(tmp_path):
    """180 keys of one HOUR window into a 256-slot region (load limit 192): long probe chains,
    some past the region's end."""
    t = 1_700_000_000
    assert oracle.place(t // 3600 * 3600)[0] == 4  # an HOUR-home region
    rules = [(3, hiprl.HOUR)]
    batches = [hiprl.build_batch([("tight", [[("k", str(i))]], [0], 2, t) for i in range(j, j + 10)])
               for j in range(0, 180, 10)]
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)
    a = engine(True, rules=rules, max_batch_desc=64)
    streams.assert_same(*run(o, batches), *run(a, batches), "tight: first pass")
    path = tmp_path / "tight.rlsnap"
    h = a.save(path)
    assert h.n_records == 180 and list(h.live)[4] == 180
    a.close()
    b = engine(True, rules=rules, max_batch_desc=64, log2_slots=(8, 8, 8, 8))
    b.load(path)
    occ = b.occupancy()
    assert occ["live"][4] == 180 and occ["limit"][4] == 192 and occ["slots"][4] == 256, occ
    streams.assert_same(*run(o, batches), *run(b, batches), "tight: second pass")
    assert b.occupancy()["live"][4] == 180
    assert b.stats()["inserted_keys"] == 0  # every key found its restored slot


def test_record_set_invariants():
    batches, cut = stream(1)
    a = engine(True)
    run(a, batches[:cut])
    h1, r1 = a.snapshot_records()
    h2, r2 = a.snapshot_records()
    assert bytes(h1) == bytes(h2)
    assert np.array_equal(sorted_set(r1), sorted_set(r2))
    occ = a.occupancy()
    # times only move forward in this stream: the occupancy mirror is exact, and without the lag
    # window no region keeps a previous generation
    assert h1.n_records == r1.shape[0] == sum(occ["live"]) and list(h1.prev) == [0] * 8
    assert list(h1.gen) == occ["gen"] and list(h1.live) == occ["live"]
    assert np.unique(r1[["ctrl", "key"]]).shape[0] == r1.shape[0]
    gens = (r1["ctrl"] & 0xFFFFFFFF).astype(np.uint32)
    regions = (r1["key"] >> np.uint64(61)).astype(np.int64)
    assert np.array_equal(gens, np.array(list(h1.gen), np.uint32)[regions])
    assert np.array_equal(np.bincount(regions, minlength=8), np.array(list(h1.live)))
    b = engine(True, log2_slots=(15, 17, 15, 16))
    b.restore_records(h1, r1)
    h3, r3 = b.snapshot_records()
    assert np.array_equal(sorted_set(r3), sorted_set(r1))
    assert list(h3.gen) == list(h1.gen) and list(h3.live) == list(h1.live) and h3.n_records == h1.n_records
    assert list(h3.src_log2) == [15, 15, 17, 17, 15, 15, 16, 16] and list(h1.src_log2) == [16] * 6 + [14] * 2
    ob = b.occupancy()
    assert ob["gen"] == occ["gen"] and ob["live"] == occ["live"]
    assert b.stats()["live_keys"] == a.stats()["live_keys"] == h1.n_records


@functools.lru_cache(maxsize=None)
def chunk_state():
    """5,000 live records over three regions (MINUTE, HOUR, DAY homes), from one engine."""
    t = 1_700_000_000 + 17
    rules = [(5, hiprl.MINUTE), (5, hiprl.HOUR), (5, hiprl.DAY)]
    a = engine(rules=rules)
    for j in range(0, 5000, 2500):
        a.submit(hiprl.build_batch([("chunk", [[("k", str(i))]], [i % 3], 1 + i % 4, t) for i in range(j, j + 2500)]))
    h, recs = a.snapshot_records()
    assert h.n_records == 5000
    return h, sorted_set(recs), a


@pytest.mark.parametrize("cap", [1, 7, 4096])
def test_drain_chunking(cap):
    h, want, a = chunk_state()
    h2, recs = a.snapshot_records(cap=cap)
    assert bytes(h2) == bytes(h) and np.array_equal(sorted_set(recs), want)


@pytest.mark.parametrize("chunk", [1, 63, 65, 4097])
def test_put_chunking(chunk):
    h, want, _ = chunk_state()
    b = engine(log2_slots=(14, 14, 14, 14), max_batch_desc=64)
    b.restore_records(h, want, chunk=chunk)
    h2, recs = b.snapshot_records()
    assert np.array_equal(sorted_set(recs), want) and list(h2.live) == list(h.live)


def fresh_check(e, local_cache=False, ctx="fresh", per_second_split=False):
    """`e` decides a small stream as an engine (oracle) that never saw a request."""
    reqs = make_stream(9, 500, t0=1_700_400_000 - 3)
    sizes = batch_sizes(reqs, np.random.default_rng(9), 200)
    o = oracle.Oracle(local_cache=local_cache, per_second_split=per_second_split)
    o.load_rules(RULES)
    streams.assert_same(*streams.replay(o, reqs, sizes), *streams.replay(e, reqs, sizes), ctx)


def test_empty_engine_round_trip(tmp_path):
    a = engine(True)
    h, recs = a.snapshot_records()
    assert h.n_records == 0 and recs.shape[0] == 0 and list(h.gen) == [0] * 8
    path = tmp_path / "empty.rlsnap"
    a.save(path)
    assert path.stat().st_size == 256
    b = engine(True, log2_slots=(12, 12, 12, 12))
    b.load(path)
    assert b.stats()["live_keys"] == 0 and b.occupancy()["live"] == [0] * 8
    fresh_check(b, True, "after an empty restore")


def test_snapshot_is_point_in_time():
    batches, cut = stream(2)
    exp = expected(2, True)
    a = engine(True)
    outs = [a.submit(b) for b in batches[:cut]]
    h = a.snapshot_begin()
    outs += [a.submit(b) for b in batches[cut:cut + 2]]  # the table moves on; the device copy does not
    parts = []
    while True:
        part = a.snapshot_next(1000)
        if not part.shape[0]:
            break
        parts.append(part)
    a.snapshot_end()
    recs = np.concatenate(parts)
    assert recs.shape[0] == h.n_records
    outs += [a.submit(b) for b in batches[cut + 2:]]
    streams.assert_same(*cat(exp), *cat(outs), "the saving engine, throughout")
    b = engine(True)
    b.restore_records(h, recs)
    streams.assert_same(*cat(exp[cut:]), *run(b, batches[cut:]), "replay from the cut")


def hot_batches(n_batches, per_batch, t0, seed=3):
    """Batches dominated by three keys (SECOND, MINUTE and HOUR rules) over a cold tail, 1 s a batch."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(n_batches):
        reqs = []
        for _ in range(per_batch):
            x = rng.random()
            if x < 0.4:
                k, r = "h0", 2            # SECOND L=10
            elif x < 0.6:
                k, r = "h1", 3 + 4 * 1    # MINUTE L=40
            elif x < 0.75:
                k, r = "h2", 3 + 4 * 2    # HOUR L=40
            else:
                k, r = f"c{int(rng.integers(0, 3000))}", 3 + 4 * 3  # DAY L=40
            reqs.append(("hs", [[("k", k)]], [r], int(rng.integers(0, 4)), t0 + b))
        out.append(hiprl.build_batch(reqs))
    return out


@pytest.mark.parametrize("local_cache", [False, True])
def test_hot_set_is_relearned(local_cache, tmp_path):
    """Hot keys keep their counters in their table slots between batches: a snapshot taken while
    a hot set is in use restores them, and the loading engine learns its own hot set again."""
    batches = hot_batches(4, 12000, 1_700_000_000 - 2)
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(RULES)
    exp = [o.submit(b) for b in batches]
    a = engine(local_cache)
    first = [a.submit(b) for b in batches[:2]]
    assert a.stats()["hot_keys"] >= 2, a.stats()
    path = tmp_path / "hot.rlsnap"
    a.save(path)
    a.close()
    b = engine(local_cache)
    b.load(path)
    rest = [b.submit(x) for x in batches[2:]]
    streams.assert_same(*cat(exp), *cat(first + rest), f"hot set local={local_cache}")
    assert b.stats()["lsd_fallbacks"] <= 1 and b.stats()["hot_keys"] >= 2, b.stats()


@pytest.mark.parametrize("log2_b", [(8, 8, 8, 8), (10, 9, 8, 8)])
def test_lag_window_previous_generation_survives(log2_b, tmp_path):
    """Lag-window engines keep a SECOND region's previous generation (gen - 2) live: it is
    exported (header prev), imported beside the newest one, and a late batch finds its keys."""
    t = 1_700_000_001
    rules = [(5, hiprl.SECOND)]
    late = hiprl.build_batch([("lag", [[("a", str(i))]], [0], 1, t - 2) for i in range(30)])
    newest = hiprl.build_batch([("lag", [[("b", str(i))]], [0], 2, t) for i in range(60)])
    seq = [late, newest, late, newest, late, late, newest]
    o = oracle.Oracle()
    o.load_rules(rules)
    exp = [o.submit(b) for b in seq]
    a = engine(rules=rules, log2_slots=(8, 8, 8, 8), max_batch_desc=4096, lag_window=True)
    first = [a.submit(b) for b in seq[:3]]
    path = tmp_path / "lag.rlsnap"
    h = a.save(path)
    r = t % 2
    assert h.flags & hiprl.SNAP_LAG and list(h.gen)[r] == t + 1
    assert list(h.live)[r] == 60 and list(h.prev)[r] == 30 and h.n_records == 90
    a.close()
    b = engine(rules=rules, log2_slots=log2_b, max_batch_desc=4096, lag_window=True)
    b.load(path)
    rest = [b.submit(x) for x in seq[3:]]
    streams.assert_same(*cat(exp), *cat(first + rest), f"lag window into {log2_b}")
    assert b.stats()["inserted_keys"] == 0 and b.occupancy()["live"][r] == 60
    h2, recs = b.snapshot_records()
    assert list(h2.prev)[r] == 30 and list(h2.live)[r] == 60 and recs.shape[0] == 90


# ---- refusals --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def source():
    """A snapshot to refuse: the first half of seed 3, local cache on."""
    batches, cut = stream(3)
    a = engine(True)
    run(a, batches[:cut])
    h, recs = a.snapshot_records()
    a.close()
    return h, recs


@pytest.mark.parametrize("kw", [dict(hash_seed=0x1234), dict(per_second_split=True), dict(lag_window=True)],
                         ids=["hash_seed", "per_second_split", "lag_window"])
def test_restore_refused_before_anything_changes(kw):
    h, recs = source()
    t = engine(True, **kw)
    split = kw.get("per_second_split", False)
    o = oracle.Oracle(local_cache=True, per_second_split=split)
    o.load_rules(RULES)
    batches, _ = stream(1)
    streams.assert_same(*o.submit(batches[0]), *t.submit(batches[0]), "before the refusal")
    occ = t.occupancy()
    with pytest.raises(hiprl.RedisError) as ei:
        t.restore_begin(h)
    assert ei.value.code == EINVAL, ei.value
    assert t.occupancy() == occ
    streams.assert_same(*o.submit(batches[1]), *t.submit(batches[1]), "after the refusal: state kept")
    t.reset()
    fresh_check(t, True, "after a reset", per_second_split=split)


def test_lag_snapshot_refused_by_a_lone_engine():
    a = engine(lag_window=True)
    batches, _ = stream(1)
    a.submit(batches[0])
    h, _ = a.snapshot_records()
    t = engine()
    with pytest.raises(hiprl.RedisError) as ei:
        t.restore_begin(h)
    assert ei.value.code == EINVAL
    fresh_check(t)


def test_restore_refused_for_capacity():
    tm = 1_700_000_000
    rules = [(5, hiprl.HOUR)]
    a = engine(rules=rules)
    a.submit(hiprl.build_batch([("cap", [[("k", str(i))]], [0], 1, tm) for i in range(5000)]))
    h, recs = a.snapshot_records()
    assert h.n_records == 5000
    t = engine(rules=rules, log2_slots=(16, 16, 12, 14))  # HOUR regions: 4096 slots, limit 3072
    with pytest.raises(hiprl.RedisError) as ei:
        t.restore_begin(h)
    assert ei.value.code == ENOSPC, ei.value
    assert t.occupancy()["live"] == [0] * 8 and t.occupancy()["gen"] == [0] * 8 and t.stats()["live_keys"] == 0
    t.load_rules(RULES)
    fresh_check(t)


def test_duplicate_record_fails_restore_end():
    h, recs = source()
    for how in ("replaced", "far", "adjacent"):
        bad = recs.copy()
        if how == "replaced":      # same count, one identity twice — in one chunk
            bad[17] = bad[400]
        elif how == "far":         # the second copy arrives in a later chunk (found by the claim)
            bad[len(bad) - 1] = bad[3]
        else:                      # neighbours in one wave
            bad[101] = bad[100]
        t = engine(True)
        t.restore_begin(h)
        for i in range(0, len(bad), 1000):
            t.restore_put(bad[i:i + 1000])
        with pytest.raises(hiprl.RedisError) as ei:
            t.restore_end()
        assert ei.value.code == EINVAL, ei.value
        assert t.occupancy()["live"] == [0] * 8 and t.stats()["live_keys"] == 0
        assert t.snapshot_records()[0].n_records == 0
        fresh_check(t, True, f"after a failed restore ({how})")
        t.close()


def test_bad_generation_and_short_restore_fail_restore_end():
    h, recs = source()
    bad = recs.copy()
    bad["ctrl"][5] -= np.uint64(1)  # a generation that is not its region's
    for put in (bad, recs[:-1]):
        t = engine(True)
        t.restore_begin(h)
        t.restore_put(put)
        with pytest.raises(hiprl.RedisError) as ei:
            t.restore_end()
        assert ei.value.code == EINVAL
        assert t.occupancy()["live"] == [0] * 8
        fresh_check(t, True, "after a failed restore")
        t.close()


def test_calls_out_of_order():
    h, recs = source()
    batches, _ = stream(1)
    t = engine(True)
    t.restore_begin(h)
    with pytest.raises(hiprl.RedisError) as ei:
        t.submit(batches[0])
    assert ei.value.code == ESTATE, ei.value
    with pytest.raises(hiprl.RedisError) as ei:
        t.snapshot_begin()
    assert ei.value.code == ESTATE
    t.reset()  # closes the restore
    with pytest.raises(hiprl.RedisError) as ei:
        t.restore_put(recs[:1])
    assert ei.value.code == ESTATE
    fresh_check(t, True, "after a restore closed by reset")
    t.reset()
    # a snapshot needs nothing in flight
    t.submit_host_async(batches[0])
    with pytest.raises(hiprl.RedisError) as ei:
        t.snapshot_begin()
    assert ei.value.code == ESTATE
    t.wait_into(batches[0].n_desc, batches[0].n_req)
    h2 = t.snapshot_begin()
    with pytest.raises(hiprl.RedisError) as ei:
        t.snapshot_begin()  # one at a time
    assert ei.value.code == ESTATE
    t.snapshot_end()
    t.snapshot_end()  # legal at any point
    assert h2.n_records > 0


# ---- the C++ RateLimitCache mirror -------------------------------------------------------------
def test_cache_mirror_save_and_load(tmp_path):
    """HipRateLimitCache::Save / Load (rl_cache.hpp) through the batcher's queue: a cache that
    saves and a new one — with a smaller table — that loads answer as one oracle that never
    stopped; a missing or cut file is refused with the table kept."""
    import ctypes as C
    from pathlib import Path
    lib = C.CDLL(str(Path(__file__).resolve().parent / "cshim_snapshot" / "librl_snapshot_shim.so"))
    lib.rls_create.restype = C.c_void_p
    lib.rls_create.argtypes = [C.c_int, C.POINTER(C.c_uint32)]
    lib.rls_error.restype = C.c_char_p
    for f in (lib.rls_destroy, lib.rls_error):
        f.argtypes = [C.c_void_p]
    lib.rls_set_time.argtypes = [C.c_void_p, C.c_int64]
    lib.rls_add_rule.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.rls_do_limit.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.rls_save.argtypes = lib.rls_load.argtypes = [C.c_void_p, C.c_char_p]
    rules = [(3, hiprl.MINUTE), (5, hiprl.HOUR), (2, hiprl.DAY)]
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)

    def create(log2):
        p = lib.rls_create(1, (C.c_uint32 * 4)(*log2))
        assert p
        for L, u in rules:
            lib.rls_add_rule(p, L, u)
        return p

    def calls(p, t, n, ctx):
        lib.rls_set_time(p, t)
        for i in range(n):
            rule, hits, val = i % 3, 1 + i % 2, f"v{i % 11}"
            out = (C.c_uint32 * 3)()
            assert lib.rls_do_limit(p, val.encode(), rule, hits, out) == 0, lib.rls_error(p)
            st, thr = o.submit(hiprl.build_batch([("snap", [[("k", val)]], [rule], hits, t)]))
            want = [int(st[0]["code_flags"]) & 0xFF, int(st[0]["limit_remaining"]), int(thr[0])]
            assert list(out) == want, (ctx, i, list(out), want)

    t = 1_700_000_000
    a = create((12, 12, 12, 12))
    calls(a, t, 40, "before the save")
    path = str(tmp_path / "cache.rlsnap").encode()
    assert lib.rls_save(a, path) == 0, lib.rls_error(a)
    lib.rls_destroy(a)
    h, recs = hiprl.read_snapshot(path.decode())
    assert h.n_records == recs.shape[0] == 33 and h.flags & hiprl.SNAP_LOCAL_CACHE  # 11 values x 3 rules
    b = create((8, 9, 10, 8))
    assert lib.rls_load(b, path) == 0, lib.rls_error(b)
    calls(b, t + 5, 40, "after the load")
    # refused files change nothing
    assert lib.rls_load(b, str(tmp_path / "missing").encode()) == -1
    cut = tmp_path / "cut.rlsnap"
    cut.write_bytes((tmp_path / "cache.rlsnap").read_bytes()[:-32])
    assert lib.rls_load(b, str(cut).encode()) == -1 and b"n_records" in lib.rls_error(b)
    calls(b, t + 6, 40, "after the refused loads")
    lib.rls_destroy(b)
