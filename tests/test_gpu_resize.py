"""rl_resize (rl_hip.h "Resize") on the GPU: an engine that resizes its counter table between
two batches — larger, smaller, or the same size — continues a request stream bit-exactly as one
oracle that never stopped decides it, the live set moves exactly, and a refused resize changes
nothing."""
import functools

import numpy as np
import pytest
import torch

import hiprl
import oracle
import router
import streams
from streams import RULES, batch_sizes, make_stream

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC, ESTATE = -1, -3, -5
MAX_DESC = 1 << 14
SIZES_B = [(14, 15, 17, 15), (18, 14, 14, 14), (0, 0, 0, 0)]


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


def refused(code, f, *a):
    with pytest.raises(hiprl.RedisError) as ei:
        f(*a)
    assert ei.value.code == code, ei.value


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


def new_sizes(old, req):
    return [r or o for o, r in zip(old, req)]


# ---- 1. continuation parity ---------------------------------------------------------------------
def continue_across(seed, pipeline, log2_b):
    batches, cut = stream(seed)
    want = cat(expected(seed, True))
    e = engine(True, pipeline)
    first = run(e, batches[:cut])
    e.resize(log2_b)
    lg = new_sizes((16, 16, 16, 14), log2_b)
    assert e.occupancy()["slots"] == [1 << lg[r // 2] for r in range(8)]
    rest = run(e, batches[cut:])
    got = np.concatenate([first[0], rest[0]]), np.concatenate([first[1], rest[1]])
    streams.assert_same(want[0], want[1], got[0], got[1], f"seed={seed} pipeline={pipeline} B={log2_b}")
    e.close()


@pytest.mark.parametrize("log2_b", SIZES_B)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_continuation_parity(seed, log2_b):
    continue_across(seed, "v4", log2_b)


@pytest.mark.parametrize("log2_b", SIZES_B)
def test_continuation_parity_lsd(log2_b):
    continue_across(1, "lsd", log2_b)


# ---- 2. the live set is moved exactly -----------------------------------------------------------
def test_live_set_is_moved_exactly():
    batches, cut = stream(1)
    e = engine(True)
    run(e, batches[:cut])
    h1, r1 = e.snapshot_records()
    s1 = e.stats()
    assert h1.n_records > 1000
    e.resize((14, 15, 17, 15))
    h2, r2 = e.snapshot_records()
    assert list(h2.gen) == list(h1.gen) and list(h2.live) == list(h1.live) and list(h2.prev) == list(h1.prev)
    assert h2.n_records == h1.n_records
    assert list(h1.src_log2) == [16] * 6 + [14] * 2 and list(h2.src_log2) == [14, 14, 15, 15, 17, 17, 15, 15]
    assert np.array_equal(sorted_set(r1), sorted_set(r2))
    occ = e.occupancy()
    slots = [1 << g for g in h2.src_log2]
    assert occ["slots"] == slots and occ["limit"] == [s * 750 // 1000 for s in slots]
    assert occ["live"] == list(h1.live) and occ["gen"] == list(h1.gen)
    s2 = e.stats()
    assert s2["live_keys"] == s1["live_keys"] == h1.n_records and s2["inserted_keys"] == s1["inserted_keys"]


# ---- 3. lag window ----------------------------------------------------------------------------
@pytest.mark.parametrize("log2_b", [(10, 0, 0, 0), (7, 0, 0, 0)])
def test_lag_window_both_generations_survive(log2_b):
    """Lag-window engines keep a SECOND region's previous generation (gen - 2) live: the resize
    moves it beside the newest one, and a late batch still finds its keys. 90 live slots fit the
    96-slot load limit of a 128-slot region and not the 48 of a 64-slot one. The capacity check
    counts every descriptor of a batch as a possible new slot, so the batches after the resize
    carry 6 descriptors: 90 + 6 is what a 96-slot limit admits."""
    t = 1_700_000_001
    rules = [(5, hiprl.SECOND)]
    late = hiprl.build_batch([("lag", [[("a", str(i))]], [0], 1, t - 2) for i in range(30)])
    newest = hiprl.build_batch([("lag", [[("b", str(i))]], [0], 2, t) for i in range(60)])
    late6 = hiprl.build_batch([("lag", [[("a", str(i))]], [0], 1, t - 2) for i in range(5, 30, 5)] +
                              [("lag", [[("a", "7")]], [0], 3, t - 2)])
    newest6 = hiprl.build_batch([("lag", [[("b", str(i))]], [0], 2, t) for i in range(3, 60, 10)])
    seq = [late, newest, late, newest6, late6, late6, newest6]
    assert late6.n_desc == newest6.n_desc == 6
    o = oracle.Oracle()
    o.load_rules(rules)
    exp = [o.submit(b) for b in seq]
    e = engine(rules=rules, log2_slots=(8, 8, 8, 8), max_batch_desc=4096, lag_window=True)
    first = [e.submit(b) for b in seq[:3]]
    r = t % 2
    h, recs = e.snapshot_records()
    assert list(h.gen)[r] == t + 1 and list(h.live)[r] == 60 and list(h.prev)[r] == 30 and h.n_records == 90
    inserted = e.stats()["inserted_keys"]
    e.resize(log2_b)
    h2, recs2 = e.snapshot_records()
    assert list(h2.gen) == list(h.gen) and list(h2.live) == list(h.live) and list(h2.prev) == list(h.prev)
    assert np.array_equal(sorted_set(recs), sorted_set(recs2))
    assert e.occupancy()["slots"][r] == 1 << log2_b[0]
    rest = [e.submit(x) for x in seq[3:]]
    streams.assert_same(*cat(exp), *cat(first + rest), f"lag window into {log2_b}")
    assert e.stats()["inserted_keys"] == inserted and e.occupancy()["live"][r] == 60
    occ = e.occupancy()
    refused(ENOSPC, e.resize, (6, 0, 0, 0))
    assert e.occupancy() == occ
    h3, recs3 = e.snapshot_records()
    assert list(h3.prev)[r] == 30 and list(h3.live)[r] == 60 and recs3.shape[0] == 90


# ---- 4. tight region, probe wrap --------------------------------------------------------------
def test_tight_region_with_probe_wrap():
    """180 keys of one HOUR window into a 256-slot region (load limit 192): long probe chains,
    some past the region's end; then out of it again into 4096 slots."""
    t = 1_700_000_000
    assert oracle.place(t // 3600 * 3600)[0] == 4  # an HOUR-home region
    rules = [(3, hiprl.HOUR)]
    batches = [hiprl.build_batch([("tight", [[("k", str(i))]], [0], 2, t) for i in range(j, j + 10)])
               for j in range(0, 180, 10)]
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)
    e = engine(True, rules=rules, max_batch_desc=64)
    streams.assert_same(*run(o, batches), *run(e, batches), "tight: first pass")
    inserted = e.stats()["inserted_keys"]
    assert inserted == 180
    e.resize((8, 8, 8, 8))
    occ = e.occupancy()
    assert occ["live"][4] == 180 and occ["limit"][4] == 192 and occ["slots"][4] == 256, occ
    streams.assert_same(*run(o, batches), *run(e, batches), "tight: second pass")
    assert e.occupancy()["live"][4] == 180
    assert e.stats()["inserted_keys"] == inserted  # every key found its slot
    e.resize((0, 0, 12, 0))
    occ = e.occupancy()
    assert occ["live"][4] == 180 and occ["limit"][4] == 3072 and occ["slots"] == [256] * 4 + [4096] * 2 + [256] * 2, occ
    streams.assert_same(*run(o, batches), *run(e, batches), "tight: third pass")
    assert e.occupancy()["live"][4] == 180 and e.stats()["inserted_keys"] == inserted


# ---- 5. the refusal it cures ------------------------------------------------------------------
def test_resize_cures_the_capacity_refusal():
    t = 1_700_000_000
    rules = [(3, hiprl.HOUR)]
    def batch(lo, hi):
        return hiprl.build_batch([("full", [[("k", str(i))]], [0], 2, t) for i in range(lo, hi)])
    accepted = [batch(j, j + 10) for j in range(0, 180, 10)]
    more = batch(180, 200)
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)
    e = engine(True, rules=rules, max_batch_desc=64, log2_slots=(16, 16, 8, 14))
    streams.assert_same(*run(o, accepted), *run(e, accepted), "full: 180 keys")
    occ = e.occupancy()
    assert occ["live"][4] == 180 and occ["limit"][4] == 192
    refused(ENOSPC, e.submit, more)  # 180 + 20 > 192
    assert e.occupancy() == occ
    e.resize((0, 0, 9, 0))
    assert e.occupancy()["limit"][4] == 384
    # the oracle has no capacity bound: it saw the accepted batches only
    streams.assert_same(*o.submit(more), *e.submit(more), "full: the refused batch, after the resize")
    assert e.occupancy()["live"][4] == 200
    streams.assert_same(*run(o, accepted + [more]), *run(e, accepted + [more]), "full: every key again")
    assert e.stats()["inserted_keys"] == 200


# ---- 6. refusals change nothing ---------------------------------------------------------------
def test_refusals_change_nothing():
    batches, cut = stream(3)
    exp = expected(3, True)
    e = engine(True)
    outs = [e.submit(b) for b in batches[:cut]]
    k = cut

    def state():
        h, recs = e.snapshot_records()
        return e.occupancy(), bytes(h), sorted_set(recs)

    def unchanged(before, ctx):
        """Occupancy and record set as before; then the stream's next batch, decided exactly."""
        nonlocal k
        after = state()
        assert after[0] == before[0] and after[1] == before[1] and np.array_equal(after[2], before[2]), ctx
        outs.append(e.submit(batches[k]))
        streams.assert_same(*exp[k], *outs[-1], ctx)
        k += 1

    assert len(batches) - cut >= 5 and max(e.occupancy()["live"]) > 12
    for bad in ((3, 0, 0, 0), (0, 0, 0, 32), (16, 16, 16, 3)):
        before = state()
        refused(EINVAL, e.resize, bad)
        unchanged(before, f"after EINVAL {bad}")
    before = state()
    refused(ENOSPC, e.resize, (4, 4, 4, 4))  # 16 slots, load limit 12: below the live count
    unchanged(before, "after ENOSPC")
    # a host batch in flight
    before = state()
    e.submit_host_async(batches[k])
    refused(ESTATE, e.resize, (17, 17, 17, 17))
    assert e.occupancy() == before[0]
    outs.append(e.wait_into(batches[k].n_desc, batches[k].n_req))
    streams.assert_same(*exp[k], *outs[-1], "the batch in flight at the refusal")
    k += 1
    # an open snapshot does not block a resize, and still drains the records of its begin
    before = state()
    h = e.snapshot_begin()
    e.resize((15, 15, 15, 15))
    parts = []
    while True:
        part = e.snapshot_next(1000)
        if not part.shape[0]:
            break
        parts.append(part)
    e.snapshot_end()
    assert bytes(h) == before[1] and np.array_equal(sorted_set(np.concatenate(parts)), before[2])
    assert np.array_equal(state()[2], before[2])
    outs += [e.submit(b) for b in batches[k:]]
    streams.assert_same(*cat(exp), *cat(outs), "the whole stream")
    # between rl_restore_begin and rl_restore_end (the begin clears the table, so on another engine)
    t = engine(True, log2_slots=(15, 15, 15, 15))
    hs, recs = before[1], before[2]
    hdr = hiprl.RlSnapshotHeader.from_buffer_copy(hs)
    t.restore_begin(hdr)
    occ = t.occupancy()
    refused(ESTATE, t.resize, (16, 16, 16, 16))
    assert t.occupancy() == occ
    t.restore_put(recs)
    t.restore_end()
    assert t.occupancy()["slots"] == [1 << 15] * 8
    streams.assert_same(*cat(exp[k:]), *run(t, batches[k:]), "the restore the refusal interrupted")


# ---- 7. hot set kept --------------------------------------------------------------------------
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
def test_hot_set_is_kept(local_cache):
    """The hot set holds prefixes, not slots (HotBucket.slot is rewritten by k4_scan every batch,
    and nothing else keeps a table address across batches): the batches after a resize use it as
    before, with no fall-back to learn it again."""
    batches = hot_batches(6, 4000, 1_700_000_000 - 2)  # every hot prefix: >= 128 descriptors a batch
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(RULES)
    exp = [o.submit(b) for b in batches]
    e = engine(local_cache)
    first = [e.submit(b) for b in batches[:3]]
    s = e.stats()
    assert s["hot_keys"] > 0, s
    e.resize((15, 17, 15, 16))
    rest = [e.submit(b) for b in batches[3:]]
    streams.assert_same(*cat(exp), *cat(first + rest), f"hot set local={local_cache}")
    s2 = e.stats()
    assert s2["hot_keys"] > 0 and s2["lsd_fallbacks"] == s["lsd_fallbacks"], (s, s2)


# ---- 8. two in flight ---------------------------------------------------------------------------
def test_two_in_flight_around_a_resize():
    dev = torch.device("cuda", 0)
    batches, cut = stream(2)
    want = cat(expected(2, True))
    e = engine(True)

    def pipelined(host_batches, depth=2):
        dbs = [router.DeviceBatch.from_host(hb, dev) for hb in host_batches]
        outs = [torch.zeros(max(1, db.n_desc) * 20, dtype=torch.uint8, device=dev) for db in dbs]
        thrs = [torch.zeros(max(1, db.n_req), dtype=torch.int32, device=dev) for db in dbs]
        torch.cuda.synchronize()
        pending = 0
        for k, db in enumerate(dbs):
            e.submit_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), outs[k].data_ptr(), thrs[k].data_ptr())
            pending += 1
            if pending == depth:
                e.wait()
                pending -= 1
        for _ in range(pending):
            e.wait()
        torch.cuda.synchronize()
        st = np.concatenate([outs[k][:db.n_desc * 20].cpu().numpy().view(hiprl.STATUS_DTYPE)
                             for k, db in enumerate(dbs)])
        thr = np.concatenate([thrs[k][:db.n_req].cpu().numpy().view(np.uint32) for k, db in enumerate(dbs)])
        return st, thr

    first = pipelined(batches[:cut])
    e.resize((17, 15, 17, 15))
    rest = pipelined(batches[cut:])
    got = np.concatenate([first[0], rest[0]]), np.concatenate([first[1], rest[1]])
    streams.assert_same(want[0], want[1], got[0], got[1], "two in flight, resized between")
