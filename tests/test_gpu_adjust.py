"""rl_adjust (rl_hip.h "Adjust") on the GPU: signed corrections by key. The oracle has no such
command, so every expected state is reached two ways: by requests (an engine that charged h and got
r back decides the rest of a stream exactly as an oracle that was charged h - r), and by the dict
model of adjust_model.py (peek before + deltas + rules -> peek after and the report). Every
comparison is of exact integers."""
import ctypes as C

import numpy as np
import pytest

import hiprl
import oracle
import streams
from adjust_model import adjust_model, string_of
from streams import RULES, batch_sizes, make_stream

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC, ECAPACITY, ESTATE = -1, -3, -4, -5
NIL = hiprl.NIL_RULE
MAX_NOW = 0xFFFD0000
F, LC, PS, NILF = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_PER_SECOND, hiprl.PEEK_NIL
S, M, H, D = hiprl.SECOND, hiprl.MINUTE, hiprl.HOUR, hiprl.DAY
SMALL = (8, 8, 7, 6)  # slots per home unit: probe chains wrap
BIG = (11, 12, 12, 12)  # the parity streams hold a few thousand strings per home unit
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
M0 = (1_700_000_000 // 60 + 1) * 60  # a minute's first second (not an hour's)
assert M0 % 60 == 0 and M0 % 3600


def engine(local_cache=False, log2_slots=SMALL, rules=RULES, **kw):
    kw.setdefault("max_batch_desc", 1 << 13)
    e = hiprl.Engine(local_cache=local_cache, log2_slots=log2_slots, **kw)
    e.load_rules(rules)
    return e


def make_oracle(local_cache=False, rules=RULES, **kw):
    o = oracle.Oracle(local_cache=local_cache, **kw)
    o.load_rules(rules)
    return o


def run(backend, batches):
    out = [backend.submit(b) for b in batches]
    return np.concatenate([s for s, _ in out]), np.concatenate([t for _, t in out])


def key_batch(items, now):
    """[(prefix bytes, rule id)] -> one request at `now`, or one request per descriptor when `now`
    is a sequence."""
    lens = [len(p) for p, _ in items]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    blob = np.frombuffer(b"".join(p for p, _ in items), np.uint8).copy()
    rule = np.array([r for _, r in items], np.uint32)
    if np.ndim(now) == 0:
        return hiprl.Batch(blob, off, rule, np.zeros(len(items), np.uint32), np.array([now], np.int64),
                           np.ones(1, np.uint32))
    return hiprl.Batch(blob, off, rule, np.arange(len(items), dtype=np.uint32), np.array(now, np.int64),
                       np.ones(len(items), np.uint32))


def vals(rows):
    """[(count, ttl_s, cached_s, flags)] -> PEEK_DTYPE."""
    return np.array([tuple(r) for r in rows], hiprl.PEEK_DTYPE).reshape(len(rows))


def pfx(name, dom="adj"):
    return hiprl.cache_key_prefix(dom, [("k", str(name))])


def state(e, now):
    """Everything a refused or empty call must leave alone."""
    c = e.census(now)
    return e.occupancy(), e.stats()["inserted_keys"], e.stats()["live_keys"], {k: v.tolist() for k, v in c.items()}


def rec_set(e):
    return {r.tobytes() for r in e.snapshot_records()[1]}


def strings_of(b, rules):
    return [None if int(b.rule[i]) == NIL else
            string_of(b.prefix(i), rules[int(b.rule[i])][1], int(b.now[b.req_of[i]])) for i in range(b.n_desc)]


def adjust_checked(e, b, deltas, rules, local_cache, keep_cache=False):
    """One rl_adjust held against the model: out is the peek before, the peek after and the report
    are the model's. -> (before, after, report)"""
    before = e.peek(b)
    limits = [0 if int(r) == NIL else rules[int(r)][0] for r in b.rule]
    want, want_rep = adjust_model(strings_of(b, rules), before, deltas, limits, local_cache, keep_cache)
    out, rep = e.adjust(b, np.array(deltas, np.int64), keep_cache=keep_cache)
    assert np.array_equal(out, before), "out is the state before the call"
    after = e.peek(b)
    bad = np.nonzero(after != want)[0]
    assert not bad.size, (int(bad[0]), before[bad[0]], deltas[int(bad[0])], after[bad[0]], want[bad[0]])
    assert rep == want_rep, (rep, want_rep)
    assert rep["descriptors"] == rep["nil"] + rep["absent"] + rep["applied"] == b.n_desc
    return before, after, rep


def check_against_oracle(rep, b, o, rules, split, ctx=""):
    """Every reply of a peek of b against the oracle's GET / freecache Get."""
    for i in range(b.n_desc):
        r, fl = rep[i], int(rep[i]["flags"])
        now = int(b.now[b.req_of[i]])
        unit = rules[int(b.rule[i])][1]
        k = oracle.cache_key(b.prefix(i), unit, now)
        ps = split and unit == S
        c, lc = o.counter(k, now, per_second=ps), o.local_cached(k, now)
        assert bool(fl & F) == (c >= 0) and int(r["count"]) == max(c, 0), (ctx, i, k, r, c)
        assert bool(fl & LC) == lc and (int(r["cached_s"]) > 0) == lc, (ctx, i, k, r, lc)
        assert bool(fl & PS) == ps and (int(r["ttl_s"]) > 0) == (c >= 0 and not ps), (ctx, i, r)


# ---- 1 / 2. a refund equals never having spent it, a true-up equals having spent it ---------------
L1 = 10
RULES1 = [(L1, S), (L1, M), (L1, H), (L1, D)]
# (charged h, correction r < h): under the limit; frozen by the charge and back to the limit / under
# it; over it on both sides; no correction; one unit
CASES = [(6, 2), (12, 2), (13, 5), (20, 3), (4, 0), (9, 8), (11, 1)]
T1 = M0 - 2


def later_batches(names):
    """The same keys again, across a SECOND edge (every batch) and a MINUTE edge (the third)."""
    out = []
    for j, t in enumerate([T1, T1 + 1, T1 + 2, T1 + 3, T1 + 3]):
        assert (t == M0) == (j == 2)
        out.append(hiprl.build_batch([("adj", [[("k", nm)]], [rl], 1 + (i + j) % 3, t)
                                      for i, (nm, rl) in enumerate(names) for _ in range(1 + (i + j) % 2)]))
    return out


@pytest.mark.parametrize("sign,local_cache,split,keep", [
    (-1, False, False, False), (-1, True, False, False), (-1, False, True, False), (-1, True, True, False),
    (-1, True, False, True), (-1, True, True, True), (+1, False, False, False), (+1, False, True, False)])
def test_correction_equals_requests(sign, local_cache, split, keep):
    names = [(f"u{u}c{c}", u) for u in range(4) for c in range(len(CASES))]
    hr = [CASES[c] for _ in range(4) for c in range(len(CASES))]
    if sign > 0:
        assert any(h <= L1 < h + r for h, r in hr), "guard: a key pushed over its limit"
    else:
        assert any(h > L1 >= h - r for h, r in hr) and any(h - r > L1 for h, r in hr) and any(h <= L1 for h, r in hr)
    e = engine(local_cache, rules=RULES1, per_second_split=split)
    o = make_oracle(local_cache, rules=RULES1, per_second_split=split)
    e.submit(hiprl.build_batch([("adj", [[("k", nm)]], [rl], h, T1) for (nm, rl), (h, _) in zip(names, hr)]))
    o.submit(hiprl.build_batch([("adj", [[("k", nm)]], [rl], h + sign * r, T1) for (nm, rl), (h, r) in zip(names, hr)]))
    pb = key_batch([(pfx(nm), rl) for nm, rl in names], T1)
    before, after, rep = adjust_checked(e, pb, [sign * r for _, r in hr], RULES1, local_cache, keep)
    assert before["count"].tolist() == [h for h, _ in hr] and rep["applied"] == len(names)
    frozen = np.array([local_cache and h > L1 for h, _ in hr])
    released = np.array([local_cache and sign < 0 and r > 0 and h > L1 >= h - r for h, r in hr])
    assert np.array_equal((before["flags"] & LC) != 0, frozen)
    if keep:
        # the counters moved, every deadline stayed: the released keys are still LOCAL_CACHED
        assert released.any() and np.array_equal((after["flags"] & LC) != 0, frozen) and rep["unfrozen"] == 0
        assert after["count"].tolist() == [h - r for h, r in hr]
        e.close()
        return
    assert rep["unfrozen"] == int(released.sum()) and (not local_cache or sign > 0 or released.sum() >= 8)
    check_against_oracle(after, pb, o, RULES1, split, f"{sign} {local_cache} {split}")
    nb = later_batches(names)
    streams.assert_same(*run(o, nb), *run(e, nb), f"after the correction: {sign} {local_cache} {split}")
    e.close()


# ---- 3. duplicates and order ---------------------------------------------------------------------
def test_duplicates_are_one_incrby_of_the_net():
    t = 1_700_000_007
    rules = [(1 << 30, M)]
    a, b = engine(rules=rules), engine(rules=rules)
    fill = hiprl.build_batch([("adj", [[("k", f"p{j}")]], [0], 5, t) for j in range(3)])
    a.submit(fill)
    b.submit(fill)
    dup = key_batch([(pfx("p0"), 0), (pfx("p0"), 0), (pfx("p1"), 0), (pfx("p1"), 0), (pfx("p2"), 0), (pfx("p2"), 0)], t)
    before, after, rep = adjust_checked(a, dup, [-10, 3, 3, -10, -4, 4], rules, False)
    assert before["count"].tolist() == [5] * 6, "every duplicate reads the state before the call"
    assert after["count"].tolist() == [0, 0, 0, 0, 5, 5]  # 5 - 10 + 3 stops at 0 once: not 3
    assert (rep["applied"], rep["floored"]) == (6, 2) and (after["flags"] == F).all()
    one = key_batch([(pfx(f"p{j}"), 0) for j in range(3)], t)
    _, after_b, rep_b = adjust_checked(b, one, [-7, -7, 0], rules, False)
    assert after_b["count"].tolist() == [0, 0, 5] and rep_b["floored"] == 2
    assert rec_set(a) == rec_set(b), "k descriptors of a string are one call with the net"
    a.close()
    b.close()


@pytest.mark.parametrize("n", [1, 65, 257, 1025, 3001])
def test_sizes_with_duplicates_in_one_wave_in_other_waves_and_in_other_blocks(n):
    """n descriptors over 2n/3 + 1 strings: key j recurs at j + distinct, so its duplicate sits in
    the same wave, another wave or another block depending on n. A fifth of the strings are absent,
    some are frozen. Every run equals the model, and two equal engines end with equal records."""
    t = 1_700_000_007
    L = 9
    rules = [(L, H)]
    distinct = 2 * n // 3 + 1
    present = [j for j in range(distinct) if j % 5 != 4 or n == 1]
    fill = hiprl.build_batch([("adj", [[("k", f"z{j}")]], [0], 1 + j % 12, t) for j in present])
    pb = key_batch([(pfx(f"z{j % distinct}"), 0) for j in range(n)], t)
    deltas = np.random.default_rng(n).integers(-8, 7, n)
    recs = []
    for _ in range(2):
        e = engine(True, rules=rules, log2_slots=(4, 4, 12, 4), max_batch_desc=3001)  # 2001 strings of one hour
        e.submit(fill)
        s0 = state(e, t)
        before, after, rep = adjust_checked(e, pb, deltas, rules, True)
        assert rep["absent"] == sum((j % distinct) not in present for j in range(n))
        assert n < 65 or (rep["unfrozen"] > 0 and rep["floored"] > 0 and (before["flags"] & LC).sum() > rep["unfrozen"])
        assert state(e, t)[:3] == s0[:3]
        recs.append(rec_set(e))
        e.close()
    assert recs[0] == recs[1] and len(recs[0]) == len(present)


# ---- 4. two stores of one string -------------------------------------------------------------------
@pytest.mark.parametrize("local_cache", [False, True])
def test_two_stores_of_one_string(local_cache):
    t = M0
    L = 4
    rules = [(L, S), (L, M)]
    e = engine(local_cache, rules=rules, per_second_split=True)
    e.submit(hiprl.build_batch([("adj", [[("k", "two")], [("k", "two")]], [0, 1], 5, t)]))
    both = key_batch([(pfx("two"), 0), (pfx("two"), 1)], t)
    sec, minute = key_batch([(pfx("two"), 0)], t), key_batch([(pfx("two"), 1)], t)
    assert string_of(pfx("two"), S, t) == string_of(pfx("two"), M, t)
    p = e.peek(both)
    lc = LC if local_cache else 0
    assert [(int(x["count"]), int(x["flags"])) for x in p] == [(5, F | PS | lc), (5, F | lc)], "guard"
    n_slots = len(rec_set(e))

    def counts():
        r = e.peek(both)
        return [(int(x["count"]), bool(int(x["flags"]) & F)) for x in r]

    # each store alone: the other store's word is untouched (positive nets: the deadline stays)
    adjust_checked(e, sec, [2], rules, local_cache)
    assert counts() == [(7, True), (5, True)]
    adjust_checked(e, minute, [4], rules, local_cache)
    assert counts() == [(7, True), (9, True)]
    assert not local_cache or (e.peek(both)["flags"] & LC).all()
    # together, two pairs in one slot; both come back to the limit: one string, one deadline, counted once
    _, after, rep = adjust_checked(e, both, [-3, -5], rules, local_cache)
    assert counts() == [(4, True), (4, True)] and rep["unfrozen"] == int(local_cache)
    assert not (after["flags"] & LC).any()
    # the per-second counter to 0 reads back not found; the main counter at 0 stays found
    _, after, rep = adjust_checked(e, both, [-4, -4], rules, local_cache)
    assert counts() == [(0, False), (0, True)] and rep["floored"] == 0
    assert int(after[1]["ttl_s"]) == int(p[1]["ttl_s"]) > 0
    # ... and is absent for the next correction
    _, _, rep = adjust_checked(e, both, [3, 3], rules, local_cache)
    assert counts() == [(0, False), (3, True)] and (rep["absent"], rep["applied"]) == (1, 1)
    assert len(rec_set(e)) == n_slots == 1
    e.close()


# ---- 5. edges ----------------------------------------------------------------------------------------
def test_edges():
    t = 1_700_000_007
    L = 50
    rules = [(L, M), (L, D)]
    e = engine(rules=rules)
    # INT32_MIN on a small counter; INT32_MAX on a counter rl_set left 16 below the top; a nil descriptor
    e.submit(hiprl.build_batch([("adj", [[("k", "small")], [("k", "zero")]], [0, 0], 7, t)]))
    e.set(key_batch([(pfx("top"), 0)], t), vals([(0xFFFFFFF0, 40, 0, F)]))
    e.set(key_batch([(pfx("short"), 0)], t), vals([(5, 10, 0, F)]))  # expires at t + 10
    e.submit(hiprl.build_batch([("adj", [[("k", "prev")]], [0], 5, t - 60)]))  # the window before
    assert (t + 10) // 60 == t // 60
    pb = key_batch([(pfx("small"), 0), (pfx("top"), 0), (pfx("nil"), NIL), (pfx("zero"), 0)], t)
    before, after, rep = adjust_checked(e, pb, [INT32_MIN, INT32_MAX, 5, -7], rules, False)
    assert after["count"].tolist() == [0, 0xFFFFFFFF, 0, 0] and int(after[2]["flags"]) == NILF
    assert rep == dict(descriptors=4, nil=1, absent=0, applied=3, floored=1, capped=1, unfrozen=0)
    # a floored counter and one brought to exactly 0 keep their TTL and read back found
    assert after["ttl_s"].tolist() == before["ttl_s"].tolist() and (after["flags"][[0, 3]] == F).all()
    # a main key at t == its expiry, and a key of the previous window: absent, the slot words stay
    recs = rec_set(e)
    s0 = state(e, t + 10)
    late = key_batch([(pfx("short"), 0), (pfx("prev"), 0)], t + 10)
    assert int(e.peek(key_batch([(pfx("short"), 0)], t + 9))[0]["ttl_s"]) == 1
    before, _, rep = adjust_checked(e, late, [3, 3], rules, False)
    assert not before["flags"].any() and (rep["absent"], rep["applied"]) == (2, 0)
    assert rec_set(e) == recs and state(e, t + 10) == s0
    assert int(e.peek(key_batch([(pfx("prev"), 0)], t - 60))[0]["count"]) == 5
    # the next submit counts from 0
    st, _ = e.submit(hiprl.build_batch([("adj", [[("k", "small")]], [0], 2, t)]))
    assert (int(st[0]["code_flags"]) & 0xFF, int(st[0]["limit_remaining"])) == (hiprl.CODE_OK, L - 2)
    assert int(e.peek(key_batch([(pfx("small"), 0)], t))[0]["count"]) == 2
    # the last admissible second, a DAY rule
    e.submit(hiprl.build_batch([("adj", [[("k", "last")]], [1], 5, MAX_NOW)]))
    _, after, _ = adjust_checked(e, key_batch([(pfx("last"), 1)], MAX_NOW), [-2], rules, False)
    assert (int(after[0]["count"]), int(after[0]["flags"])) == (3, F)
    e.close()


# ---- 6. nothing but counters moves -----------------------------------------------------------------
def test_nothing_but_counters_moves():
    t = 1_700_000_007
    L = 6
    rules = [(L, M), (L, H)]
    e = engine(True, rules=rules)
    names = [f"m{j}" for j in range(40)]
    e.submit(hiprl.build_batch([("adj", [[("k", nm)]], [j % 2], 1 + j % 9, t) for j, nm in enumerate(names)]))
    hit = [(pfx(nm), j % 2) for j, nm in enumerate(names)]
    miss = [(pfx(f"gone{j}"), j % 2) for j in range(40)]
    stay = ("slots", "live", "prev", "stale", "keys_main", "keys_per_second", "cache_expired")
    ins0, unfrozen = e.stats(), []
    for items in (hit, miss, [x for pair in zip(hit, miss) for x in pair]):
        pb = key_batch(items, t)
        # all deltas 0: a peek, the records byte for byte
        recs, s0 = rec_set(e), state(e, t)
        _, _, rep = adjust_checked(e, pb, [0] * pb.n_desc, rules, True)
        assert rec_set(e) == recs and state(e, t) == s0 and rep["floored"] == rep["capped"] == rep["unfrozen"] == 0
        # counters move (and with them the census' histogram of counters), deadlines are cleared: nothing else
        deltas = [(-2, 1, -1)[j % 3] for j in range(pb.n_desc)]
        _, _, rep = adjust_checked(e, pb, deltas, rules, True)
        s1 = state(e, t)
        assert s1[:3] == s0[:3]
        for f in stay:
            assert s1[3][f] == s0[3][f], f
        assert sum(s0[3]["cached"]) - sum(s1[3]["cached"]) == rep["unfrozen"]
        unfrozen.append(rep["unfrozen"])
        assert len(rec_set(e)) == len(recs) == len(names)
    assert unfrozen[0] == 4 and unfrozen[1] == 0, unfrozen  # the keys charged 7 that got 2 back
    assert e.stats() == ins0, "rl_engine_stats does not move"
    e.close()


# ---- 7. a live engine with a learned hot set --------------------------------------------------------
def test_live_engine_with_hot_set():
    t0 = 1_700_000_007
    LH = 1000
    rules = RULES + [(LH, H)]
    hot_rule = len(RULES)
    reqs = make_stream(21, 1600, t0=t0, dt_max=1)
    sizes = batch_sizes(reqs, np.random.default_rng(3), 260)
    batches, i = [], 0
    for k, bs in enumerate(sizes):
        hot = [("adj", [[("k", "hot")]], [hot_rule], 1 + (k + j) % 2, reqs[i][4]) for j in range(150)]
        batches.append(hiprl.build_batch(hot + reqs[i:i + bs]))
        i += bs
    assert len(batches) >= 8 and all((b.rule == hot_rule).sum() >= 128 for b in batches)
    o, e = make_oracle(True, rules=rules), engine(True, rules=rules, log2_slots=BIG)
    seen = {}
    for k, b in enumerate(batches):
        streams.assert_same(*o.submit(b), *e.submit(b), f"batch {k}")
        for d in range(b.n_desc):
            if int(b.rule[d]) != NIL:
                seen.setdefault((b.prefix(d), rules[int(b.rule[d])][1]), int(b.rule[d]))
        # an all-zero adjust of every key seen so far, at the next batch's time, between every two batches
        t = int(batches[min(k + 1, len(batches) - 1)].now[0])
        pb = key_batch([(p, r) for (p, _), r in seen.items()], t)
        p0 = e.peek(pb)
        out, rep = e.adjust(pb, np.zeros(pb.n_desc, np.int32))
        assert np.array_equal(out, p0) and np.array_equal(e.peek(pb), p0)
        assert rep["applied"] == int(((p0["flags"] & F) != 0).sum()) > 0 and rep["unfrozen"] == 0
    assert e.stats()["hot_keys"] >= 1, "guard: the dominant key is in the hot set"
    # the refund of test 1 on the hot key: charged c (over the limit, frozen), r back
    t = int(batches[-1].now[-1])
    hot_key = key_batch([(pfx("hot"), hot_rule)], t)
    c = int(e.peek(hot_key)[0]["count"])
    assert c > LH and int(e.peek(hot_key)[0]["flags"]) == F | LC
    r = c - (LH - 10)
    _, after, rep = adjust_checked(e, hot_key, [-r], rules, True)
    assert (int(after[0]["count"]), int(after[0]["flags"]), rep["unfrozen"]) == (LH - 10, F, 1)
    o2 = make_oracle(True, rules=rules)
    o2.submit(hiprl.build_batch([("adj", [[("k", "hot")]], [hot_rule], c - r, t)]))
    hot_only = [hiprl.build_batch([("adj", [[("k", "hot")]], [hot_rule], 1 + j % 2, t + j // 300) for j in range(600)])]
    st_e, thr_e = run(e, hot_only)
    streams.assert_same(*run(o2, hot_only), st_e, thr_e, "hot key after a refund")
    codes = st_e["code_flags"] & 0xFF
    assert (codes == hiprl.CODE_OVER_LIMIT).sum() > 100 and (codes == hiprl.CODE_OK).sum() > 5
    e.close()


# ---- 8. refusals change nothing ----------------------------------------------------------------------
def test_refusals_change_nothing():
    t = 1_700_000_007
    rules = [(5, M), (5, S), (5, H)]
    e = engine(True, rules=rules, max_batch_desc=64, max_batch_req=64)
    e.submit(hiprl.build_batch([("adj", [[("k", "old")], [("k", "sec")], [("k", "hr")]], [0, 1, 2], 9, t)]))
    watch = key_batch([(pfx("old"), 0), (pfx("sec"), 1), (pfx("hr"), 2), (pfx("none"), 0)], t)
    p0, s0, r0 = e.peek(watch), state(e, t), rec_set(e)
    assert (p0["flags"][:3] & (F | LC) == F | LC).all()
    one = key_batch([(pfx("old"), 0)], t)

    def refused(code, b, delta, flags=0, check=True):
        """The raw call with sentinels in out and *report."""
        out = np.full(max(1, b.n_desc), 0xAB, np.uint8).repeat(16).view(hiprl.PEEK_DTYPE)
        rep = hiprl.RlAdjustReport()
        C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
        d = None if delta is None else np.ascontiguousarray(delta, np.int32)
        s = hiprl._batch_struct(b)
        rc = e.lib.rl_adjust(e.h, C.byref(s), None if d is None else d.ctypes.data, flags, out.ctypes.data, C.byref(rep))
        assert rc == code, (rc, code)
        assert bytes(out.tobytes()) == b"\xAB" * out.nbytes and bytes(rep) == b"\x5A" * 64
        if check:
            assert np.array_equal(e.peek(watch), p0) and state(e, t) == s0 and rec_set(e) == r0, code

    refused(EINVAL, one, None)                                                   # delta == NULL
    refused(EINVAL, one, [-3], flags=2)                                          # an unknown flag bit
    refused(EINVAL, one, [-3], flags=hiprl.ADJUST_KEEP_CACHE | 0x80000000)
    refused(ECAPACITY, key_batch([(pfx(f"x{i}"), 0) for i in range(65)], t), [-1] * 65)
    refused(EINVAL, key_batch([(pfx("old"), 7)], t), [-3])                       # rl_peek's list: an unknown rule
    refused(EINVAL, key_batch([(pfx("old"), 0)], MAX_NOW + 1), [-3])             # ... the time
    # a routed-set plan open (an empty one)
    e.set_routed_plan(0, 0, 0)
    refused(ESTATE, one, [-3], check=False)
    e.set_routed_commit(False)
    assert np.array_equal(e.peek(watch), p0) and state(e, t) == s0 and rec_set(e) == r0
    # a restore open; an open snapshot does not block the call
    h = e.snapshot_begin()
    out, rep = e.adjust(key_batch([(pfx("none"), 0)], t), [4])  # absent: nothing moves
    assert rep["absent"] == 1 and not out["flags"].any()
    recs = e.snapshot_next(4096)
    e.snapshot_end()
    e.restore_begin(h)
    refused(ESTATE, one, [-3], check=False)
    e.restore_put(recs)
    e.restore_end()
    assert np.array_equal(e.peek(watch), p0) and rec_set(e) == r0
    # a batch in flight: it counts "hr" once more, the refused call moved nothing
    s0 = state(e, t)
    b = hiprl.build_batch([("adj", [[("k", "hr")]], [2], 1, t)])
    e.submit_host_async(b)
    refused(ESTATE, one, [-3], check=False)
    st, _ = e.wait_into(b.n_desc, b.n_req)
    assert int(st[0]["code_flags"]) >> 8 & hiprl.FLAG_LOCAL_CACHE_HIT  # frozen: not even that
    assert np.array_equal(e.peek(watch), p0) and state(e, t) == s0 and rec_set(e) == r0
    # the same call, accepted
    _, after, rep = adjust_checked(e, one, [-4], rules, True)
    assert (int(after[0]["count"]), int(after[0]["flags"]), rep["unfrozen"]) == (5, F, 1)
    # n_desc == 0 returns 0 and zeroes the report
    rep = hiprl.RlAdjustReport()
    C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
    empty = key_batch([], t)  # kept alive: the struct points into its arrays
    s = hiprl._batch_struct(empty)
    assert e.lib.rl_adjust(e.h, C.byref(s), None, 0, None, C.byref(rep)) == 0 and bytes(rep) == bytes(64)
    e.close()


def test_python_mirror_adjust():
    t = 1_700_000_007
    c = hiprl.HipRateLimitCache(lambda: t, local_cache=True, log2_slots=SMALL, max_batch_desc=256)
    lim = hiprl.NewRateLimit(5, M, "k", hiprl.StatsStore())
    req = hiprl.NewRateLimitRequest("adj", [[("k", "m")], [("k", "nil")]], 7)
    assert c.DoLimit(req, [lim, None]).DescriptorStatuses[0].Code == hiprl.CODE_OVER_LIMIT
    hits = lim.Stats.TotalHits.Value()
    before = c.adjust(req, [lim, None], [-3, -3])
    assert [(int(x["count"]), int(x["flags"])) for x in before] == [(7, F | LC), (0, NILF)]
    assert lim.Stats.TotalHits.Value() == hits
    one = hiprl.NewRateLimitRequest("adj", [[("k", "m")], [("k", "nil")]], 1)
    r = c.DoLimit(one, [lim, None])
    assert (r.DescriptorStatuses[0].Code, r.DescriptorStatuses[0].LimitRemaining) == (hiprl.CODE_OK, 0)  # 4 + 1
    before = c.adjust(req, [lim, None], [2, 0], keep_cache=True)
    assert (int(before[0]["count"]), int(before[0]["flags"])) == (5, F)
    assert c.DoLimit(one, [lim, None]).DescriptorStatuses[0].Code == hiprl.CODE_OVER_LIMIT  # 7 + 1
    c.engine.close()
