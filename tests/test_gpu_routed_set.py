"""Routed set (rl_hip.h "Routed set") on the GPU.

Engine level: rl_set_routed_plan + rl_set_routed_commit over host-built records leave an engine
exactly where Engine.set (pinned to the oracle by test_gpu_set.py) leaves its twin. Router level,
local transport, emulated collectives and a one-rank RCCL communicator: counters peeked in a world
of three shards and set into a world of another size make that world decide the rest of the stream
as the oracle that ran all of it; duplicates resolve in the router's serial order, per part; and a
call refused at one origin or at one owner (after the records moved) leaves every engine untouched.
Every plan (key pools, owners, guards) is made on the CPU from the oracle alone.
"""
import functools

import numpy as np
import pytest
import torch

import hiprl
import oracle
import routing
from streams import RULES
from test_gpu_combining import Bufs
from test_gpu_emulated_router import parallel
from test_gpu_routed_peek import (DEV, MAXD, NIL, SEED, T0, EmuWorld, LocalWorld, check_against_oracle, check_step,
                                  distinct_keys, engine_plan, key_batch, key_string, make_oracle, new_engines,
                                  owner_of, records_of, state_of, steps_of, unseen_keys)
from test_gpu_set import SMALL, rec_set, state, vals

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC, ECAPACITY, ESTATE, EPEER = -1, -3, -4, -5, -7
F, LC, PS = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_PER_SECOND
KC, KF = hiprl.SET_KEEP_COUNTER, hiprl.SET_KEEP_CACHE
P = hiprl.PEEK_DTYPE
MINUTE_RULES = [i for i, (_, u) in enumerate(RULES) if u == hiprl.MINUTE]
assert MINUTE_RULES and T0 % 60 < 50  # T0 .. T0 + 9 lie in one minute


def code_of(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except hiprl.RedisError as e:
        return e.code
    return None


def to_dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(DEV)


def plan_commit(e, pb, v, apply=True, rec=None):
    """Engine.set's twin: plan + commit over the host-built records of pb. -> the replies."""
    rec = records_of(pb) if rec is None else rec
    n = rec.shape[0]
    d_rec, d_val = to_dev(rec), to_dev(v)
    d_rep = torch.full((max(1, n) * 16,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    e.set_routed_plan(d_rec.data_ptr(), d_val.data_ptr(), n, d_rep.data_ptr())
    e.set_routed_commit(apply)
    torch.cuda.synchronize()
    return d_rep.cpu().numpy().view(P)[:n].copy()


def set_values(items, n, split, local_cache):
    """n values over the items, every kind of write: FOUND with and without a cache entry, DEL, the
    KEEP bits, a peek; a later duplicate of a string always differs from an earlier one (count)."""
    rows = []
    for i in range(n):
        k = i % 6
        c, ttl, cs = i + 1, 30 + i % 50, 5 + i % 9
        rows.append([(c, ttl, cs, F | LC), (0, 0, 0, 0), (c, ttl, 0, F | KF), (0, 0, cs, LC | KC),
                     (c, ttl, cs, F | LC | KC | KF), (c, ttl, 0, F)][k])
    return vals(rows)


# ---- 1. the record form equals the host form ---------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("local_cache", [False, True])
def test_record_form_equals_host_form(local_cache, split):
    batches, t, pool = engine_plan(local_cache, split)
    a, b = (hiprl.Engine(local_cache=local_cache, per_second_split=split, max_batch_desc=1 << 12) for _ in range(2))
    for e in (a, b):
        e.load_rules(RULES)
        for bt in batches:
            e.submit(bt)
    assert rec_set(a) == rec_set(b)
    for n in (1, 255, 256, 257, 3001):
        items = [pool[(7 * n + i) % len(pool)] for i in range(n)]  # seen and unseen strings, interleaved
        if n > 1:  # duplicates in one wave, in another wave and (3001 > the pool) in other blocks
            items[n - 1] = items[0]
            items[n // 2] = items[0]
        pb = key_batch(items, t)
        v = set_values(items, n, split, local_cache)
        dup = len(items) - len(set(items))
        assert n == 1 or dup >= 2
        want = a.set(pb, v)
        got = plan_commit(b, pb, v)
        assert got.tobytes() == want.tobytes(), (n, np.flatnonzero(got != want)[:5])
        assert rec_set(a) == rec_set(b), n
        assert a.occupancy() == b.occupancy(), n
        sa, sb = a.stats(), b.stats()
        assert (sa["inserted_keys"], sa["live_keys"]) == (sb["inserted_keys"], sb["live_keys"]), n
        assert np.array_equal(a.peek(pb), b.peek(pb))
    assert b.stats()["inserted_keys"] > 0

    # commit(0) drops the plan: census, occupancy, stats and the table word for word
    n = 300
    items = unseen_keys(n - 100, "drop") + pool[:100]
    pb = key_batch(items, t)
    v = vals([(i + 1, 40, 0, F) for i in range(n)])
    s0, r0 = state(b, t), rec_set(b)
    rec = records_of(pb)
    d_rec, d_val = to_dev(rec), to_dev(v)
    torch.cuda.synchronize()
    assert code_of(b.set_routed_commit, True) == ESTATE  # no plan open
    b.set_routed_plan(d_rec.data_ptr(), d_val.data_ptr(), n)
    assert code_of(b.set_routed_plan, d_rec.data_ptr(), d_val.data_ptr(), n) == ESTATE  # a plan is open
    assert code_of(b.submit, batches[-1]) == ESTATE
    assert code_of(b.peek, pb) == ESTATE
    b.set_routed_commit(False)
    assert code_of(b.set_routed_commit, False) == ESTATE
    assert state(b, t) == s0 and rec_set(b) == r0
    # an empty plan opens and commits
    b.set_routed_plan(0, 0, 0)
    b.set_routed_commit(True)
    assert state(b, t) == s0

    # malformed records and values between good neighbours: nothing written, not even the neighbours
    main = next(i for i in range(150, n) if not (split and RULES[items[i][1]][1] == hiprl.SECOND))
    for what in ("rule", "now", "ttl"):
        rec2, v2 = rec.copy(), v.copy()
        if what == "rule":
            rec2["rule"][5] = len(RULES)
        elif what == "now":
            rec2["now"][100] = 0xFFFD0001
        else:
            v2[main] = (3, 0, 0, F)
        d_rec2, d_val2 = to_dev(rec2), to_dev(v2)
        torch.cuda.synchronize()
        assert code_of(b.set_routed_plan, d_rec2.data_ptr(), d_val2.data_ptr(), n) == EINVAL, what
        assert code_of(b.set_routed_commit, True) == ESTATE  # the refused plan is not open
        assert state(b, t) == s0 and rec_set(b) == r0, what
    assert code_of(b.set_routed_plan, d_rec.data_ptr(), d_val.data_ptr(), (1 << 12) + 1) == ECAPACITY
    assert code_of(b.set_routed_plan, 0, d_val.data_ptr(), n) == EINVAL
    # and the same records are accepted afterwards
    b.set_routed_plan(d_rec.data_ptr(), d_val.data_ptr(), n)
    b.set_routed_commit(True)
    assert np.array_equal(b.peek(pb)["count"], v["count"])
    # rl_reset closes an open plan
    b.set_routed_plan(d_rec.data_ptr(), d_val.data_ptr(), n)
    b.reset()
    assert code_of(b.set_routed_commit, True) == ESTATE
    assert sum(b.occupancy()["live"]) == 0
    a.close()
    b.close()


# ---- worlds over given engines -----------------------------------------------------------------------
class LocalW(LocalWorld):
    def __init__(self, engines):
        self.G = len(engines)
        self.engines = engines
        self.router = hiprl.Router(engines, max_desc=MAXD)


class EmuW(EmuWorld):
    def __init__(self, engines):
        G = self.G = len(engines)
        wid = hiprl.Router.emu_world(G)
        self.engines = engines
        self.routers = [None] * G

        def mk(r):
            self.routers[r] = hiprl.Router([engines[r]], max_desc=MAXD, n_shards=G, rank=r, rccl_id=wid,
                                           emulated=True, host=True)
        parallel(G, mk)
        assert all(r is not None for r in self.routers)


def world_of(transport, engines):
    return LocalW(engines) if transport == "local" else EmuW(engines)


def set_call(w, batches, values, want_out=True):
    """One Router.set of the world. -> (one reply array per origin or None, the code per origin)."""
    G = w.G
    if isinstance(w, LocalWorld):
        try:
            return w.router.set(batches, values, want_out=want_out), [None] * G
        except hiprl.RedisError as e:
            return None, [e.code] * G
    reps, codes = [None] * G, [None] * G

    def worker(r):
        try:
            got = w.routers[r].set([batches[r]], [values[r]], want_out=want_out)
            reps[r] = got[0] if want_out else None
        except hiprl.RedisError as e:
            codes[r] = e.code
    parallel(G, worker)
    return (reps if all(c is None for c in codes) else None), codes


def deal(row, G2):
    """A row of three origin batches as steps of a world of G2 origins, the serial order kept (one
    origin takes the three batches as three steps: together they pass its max_desc)."""
    if G2 == 1:
        return [[b] for b in row]
    if G2 == 2:
        return [[routing.concat_batches(row[:2]), row[2]]]
    assert G2 == 4 and row[2].jit is None
    h = row[2].n_req // 2
    return [[row[0], row[1], row[2].slice_requests(0, h), row[2].slice_requests(h, row[2].n_req)]]


# ---- 2. resharding -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reshard_plan(local_cache):
    steps = steps_of(3, 6, 131)
    cut = 3
    t = T0 + cut
    o = make_oracle(local_cache)
    for row in steps[:cut]:
        o.submit(routing.concat_batches(row))
    seen = distinct_keys([b for row in steps[:cut] for b in row])
    st = {it: state_of(o, it, t) for it in seen}
    found = [it for it in seen if st[it][0] >= 0]
    cached = [it for it in seen if st[it][1]]
    assert len(found) >= 30 and (not local_cache or len(cached) >= 10), (len(found), len(cached))
    # a world that was not set decides the rest differently
    full, fresh = make_oracle(local_cache), make_oracle(local_cache)
    for row in steps[:cut]:
        full.submit(routing.concat_batches(row))
    differ = 0
    for row in steps[cut:]:
        sb = routing.concat_batches(row)
        differ += int((full.submit(sb)[0] != fresh.submit(sb)[0]).sum())
    assert differ >= 5, differ
    return steps, cut, t, seen, found


@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("transport,G2", [("emulated", 4), ("local", 2), ("local", 1)])
def test_resharding(transport, G2, local_cache):
    steps, cut, t, seen, found = reshard_plan(local_cache)
    ctx = f"reshard {transport} G2={G2} local={local_cache}"
    for j in range(G2):  # every owner of the new world receives live keys
        assert any(owner_of(it, G2) == j for it in found), (ctx, j)
    old = LocalWorld(3, local_cache)
    o = make_oracle(local_cache)
    for s, row in enumerate(steps[:cut]):
        check_step(o, row, old.step(row), f"{ctx} step={s}")
    asks = [key_batch(seen[g::3], t) for g in range(3)]
    reps, codes = old.ask("peek", asks)
    assert reps is not None, (ctx, codes)
    value = {}
    for b, rep in zip(asks, reps):
        check_against_oracle(rep, b, o, ctx=ctx)
        for i in range(b.n_desc):
            value[(b.prefix(i), int(b.rule[i]))] = rep[i]
    old.close()
    # dealt to the new world's origins round-robin regardless of owner; origin 1 (if any) passes
    # nothing; as many calls as the origins' max_desc asks for (one where three origins share the keys)
    origins = [g for g in range(G2) if g != 1 or G2 == 1]
    new = world_of(transport, new_engines(G2, local_cache))
    per_call = MAXD * len(origins)
    for c0 in range(0, len(seen), per_call):
        share = {g: [] for g in range(G2)}
        for i, it in enumerate(seen[c0:c0 + per_call]):
            share[origins[i % len(origins)]].append(it)
        batches = [key_batch(share[g], t) for g in range(G2)]
        values = [np.array([value[it] for it in share[g]], P).reshape(len(share[g])) for g in range(G2)]
        assert G2 == 1 or batches[1].n_desc == 0
        before, codes = set_call(new, batches, values)
        assert before is not None, (ctx, codes)
        # a fresh world: nothing found (a later call may meet a string an earlier one set: two rules
        # of one unit share their key strings)
        assert c0 or not any((r["flags"] & (F | LC)).any() for r in before)
    for s, row in enumerate(steps[cut:], cut):
        for row2 in deal(row, G2):
            check_step(o, row2, new.step(row2), f"{ctx} step={s}")
    new.close()


# ---- 3. duplicates across origins --------------------------------------------------------------------
def test_duplicates_across_origins_last_in_serial_order_wins_per_part():
    G = 3
    steps = steps_of(G, 2, 77)
    w = LocalWorld(G, True)
    o = make_oracle(True)
    check_step(o, steps[0], w.step(steps[0]), "dup step=0")
    t = T0 + 1
    live = [it for it in distinct_keys(steps[0]) if state_of(o, it, t)[0] >= 0 and RULES[it[1]][1] != hiprl.SECOND]
    assert len(live) >= 12
    keys = live[:12] + [(p, MINUTE_RULES[0]) for p, _ in unseen_keys(12, "dup")]
    parts = [(p, MINUTE_RULES[0]) for p, _ in unseen_keys(8, "parts")]
    assert {owner_of(it, G) for it in keys} == {0, 1, 2}
    n = len(keys)
    b0 = key_batch(keys + parts, t)
    v0 = vals([(100 + i, 50, 0, F) for i in range(n)] + [(7 + i, 45, 0, F | KF) for i in range(len(parts))])
    b2 = key_batch(keys + keys[::-1] + parts, t)
    first = [(200 + i, 51, 9, F | LC) for i in range(n)]
    last = [(300 + i, 52 + i, 11 + i, F | LC) if i % 3 else (0, 0, 0, 0) for i in range(n)]  # (every third: a DEL)
    v2 = vals(first + last[::-1] + [(0, 0, 20 + i, LC | KC) for i in range(len(parts))])
    b1 = key_batch([], t)
    ask = key_batch(keys + parts, t)
    before = w.router.peek([ask, b1, b1])[0]
    check_against_oracle(before, ask, o, ctx="dup before")
    assert (before["flags"] & F).sum() == 12
    outs = w.router.set([b0, b1, b2], [v0, vals([]), v2])
    # out of every duplicate, across origins and inside origin 2, is the state before the call
    assert np.array_equal(outs[0], before)
    assert np.array_equal(outs[2], np.concatenate([before[:n], before[:n][::-1], before[n:]]))
    after = w.router.peek([b1, ask, b1])[1]
    for i in range(n):  # origin 2's last value, per part
        c, ttl, cs, fl = last[i]
        assert tuple(int(x) for x in after[i]) == (c, ttl, cs, fl), (i, after[i])
    for i in range(len(parts)):  # the counter from origin 0, the cache entry from origin 2
        assert tuple(int(x) for x in after[n + i]) == (7 + i, 45, 20 + i, F | LC), (i, after[n + i])
    w.close()


# ---- 4. all-or-nothing across ranks ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def aon_plan():
    G = 3
    steps = steps_of(G, 3, 91)
    o = make_oracle(True)
    o.submit(routing.concat_batches(steps[0]))
    t = T0 + 1
    live = [it for it in distinct_keys(steps[0]) if state_of(o, it, t)[0] >= 0]
    assert len(live) >= 110
    return steps, t, live[:40], live[40:80], live[80:110]


def good_values(n, base=500):
    return vals([(base + i, 44, 0, F) for i in range(n)])


def states(w, t):
    return [state(e, t) for e in w.engines]


@pytest.mark.parametrize("case", ["rule", "ttl", "capacity"])
@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_origin_refusals_change_nothing(transport, case):
    steps, t, good0, good2, mid = aon_plan()
    G = 3
    ctx = f"origin refusal {transport} {case}"
    w = world_of(transport, new_engines(G, True))
    o = make_oracle(True)
    check_step(o, steps[0], w.step(steps[0]), f"{ctx} step=0")
    b0, b2 = key_batch(good0, t), key_batch(good2, t)
    if case == "rule":
        b = key_batch(mid, t)
        rule = b.rule.copy()
        rule[3] = 99
        bad, vbad, code = hiprl.Batch(b.blob, b.off, rule, b.req_of, b.now, b.hits), good_values(len(mid)), EINVAL
    elif case == "ttl":
        vbad = good_values(len(mid))
        vbad[7] = (3, 0, 0, F)
        # (no per-second split here: every counter is main-store)
        bad, code = key_batch(mid, t), EINVAL
    else:
        items = [mid[i % len(mid)] for i in range(MAXD + 1)]
        bad, vbad, code = key_batch(items, t), good_values(MAXD + 1), ECAPACITY
    s0 = states(w, t)
    reps, codes = set_call(w, [b0, bad, b2], [good_values(len(good0)), vbad, good_values(len(good2))])
    assert reps is None
    assert codes == ([code] * 3 if transport == "local" else [EPEER, code, EPEER]), (ctx, codes)
    assert states(w, t) == s0, ctx
    check_step(o, steps[1], w.step(steps[1]), f"{ctx} step=1")
    w.close()


@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_owner_enospc_after_the_records_moved_writes_nothing_anywhere(transport):
    """Owner 1's MINUTE region is too small for its share, owners 0 and 2 fit theirs. This is the
    test a one-phase design fails: with every owner committing right after its own plan (tried
    once, not kept), owners 0 and 2 each held 40 live MINUTE slots after the refused call, on both
    transports."""
    G = 3
    t = T0 + 1
    ctx = f"owner ENOSPC {transport}"
    engines = new_engines(G, True)
    engines[1].close()
    engines[1] = hiprl.Engine(local_cache=True, max_batch_desc=MAXD * G, log2_slots=SMALL)
    engines[1].load_rules(RULES)
    region = (hiprl.MINUTE - 1) * 2 + ((t // 60) & 1)
    assert t // 60 * 60 % 3600  # the minute's strings are at home in the MINUTE regions
    limit = engines[1].occupancy()["limit"][region]
    assert 0 < limit < 1024
    cand = [(p, MINUTE_RULES[0]) for p, _ in unseen_keys(6 * limit + 400, "nospc")]
    own = [owner_of(it, G) for it in cand]
    mine1 = [it for it, j in zip(cand, own) if j == 1][:limit + 1]
    others = [it for it, j in zip(cand, own) if j == 0][:40] + [it for it, j in zip(cand, own) if j == 2][:40]
    assert len(mine1) == limit + 1 and len(others) == 80
    for j in (0, 2):
        assert engines[j].occupancy()["limit"][region] > len(cand)
    w = world_of(transport, engines)
    # dealt over the origins regardless of owner: every origin holds keys of every owner
    allk = others + mine1
    share = [allk[g::G] for g in range(G)]
    for g in range(G):
        assert {owner_of(it, G) for it in share[g]} == {0, 1, 2}
    batches = [key_batch(share[g], t) for g in range(G)]
    values = [good_values(len(share[g])) for g in range(G)]
    s0 = states(w, t)
    r0 = [rec_set(e) for e in w.engines]
    reps, codes = set_call(w, batches, values)
    assert reps is None
    assert codes == ([ENOSPC] * 3 if transport == "local" else [EPEER, ENOSPC, EPEER]), (ctx, codes)
    # owners 0 and 2 planned successfully and have written nothing
    assert states(w, t) == s0, ctx
    assert [rec_set(e) for e in w.engines] == r0, ctx
    # one string fewer at owner 1 fits, everywhere
    g1 = next(g for g in range(G) if mine1[0] in share[g])
    batches[g1] = key_batch([it for it in share[g1] if it != mine1[0]], t)
    assert batches[g1].n_desc == len(share[g1]) - 1
    reps, codes = set_call(w, batches, [good_values(b.n_desc) for b in batches])
    assert reps is not None, (ctx, codes)
    assert [e.stats()["inserted_keys"] for e in w.engines] == [40, limit, 40]
    w.close()


@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_two_generations_of_one_region_from_two_origins(transport):
    """Origin 0 at t, origin 2 two minutes later (the same MINUTE region: the minute between them
    lives in the region of the other parity), with owner 1's keys among both."""
    G = 3
    t = T0 + 1
    ctx = f"two generations {transport}"
    cand = [(p, MINUTE_RULES[0]) for p, _ in unseen_keys(400, "gens")]
    by = {j: [it for it in cand if owner_of(it, G) == j] for j in range(G)}
    assert all(len(by[j]) >= 40 for j in range(G))
    k0 = by[0][:20] + by[1][:20]    # origin 0: owners 0 and 1
    k2 = by[1][20:40] + by[2][:20]  # origin 2: owners 1 and 2
    w = world_of(transport, new_engines(G, True))
    empty = key_batch([], t)
    batches = [key_batch(k0, t), empty, key_batch(k2, t + 120)]
    values = [good_values(len(k0)), vals([]), good_values(len(k2), 900)]
    s0 = states(w, t)
    reps, codes = set_call(w, batches, values)
    assert reps is None
    assert codes == ([EINVAL] * 3 if transport == "local" else [EPEER, EINVAL, EPEER]), (ctx, codes)
    assert states(w, t) == s0, ctx
    # each origin's batch alone is accepted
    reps, codes = set_call(w, [batches[0], empty, key_batch([], t + 120)], [values[0], vals([]), vals([])])
    assert reps is not None, (ctx, codes)
    reps, codes = set_call(w, [empty, empty, batches[2]], [vals([]), vals([]), values[2]])
    assert reps is not None, (ctx, codes)
    assert sum(e.stats()["inserted_keys"] for e in w.engines) == len(k0) + len(k2)
    w.close()


@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_set_with_a_step_in_flight(transport):
    steps, t, good0, good2, _ = aon_plan()
    G = 3
    ctx = f"in flight {transport}"
    w = world_of(transport, new_engines(G, True))
    o = make_oracle(True)
    check_step(o, steps[0], w.step(steps[0]), f"{ctx} step=0")
    empty = key_batch([], t)
    batches = [key_batch(good0, t), empty, key_batch(good2, t)]
    bf = Bufs(steps[1])
    bs, outs, thrs = bf.args()
    torch.cuda.synchronize()
    if transport == "local":
        w.router.submit(bs, outs, thrs)
        codes = [code_of(w.router.set, batches, [good_values(b.n_desc) for b in batches])] * G
        w.router.wait()
    else:
        codes = [None] * G

        def worker(r):
            R = w.routers[r]
            R.submit([bs[r]], [outs[r]], [thrs[r]])
            codes[r] = code_of(R.set, [batches[r]], [good_values(batches[r].n_desc)])
            R.wait()
        parallel(G, worker)
    assert codes == [ESTATE] * G, (ctx, codes)
    check_step(o, steps[1], bf.results(), f"{ctx} step=1")
    # and the call works afterwards: out is the state before it
    reps, codes = set_call(w, batches, [good_values(b.n_desc) for b in batches])
    assert reps is not None, (ctx, codes)
    check_against_oracle(reps[0], batches[0], o, ctx=ctx)
    check_against_oracle(reps[2], batches[2], o, ctx=ctx)
    w.close()


# ---- 5. occupancy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_occupancy_after_a_routed_set(transport):
    G = 3
    steps = steps_of(G, 3, 57)
    ctx = f"occupancy {transport}"
    w = world_of(transport, new_engines(G, True))
    o = make_oracle(True)
    check_step(o, steps[0], w.step(steps[0]), f"{ctx} step=0")
    t = T0 + 1
    live = [it for it in distinct_keys(steps[0]) if state_of(o, it, t)[0] >= 0][:60]
    absent = [(p, MINUTE_RULES[i % len(MINUTE_RULES)]) for i, (p, _) in enumerate(unseen_keys(150, "occ"))]
    allk = absent + live + absent[:30]  # U = 150 distinct absent strings, overwrites, duplicates
    share = [allk[g::G] for g in range(G)]
    batches = [key_batch(share[g], t) for g in range(G)]
    # an overwrite keeps what the key holds (the oracle has no setter): its own peek reply fed back
    reps, codes = w.ask("peek", batches)
    assert reps is not None, codes
    values = []
    for g in range(G):
        v = reps[g].copy()
        for i, it in enumerate(share[g]):
            if it in absent:
                v[i] = (3, 50, 0, F)
        values.append(v)
    ins0 = [e.stats()["inserted_keys"] for e in w.engines]
    cen0 = [int(np.sum(e.census(t)["live"])) for e in w.engines]
    reps, codes = set_call(w, batches, values, want_out=False)
    assert codes == [None] * G, (ctx, codes)
    ins1 = [e.stats()["inserted_keys"] for e in w.engines]
    per_owner = [sum(1 for it in absent if owner_of(it, G) == j) for j in range(G)]
    assert min(per_owner) >= 20
    assert [b - a for a, b in zip(ins0, ins1)] == per_owner and sum(per_owner) == 150
    for j, e in enumerate(w.engines):
        assert int(np.sum(e.census(t)["live"])) == cen0[j] + per_owner[j], (ctx, j)
    # the set strings are outside the stream and every overwrite kept its value: the following
    # routed steps (whose capacity checks read the occupancy the set published) are the oracle's
    for s in (1, 2):
        check_step(o, steps[s], w.step(steps[s]), f"{ctx} step={s}")
    w.close()


# ---- 6. one-rank RCCL communicator -------------------------------------------------------------------
def test_rccl_one_rank_peek_set_elsewhere_and_continue(monkeypatch):
    monkeypatch.setenv("NCCL_SOCKET_IFNAME", "lo")
    steps = steps_of(1, 4, 19)

    def mk():
        es = new_engines(1, True)
        return es, hiprl.Router(es, max_desc=MAXD, n_shards=1, rank=0, rccl_id=hiprl.Router.unique_id())

    def step(r, row):
        bf = Bufs(row)
        torch.cuda.synchronize()
        r.step(*bf.args())
        return bf.results()
    es1, r1 = mk()
    o = make_oracle(True)
    for s, row in enumerate(steps[:2]):
        check_step(o, row, step(r1, row), f"rccl step={s}")
    t = T0 + 2
    seen = distinct_keys([b for row in steps[:2] for b in row])
    assert len(seen) <= MAXD
    pb = key_batch(seen, t)
    v = r1.peek([pb])[0]
    f, _, c = check_against_oracle(v, pb, o, ctx="rccl peek")
    assert f >= 30 and c >= 5, (f, c)
    r1.close()
    es2, r2 = mk()
    before = r2.set([pb], [v])[0]
    assert not (before["flags"] & (F | LC)).any()
    assert np.array_equal(r2.peek([pb])[0], v)
    for s, row in enumerate(steps[2:], 2):
        check_step(o, row, step(r2, row), f"rccl step={s}")
    r2.close()
