"""Routed adjust (rl_hip.h "Routed adjust") on the GPU.

Origin: rl_route_pack_adjust behind the plain pack changes two words of every record and nothing
else. Engine level: rl_adjust_routed_plan + rl_adjust_routed_commit over host-built records leave an
engine exactly where Engine.adjust (pinned to the oracle and the model by test_gpu_adjust.py) leaves
its twin. Router level, local transport, emulated collectives and a one-rank RCCL communicator: a
world that charged h and got r back from another origin decides the rest of a stream as the oracle
that was charged h - r; every call equals the dict model of routed_adjust_model.py; and a call
refused at one origin or at one owner (after the records moved) leaves every engine untouched.
Every plan (keys, owners, guards) is made on the CPU from the oracle and the model alone.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hiprl
import oracle
import router as pyrouter
import routing
from routed_adjust_model import routed_adjust_model
from test_gpu_adjust import CASES, M0, RULES1, T1, pfx, strings_of
from test_gpu_combining import Bufs
from test_gpu_emulated_router import parallel
from test_gpu_routed_peek import (DEV, MAXD, NIL, LocalWorld, check_against_oracle, check_step, engine_plan, key_batch,
                                  owner_of, records_of, unseen_keys)
from test_gpu_routed_set import code_of, states, to_dev, world_of
from test_gpu_set import rec_set, state
from streams import RULES

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE, EPEER = -1, -4, -5, -7
F, LC, NILF, PS, BAD = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND, hiprl.PEEK_BAD
P = hiprl.PEEK_DTYPE
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
KEEP_BIT = 1 << 16  # a record's rule word: RL_ADJUST_KEEP_CACHE
REPORT_SUMS = ("absent", "applied", "floored", "capped", "unfrozen")


def adjust_records(pb, deltas, keep=False):
    """The records an origin's two pack steps write for pb: h is the delta, bit 16 of rule the flag."""
    rec = records_of(pb)
    rec["h"] = np.asarray(deltas, np.int64).astype(np.int32).view(np.uint32)
    if keep:
        rec["rule"] |= KEEP_BIT
    return rec


def plan_commit(e, rec, apply=True):
    """Engine.adjust's twin: plan + commit over records. -> (the replies, the report)"""
    n = rec.shape[0]
    d_rec = to_dev(rec)
    d_rep = torch.full((max(1, n) * 16,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    e.adjust_routed_plan(d_rec.data_ptr(), n, d_rep.data_ptr())
    rep = e.adjust_routed_commit(apply)
    torch.cuda.synchronize()
    return d_rep.cpu().numpy().view(P)[:n].copy(), rep


# ---- 1. the origin's second pack step ------------------------------------------------------------------
@pytest.mark.parametrize("keep", [False, True])
def test_pack_adjust_changes_two_words_of_every_record_and_nothing_else(keep):
    G = 3
    e = hiprl.Engine(max_batch_desc=1 << 10)
    e.load_rules(RULES)
    t = 1_700_000_007
    rng = np.random.default_rng(11)
    for n in (1, 255, 256, 257):
        items = [(p, NIL if i % 3 == 1 else r) for i, (p, r) in enumerate(unseen_keys(n, f"pack{n}"))]
        hb = key_batch(items, t)
        nil = hb.rule == NIL
        assert n == 1 or (nil.sum() >= n // 3 and (~nil).sum() >= n // 3)
        db = pyrouter.DeviceBatch.from_host(hb, DEV)
        stride = n + 5
        send = torch.full((G * stride * 32 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        x = torch.zeros(2 * G, dtype=torch.int32, device=DEV)
        perm = torch.zeros(n, dtype=torch.int32, device=DEV)
        deltas = rng.integers(-50, 50, n).astype(np.int32)
        deltas[0], deltas[n // 2] = INT32_MIN, INT32_MAX
        d_delta = torch.from_numpy(deltas).to(DEV)
        torch.cuda.synchronize()
        e.route_pack_strided(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), 1, G, stride, send.data_ptr(),
                             x.data_ptr(), perm.data_ptr())
        torch.cuda.synchronize()
        plain = send.cpu().numpy().copy()
        pm = perm.cpu().numpy().view(np.uint32)
        assert np.array_equal(pm == hiprl.ROUTE_LOCAL, nil) and not x.cpu().numpy()[1::2].any()
        e.route_pack_adjust(n, db.rule.data_ptr(), perm.data_ptr(), d_delta.data_ptr(), send.data_ptr(), keep_cache=keep)
        torch.cuda.synchronize()
        got = send.cpu().numpy()
        want = plain.copy()
        wrec = want[:G * stride * 32].view(routing.REC_DTYPE)
        for i in np.flatnonzero(~nil):
            assert int(wrec[pm[i]]["rule"]) == int(hb.rule[i]) and int(wrec[pm[i]]["h"]) == 1  # the plain pack's
            wrec[pm[i]]["h"] = deltas[i:i + 1].view(np.uint32)[0]
            wrec[pm[i]]["rule"] = int(hb.rule[i]) | (KEEP_BIT if keep else 0)
        # every record equals the plain pack's but for h and the rule word's upper half; every byte
        # outside the records (the owners' unused tails, the slack) is untouched
        assert got.tobytes() == want.tobytes(), (n, np.flatnonzero(got != want)[:8])
        assert (got[G * stride * 32:] == 0xA5).all()
    # refusals: a null array with n_desc > 0, a flag bit other than KEEP_CACHE; n_desc == 0 launches nothing
    s = hiprl.RlBatch()
    s.n_desc, s.rule_id = 4, db.rule.data_ptr()
    pa, da, sa = perm.data_ptr(), d_delta.data_ptr(), send.data_ptr()
    assert e.lib.rl_route_pack_adjust(e.h, C.byref(s), None, da, 0, sa) == EINVAL
    assert e.lib.rl_route_pack_adjust(e.h, C.byref(s), pa, None, 0, sa) == EINVAL
    assert e.lib.rl_route_pack_adjust(e.h, C.byref(s), pa, da, 0, None) == EINVAL
    assert e.lib.rl_route_pack_adjust(e.h, C.byref(s), pa, da, 2, sa) == EINVAL
    s.n_desc = 0
    assert e.lib.rl_route_pack_adjust(e.h, C.byref(s), None, None, 1, None) == 0
    torch.cuda.synchronize()
    assert send.cpu().numpy().tobytes() == got.tobytes()
    e.close()


# ---- 2. the record form equals the host form -----------------------------------------------------------
def twin_engines(local_cache, split):
    batches, t, pool = engine_plan(local_cache, split)
    es = [hiprl.Engine(local_cache=local_cache, per_second_split=split, max_batch_desc=1 << 12) for _ in range(2)]
    for e in es:
        e.load_rules(RULES)
        for bt in batches:
            e.submit(bt)
    return es, batches, t, pool


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("local_cache", [False, True])
def test_record_form_equals_host_form(local_cache, split):
    (a, b), _, t, pool = twin_engines(local_cache, split)
    assert rec_set(a) == rec_set(b)
    rng = np.random.default_rng(7)
    applied = 0
    for keep in (False, True):
        for n in (1, 255, 256, 257, 3001):
            items = [pool[(7 * n + i) % len(pool)] for i in range(n)]  # seen and unseen strings, interleaved
            if n > 1:  # duplicates in one wave, in another wave and (3001 > the pool) in other blocks
                items[n - 1] = items[0]
                items[n // 2] = items[0]
            assert n == 1 or len(items) - len(set(items)) >= 2
            pb = key_batch(items, t)
            d = rng.integers(-6, 4, n).astype(np.int64)  # mostly small, more refunds than charges
            if n > 1:
                d[3], d[n - 2] = INT32_MIN, INT32_MAX
                assert (d == INT32_MIN).sum() >= 1 and (d == INT32_MAX).sum() >= 1 and (d < 0).sum() >= n // 3
            want, want_rep = a.adjust(pb, d, keep_cache=keep)
            got, rep = plan_commit(b, adjust_records(pb, d, keep))
            assert got.tobytes() == want.tobytes(), (n, keep, np.flatnonzero(got != want)[:5])
            assert rep == want_rep and rep["nil"] == 0 and rep["descriptors"] == n == rep["absent"] + rep["applied"]
            assert rec_set(a) == rec_set(b), (n, keep)
            assert a.occupancy() == b.occupancy() and a.stats() == b.stats(), (n, keep)
            assert np.array_equal(a.peek(pb), b.peek(pb))
            applied += rep["applied"]
            assert not keep or rep["unfrozen"] == 0
    assert applied >= 30, applied  # engine_plan's guard: at least 30 strings of the pool are found
    a.close()
    b.close()


# ---- 3. the plan's lifecycle, malformed records ----------------------------------------------------------
def test_plan_lifecycle_and_malformed_records():
    (a, b), batches, t, pool = twin_engines(True, False)
    n = 300
    items = unseen_keys(100, "life") + pool[:200]
    pb = key_batch(items, t)
    d = np.array([-3 + i % 5 for i in range(n)], np.int64)
    rec = adjust_records(pb, d)
    found = int((b.peek(pb)["flags"] & F != 0).sum())
    assert found >= 50 and n - found >= 100
    s0, r0 = state(b, t), rec_set(b)
    d_rec = to_dev(rec)
    d_val = to_dev(np.zeros(n, P))
    torch.cuda.synchronize()
    assert code_of(b.adjust_routed_commit, True) == ESTATE  # no plan open
    b.adjust_routed_plan(d_rec.data_ptr(), n)
    # with a plan open: submit, peek, adjust, a set plan, a second plan, the set's commit
    assert code_of(b.submit, batches[-1]) == ESTATE
    assert code_of(b.peek, pb) == ESTATE
    assert code_of(b.adjust, pb, d) == ESTATE
    assert code_of(b.set_routed_plan, d_rec.data_ptr(), d_val.data_ptr(), n) == ESTATE
    assert code_of(b.adjust_routed_plan, d_rec.data_ptr(), n) == ESTATE
    assert code_of(b.set_routed_commit, True) == ESTATE
    assert code_of(b.set_routed_commit, False) == ESTATE
    # commit(0) drops the plan: census, occupancy, stats and the table word for word
    assert b.adjust_routed_commit(False) == dict.fromkeys(hiprl.ADJUST_REPORT_FIELDS, 0)
    assert code_of(b.adjust_routed_commit, False) == ESTATE
    assert state(b, t) == s0 and rec_set(b) == r0
    # the reverse: an adjust commit on a set plan, which stays open
    b.set_routed_plan(0, 0, 0)
    assert code_of(b.adjust_routed_commit, True) == ESTATE
    assert code_of(b.adjust_routed_plan, d_rec.data_ptr(), n) == ESTATE
    b.set_routed_commit(True)
    # an empty plan opens and commits
    b.adjust_routed_plan(0, 0)
    assert b.adjust_routed_commit(True) == dict.fromkeys(hiprl.ADJUST_REPORT_FIELDS, 0)
    assert state(b, t) == s0 and rec_set(b) == r0

    # malformed records between good neighbours: nothing written, not even the neighbours
    for what in ("rule", "now", "bit17"):
        rec2 = rec.copy()
        if what == "rule":
            rec2["rule"][5] = len(RULES)
        elif what == "now":
            rec2["now"][150] = 0xFFFD0001
        else:
            rec2["rule"][257] |= 1 << 17
        d_rec2 = to_dev(rec2)
        d_rep = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        assert code_of(b.adjust_routed_plan, d_rec2.data_ptr(), n, d_rep.data_ptr()) == EINVAL, what
        assert code_of(b.adjust_routed_commit, True) == ESTATE  # the refused plan is not open
        assert state(b, t) == s0 and rec_set(b) == r0, what
        torch.cuda.synchronize()
        got = d_rep.cpu().numpy().view(P)
        i = {"rule": 5, "now": 150, "bit17": 257}[what]
        assert tuple(int(v) for v in got[i]) == (0, 0, 0, BAD), (what, got[i])
    assert code_of(b.adjust_routed_plan, d_rec.data_ptr(), (1 << 12) + 1) == ECAPACITY
    assert code_of(b.adjust_routed_plan, 0, n) == EINVAL
    assert state(b, t) == s0 and rec_set(b) == r0
    # and the same records are accepted afterwards, as the host form applies them
    want, want_rep = a.adjust(pb, d)
    got, rep = plan_commit(b, rec)
    assert got.tobytes() == want.tobytes() and rep == want_rep and rec_set(a) == rec_set(b)
    assert rep["applied"] == found
    # rl_reset closes an open plan
    b.adjust_routed_plan(d_rec.data_ptr(), n)
    b.reset()
    assert code_of(b.adjust_routed_commit, True) == ESTATE
    # the new kernels have timing slots, and Engine.kernel_times' arrays hold every slot
    assert {"k_adjust_index_routed", "k_adjust_pack", "k_adjust_index", "k_adjust_apply"} <= set(b.kernel_times())
    assert sum(b.occupancy()["live"]) == 0
    a.close()
    b.close()


# ---- worlds -----------------------------------------------------------------------------------------------
def make_oracle(local_cache):
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(RULES1)
    return o


def engines_of(G, local_cache, small=None):
    es = []
    for j in range(G):
        e = hiprl.Engine(local_cache=local_cache, max_batch_desc=256 if j == small else MAXD * G)
        e.load_rules(RULES1)
        es.append(e)
    return es


def routers_of(w):
    return [w.router] if isinstance(w, LocalWorld) else w.routers


def adjust_call(w, batches, deltas, keeps=False, want_out=True):
    """One Router.adjust of the world. -> (replies per origin or None, reports per engine or None, codes)"""
    G = w.G
    ks = [bool(keeps)] * G if isinstance(keeps, bool) else list(keeps)
    if isinstance(w, LocalWorld):
        try:
            outs, reps = w.router.adjust(batches, deltas, ks, want_out=want_out)
            return outs, reps, [None] * G
        except hiprl.RedisError as e:
            return None, None, [e.code] * G
    outs, reps, codes = [None] * G, [None] * G, [None] * G

    def worker(r):
        try:
            o, rp = w.routers[r].adjust([batches[r]], [deltas[r]], [ks[r]], want_out=want_out)
            outs[r], reps[r] = (o[0] if want_out else None), rp[0]
        except hiprl.RedisError as e:
            codes[r] = e.code
    parallel(G, worker)
    ok = all(c is None for c in codes)
    return (outs if ok else None), (reps if ok else None), codes


def raw_call(R, batches, deltas, flags):
    """rl_router_adjust itself with sentinels in every out array and report (deltas[s] None: a NULL
    delta array). -> (the code, whether out and the reports are untouched)"""
    n = len(batches)
    structs = [hiprl._batch_struct(b) for b in batches]
    for s in structs:
        s.hits_addend, s.ttl_jitter = None, None
    arr = (hiprl.RlBatch * n)(*structs)
    ds = [None if d is None else np.ascontiguousarray(d if len(d) else [0], np.int32) for d in deltas]
    da = (C.c_void_p * n)(*[None if d is None else d.ctypes.data for d in ds])
    fl = (C.c_uint32 * n)(*flags)
    outs = [np.full(max(1, b.n_desc) * 16, 0xAB, np.uint8) for b in batches]
    oa = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    reps = (hiprl.RlAdjustReport * n)()
    C.memset(C.byref(reps), 0x5A, C.sizeof(reps))
    ra = (C.c_void_p * n)(*[C.addressof(reps[i]) for i in range(n)])
    rc = R.lib.rl_router_adjust(R.h, arr, da, fl, oa, ra)
    untouched = all((o == 0xAB).all() for o in outs) and bytes(reps) == b"\x5A" * C.sizeof(reps)
    return rc, untouched


def raw_world_call(w, batches, deltas, flags):
    """-> (the code per origin, out and the reports untouched on every rank)"""
    G = w.G
    if isinstance(w, LocalWorld):
        rc, un = raw_call(w.router, batches, deltas, flags)
        return [rc] * G, un
    codes, un = [None] * G, [None] * G

    def worker(r):
        codes[r], un[r] = raw_call(w.routers[r], [batches[r]], [deltas[r]], [flags[r]])
    parallel(G, worker)
    return codes, all(un)


def adjust_checked(w, batches, deltas, keeps, local_cache, ctx):
    """One Router.adjust held against the model: out is Router.peek before, Router.peek after is the
    model's, the owners' reports sum to the model's totals, every origin's nil count is its NIL
    replies, and rl_router_stats does not move. -> (before, after, the summed report)"""
    G = w.G
    before, codes = w.ask("peek", batches)
    assert before is not None, (ctx, codes)
    st0 = [r.stats() for r in routers_of(w)]
    outs, reps, codes = adjust_call(w, batches, deltas, keeps)
    assert outs is not None, (ctx, codes)
    assert [r.stats() for r in routers_of(w)] == st0, ctx
    after, codes = w.ask("peek", batches)
    assert after is not None, (ctx, codes)
    strings = [strings_of(b, RULES1) for b in batches]
    limits = [[0 if int(r) == NIL else RULES1[int(r)][0] for r in b.rule] for b in batches]
    ks = [bool(keeps)] * G if isinstance(keeps, bool) else list(keeps)
    want, want_rep = routed_adjust_model(strings, before, deltas, limits, ks, local_cache)
    for g in range(G):
        assert np.array_equal(outs[g], before[g]), (ctx, g, "out is the state before the call")
        bad = np.nonzero(after[g] != want[g])[0]
        assert not bad.size, (ctx, g, int(bad[0]), before[g][bad[0]], after[g][bad[0]], want[g][bad[0]])
        assert int((outs[g]["flags"] & NILF != 0).sum()) == sum(s is None for s in strings[g]), (ctx, g)
    total = {f: sum(rp[f] for rp in reps) for f in REPORT_SUMS}
    assert total == {f: want_rep[f] for f in REPORT_SUMS}, (ctx, total, want_rep)
    assert sum(rp["descriptors"] for rp in reps) == want_rep["descriptors"] - want_rep["nil"], ctx
    for rp in reps:
        assert rp["nil"] == 0 and rp["descriptors"] == rp["absent"] + rp["applied"], (ctx, rp)
    return before, after, total


# ---- 4. a refund from another origin equals never having spent it ---------------------------------------
@functools.lru_cache(maxsize=None)
def parity_plan(G, local_cache):
    """(name, rule, charged h, given back r, refund time): the main keys (test_gpu_adjust's cases, on
    every unit); SECOND keys whose refund comes a second late (their window is over: dropped); keys
    given back more than they were charged (they stop at 0)."""
    main = [(f"u{u}c{c}k{k}", u, h, r, T1) for u in range(4) for c, (h, r) in enumerate(CASES) for k in range(2)]
    over = [(f"over{i}", 0, 3 + i % 5, 1 + i % 2, T1 + 1) for i in range(12)]
    floor = [(f"floor{i}", 1 + i % 3, 4, 9, T1) for i in range(8)]
    keys = main + over + floor

    def charge(who, hits):
        return [hiprl.build_batch([("adj", [[("k", nm)]], [rl], hits(k), T1)
                                   for i, k in enumerate(keys) for nm, rl in [k[:2]] if i % G == g and who(k)])
                for g in range(G)]
    charged = charge(lambda k: True, lambda k: k[2])
    # the oracle was charged h - r where the refund arrives in time, h where it does not, and never
    # saw the keys that were given everything back
    spent = charge(lambda k: k not in floor, lambda k: k[2] - k[3] if k in main else k[2])
    assert all(b.n_desc >= 4 for b in charged)
    # the refund of key i comes from the origin after the one that charged it
    refunds, deltas = [], []
    for g in range(G):
        mine = [k for i, k in enumerate(keys) if (i + 1) % G == g]
        refunds.append(key_batch([(pfx(nm), rl) for nm, rl, *_ in mine], [k[4] for k in mine]))
        deltas.append(np.array([-k[3] for k in mine], np.int64))
    # guards, from the oracle that was charged h and the one that was charged h - r
    oh, o = make_oracle(local_cache), make_oracle(local_cache)
    oh.submit(routing.concat_batches(charged))
    o.submit(routing.concat_batches(spent))

    def string(k, t):
        return oracle.cache_key(pfx(k[0]), RULES1[k[1]][1], t)
    released = sum(oh.local_cached(string(k, T1), T1) and not o.local_cached(string(k, T1), T1) for k in main)
    dropped = sum(oh.counter(string(k, k[4]), k[4]) < 0 for k in over)
    floored = sum(0 <= oh.counter(string(k, T1), T1) < k[3] for k in floor)
    assert (released >= 10 if local_cache else released == 0) and dropped >= 10 and floored >= 5
    later = []
    for j, t in enumerate([T1, T1 + 1, T1 + 2, T1 + 3, T1 + 3]):
        assert (t == M0) == (j == 2)
        later.append([hiprl.build_batch([("adj", [[("k", k[0])]], [k[1]], 1 + (i + j) % 3, t)
                                         for i, k in enumerate(keys) if (i + j) % G == g for _ in range(1 + (i + j) % 2)])
                      for g in range(G)])
    main_ask = [key_batch([(pfx(k[0]), k[1]) for i, k in enumerate(main) if i % G == g], T1) for g in range(G)]
    return charged, spent, refunds, deltas, later, main_ask, released, dropped, floored


@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("transport,G", [("local", 2), ("local", 3), ("local", 4), ("emulated", 2), ("emulated", 3)])
def test_refund_from_another_origin_equals_never_having_spent_it(transport, G, local_cache):
    charged, spent, refunds, deltas, later, main_ask, released, dropped, floored = parity_plan(G, local_cache)
    ctx = f"refund {transport} G={G} local={local_cache}"
    w = world_of(transport, engines_of(G, local_cache))
    o = make_oracle(local_cache)
    w.step(charged)
    o.submit(routing.concat_batches(spent))
    before, after, total = adjust_checked(w, refunds, deltas, False, local_cache, ctx)
    assert total["unfrozen"] == released and total["floored"] == floored and total["absent"] == dropped, (ctx, total)
    reps, codes = w.ask("peek", main_ask)
    assert reps is not None, (ctx, codes)
    for g in range(G):
        check_against_oracle(reps[g], main_ask[g], o, rules=RULES1, ctx=ctx)
    for j, row in enumerate(later):
        check_step(o, row, w.step(row), f"{ctx} later={j}")
    w.close()


# ---- 5. sums and flags across origins, the step clock ------------------------------------------------------
@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_sums_and_keep_flags_across_origins(transport):
    G = 3
    ctx = f"across {transport}"
    w = world_of(transport, engines_of(G, True))
    o = make_oracle(True)
    frozen = ["mixed_a", "mixed_b", "both_keep"]
    none = hiprl.build_batch([])
    charge = [hiprl.build_batch([("adj", [[("k", "five")]], [1], 5, T1)] +
                                [("adj", [[("k", nm)]], [2], 12, T1) for nm in frozen]),
              hiprl.build_batch([("adj", [[("k", "two")]], [3], 6, T1)]), none]
    check_step(o, charge, w.step(charge), f"{ctx} charge")
    empty = key_batch([], T1)

    def k(nm, rl):
        return (pfx(nm), rl)
    # origin 0 gives the counter of 5 -10 and origin 1 +3: 0, floored once, whichever comes first. A key
    # frozen at 12 under a limit of 10 gets -1 from either: released when one of the two comes without
    # the flag, whichever. Origin 2 asks a nil descriptor far in the future.
    for call, (mixed, d_five, keeps) in enumerate([("mixed_a", (-10, 3), [True, False, False]),
                                                   ("mixed_b", (3, -10), [False, True, True])]):
        b0 = key_batch([k("five", 1), k(mixed, 2), (pfx("nil"), NIL)], T1)
        b1 = key_batch([k("five", 1), k(mixed, 2), k("gone", 1)], T1)
        b2 = key_batch([k("two", 3), (pfx("nil"), NIL)], [T1, T1 + 1000])
        before, after, total = adjust_checked(w, [b0, b1, b2], [[d_five[0], -1, 7], [d_five[1], -1, 7], [-1, 0]], keeps,
                                              True, f"{ctx} call={call}")
        assert [int(x) for x in before[1]["count"]] == [5, 12, 0] and int(before[1]["flags"][1]) == F | LC
        assert [int(x) for x in after[0]["count"][:2]] == [0, 10] and int(after[0]["flags"][1]) == F
        assert (total["floored"], total["unfrozen"], total["absent"], total["applied"]) == (1, 1, 1, 5), (ctx, total)
        assert int(after[2]["count"][0]) == 5 - call
        w.step([hiprl.build_batch([("adj", [[("k", "five")]], [1], 5, T1)]), none, none])  # back to 5
    # every found record of the pair carries the flag: the counter moves, the key stays frozen
    bk = key_batch([k("both_keep", 2)], T1)
    before, after, total = adjust_checked(w, [bk, bk, empty], [[-1], [-1], []], [True, True, False], True,
                                          f"{ctx} both keep")
    assert int(before[0]["flags"][0]) == F | LC and (int(after[0]["count"][0]), int(after[0]["flags"][0])) == (10, F | LC)
    assert total["unfrozen"] == 0 and total["applied"] == 2
    # the step clock did not move: a step at T1 is not late after the calls that named T1 + 1000
    w.step([hiprl.build_batch([("adj", [[("k", "five")]], [1], 1, T1)]), none, none])
    w.close()


# ---- 6. refusals change nothing ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refusal_plan():
    names = [(f"r{i}", i % 4) for i in range(90)]
    charge = [hiprl.build_batch([("adj", [[("k", nm)]], [rl], 3 + i % 9, T1) for i, (nm, rl) in enumerate(names) if i % 3 == g])
              for g in range(3)]
    items = [(pfx(nm), rl) for nm, rl in names]
    return charge, items[:30], items[30:60], items[60:]


@pytest.mark.parametrize("case", ["rule", "time", "null_delta", "flag", "capacity"])
@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_origin_refusals_change_nothing(transport, case):
    charge, good0, mid, good2 = refusal_plan()
    G = 3
    ctx = f"origin refusal {transport} {case}"
    w = world_of(transport, engines_of(G, True))
    o = make_oracle(True)
    check_step(o, charge, w.step(charge), f"{ctx} charge")
    b0, b2 = key_batch(good0, T1), key_batch(good2, T1)
    bad, dbad, flag, code = key_batch(mid, T1), [-1] * len(mid), 0, EINVAL
    if case == "rule":
        rule = bad.rule.copy()
        rule[3] = 99
        bad = hiprl.Batch(bad.blob, bad.off, rule, bad.req_of, bad.now, bad.hits)
    elif case == "time":
        bad = key_batch(mid, 0xFFFD0001)
    elif case == "null_delta":
        dbad = None
    elif case == "flag":
        flag = 2
    else:
        bad, dbad, code = key_batch([mid[i % len(mid)] for i in range(MAXD + 1)], T1), [-1] * (MAXD + 1), ECAPACITY
    s0, r0 = states(w, T1), [rec_set(e) for e in w.engines]
    codes, untouched = raw_world_call(w, [b0, bad, b2], [[-1] * len(good0), dbad, [-1] * len(good2)], [0, flag, 0])
    assert codes == ([code] * 3 if transport == "local" else [EPEER, code, EPEER]), (ctx, codes)
    assert untouched, ctx
    assert states(w, T1) == s0 and [rec_set(e) for e in w.engines] == r0, ctx
    # no plan was left open anywhere, and the same call without the fault is applied
    adjust_checked(w, [b0, key_batch(mid, T1), b2], [[-1] * 30] * 3, False, True, ctx)
    w.close()


@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_owner_capacity_after_the_records_moved_applies_nothing_anywhere(transport):
    """Owner 1 can take 256 records and receives 257; owners 0 and 2 plan theirs successfully. With
    every owner committing right after its own plan they would have applied their share of a call
    that owner 1 refused: a refund nobody can retry."""
    G = 3
    ctx = f"owner capacity {transport}"
    cand = [(pfx(f"cap{i}"), 1 + i % 3) for i in range(1400)]
    own = [owner_of(it, G) for it in cand]
    mine1 = [it for it, j in zip(cand, own) if j == 1][:257]
    others = [it for it, j in zip(cand, own) if j == 0][:40] + [it for it, j in zip(cand, own) if j == 2][:40]
    assert len(mine1) == 257 and len(others) == 80
    w = world_of(transport, engines_of(G, True, small=1))
    allk = others + mine1
    # charged in two steps (owner 1 takes at most 256 records a step), from origins 0 and 2
    name = {it: f"cap{i}" for i, it in enumerate(cand)}
    for half in (allk[:160], allk[160:]):
        row = [hiprl.build_batch([("adj", [[("k", name[it])]], [it[1]], 7, T1) for it in half[g::2]]) for g in range(2)]
        w.step([row[0], hiprl.build_batch([]), row[1]])
    share = [allk[0::2], [], allk[1::2]]  # origin 1, the small engine, asks nothing
    for g in (0, 2):
        assert {owner_of(it, G) for it in share[g]} == {0, 1, 2}
    batches = [key_batch(share[g], T1) for g in range(G)]
    deltas = [[-2] * len(share[g]) for g in range(G)]
    s0, r0 = states(w, T1), [rec_set(e) for e in w.engines]
    codes, untouched = raw_world_call(w, batches, deltas, [0, 0, 0])
    assert codes == ([ECAPACITY] * 3 if transport == "local" else [EPEER, ECAPACITY, EPEER]), (ctx, codes)
    assert untouched, ctx
    # owners 0 and 2 planned successfully and have written nothing; nobody holds a plan
    assert states(w, T1) == s0 and [rec_set(e) for e in w.engines] == r0, ctx
    # the same corrections in two calls: each applied exactly once
    empty = key_batch([], T1)
    for part in (allk[:160], allk[160:]):
        sh = [part[0::2], [], part[1::2]]
        before, after, total = adjust_checked(w, [key_batch(s, T1) for s in sh], [[-2] * len(s) for s in sh], False, True, ctx)
        assert total["applied"] == len(part) and total["absent"] == 0
        for g in (0, 2):
            assert (before[g]["count"] == 7).all() and (after[g]["count"] == 5).all(), (ctx, g)
    for part in (allk[:160], allk[160:]):
        reps, codes = w.ask("peek", [key_batch(part, T1), empty, empty])
        assert reps is not None and (reps[0]["count"] == 5).all(), (ctx, codes)
    w.close()


@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_adjust_with_a_step_in_flight(transport):
    charge, good0, mid, good2 = refusal_plan()
    G = 3
    ctx = f"in flight {transport}"
    w = world_of(transport, engines_of(G, True))
    o = make_oracle(True)
    check_step(o, charge, w.step(charge), f"{ctx} charge")
    empty = key_batch([], T1)
    batches = [key_batch(good0, T1), empty, key_batch(good2, T1)]
    deltas = [[-1] * b.n_desc for b in batches]
    bf = Bufs(charge)
    bs, outs, thrs = bf.args()
    torch.cuda.synchronize()
    if transport == "local":
        w.router.submit(bs, outs, thrs)
        codes = [code_of(w.router.adjust, batches, deltas)] * G
        w.router.wait()
    else:
        codes = [None] * G

        def worker(r):
            R = w.routers[r]
            R.submit([bs[r]], [outs[r]], [thrs[r]])
            codes[r] = code_of(R.adjust, [batches[r]], [deltas[r]])
            R.wait()
        parallel(G, worker)
    assert codes == [ESTATE] * G, (ctx, codes)
    check_step(o, charge, bf.results(), f"{ctx} the step in flight")
    # and the call works afterwards
    adjust_checked(w, batches, deltas, False, True, ctx)
    w.close()


# ---- 7. one-rank RCCL communicator -----------------------------------------------------------------------
def test_rccl_one_rank_round_trip(monkeypatch):
    monkeypatch.setenv("NCCL_SOCKET_IFNAME", "lo")
    charged, spent, refunds, deltas, later, main_ask, released, dropped, floored = parity_plan(1, True)
    es = engines_of(1, True)
    r = hiprl.Router(es, max_desc=MAXD, n_shards=1, rank=0, rccl_id=hiprl.Router.unique_id())

    def step(row):
        bf = Bufs(row)
        torch.cuda.synchronize()
        r.step(*bf.args())
        return bf.results()
    o = make_oracle(True)
    step(charged)
    o.submit(routing.concat_batches(spent))
    before = r.peek(refunds)[0]
    outs, reps = r.adjust(refunds, deltas)
    assert np.array_equal(outs[0], before)
    assert (reps[0]["unfrozen"], reps[0]["absent"], reps[0]["floored"]) == (released, dropped, floored)
    assert reps[0]["descriptors"] == refunds[0].n_desc == reps[0]["absent"] + reps[0]["applied"]
    check_against_oracle(r.peek(main_ask)[0], main_ask[0], o, rules=RULES1, ctx="rccl")
    for j, row in enumerate(later):
        check_step(o, row, step(row), f"rccl later={j}")
    r.close()
