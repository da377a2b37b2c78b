"""Routed refund (rl_hip.h "Routed refund") on the GPU.

Origin: rl_refund_route_owed makes refund_amounts' amounts and the rule ids that keep every unowed
descriptor at home, and the two packs behind it write the owed records and nothing else. Engine
level: the origin pass, the packs and rl_refund_routed_plan + rl_refund_routed_commit leave an engine
exactly where rl_refund_pipelined (pinned to the model by test_gpu_refund.py) leaves its twin. Router
level, local transport, emulated collectives and a one-rank RCCL communicator: a world whose steps
alternate with a Router.refund of the step's own statuses decides and peeks as RoutedRefundOracle
(routed_refund_model.py); a call refused at one origin or at one owner (after the records moved)
leaves every engine untouched. Every plan (keys, owners, guards) is made on the CPU from the oracle
and the models alone.
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
import streams
from refund_model import RefundOracle, refund_amounts
from routed_refund_model import OWNER_FIELDS, RoutedRefundOracle
from streams import RULES
from test_gpu_emulated_router import parallel
from test_gpu_refund import model_peeks
from test_gpu_routed_adjust import adjust_call, routers_of
from test_gpu_routed_peek import DEV, MAXD, NIL, SEED, LocalWorld, engine_plan, key_batch, owner_of, unseen_keys
from test_gpu_routed_peek import make_oracle as stream_oracle
from test_gpu_routed_set import code_of, states, to_dev, world_of
from test_gpu_set import rec_set, state

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE, EPEER = -1, -4, -5, -7
F, LC, NILF, PS, BAD = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND, hiprl.PEEK_BAD
P = hiprl.PEEK_DTYPE
KEEP_BIT = 1 << 16  # a record's rule word: RL_REFUND_KEEP_CACHE
OK, OVER, LCHIT, SHADOW, HASLIM = 1, 2, 2 << 8, 4 << 8, 1 << 8
T0 = 1_700_000_000
SIZES = (1, 63, 64, 65, 255, 256, 257, 3001)


# ---- batches and statuses made by hand ---------------------------------------------------------------
def req_batch(items, sizes, now, hits):
    """[(prefix, rule)] cut into requests of the given sizes, request q at now (or now[q]) with hits[q]."""
    kb = key_batch(items, 0)
    assert sum(sizes) == len(items)
    req_of = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    t = np.full(len(sizes), now, np.int64) if np.ndim(now) == 0 else np.array(now, np.int64)
    return hiprl.Batch(kb.blob, kb.off, kb.rule, req_of, t, np.array(hits, np.uint32))


def statuses(codes):
    st = np.zeros(len(codes), hiprl.STATUS_DTYPE)
    st["code_flags"] = codes
    return st


def model_amounts(hb, st):
    am, n_rej = refund_amounts(st["code_flags"], hb.rule, hb.req_of, hb.hits, hb.n_req)
    return np.array(am, np.uint64), n_rej


@functools.lru_cache(maxsize=None)
def random_case(n, seed=3):
    """n descriptors in requests of 1-4 with every kind of status: not over, over, a local-cache hit,
    a shadowed over-limit, a nil rule; hits_addend of every edge. Guard: a third owed, a third not."""
    rng = np.random.default_rng(seed + n)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 5)), n - sum(sizes)))
    items = [(p, NIL if rng.random() < 0.12 else r) for p, r in unseen_keys(n, f"own{n}")]
    codes = []
    for _, r in items:
        x = rng.random()
        codes.append(OK if r == NIL else OVER | HASLIM if x < 0.3 else OVER | LCHIT | HASLIM if x < 0.42
                     else OK | SHADOW | HASLIM if x < 0.5 else OK | HASLIM)
    edge = [0, 1, 2**31, 2**32 - 1]
    hits = [edge[q % 4] if q % 3 == 0 else int(rng.integers(2, 5000)) for q in range(len(sizes))]
    hb = req_batch(items, sizes, T0 + 3, hits)
    st = statuses(codes)
    am, _ = model_amounts(hb, st)
    owed = int((am != 0).sum())
    assert n == 1 or (owed >= n // 3 and n - owed >= n // 3), (n, owed)
    assert n < 255 or {int(x) for x in am} >= {1, 2**31, 2**32 - 1}  # (1: hits_addend of 0 and of 1)
    return hb, st


def edge_case():
    """3001 descriptors. Request 0 ends at lane 63 and is rejected by its last descriptor; the next
    ends at 253 and is not; 254..258 has its only over-limit descriptor at 258, in the block after its
    first two; 259..2799 are requests of one, every fifth rejected; 2800..3000 is rejected by 3000 alone,
    a block after its first descriptors."""
    sizes = [64, 190, 5] + [1] * 2541 + [201]
    n = sum(sizes)
    assert n == 3001
    codes = np.full(n, OK | HASLIM, np.uint32)
    codes[[63, 258, 3000]] = OVER | HASLIM
    codes[259:2800:5] = OVER | HASLIM
    items = unseen_keys(n, "edge")
    hb = req_batch(items, sizes, T0 + 3, [7 + q % 5 for q in range(len(sizes))])
    am, n_rej = model_amounts(hb, statuses(codes))
    assert am[:64].all() and not am[64:254].any() and am[254:259].all() and am[2800:].all() and n_rej == 3 + 509
    return hb, statuses(codes)


def boundary_case():
    """Request boundaries at lanes 63/64 and 255/256 with the rejected request on either side: the
    mark of one request does not leak into its neighbour."""
    sizes = [64, 64, 128, 1, 63]  # 0..63 | 64..127 | 128..255 | 256 | 257..319
    n = sum(sizes)
    codes = np.full(n, OK | HASLIM, np.uint32)
    codes[[64, 255]] = OVER | HASLIM  # the first descriptor of request 1, the last of request 2
    hb = req_batch(unseen_keys(n, "bnd"), sizes, T0 + 3, [3, 4, 5, 6, 7])
    am, n_rej = model_amounts(hb, statuses(codes))
    assert not am[:64].any() and (am[64:128] == 4).all() and (am[128:256] == 5).all() and not am[256:].any() and n_rej == 2
    return hb, statuses(codes)


def nothing_rejected_case():
    n = 300
    codes = [OK | SHADOW | HASLIM if i % 7 == 0 else OK | HASLIM for i in range(n)]
    hb = req_batch(unseen_keys(n, "none"), [3] * 100, T0 + 3, [9] * 100)
    return hb, statuses(codes)


def origin_pass(e, hb, st, G, alias, keep):
    """rl_refund_route_owed, the plain pack with the rewritten rules, the amount and keep pack.
    -> (amounts, rule_out, counts, perm, x, the send buffer's bytes, stride)"""
    n = hb.n_desc
    db = pyrouter.DeviceBatch.from_host(hb, DEV)
    d_st = to_dev(st)
    stride = n + 5
    send = torch.full((G * stride * 32 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    x = torch.zeros(2 * G, dtype=torch.int32, device=DEV)
    perm = torch.zeros(n, dtype=torch.int32, device=DEV)
    amt = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cnt = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    rule_out = db.rule if alias else torch.full((n,), 7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    e.refund_route_owed(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), d_st.data_ptr(), rule_out.data_ptr(),
                        amt.data_ptr(), cnt.data_ptr())
    ptrs = db.ptrs()
    ptrs[2] = rule_out.data_ptr()
    e.route_pack_strided(db.n_desc, db.n_req, db.blob_bytes(), ptrs, min(1, G - 1), G, stride, send.data_ptr(), x.data_ptr(),
                         perm.data_ptr())
    e.route_pack_adjust(n, rule_out.data_ptr(), perm.data_ptr(), amt.data_ptr(), send.data_ptr(), keep_cache=keep)
    torch.cuda.synchronize()
    if not alias:
        assert np.array_equal(db.rule.cpu().numpy().view(np.uint32), hb.rule), "the batch's own rules are only read"
    return (amt.cpu().numpy().view(np.uint32), rule_out.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32),
            perm.cpu().numpy().view(np.uint32), x.cpu().numpy(), send.cpu().numpy(), stride)


def expected_records(hb, am, keep):
    """What the two packs write for the owed descriptors of hb, in descriptor order."""
    rec = np.zeros(hb.n_desc, routing.REC_DTYPE)
    for i in np.flatnonzero(am):
        a, b = oracle.prefix_lanes(hb.prefix(i), SEED)
        rec[i] = (a, b, int(hb.now[hb.req_of[i]]), int(hb.rule[i]) | (KEEP_BIT if keep else 0), int(am[i]), 0)
    return rec


def check_origin_pass(e, hb, st, G, alias, keep, ctx):
    am, n_rej = model_amounts(hb, st)
    owed = am != 0
    got_am, rule_out, cnt, perm, x, send, stride = origin_pass(e, hb, st, G, alias, keep)
    assert np.array_equal(got_am.astype(np.uint64), am), (ctx, np.flatnonzero(got_am != am)[:5])
    assert np.array_equal(rule_out, np.where(owed, hb.rule, NIL)), ctx
    assert cnt.tolist() == [n_rej, int(owed.sum())], (ctx, cnt)
    # no record for an unowed descriptor; the owed ones grouped by owner, in descriptor order
    assert np.array_equal(perm == hiprl.ROUTE_LOCAL, ~owed), ctx
    assert not x[1::2].any() and int(x[0::2].sum()) == int(owed.sum()), (ctx, x)
    want = np.full(send.shape, 0xA5, np.uint8)
    wrec = want[:G * stride * 32].view(routing.REC_DTYPE)
    grec = send[:G * stride * 32].view(routing.REC_DTYPE)
    exp = expected_records(hb, am, keep)
    nxt = [j * stride for j in range(G)]
    for i in np.flatnonzero(owed):
        j = owner_of((hb.prefix(i), 0), G)
        assert int(perm[i]) == nxt[j], (ctx, i, j)
        nxt[j] += 1
        wrec[perm[i]] = exp[i]
        wrec[perm[i]]["greq"] = grec[perm[i]]["greq"]  # (the plain pack's word; an owner's refund reads none of it)
    assert [nxt[j] - j * stride for j in range(G)] == x[0::2].tolist(), ctx
    # every byte of the send buffer outside the owed records is untouched
    assert send.tobytes() == want.tobytes(), (ctx, np.flatnonzero(send != want)[:8])
    return grec, perm


# ---- 1. the origin pass ------------------------------------------------------------------------------------
@pytest.mark.parametrize("alias", [False, True])
def test_origin_pass_amounts_rules_counts_and_records(alias):
    e = hiprl.Engine(max_batch_desc=1 << 12)
    e.load_rules(RULES)
    for n in SIZES:
        hb, st = random_case(n)
        check_origin_pass(e, hb, st, 3, alias, n % 2 == 0, f"n={n} alias={alias}")
    for name, (hb, st) in (("edge", edge_case()), ("boundary", boundary_case())):
        check_origin_pass(e, hb, st, 3, alias, False, f"{name} alias={alias}")
    # nothing rejected: all zeros, every rule nil, and the pack sends no record
    hb, st = nothing_rejected_case()
    got_am, rule_out, cnt, perm, x, send, stride = origin_pass(e, hb, st, 3, alias, False)
    assert not got_am.any() and (rule_out == NIL).all() and cnt.tolist() == [0, 0]
    assert (perm == hiprl.ROUTE_LOCAL).all() and not x.any() and (send == 0xA5).all()
    assert {"k_refund_mark", "k_refund_owed"} <= set(e.kernel_times())
    e.close()


def test_origin_pass_refusals_launch_nothing():
    e = hiprl.Engine(max_batch_desc=256, max_batch_req=128)
    e.load_rules(RULES)
    hb, st = random_case(64)
    db = pyrouter.DeviceBatch.from_host(hb, DEV)
    d_st = to_dev(st)
    out = torch.full((64 * 2 + 2,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ro, am, cn = out.data_ptr(), out.data_ptr() + 256, out.data_ptr() + 512
    torch.cuda.synchronize()

    def call(n_desc=hb.n_desc, n_req=hb.n_req, ptrs=None, st_ptr=d_st.data_ptr(), ro=ro, am=am, cn=cn):
        return code_of(e.refund_route_owed, n_desc, n_req, db.blob_bytes(), ptrs or db.ptrs(), st_ptr, ro, am, cn)
    for k in (2, 3, 5):  # rule_id, req_of, hits_addend
        ptrs = db.ptrs()
        ptrs[k] = 0
        assert call(ptrs=ptrs) == EINVAL, k
    assert call(st_ptr=0) == EINVAL and call(ro=0) == EINVAL and call(am=0) == EINVAL and call(cn=0) == EINVAL
    assert call(n_desc=257) == ECAPACITY and call(n_req=129) == ECAPACITY
    e.refund_routed_plan(0, 0)
    assert call() == ESTATE  # a plan is open: the scratch is shared
    e.refund_routed_commit(False)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A5A5A).all(), "a refused call launches nothing"
    # n_desc == 0 writes zeros to the counts and nothing else
    assert call(n_desc=0, n_req=0) is None
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[128:130].tolist() == [0, 0] and (got[:128] == 0x5A5A5A5A).all()
    assert call() is None
    e.close()


# ---- 2. the record form equals the flight form --------------------------------------------------------------
def twin_engines(local_cache, split):
    batches, t, pool = engine_plan(local_cache, split)
    es = [hiprl.Engine(local_cache=local_cache, per_second_split=split, max_batch_desc=1 << 12, pipeline="v4")
          for _ in range(2)]
    for e in es:
        e.load_rules(RULES)
        for bt in batches:
            e.submit(bt)
    return es, batches, t, pool


def pool_state(local_cache, split):
    batches, t, pool = engine_plan(local_cache, split)
    o = stream_oracle(local_cache, per_second_split=split)
    for b in batches:
        o.submit(b)
    rows = []
    for it in pool:
        k = oracle.cache_key(it[0], RULES[it[1]][1], t)
        rows.append((o.counter(k, t, per_second=split and RULES[it[1]][1] == hiprl.SECOND), o.local_cached(k, t)))
    return rows


def flight_form(e, hb, st, keep):
    db = pyrouter.DeviceBatch.from_host(hb, DEV)
    d_st = to_dev(st)
    amt = torch.full((hb.n_desc,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    e.refund_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), d_st.data_ptr(), keep, amt.data_ptr())
    rep = e.wait_refund()
    torch.cuda.synchronize()
    return amt.cpu().numpy().view(np.uint32), rep


def record_form(e, hb, st, keep, ctx):
    """The origin pass and the packs to one owner, the records checked on the host, plan + commit."""
    grec, perm = check_origin_pass(e, hb, st, 1, True, keep, ctx)
    am, _ = model_amounts(hb, st)
    n = int((am != 0).sum())
    rec = grec[:n].copy()
    d_rec = to_dev(rec) if n else None
    d_rep = torch.full((max(1, n) * 16,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    e.refund_routed_plan(d_rec.data_ptr() if n else 0, n, d_rep.data_ptr())
    rep = e.refund_routed_commit(True)
    torch.cuda.synchronize()
    return d_rep.cpu().numpy().view(P)[:n].copy(), rep


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("local_cache", [False, True])
def test_record_form_equals_flight_form(local_cache, split):
    (a, b), _, t, pool = twin_engines(local_cache, split)
    ps = pool_state(local_cache, split)
    assert rec_set(a) == rec_set(b)
    rng = np.random.default_rng(17)
    # the guards come from the model over the same history and the same calls
    m = RefundOracle(RULES, local_cache=local_cache, per_second_split=split)
    for bt in engine_plan(local_cache, split)[0]:
        m.submit(bt)
    found_strings, floored, unfrozen = set(), 0, 0
    # the key of the one-key call: found, and frozen when the cache is on
    hot = next(i for i, (c, lc) in enumerate(ps) if c > 0 and (lc or not local_cache))
    for keep in (False, True):
        for n in SIZES + ("hot",):
            if n == "hot":  # 257 records of one pair: five waves, two blocks, a sum over 2^32
                n = 257
                items, sizes, hits = [pool[hot]] * n, [1] * n, [1 << 24] * n
                codes = [OVER | HASLIM] * n
                assert sum(hits) > 2**32
            else:
                items = [pool[(7 * n + i) % len(pool)] for i in range(n)]
                if n > 1:  # duplicates in one wave, in another wave and (3001 > the pool) in other blocks
                    items[n - 1] = items[0]
                    items[n // 2] = items[0]
                sizes = []
                while sum(sizes) < n:
                    sizes.append(min(int(rng.integers(1, 4)), n - sum(sizes)))
                hits = [int(rng.integers(0, 4)) for _ in sizes]
                if len(sizes) > 3:
                    hits[1], hits[3] = 2**31, 2**32 - 1
                codes = [OVER | HASLIM if x < 0.35 else OVER | LCHIT | HASLIM if x < 0.45 else OK | HASLIM
                         for x in rng.random(n)]
                if n == 1:
                    codes = [OVER | HASLIM]
            hb, st = req_batch(items, sizes, t, hits), statuses(codes)
            ctx = f"n={n} keep={keep} local={local_cache} split={split}"
            am, n_rej = model_amounts(hb, st)
            assert n == 1 or (am != 0).sum() >= n // 3, ctx
            found_strings |= {m._key(hb, i) for i in np.flatnonzero(am)
                              if m.peek(*m._key(hb, i), int(hb.now[hb.req_of[i]]))[3] & F}
            _, model = m.refund(hb, st, keep)
            floored += model["floored"]
            unfrozen += model["unfrozen"]
            want_am, want = flight_form(a, hb, st, keep)
            assert want == model, (ctx, want, model)
            got_rep, rep = record_form(b, hb, st, keep, ctx)
            assert np.array_equal(want_am.astype(np.uint64), am), ctx
            assert {f: rep[f] for f in OWNER_FIELDS} == {f: want[f] for f in OWNER_FIELDS}, (ctx, rep, want)
            assert rep["descriptors"] == rep["absent"] + rep["refunded"] == int((am != 0).sum()), (ctx, rep)
            assert (rep["rejected_req"], rep["skipped"]) == (0, 0) and want["rejected_req"] == n_rej, ctx
            assert rec_set(a) == rec_set(b), ctx
            assert a.occupancy() == b.occupancy() and a.stats() == b.stats(), ctx
            pk = key_batch(items, t)
            assert np.array_equal(a.peek(pk), b.peek(pk)), ctx
            assert not keep or rep["unfrozen"] == 0, ctx
    assert len(found_strings) >= 30 and floored >= 1 and (unfrozen >= 1 or not local_cache), (len(found_strings), floored, unfrozen)
    a.close()
    b.close()


# ---- 3. the plan's lifecycle, malformed records -------------------------------------------------------------
def refund_records(pb, amounts, keep=False):
    rec = np.zeros(pb.n_desc, routing.REC_DTYPE)
    for i in range(pb.n_desc):
        a, b = oracle.prefix_lanes(pb.prefix(i), SEED)
        rec[i] = (a, b, int(pb.now[pb.req_of[i]]), int(pb.rule[i]) | (KEEP_BIT if keep else 0), int(amounts[i]), 0)
    return rec


def test_plan_lifecycle_and_malformed_records():
    (a, b), batches, t, pool = twin_engines(True, False)
    n = 300
    items = unseen_keys(100, "life") + pool[:200]
    pb = key_batch(items, t)
    amounts = [1 + i % 5 for i in range(n)]
    rec = refund_records(pb, amounts)
    found = int((b.peek(pb)["flags"] & F != 0).sum())
    assert found >= 50 and n - found >= 100
    s0, r0 = state(b, t), rec_set(b)
    d_rec = to_dev(rec)
    d_val = to_dev(np.zeros(n, P))
    zero = dict.fromkeys(hiprl.REFUND_REPORT_FIELDS, 0)
    torch.cuda.synchronize()
    assert code_of(b.refund_routed_commit, True) == ESTATE  # no plan open
    b.refund_routed_plan(d_rec.data_ptr(), n)
    # with a plan open: submit, peek, adjust, the other plans, a second plan, the other kinds' commits
    assert code_of(b.submit, batches[-1]) == ESTATE
    assert code_of(b.peek, pb) == ESTATE
    assert code_of(b.adjust, pb, [-1] * n) == ESTATE
    assert code_of(b.set_routed_plan, d_rec.data_ptr(), d_val.data_ptr(), n) == ESTATE
    assert code_of(b.adjust_routed_plan, d_rec.data_ptr(), n) == ESTATE
    assert code_of(b.refund_routed_plan, d_rec.data_ptr(), n) == ESTATE
    for apply in (True, False):
        assert code_of(b.set_routed_commit, apply) == ESTATE
        assert code_of(b.adjust_routed_commit, apply) == ESTATE
    # ... which left it open; commit(0) drops it: census, occupancy, stats and the table word for word
    assert b.refund_routed_commit(False) == zero
    assert code_of(b.refund_routed_commit, False) == ESTATE
    assert state(b, t) == s0 and rec_set(b) == r0
    # the reverse: a refund commit on a set plan and on an adjust plan, which stay open
    b.set_routed_plan(0, 0, 0)
    assert code_of(b.refund_routed_commit, True) == ESTATE
    assert code_of(b.refund_routed_plan, d_rec.data_ptr(), n) == ESTATE
    b.set_routed_commit(True)
    b.adjust_routed_plan(0, 0)
    assert code_of(b.refund_routed_commit, True) == ESTATE
    b.adjust_routed_commit(True)
    # an empty plan opens and commits
    b.refund_routed_plan(0, 0)
    assert b.refund_routed_commit(True) == zero
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
        assert code_of(b.refund_routed_plan, d_rec2.data_ptr(), n, d_rep.data_ptr()) == EINVAL, what
        assert code_of(b.refund_routed_commit, True) == ESTATE  # the refused plan is not open
        assert state(b, t) == s0 and rec_set(b) == r0, what
        torch.cuda.synchronize()
        got = d_rep.cpu().numpy().view(P)
        i = {"rule": 5, "now": 150, "bit17": 257}[what]
        assert tuple(int(v) for v in got[i]) == (0, 0, 0, BAD), (what, got[i])
    assert code_of(b.refund_routed_plan, d_rec.data_ptr(), (1 << 12) + 1) == ECAPACITY
    assert code_of(b.refund_routed_plan, 0, n) == EINVAL
    assert state(b, t) == s0 and rec_set(b) == r0
    # and the same records are accepted afterwards, as the adjust of the negated amounts applies them
    want, want_rep = a.adjust(pb, [-x for x in amounts])
    d_rep = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    b.refund_routed_plan(d_rec.data_ptr(), n, d_rep.data_ptr())
    rep = b.refund_routed_commit(True)
    torch.cuda.synchronize()
    assert d_rep.cpu().numpy().view(P).tobytes() == want.tobytes() and rec_set(a) == rec_set(b)
    assert rep == dict(zero, descriptors=n, absent=want_rep["absent"], refunded=found, floored=want_rep["floored"],
                       unfrozen=want_rep["unfrozen"])
    # rl_reset closes an open plan
    b.refund_routed_plan(d_rec.data_ptr(), n)
    b.reset()
    assert code_of(b.refund_routed_commit, True) == ESTATE
    # the new kernels have timing slots
    assert {"k_refund_index_routed", "k_refund_owed", "k_adjust_apply"} <= set(b.kernel_times())
    assert sum(b.occupancy()["live"]) == 0
    a.close()
    b.close()


# ---- worlds ---------------------------------------------------------------------------------------------------
S_, M_, H_, D_ = hiprl.SECOND, hiprl.MINUTE, hiprl.HOUR, hiprl.DAY
# a cost limiter: 10^4 units a window, requests of up to a few thousand; rule 4 is the hand cases'
# "global" descriptor, over its limit from the second request on
WRULES = [(10**4, S_), (10**4, M_), (10**4, H_), (10**4, D_), (1, D_), (10, M_)]


def world_engines(G, local_cache, small=None):
    es = []
    for j in range(G):
        e = hiprl.Engine(local_cache=local_cache, max_batch_desc=256 if j == small else MAXD * G)
        e.load_rules(WRULES)
        es.append(e)
    return es


def wreq(keys, rules, hits, t=T0):
    return ("cost", [[("k", str(k))] for k in keys], rules, hits, t)


def item_of(b, i):
    return (b.prefix(i), int(b.rule[i]))


def refund_call(w, batches, sts, keeps=False, want_out=True):
    """One Router.refund of the world. -> (amounts, outs, reports per origin or None, the codes)"""
    G = w.G
    ks = [bool(keeps)] * G if isinstance(keeps, bool) else list(keeps)
    if isinstance(w, LocalWorld):
        try:
            return (*w.router.refund(batches, sts, ks, want_out=want_out), [None] * G)
        except hiprl.RedisError as e:
            print("Router.refund:", e)
            return None, None, None, [e.code] * G
    am, outs, reps, codes = [None] * G, [None] * G, [None] * G, [None] * G

    def worker(r):
        try:
            a, o, rp = w.routers[r].refund([batches[r]], [sts[r]], [ks[r]], want_out=want_out)
            am[r], outs[r], reps[r] = a[0], (o[0] if want_out else None), rp[0]
        except hiprl.RedisError as e:
            print(f"Router.refund rank {r}:", e)
            codes[r] = e.code
    parallel(G, worker)
    if any(c is not None for c in codes):
        return None, None, None, codes
    return am, outs, reps, codes


def model_step(m, row, got, ctx):
    """The world's step against the model's. -> the statuses per origin"""
    est, ethr = m.submit(routing.concat_batches(row))
    d0 = r0 = 0
    for g, (b, (st, thr)) in enumerate(zip(row, got)):
        streams.assert_same(est[d0:d0 + b.n_desc], ethr[r0:r0 + b.n_req], st, thr, f"{ctx} origin={g}")
        d0 += b.n_desc
        r0 += b.n_req
    return [st for st, _ in got]


def refund_checked(w, m, row, sts, keeps, ctx):
    """One Router.refund held against the model. -> (the model's amounts, origin fields, owner totals)"""
    G = w.G
    st0 = [r.stats() for r in routers_of(w)]
    am, outs, reps, codes = refund_call(w, row, sts, keeps)
    assert am is not None, (ctx, codes)
    assert [r.stats() for r in routers_of(w)] == st0, ctx
    want_am, want_outs, origin, owner = m.refund_routed(row, sts, keeps)
    for g in range(G):
        assert [int(x) for x in am[g]] == want_am[g], (ctx, g)
        bad = np.nonzero(outs[g] != want_outs[g])[0]
        assert not bad.size, (ctx, g, int(bad[0]), outs[g][bad[0]], want_outs[g][bad[0]])
        assert {f: reps[g][f] for f in origin[g]} == origin[g], (ctx, g, reps[g], origin[g])
    assert {f: sum(rp[f] for rp in reps) for f in OWNER_FIELDS} == owner, (ctx, reps, owner)
    # the world identity that replaces the lone engine's per-report one
    assert sum(rp["descriptors"] - rp["skipped"] for rp in reps) == sum(rp["absent"] + rp["refunded"] for rp in reps), ctx
    return want_am, origin, owner


def peeks_checked(w, m, row, ctx):
    reps, codes = w.ask("peek", row)
    assert reps is not None, (ctx, codes)
    for g, b in enumerate(row):
        want = model_peeks(m, b)
        bad = np.nonzero(reps[g] != want)[0]
        assert not bad.size, (ctx, g, int(bad[0]), reps[g][bad[0]], want[bad[0]])


# ---- 4. world parity ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parity_plan(G, local_cache):
    """Three steps of a cost-limiter stream, one second apart, a refund of its own statuses behind
    each; between the second step and its refund one owed key is set down to 1, so that its refund
    stops at 0. Guards from the model alone."""
    rng = np.random.default_rng(100 + G)
    rows = []
    for s in range(3):
        row = []
        for g in range(G):
            reqs = []
            for _ in range(240 // G):
                nd = int(rng.integers(1, 4))
                rules = [int(rng.choice([0, 1, 2, 3, NIL], p=[.2, .3, .2, .2, .1])) for _ in range(nd)]
                reqs.append(wreq([int(60 * rng.random() ** 2.5) for _ in range(nd)], rules, int(rng.integers(0, 3000)), T0 + s))
            row.append(hiprl.build_batch(reqs))
        rows.append(row)
    m = RoutedRefundOracle(WRULES, local_cache=local_cache)
    floor_key, unfrozen, floored = None, 0, 0
    for s, row in enumerate(rows):
        est, _ = m.submit(routing.concat_batches(row))
        cuts = np.cumsum([0] + [b.n_desc for b in row])
        sts = [est[cuts[g]:cuts[g + 1]] for g in range(G)]
        ams = [refund_amounts(st["code_flags"], b.rule, b.req_of, b.hits, b.n_req) for b, st in zip(row, sts)]
        owed = [[i for i in range(b.n_desc) if am[i]] for b, (am, _) in zip(row, ams)]
        assert sum(n_rej for _, n_rej in ams) >= 10, (s, "rejected requests")
        assert sum(owner_of(item_of(b, i), G) != g for g, b in enumerate(row) for i in owed[g]) >= 10 or G == 1, s
        by_key = {}
        for g, b in enumerate(row):
            for i in owed[g]:
                by_key.setdefault(m._key(b, i), set()).add(g)
        assert sum(len(v) >= 2 for v in by_key.values()) >= 3 or G == 1, (s, "keys owed from two origins")
        if s == 1:  # a minute key owed in this call, found, with more than 1 on it
            floor_key = next((b.prefix(i), int(b.rule[i])) for g, b in enumerate(row) for i in owed[g]
                             if int(b.rule[i]) == 1 and m.peek(*m._key(b, i), T0 + s)[0] > 1)
            key = floor_key[0] + str((T0 + s) // 60 * 60).encode()
            floor_delta = 1 - m.redis[0][key][0]
            m.redis[0][key][0] = 1
        _, _, _, owner = m.refund_routed(row, sts)
        unfrozen += owner["unfrozen"]
        floored += owner["floored"]
    assert floored >= 1 and (unfrozen >= 5 if local_cache else unfrozen == 0), (floored, unfrozen)
    return rows, floor_key, floor_delta


def run_parity(w, G, local_cache, ctx):
    rows, floor_key, floor_delta = parity_plan(G, local_cache)
    m = RoutedRefundOracle(WRULES, local_cache=local_cache)
    empty = key_batch([], T0)
    for s, row in enumerate(rows):
        sts = model_step(m, row, w.step(row), f"{ctx} step={s}")
        if s == 1:
            kb = key_batch([floor_key], T0 + s)
            outs, reps, codes = adjust_call(w, [kb] + [empty] * (G - 1), [[floor_delta]] + [[]] * (G - 1), True)
            assert outs is not None, (ctx, codes)
            key = floor_key[0] + str((T0 + s) // 60 * 60).encode()
            assert int(outs[0]["count"][0]) == m.redis[0][key][0] and m.redis[0][key][0] + floor_delta == 1
            m.redis[0][key][0] = 1
        refund_checked(w, m, row, sts, False, f"{ctx} refund={s}")
        peeks_checked(w, m, row, f"{ctx} peeks={s}")
    # the step clock did not move past the steps' own times: a step at the last step's time is not late
    last = [hiprl.build_batch([wreq(["late"], [1], 1, T0 + 2)])] + [hiprl.build_batch([])] * (G - 1)
    model_step(m, last, w.step(last), f"{ctx} not late")


@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("transport,G", [("local", 2), ("local", 3), ("local", 4), ("emulated", 2), ("emulated", 3)])
def test_world_with_refunds_equals_the_refund_oracle(transport, G, local_cache):
    w = world_of(transport, world_engines(G, local_cache))
    run_parity(w, G, local_cache, f"parity {transport} G={G} local={local_cache}")
    w.close()


def test_rccl_one_rank_round_trip(monkeypatch):
    monkeypatch.setenv("NCCL_SOCKET_IFNAME", "lo")
    es = world_engines(1, True)

    class W(LocalWorld):
        def __init__(self):
            self.G, self.engines = 1, es
            self.router = hiprl.Router(es, max_desc=MAXD, n_shards=1, rank=0, rccl_id=hiprl.Router.unique_id())
    w = W()
    run_parity(w, 1, True, "rccl")
    w.close()


# ---- 5. sums and keep flags across origins -------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_sums_and_keep_flags_across_origins(transport):
    G = 3
    ctx = f"across {transport}"
    w = world_of(transport, world_engines(G, True))
    m = RoutedRefundOracle(WRULES, local_cache=True)
    none = hiprl.build_batch([])
    # (a "global" key of rule 4, 1 a day, rejects the request that asks 6 of it)
    # a counter of 9 owed 6 by origin 0 and 6 by origin 1: charged 6 + 6, given -3 in between
    row = [hiprl.build_batch([wreq(["nine", "g0"], [1, 4], 6)]), hiprl.build_batch([wreq(["nine", "g1"], [1, 4], 6)]), none]
    sts = model_step(m, row, w.step(row), f"{ctx} nine")
    kb = key_batch([item_of(row[0], 0)], T0)
    outs, _, codes = adjust_call(w, [none, none, kb], [[], [], [-3]], True)
    assert outs is not None and int(outs[2]["count"][0]) == 12, (ctx, codes)
    m.redis[0][m._key(row[0], 0)[0]][0] = 9
    am, origin, owner = refund_checked(w, m, row, sts, False, f"{ctx} nine")
    assert am == [[6, 6], [6, 6], []] and owner["floored"] == 1 and owner["refunded"] == 4
    peeks_checked(w, m, row, f"{ctx} nine")
    assert m.redis[0][m._key(row[0], 0)[0]][0] == 0
    # a key frozen at 12 / 10, owed 6 by origins 0 and 2: released when either record comes without the
    # keep bit, frozen still when both carry it (the refund is applied all the same)
    for name, keeps, released in (("fa", [True, False, False], True), ("fb", [False, False, True], True),
                                  ("fc", [True, False, True], False)):
        row = [hiprl.build_batch([wreq([name, f"g0{name}"], [5, 4], 6)]), none,
               hiprl.build_batch([wreq([name, f"g2{name}"], [5, 4], 6)])]
        sts = model_step(m, row, w.step(row), f"{ctx} {name}")
        key = m._key(row[0], 0)[0]
        assert m.redis[0][key][0] == 12 and key in m.lcache
        am, origin, owner = refund_checked(w, m, row, sts, keeps, f"{ctx} {name}")
        assert am == [[6, 6], [], [6, 6]] and m.redis[0][key][0] == 0 and (key not in m.lcache) == released, (ctx, name)
        peeks_checked(w, m, row, f"{ctx} {name}")
    w.close()


# ---- 6. refusals change nothing --------------------------------------------------------------------------------
def raw_call(R, batches, sts, flags, null_hits=()):
    """rl_router_refund itself with sentinels in every amount array, out array and report (sts[s] None:
    a NULL status array; s in null_hits: a NULL hits_addend). -> (the code, every output untouched)"""
    n = len(batches)
    structs = [hiprl._batch_struct(b) for b in batches]
    for s, x in enumerate(structs):
        x.ttl_jitter = None
        if s in null_hits:
            x.hits_addend = None
    arr = (hiprl.RlBatch * n)(*structs)
    ss = [None if st is None else np.ascontiguousarray(st if len(st) else np.zeros(1, hiprl.STATUS_DTYPE)) for st in sts]
    sa = (C.c_void_p * n)(*[None if st is None else st.ctypes.data for st in ss])
    fl = (C.c_uint32 * n)(*flags)
    ams = [np.full(max(1, b.n_desc) * 4, 0xAB, np.uint8) for b in batches]
    aa = (C.c_void_p * n)(*[a.ctypes.data for a in ams])
    outs = [np.full(max(1, b.n_desc) * 16, 0xAB, np.uint8) for b in batches]
    oa = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    reps = (hiprl.RlRefundReport * n)()
    C.memset(C.byref(reps), 0x5A, C.sizeof(reps))
    ra = (C.c_void_p * n)(*[C.addressof(reps[i]) for i in range(n)])
    rc = R.lib.rl_router_refund(R.h, arr, sa, fl, aa, oa, ra)
    untouched = (all((o == 0xAB).all() for o in outs + ams) and bytes(reps) == b"\x5A" * C.sizeof(reps))
    return rc, untouched


def raw_world_call(w, batches, sts, flags, null_hits=()):
    G = w.G
    if isinstance(w, LocalWorld):
        rc, un = raw_call(w.router, batches, sts, flags, null_hits)
        return [rc] * G, un
    codes, un = [None] * G, [None] * G

    def worker(r):
        codes[r], un[r] = raw_call(w.routers[r], [batches[r]], [sts[r]], [flags[r]], (0,) if r in null_hits else ())
    parallel(G, worker)
    return codes, all(un)


def charged_world(transport, ctx, small=None):
    """Three origins, 30 keys each charged in a step; every request is rejected by a "global" key of
    its own (rule 4: 1 a day), so every descriptor of the step is owed."""
    G = 3
    w = world_of(transport, world_engines(G, True, small))
    m = RoutedRefundOracle(WRULES, local_cache=True)
    row = [hiprl.build_batch([wreq([f"r{g}_{i}", f"g{g}_{i}"], [i % 4, 4], 3 + i % 9) for i in range(30)]) for g in range(G)]
    sts = model_step(m, row, w.step(row), f"{ctx} charge")
    return w, m, row, sts


@pytest.mark.parametrize("case", ["rule", "time", "null_status", "null_hits", "flag", "capacity"])
@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_origin_refusals_change_nothing(transport, case):
    ctx = f"origin refusal {transport} {case}"
    w, m, row, sts = charged_world(transport, ctx)
    bad, sbad, flag, code, null_hits = row[1], sts[1], 0, EINVAL, ()
    if case == "rule":
        rule = bad.rule.copy()
        rule[3] = 99
        bad = hiprl.Batch(bad.blob, bad.off, rule, bad.req_of, bad.now, bad.hits)
    elif case == "time":
        bad = hiprl.Batch(bad.blob, bad.off, bad.rule, bad.req_of, np.full(bad.n_req, 0xFFFD0001, np.int64), bad.hits)
    elif case == "null_status":
        sbad = None
    elif case == "null_hits":
        null_hits = (1,)
    elif case == "flag":
        flag = 2
    else:
        n = MAXD + 1
        bad = req_batch([item_of(row[1], i % row[1].n_desc) for i in range(n)], [1] * n, T0, [1] * n)
        sbad, code = statuses([OVER | HASLIM] * n), ECAPACITY
    s0, r0 = states(w, T0), [rec_set(e) for e in w.engines]
    codes, untouched = raw_world_call(w, [row[0], bad, row[2]], [sts[0], sbad, sts[2]], [0, flag, 0], null_hits)
    assert codes == ([code] * 3 if transport == "local" else [EPEER, code, EPEER]), (ctx, codes)
    assert untouched, ctx
    assert states(w, T0) == s0 and [rec_set(e) for e in w.engines] == r0, ctx
    # no plan was left open anywhere, and the same call without the fault is applied
    am, origin, owner = refund_checked(w, m, row, sts, False, ctx)
    assert owner["refunded"] == 180 and owner["absent"] == 0
    peeks_checked(w, m, row, ctx)
    w.close()


@pytest.mark.parametrize("transport", ["local", "emulated"])
def test_owner_capacity_after_the_records_moved_applies_nothing_anywhere(transport):
    """Owner 1 can take 256 records and receives 257 owed descriptors; owners 0 and 2 plan theirs
    successfully. With every owner committing right after its own plan they would have applied their
    share of a refund that owner 1 refused."""
    G = 3
    ctx = f"owner capacity {transport}"
    cand = [(hiprl.cache_key_prefix("cost", [("k", f"cap{i}")]), 1 + i % 3) for i in range(1400)]
    own = [owner_of(it, G) for it in cand]
    name = {it: f"cap{i}" for i, it in enumerate(cand)}
    mine1 = [it for it, j in zip(cand, own) if j == 1][:257]
    others = [it for it, j in zip(cand, own) if j == 0][:40] + [it for it, j in zip(cand, own) if j == 2][:40]
    assert len(mine1) == 257 and len(others) == 80
    w = world_of(transport, world_engines(G, True, small=1))
    m = RoutedRefundOracle(WRULES, local_cache=True)
    allk = others + mine1
    none = hiprl.build_batch([])
    # charged in two steps (owner 1 takes at most 256 records a step), from origins 0 and 2
    halves = []
    for half in (allk[:160], allk[160:]):
        r = [hiprl.build_batch([wreq([name[it]], [it[1]], 7) for it in half[g::2]]) for g in range(2)]
        halves.append([r[0], none, r[1]])
        model_step(m, halves[-1], w.step(halves[-1]), f"{ctx} charge")
    # the statuses are built so that all 337 descriptors are owed: every request is over its limit
    both = [routing.concat_batches([halves[0][g], halves[1][g]]) for g in range(G)]
    sts = [statuses([OVER | HASLIM] * b.n_desc) for b in both]
    assert sum(owner_of(item_of(b, i), G) == 1 for b in both for i in range(b.n_desc)) == 257
    s0, r0 = states(w, T0), [rec_set(e) for e in w.engines]
    codes, untouched = raw_world_call(w, both, sts, [0, 0, 0])
    assert codes == ([ECAPACITY] * 3 if transport == "local" else [EPEER, ECAPACITY, EPEER]), (ctx, codes)
    assert untouched, ctx
    # owners 0 and 2 planned successfully and have written nothing; nobody holds a plan
    assert states(w, T0) == s0 and [rec_set(e) for e in w.engines] == r0, ctx
    # the same refunds in two calls: each applied exactly once
    for part in halves:
        psts = [statuses([OVER | HASLIM] * b.n_desc) for b in part]
        am, origin, owner = refund_checked(w, m, part, psts, False, ctx)
        assert owner["refunded"] == sum(b.n_desc for b in part) and owner["absent"] == 0
        peeks_checked(w, m, part, ctx)
    for part in halves:
        reps, codes = w.ask("peek", part)
        assert reps is not None and all((r["count"] == 0).all() for r in reps), (ctx, codes)
    w.close()
