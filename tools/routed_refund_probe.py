#!/usr/bin/env python3
"""rl_router_refund cost on this box ("Routed refund").

Two parts.

1. Router.refund of N descriptors over 4 logical shards (local transport: four engines and their
   exchange copies on this one GPU, N / 4 descriptors per origin, one descriptor per request) on a
   world prefilled by Router.set, at about 0 %, 5 % and 30 % rejected requests, beside the host path
   it replaces: the amounts made on the host from the statuses (numpy), then Router.adjust of the
   negated amounts over every descriptor. The arms alternate in one process, REPEATS times after one
   untimed round, as wall-clock µs per call (host clock around each synchronous call), with the
   share of descriptors that travel.

2. On a lone engine holding the same N keys: k_refund_index_routed beside k_adjust_index_routed on
   the same records (h = 3: an amount to one, a delta to the other, so the counters come back),
   alternating, spread over distinct keys and with half of them on 256 hot keys; and k_refund_mark
   and k_refund_owed at the three rejection rates. Kernel timing is the engine's (events around each
   launch): median and min-max.

Beside them the random 32-B slot read-modify-write rate of bench.py --full's probe (tools/microbench).

  python tools/routed_refund_probe.py --n 1000000 --out profiles/routed_refund_probe.json
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "api-ratelimit_amd"))
import hiprl  # noqa: E402
import router as pyrouter  # noqa: E402

G = 4
RATES = {"rejected_0": 0.0, "rejected_5": 0.05, "rejected_30": 0.30}
OVER, OK, HASLIM = 2, 1, 1 << 8
HITS = 3


def keys(numbers, now, tag="rk"):
    """One-entry descriptors of 16-byte prefixes under rule 0, one request each, HITS hits."""
    n = len(numbers)
    blob = np.frombuffer("".join(f"{tag}_k_{i:010d}_" for i in numbers).encode(), np.uint8).copy()
    assert blob.shape[0] == 16 * n
    return hiprl.Batch(blob, (np.arange(n + 1, dtype=np.uint32) * 16).astype(np.uint32), np.zeros(n, np.uint32),
                       np.arange(n, dtype=np.uint32), np.full(n, now, np.int64), np.full(n, HITS, np.uint32))


def statuses(n, rate, rng):
    st = np.zeros(n, hiprl.STATUS_DTYPE)
    st["code_flags"] = np.where(rng.random(n) < rate, OVER | HASLIM, OK | HASLIM)
    return st


def host_amounts(b, st):
    """The rule the host path has to rebuild: rejected request, not nil, not a local-cache hit."""
    cf = st["code_flags"]
    rej = np.zeros(b.n_req, bool)
    rej[b.req_of[(cf & 0xFF) == OVER]] = True
    owed = rej[b.req_of] & (b.rule != hiprl.NIL_RULE) & (((cf >> 8) & 2) == 0)
    return np.where(owed, np.maximum(b.hits[b.req_of], 1), 0).astype(np.int64)


def spread(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="descriptors per call, over all origins")
    ap.add_argument("--log2", type=int, default=22, help="log2 slots of the lone engine's HOUR regions (the world's: 2 less)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("routed_refund_probe: no GPU (a measurement does not fall back)")
    assert a.n % (2 * G) == 0
    dev = torch.device("cuda", 0)
    now = 1_700_000_000
    rules = [(1 << 30, hiprl.HOUR)]
    per = a.n // G
    rng = np.random.default_rng(1)

    def timed(f, *args, **kw):
        t0 = time.perf_counter()
        r = f(*args, **kw)
        return time.perf_counter() - t0, r

    def value(n):
        v = np.zeros(n, hiprl.PEEK_DTYPE)
        v["count"], v["ttl_s"], v["flags"] = 1_000_000, 3000, hiprl.PEEK_FOUND
        return v

    # ---- 1. the router call beside the host path ----
    engines = []
    for _ in range(G):
        e = hiprl.Engine(log2_slots=(12, 12, a.log2 - 2, 12), local_cache=True, max_batch_desc=a.n, max_batch_req=a.n)
        e.load_rules(rules)
        engines.append(e)
    rt = hiprl.Router(engines, max_desc=per, max_blob_bytes=16 * per + 64)
    batches = [keys(range(g * per, (g + 1) * per), now) for g in range(G)]
    rt.set(batches, [value(per) for _ in range(G)], want_out=False)
    assert sum(sum(e.occupancy()["live"]) for e in engines) == a.n
    sts = {name: [statuses(per, rate, rng) for _ in range(G)] for name, rate in RATES.items()}

    def host_path(st):
        deltas = [-host_amounts(b, s) for b, s in zip(batches, st)]
        return rt.adjust(batches, deltas, want_out=False)

    def round_():
        out = {}
        for name, st in sts.items():
            out[f"refund_{name}"], (_, _, reps) = timed(rt.refund, batches, st, want_out=False)
            owed = sum(r["descriptors"] - r["skipped"] for r in reps)
            assert owed == sum(r["refunded"] for r in reps) == sum(int((host_amounts(b, s) != 0).sum()) for b, s in zip(batches, st))
            out[f"host_{name}"], (_, reps) = timed(host_path, st)
            assert sum(r["applied"] for r in reps) == a.n
        return out

    round_()
    rounds = [round_() for _ in range(a.repeats)]
    calls = {k: {"us": round(statistics.median(r[k] for r in rounds) * 1e6, 1),
                 "all_us": [round(r[k] * 1e6, 1) for r in rounds]} for k in rounds[0]}
    travel = {name: round(sum(int((host_amounts(b, s) != 0).sum()) for b, s in zip(batches, st)) / a.n, 4)
              for name, st in sts.items()}
    rt.close()
    for e in engines:
        e.close()

    # ---- 2. the kernels on a lone engine ----
    eng = hiprl.Engine(log2_slots=(12, 12, a.log2, 12), local_cache=True, max_batch_desc=a.n, max_batch_req=a.n,
                       max_blob_bytes=16 * a.n)
    eng.load_rules(rules)
    b = keys(range(a.n), now)
    hot = keys([i if i % 2 == 0 else i % 256 for i in range(a.n)], now)
    eng.set(b, value(a.n), want_out=False)
    send = torch.zeros(a.n * 32, dtype=torch.uint8, device=dev)
    perm = torch.zeros(a.n, dtype=torch.int32, device=dev)
    x = torch.zeros(2, dtype=torch.int32, device=dev)
    amt = torch.full((a.n,), HITS, dtype=torch.int32, device=dev)
    rule_out = torch.zeros(a.n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    eng.set_timing(True)

    def kt():
        return {k: v[0] for k, v in eng.kernel_times().items()}

    kernels = {}
    for name, hb in (("distinct", b), ("half_on_256_hot", hot)):
        db = pyrouter.DeviceBatch.from_host(hb, dev)
        eng.route_pack_strided(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), 0, 1, a.n, send.data_ptr(), x.data_ptr(),
                               perm.data_ptr())
        eng.route_pack_adjust(a.n, db.rule.data_ptr(), perm.data_ptr(), amt.data_ptr(), send.data_ptr())
        torch.cuda.synchronize()
        ref, adj = [], []
        for r in range(a.repeats + 1):
            t0 = kt()
            eng.adjust_routed_plan(send.data_ptr(), a.n)  # + HITS
            rep_a = eng.adjust_routed_commit(True)
            t1 = kt()
            eng.refund_routed_plan(send.data_ptr(), a.n)  # - HITS
            rep_r = eng.refund_routed_commit(True)
            t2 = kt()
            assert rep_a["applied"] == rep_r["refunded"] == a.n and rep_r["floored"] == 0
            if r:  # one untimed pair
                adj.append((t1["k_adjust_index_routed"] - t0["k_adjust_index_routed"]) * 1e3)
                ref.append((t2["k_refund_index_routed"] - t1["k_refund_index_routed"]) * 1e3)
        kernels[name] = {"k_adjust_index_routed_us": spread(adj), "k_refund_index_routed_us": spread(ref),
                         "refund_over_adjust": round(statistics.median(ref) / statistics.median(adj), 3)}
    db = pyrouter.DeviceBatch.from_host(b, dev)
    owed_pass = {}
    for name, rate in RATES.items():
        d_st = torch.from_numpy(statuses(a.n, rate, rng).view(np.uint8).copy()).to(dev)
        mark, owed = [], []
        for r in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = kt()
            eng.refund_route_owed(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), d_st.data_ptr(), rule_out.data_ptr(),
                                  amt.data_ptr(), cnt.data_ptr())
            eng.refund_routed_plan(0, 0)  # (an empty plan: synchronises, and folds the launches' events)
            eng.refund_routed_commit(True)
            torch.cuda.synchronize()
            t1 = kt()
            if r:
                mark.append((t1["k_refund_mark"] - t0["k_refund_mark"]) * 1e3)
                owed.append((t1["k_refund_owed"] - t0["k_refund_owed"]) * 1e3)
        owed_pass[name] = {"k_refund_mark_us": spread(mark), "k_refund_owed_us": spread(owed),
                           "owed": int(cnt.cpu().numpy()[1])}
    eng.set_timing(False)

    slots = 2 * (1 << a.log2) + 6 * (1 << 12)
    res = {"tool": "tools/routed_refund_probe.py", "descriptors": a.n, "shards": G, "transport": "local (one GPU)",
           "prefix_bytes": 16, "hits_addend": HITS, "log2_slots_world": [12, 12, a.log2 - 2, 12],
           "log2_slots_lone": [12, 12, a.log2, 12], "repeats": a.repeats,
           "timing": "calls: host clock around each synchronous router call, the two arms alternating; kernels: events "
                     "around each launch on one lone engine",
           "calls": calls, "share_of_descriptors_that_travel": travel,
           "refund_over_host_path": {name: round(calls[f"refund_{name}"]["us"] / calls[f"host_{name}"]["us"], 3)
                                     for name in RATES},
           "index_kernels": kernels, "origin_pass": owed_pass}
    del eng
    lp = ROOT / "tools" / "microbench" / "libroofline_probe.so"
    if lp.exists():  # the same probe bench.py --full runs: random 32-B slot RMW rate
        plib = C.CDLL(str(lp))
        plib.rl_probe_roofline.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]
        plib.rl_probe_roofline.restype = C.c_int
        gbs, rmw, rus = C.c_double(), C.c_double(), C.c_double()
        if plib.rl_probe_roofline(slots, 1 << 20, C.byref(gbs), C.byref(rmw), C.byref(rus)) == 0:
            res["bounds_same_box"] = {"slot_rmw_per_s": round(rmw.value, 1), "copy_GBps": round(gbs.value, 1)}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
