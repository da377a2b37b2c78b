#!/usr/bin/env python3
"""rl_router_adjust cost on this box ("Routed adjust").

Two parts.

1. Router.adjust of N descriptors over 4 logical shards (local transport: four engines and their
   exchange copies on this one GPU, N / 4 descriptors per origin) on a world prefilled by
   Router.set, in three mixes, each REPEATS times after one untimed round, interleaved in every
   round with Router.peek and Router.set of the same batches:

     found      every counter is found
     half       every other string is absent from the world
     dup50      origins 2 and 3 repeat the keys of origins 0 and 1

   as wall-clock µs per call and keys/s (host clock around each synchronous call: staging, both
   packs, the exchanges, plan, commit and read-backs included).

2. The record-form index kernel beside the host form's, on a lone engine holding the same N keys:
   rl_adjust (k_adjust_index, k_adjust_apply) and rl_route_pack_adjust + rl_adjust_routed_plan +
   rl_adjust_routed_commit (k_adjust_pack, k_adjust_index_routed, k_adjust_apply) over records
   packed from the same batch, alternating, REPEATS times after one untimed pair, with the engine's
   kernel timing on (events around each launch): median and min-max per kernel, and the shares of
   k_adjust_pack and k_adjust_apply in the record form's kernel time.

Beside them the random 32-B slot read-modify-write rate of bench.py --full's probe (tools/microbench).

  python tools/routed_adjust_probe.py --n 1000000 --out profiles/routed_adjust_probe.json
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
HOST_KERNELS = ["k_adjust_index", "k_adjust_apply"]
RECORD_KERNELS = ["k_adjust_pack", "k_adjust_index_routed", "k_adjust_apply"]


def keys(lo, hi, now, tag="ak"):
    """One-entry descriptors of 16-byte prefixes under rule 0, one request: key numbers [lo, hi)."""
    n = hi - lo
    blob = np.frombuffer("".join(f"{tag}_k_{i:010d}_" for i in range(lo, hi)).encode(), np.uint8).copy()
    assert blob.shape[0] == 16 * n
    return hiprl.Batch(blob, (np.arange(n + 1, dtype=np.uint32) * 16).astype(np.uint32), np.zeros(n, np.uint32),
                       np.zeros(n, np.uint32), np.array([now], np.int64), np.ones(1, np.uint32))


def half_absent(b):
    """Every other string of b replaced by one no table ever held."""
    blob = b.blob.reshape(b.n_desc, 16).copy()
    blob[1::2, 0] = ord("z")
    return hiprl.Batch(blob.reshape(-1), b.off, b.rule, b.req_of, b.now, b.hits)


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
        raise SystemExit("routed_adjust_probe: no GPU (a measurement does not fall back)")
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
        v["count"], v["ttl_s"], v["flags"] = 1000, 3000, hiprl.PEEK_FOUND
        return v

    # ---- 1. the router call ----
    engines = []
    for _ in range(G):
        e = hiprl.Engine(log2_slots=(12, 12, a.log2 - 2, 12), local_cache=True, max_batch_desc=a.n)
        e.load_rules(rules)
        engines.append(e)
    rt = hiprl.Router(engines, max_desc=per, max_blob_bytes=16 * per + 64)
    found = [keys(g * per, (g + 1) * per, now) for g in range(G)]
    half = [half_absent(b) for b in found]
    dup = [found[g % (G // 2)] for g in range(G)]
    vals = [value(per) for _ in range(G)]
    down = [-rng.integers(1, 100, per).astype(np.int32) for _ in range(G)]
    up = [-d for d in down]
    rt.set(found, vals, want_out=False)
    assert sum(sum(e.occupancy()["live"]) for e in engines) == a.n

    def total(reps, f):
        return sum(r[f] for r in reps)

    def round_():
        out = {}
        out["set_overwrite"], _ = timed(rt.set, found, vals)
        out["adjust_found"], (_, reps) = timed(rt.adjust, found, down)
        assert total(reps, "applied") == a.n and total(reps, "floored") == 0
        out["peek"], _ = timed(rt.peek, found)
        out["adjust_found_no_out"], _ = timed(rt.adjust, found, up, want_out=False)
        out["adjust_half"], (_, reps) = timed(rt.adjust, half, down)
        assert (total(reps, "applied"), total(reps, "absent")) == (a.n - a.n // 2, a.n // 2)
        out["set_overwrite_no_out"], _ = timed(rt.set, found, vals, want_out=False)
        out["adjust_dup50"], (_, reps) = timed(rt.adjust, dup, down)
        assert total(reps, "applied") == a.n
        return out

    round_()
    rounds = [round_() for _ in range(a.repeats)]
    calls = {}
    for k in rounds[0]:
        med = statistics.median(r[k] for r in rounds)
        calls[k] = {"us": round(med * 1e6, 1), "keys_per_s": round(a.n / med, 1),
                    "all_us": [round(r[k] * 1e6, 1) for r in rounds]}
    rt.close()
    for e in engines:
        e.close()

    # ---- 2. the two index kernels on a lone engine, alternating ----
    eng = hiprl.Engine(log2_slots=(12, 12, a.log2, 12), local_cache=True, max_batch_desc=a.n, max_blob_bytes=16 * a.n)
    eng.load_rules(rules)
    b = keys(0, a.n, now)
    mixes = {"found": b, "half": half_absent(b),
             "dup50": hiprl.Batch(np.concatenate([b.blob[:8 * a.n]] * 2), b.off, b.rule, b.req_of, b.now, b.hits)}
    eng.set(b, value(a.n), want_out=False)
    d_down = -rng.integers(1, 100, a.n).astype(np.int32)
    send = torch.zeros(a.n * 32, dtype=torch.uint8, device=dev)
    perm = torch.zeros(a.n, dtype=torch.int32, device=dev)
    x = torch.zeros(2, dtype=torch.int32, device=dev)
    reply = torch.zeros(a.n * 16, dtype=torch.uint8, device=dev)
    eng.set_timing(True)

    def kt():
        return {k: v[0] for k, v in eng.kernel_times().items()}

    kernels = {}
    for name, hb in mixes.items():
        db = pyrouter.DeviceBatch.from_host(hb, dev)
        host, record = {k: [] for k in HOST_KERNELS}, {k: [] for k in RECORD_KERNELS}
        for r in range(a.repeats + 1):
            d = d_down if r % 2 == 0 else -d_down  # the counters come back: never floored
            dd = torch.from_numpy(d).to(dev)
            torch.cuda.synchronize()
            t0 = kt()
            _, rep_h = eng.adjust(hb, d)
            t1 = kt()
            eng.route_pack_strided(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), 0, 1, a.n, send.data_ptr(),
                                   x.data_ptr(), perm.data_ptr())
            eng.route_pack_adjust(a.n, db.rule.data_ptr(), perm.data_ptr(), dd.data_ptr(), send.data_ptr())
            eng.adjust_routed_plan(send.data_ptr(), a.n, reply.data_ptr())
            rep_r = eng.adjust_routed_commit(True)
            t2 = kt()
            assert {k: rep_h[k] for k in ("absent", "applied", "floored")} == {k: rep_r[k] for k in ("absent", "applied", "floored")}
            assert rep_r["floored"] == 0
            if r == 0:
                continue  # one untimed pair
            for k in HOST_KERNELS:
                host[k].append((t1[k] - t0[k]) * 1e3)
            for k in RECORD_KERNELS:
                record[k].append((t2[k] - t1[k]) * 1e3)
        rec_tot = sum(statistics.median(record[k]) for k in RECORD_KERNELS)
        hi, ri = host["k_adjust_index"], record["k_adjust_index_routed"]
        kernels[name] = {
            "host_form_us": {k: spread(host[k]) for k in HOST_KERNELS},
            "record_form_us": {k: spread(record[k]) for k in RECORD_KERNELS},
            "index_routed_over_index": round(statistics.median(ri) / statistics.median(hi), 3),
            "index_spread_us": round(max(max(hi) - min(hi), max(ri) - min(ri)), 1),
            "record_form_shares": {k: round(statistics.median(record[k]) / rec_tot, 3) for k in RECORD_KERNELS}}
    eng.set_timing(False)

    slots = 2 * (1 << a.log2) + 6 * (1 << 12)
    res = {"tool": "tools/routed_adjust_probe.py", "descriptors": a.n, "shards": G, "transport": "local (one GPU)",
           "prefix_bytes": 16, "log2_slots_world": [12, 12, a.log2 - 2, 12], "log2_slots_lone": [12, 12, a.log2, 12],
           "repeats": a.repeats,
           "timing": "calls: host clock around each synchronous router call; kernels: events around each launch, "
                     "host and record form alternating on one lone engine",
           "calls": calls, "kernels": kernels,
           "adjust_over_set": {"found": round(calls["adjust_found"]["us"] / calls["set_overwrite"]["us"], 2),
                               "found_no_out": round(calls["adjust_found_no_out"]["us"] /
                                                     calls["set_overwrite_no_out"]["us"], 2),
                               "half": round(calls["adjust_half"]["us"] / calls["set_overwrite"]["us"], 2),
                               "dup50": round(calls["adjust_dup50"]["us"] / calls["set_overwrite"]["us"], 2)},
           "adjust_over_peek": round(calls["adjust_found"]["us"] / calls["peek"]["us"], 2)}
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
