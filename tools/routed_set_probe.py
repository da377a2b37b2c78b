#!/usr/bin/env python3
"""rl_set_routed_plan + rl_set_routed_commit of one engine beside rl_set of the same keys on this
box, with the per-kernel shares, and one Router.set end to end ("Routed set").

Engine part: an HOUR region of 2^LOG2 slots and N keys of 16-byte prefixes. The N keys' routed
records come from the engine's own pack (rl_route_pack_strided, one owner), the values are laid out
beside them by the pack's perm, so both forms write the same key strings: rl_set from a host batch
(staging, k_peek for the replies, k_set_index with the prefix hash, k_set_plan, k_set_apply),
plan + commit from 32-B records and 16-B values already in device memory (k_peek_routed,
k_set_index_routed, k_set_plan, k_set_apply). One untimed call of each first (the first claims the
N slots, every later call overwrites), then REPEATS calls of each, alternating, host clock around
each call, the engine's kernel timing on: the per-kernel figures are the engine's own event pairs,
averaged over the timed calls. The comparison of record is k_set_index_routed against k_set_index
in the same run.

Router part: 4 logical shards on the local transport, Router.set of the N descriptors from origin 0
(the others pass empty batches), host clock around the whole call: staging, pack, value pack,
exchanges by device copies, four owner plans, four commits, the replies back, unpack, copy out.

Beside both, the random slot read-modify-write rate of the same box (tools/microbench).

  python tools/routed_set_probe.py --n 1000000 --out profiles/routed_set_probe.json
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
sys.path.insert(0, str(ROOT / "tools"))
import hiprl  # noqa: E402
import router  # noqa: E402
from peek_probe import keys  # noqa: E402

KERNELS = ("k_set_index", "k_set_index_routed", "k_set_plan", "k_set_apply")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="records per set")
    ap.add_argument("--log2", type=int, default=22, help="log2 slots of each HOUR region")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shards", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n
    dev = torch.device("cuda", 0)
    now = 1_700_000_000
    log2 = (12, 12, a.log2, 12)
    rules = [(1 << 30, hiprl.HOUR)]
    batch = keys(n, "k", now)
    vals = np.zeros(n, hiprl.PEEK_DTYPE)
    vals["count"] = np.arange(1, n + 1, dtype=np.uint32)
    vals["ttl_s"] = 1000
    vals["flags"] = hiprl.PEEK_FOUND

    def new_engine():
        e = hiprl.Engine(log2_slots=log2, local_cache=True, max_batch_desc=max(n, 4096), max_blob_bytes=16 * max(n, 4096))
        e.load_rules(rules)
        return e

    # ---- the two forms on one table ----
    eng = new_engine()
    db = router.DeviceBatch.from_host(batch, dev)
    send = torch.zeros(n * hiprl.ROUTE_RECORD_BYTES, dtype=torch.uint8, device=dev)
    x = torch.zeros(16, dtype=torch.int32, device=dev)
    perm = torch.zeros(n, dtype=torch.int32, device=dev)
    eng.route_pack_strided(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), 0, 1, n, send.data_ptr(), x.data_ptr(),
                           perm.data_ptr())
    torch.cuda.synchronize()
    assert x.cpu().tolist()[:2] == [n, 0]
    hperm = perm.cpu().numpy().view(np.uint32)
    vrec = np.zeros(n, hiprl.PEEK_DTYPE)
    vrec[hperm] = vals
    d_val = torch.from_numpy(vrec.view(np.uint8).copy()).to(dev)
    d_rep = torch.zeros(n * 16, dtype=torch.uint8, device=dev)

    def host_form():
        eng.set(batch, vals)

    def record_form():
        eng.set_routed_plan(send.data_ptr(), d_val.data_ptr(), n, d_rep.data_ptr())
        eng.set_routed_commit(True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    host_form()  # claims the N slots
    assert sum(eng.occupancy()["live"]) == n
    record_form()
    assert np.array_equal(eng.peek(batch)["count"], vals["count"])
    eng.set_timing(True)
    ta, tb = [], []
    for _ in range(a.repeats):  # interleaved: each repeat times one form, then the other
        ta.append(timed(host_form))
        tb.append(timed(record_form))
    kt = eng.kernel_times()
    eng.set_timing(False)
    kern = {k: {"mean_us": round(kt[k][0] * 1e3 / max(1, kt[k][1]), 1), "launches": int(kt[k][1])} for k in KERNELS}
    for k in KERNELS:
        kern[k]["records_per_s"] = round(n / (kern[k]["mean_us"] * 1e-6), 1) if kern[k]["mean_us"] else None

    def side(ts):
        return {"call_ms": round(statistics.median(ts) * 1e3, 2), "sets_per_s": round(n / statistics.median(ts), 1),
                "all_call_ms": [round(t * 1e3, 2) for t in ts]}
    res = {"tool": "tools/routed_set_probe.py", "records": n, "prefix_bytes": 16, "log2_slots": list(log2),
           "region_load": round(n / (1 << a.log2), 3), "repeats": a.repeats,
           "state": "every timed call overwrites the N strings an untimed call claimed",
           "timing": "host clock around each call (rl_set: host batch in, replies out; plan + commit: device memory "
                     "in, replies left on the device); kernels: the engine's event pairs, mean over the timed calls",
           "rl_set": side(ta), "plan_commit": side(tb), "kernels": kern,
           "index_routed_over_index_time": round(kern["k_set_index_routed"]["mean_us"] / kern["k_set_index"]["mean_us"], 3)}
    eng.close()
    del eng

    # ---- one Router.set end to end ----
    G = a.shards
    engines = [new_engine() for _ in range(G)]
    rt = hiprl.Router(engines, max_desc=n, host=True, max_blob_bytes=16 * n)
    empty = hiprl.build_batch([])
    row = [batch] + [empty] * (G - 1)
    vrow = [vals] + [np.zeros(0, hiprl.PEEK_DTYPE)] * (G - 1)
    rt.set(row, vrow)  # untimed: allocates the call's buffers, claims the slots
    assert sum(sum(e.occupancy()["live"]) for e in engines) == n
    ts = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt.set(row, vrow)
        ts.append(time.perf_counter() - t0)
    rep = rt.peek(row)
    assert np.array_equal(rep[0]["count"], vals["count"])
    res["router_set"] = {"shards": G, "transport": "local", "descriptors": n, "origins_with_descriptors": 1,
                         "call_ms": round(statistics.median(ts) * 1e3, 2),
                         "sets_per_s": round(n / statistics.median(ts), 1),
                         "all_call_ms": [round(t * 1e3, 2) for t in ts]}
    rt.close()
    del rt, engines

    lp = ROOT / "tools" / "microbench" / "libroofline_probe.so"
    if lp.exists():  # the same probe peek_probe.py and bench.py --full run: random 32-B slot RMW rate
        plib = C.CDLL(str(lp))
        plib.rl_probe_roofline.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]
        plib.rl_probe_roofline.restype = C.c_int
        gbs, rmw, rus = C.c_double(), C.c_double(), C.c_double()
        slots = 2 * (1 << a.log2) + 6 * (1 << 12)
        if plib.rl_probe_roofline(slots, 1 << 20, C.byref(gbs), C.byref(rmw), C.byref(rus)) == 0:
            res["bounds_same_box"] = {
                "slot_rmw_per_s": round(rmw.value, 1), "copy_GBps": round(gbs.value, 1),
                "index_routed_frac_of_rmw": round(kern["k_set_index_routed"]["records_per_s"] / rmw.value, 3),
                "index_frac_of_rmw": round(kern["k_set_index"]["records_per_s"] / rmw.value, 3)}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
