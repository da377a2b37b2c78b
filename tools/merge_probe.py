#!/usr/bin/env python3
"""rl_merge cost of one engine on this box ("Merge").

rl_merge of N records in one call (host call: the host pass over the records, staging through
pinned memory, k_merge_plan + k_merge_check, the control block's read-back, k_merge_apply, the
occupancy publish) in three cases, each REPEATS times after one untimed round, interleaved in every
round with rl_restore_put of the same records into a second engine of the same size:

  empty    into an empty table: every record is claimed
  folded   over the table the first call filled: every identity is found
  half     into a table that holds the first half of the records

as wall-clock µs per call and records/s, then one round with the engine's kernel timing on for the
two kernels' shares. Beside them the random 32-B slot read-modify-write rate of bench.py --full's
probe (tools/microbench), which tools/set_probe.py reports too.

  python tools/merge_probe.py --n 1000000 --out profiles/merge_probe.json
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "api-ratelimit_amd"))
import hiprl  # noqa: E402

MERGE_KERNELS = ["k_merge_plan", "k_merge_apply"]


def keys(n, now):
    """N one-entry descriptors of 16-byte prefixes under rule 0, one request."""
    blob = np.frombuffer("".join(f"mk_k_{i:010d}_" for i in range(n)).encode(), np.uint8).copy()
    assert blob.shape[0] == 16 * n
    return hiprl.Batch(blob, (np.arange(n + 1, dtype=np.uint32) * 16).astype(np.uint32), np.zeros(n, np.uint32),
                       np.zeros(n, np.uint32), np.array([now], np.int64), np.ones(1, np.uint32))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="records per call")
    ap.add_argument("--log2", type=int, default=22, help="log2 slots of each HOUR region")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    now = 1_700_000_000
    rules = [(1 << 30, hiprl.HOUR)]

    def engine():
        e = hiprl.Engine(log2_slots=(12, 12, a.log2, 12), local_cache=True, max_batch_desc=max(a.n, 4096),
                         max_blob_bytes=16 * max(a.n, 4096))
        e.load_rules(rules)
        return e

    src = engine()
    v = np.zeros(a.n, hiprl.PEEK_DTYPE)
    v["count"], v["ttl_s"], v["flags"] = np.arange(a.n) % 1000 + 1, 3000, hiprl.PEEK_FOUND
    src.set(keys(a.n, now), v, want_out=False)
    h, recs = src.snapshot_records()
    assert recs.shape[0] == a.n
    del src
    tgt, rst = engine(), engine()
    half = recs[:a.n // 2]

    def timed(f, *args, **kw):
        t0 = time.perf_counter()
        r = f(*args, **kw)
        return time.perf_counter() - t0, r

    def round_():
        out = {}
        tgt.reset()
        out["merge_empty"], rep = timed(tgt.merge_chunk, h, recs, now)
        assert rep["claimed"] == a.n and sum(tgt.occupancy()["live"]) == a.n
        rst.restore_begin(h)
        # (the put only enqueues its last piece's kernels; rl_restore_end drains the stream)
        out["restore_put"], _ = timed(lambda: (rst.restore_put(recs), rst.restore_end()))
        out["merge_folded"], rep = timed(tgt.merge_chunk, h, recs, now)
        assert rep["folded"] == a.n
        tgt.reset()
        tgt.merge_chunk(h, half, now)
        out["merge_half"], rep = timed(tgt.merge_chunk, h, recs, now)
        assert (rep["folded"], rep["claimed"]) == (a.n // 2, a.n - a.n // 2)
        return out

    round_()
    rounds = [round_() for _ in range(a.repeats)]
    calls = {}
    for k in rounds[0]:
        med = statistics.median(r[k] for r in rounds)
        calls[k] = {"us": round(med * 1e6, 1), "records_per_s": round(a.n / med, 1),
                    "all_us": [round(r[k] * 1e6, 1) for r in rounds]}

    tgt.set_timing(True)
    kernels = {}

    def shares(name, f):
        t0 = {k: tgt.kernel_times()[k][0] for k in MERGE_KERNELS}
        f()
        ms = {k: tgt.kernel_times()[k][0] - t0[k] for k in MERGE_KERNELS}
        tot = sum(ms.values())
        kernels[name] = {k: {"us": round(ms[k] * 1e3, 1), "share": round(ms[k] / tot, 3)} for k in MERGE_KERNELS}
        kernels[name]["kernels_us"] = round(tot * 1e3, 1)

    tgt.reset()
    shares("merge_empty", lambda: tgt.merge_chunk(h, recs, now))
    shares("merge_folded", lambda: tgt.merge_chunk(h, recs, now))
    tgt.reset()
    tgt.merge_chunk(h, half, now)
    shares("merge_half", lambda: tgt.merge_chunk(h, recs, now))
    tgt.set_timing(False)

    slots = 2 * (1 << a.log2) + 6 * (1 << 12)
    res = {"tool": "tools/merge_probe.py", "records": a.n, "log2_slots": [12, 12, a.log2, 12],
           "region_load": round(a.n / (1 << a.log2), 3), "repeats": a.repeats,
           "timing": "host clock around each synchronous host call (host pass, staging and read-backs included; "
                     "restore_put: rl_restore_put + rl_restore_end, without begin's table clear); "
                     "kernels: events around each launch, one round (k_merge_plan includes k_merge_check)",
           "calls": calls, "kernels": kernels,
           "merge_over_restore_put": {k: round(calls[k]["us"] / calls["restore_put"]["us"], 2)
                                      for k in ("merge_empty", "merge_folded", "merge_half")}}
    del tgt, rst
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
