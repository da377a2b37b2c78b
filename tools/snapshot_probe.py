#!/usr/bin/env python3
"""Snapshot / restore rates of one engine on this box ("Snapshot and restore").

Fills the SECOND / MINUTE / HOUR regions (both window parities, 2^LOG2 slots each) to LOAD of
their slots with synthetic records — uniform 61-bit keys, as fingerprints are — by restoring
them, then measures, REPEATS times each after one untimed pass:

  restore_put      records/s from the first rl_restore_put to the return of rl_restore_end
                   (pageable host memory -> pinned staging -> k_snap_import + k_snap_verify)
  snapshot_begin   the pause in ms: buffer allocation, k_snap_export over the whole table, sync;
                   and the pass in GB/s, counting every slot read plus every record written
  drain            rl_snapshot_next into pageable host memory, GB/s

and, beside them, what bounds the two kernels on the same box: the streaming copy bandwidth and
the random slot read-modify-write rate of bench.py --full's probe (tools/microbench).

  python tools/snapshot_probe.py --log2 24 --out profiles/snapshot_probe.json
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


def synthetic(log2, load, eng, rng):
    """A header and records for regions 0..5 at `load`: keys unique by construction (the low 25
    bits count, the bits a slot's place is taken from are random)."""
    n_r = int(load * (1 << log2))
    assert n_r < (1 << 25)
    h = eng.snapshot_begin()  # an empty engine's header: magic, sizes, flags, seed_check
    eng.snapshot_end()
    recs = np.zeros(6 * n_r, hiprl.SNAP_DTYPE)
    idx = np.arange(n_r, dtype=np.uint64)
    for r in range(6):
        gen = 2 * 500_000 + (r & 1) + 1  # window index of the region's parity, + 1
        h.gen[r], h.live[r] = gen, n_r
        part = recs[r * n_r:(r + 1) * n_r]
        place = rng.integers(0, 1 << 36, n_r, dtype=np.uint64)
        part["key"] = (np.uint64(r) << np.uint64(61)) | (place << np.uint64(25)) | idx
        part["ctrl"] = np.uint64(gen) | (rng.integers(0, 1 << 32, n_r, dtype=np.uint64) << np.uint64(32))
        part["count"] = rng.integers(1, 1000, n_r, dtype=np.uint32)
        part["exp"] = 1_700_000_000
    h.n_records = recs.shape[0]
    recs = recs[rng.permutation(recs.shape[0])]  # a snapshot's record order is the table's, not the regions'
    return h, recs


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, default=24, help="log2 slots of each SECOND/MINUTE/HOUR region")
    ap.add_argument("--load", type=float, default=0.23)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--put-chunk", type=int, default=1 << 20, help="records per rl_restore_put call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    eng = hiprl.Engine(log2_slots=(a.log2, a.log2, a.log2, 12), local_cache=True, max_batch_desc=4096)
    lib = eng.lib
    rng = np.random.default_rng(1)
    h, recs = synthetic(a.log2, a.load, eng, rng)
    n = recs.shape[0]
    slots = 6 * (1 << a.log2) + 2 * (1 << 12)

    def restore():
        eng.restore_begin(h)  # clears the table: not part of the put rate
        t0 = time.perf_counter()
        for i in range(0, n, a.put_chunk):
            part = recs[i:i + a.put_chunk]
            rc = lib.rl_restore_put(eng.h, part.ctypes.data, part.shape[0])
            assert rc == 0, rc
        eng.restore_end()
        return time.perf_counter() - t0

    restore()
    put_s = [restore() for _ in range(a.repeats)]

    buf = np.zeros(1 << 20, hiprl.SNAP_DTYPE)
    got = C.c_uint32()

    def snapshot():
        t0 = time.perf_counter()
        hh = eng.snapshot_begin()
        t1 = time.perf_counter()
        assert hh.n_records == n, (hh.n_records, n)
        while True:
            rc = lib.rl_snapshot_next(eng.h, buf.ctypes.data, buf.shape[0], C.byref(got))
            assert rc == 0, rc
            if not got.value:
                break
        t2 = time.perf_counter()
        eng.snapshot_end()
        return t1 - t0, t2 - t1

    snapshot()
    snaps = [snapshot() for _ in range(a.repeats)]
    pause = [p for p, _ in snaps]
    drain = [d for _, d in snaps]
    export_bytes = 32 * (slots + n)

    res = {
        "tool": "tools/snapshot_probe.py", "log2_slots": [a.log2, a.log2, a.log2, 12], "table_slots": slots,
        "table_GiB": round(slots * 32 / 2**30, 3), "records": n, "load": a.load, "repeats": a.repeats,
        "prefill": "synthetic uniform keys, regions 0-5, restored",
        "snapshot_begin_pause_ms": {"median": med([p * 1e3 for p in pause]), "all": [round(p * 1e3, 3) for p in pause]},
        "export_GBps": {"median": med([export_bytes / p / 1e9 for p in pause]),
                        "bytes": export_bytes, "counts": "32 B per slot read + 32 B per record written; the time "
                                                         "is the whole pause (allocation, pass, synchronise)"},
        "drain_GBps": {"median": med([32 * n / d / 1e9 for d in drain]), "all": [round(32 * n / d / 1e9, 3) for d in drain],
                       "into": "pageable host memory, 2^20 records a call"},
        "restore_put_records_per_s": {"median": round(statistics.median([n / s for s in put_s]), 1),
                                      "all": [round(n / s, 1) for s in put_s],
                                      "from": f"pageable host memory, {a.put_chunk} records a call, to rl_restore_end"},
    }
    del eng
    lp = ROOT / "tools" / "microbench" / "libroofline_probe.so"
    if lp.exists():  # the same probe bench.py --full runs: copy bandwidth, random 32-B slot RMW rate
        plib = C.CDLL(str(lp))
        plib.rl_probe_roofline.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]
        plib.rl_probe_roofline.restype = C.c_int
        gbs, rate, rus = C.c_double(), C.c_double(), C.c_double()
        if plib.rl_probe_roofline(slots, 1 << 20, C.byref(gbs), C.byref(rate), C.byref(rus)) == 0:
            res["bounds_same_box"] = {"copy_GBps": round(gbs.value, 1), "slot_rmw_per_s": round(rate.value, 1),
                                      "export_frac_of_copy": round(res["export_GBps"]["median"] / gbs.value, 3),
                                      "put_frac_of_rmw": round(res["restore_put_records_per_s"]["median"] / rate.value, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
