#!/usr/bin/env python3
"""rl_resize pause of one engine on this box, against the path it replaces.

Fills the SECOND / MINUTE / HOUR regions (both window parities, 2^LOG2 slots each) to LOAD of
their slots with synthetic records (tools/snapshot_probe.py's), then measures, REPEATS times each
after one untimed pass:

  resize_one_unit   rl_resize of the SECOND unit to LOG2 + 1, the others kept (their regions are
                    rehashed too: every region goes through the one pass)
  resize_all_units  rl_resize of every unit to its log2 + 1
                    both: the whole call (allocation, clearing the new table, k_rehash,
                    synchronise, freeing the old table), records/s and GB/s of old table streamed;
                    each followed by an untimed resize back (reported as resize_back)
  memset_new_table  clearing a buffer of the new table's size alone (part of the pause)
  host_path         the path before rl_resize: snapshot_records() to host memory, then
                    restore_records() into a second engine of the new size (all units + 1); the
                    second engine's creation is timed apart and not counted

and the box's streaming copy bandwidth and random slot read-modify-write rate (tools/microbench).

  python tools/resize_probe.py --log2 24 --out profiles/resize_probe.json
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "api-ratelimit_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import hiprl  # noqa: E402
import numpy as np  # noqa: E402
from snapshot_probe import synthetic  # noqa: E402


def med(xs):
    return round(statistics.median(xs), 3)


def memset_ms(n_bytes, repeats):
    """hipMemset of n_bytes of fresh device memory, synchronised: milliseconds per repeat."""
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        try:
            hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        except OSError:
            return None
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    p = C.c_void_p()
    if hip.hipMalloc(C.byref(p), n_bytes):
        return None
    out = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        rc = hip.hipMemset(p, 0, n_bytes) or hip.hipDeviceSynchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        if rc:
            out = None
            break
    hip.hipFree(p)
    return out[1:] if out else None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, default=24, help="log2 slots of each SECOND/MINUTE/HOUR region")
    ap.add_argument("--load", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    base = (a.log2, a.log2, a.log2, 12)
    eng = hiprl.Engine(log2_slots=base, local_cache=True, max_batch_desc=4096)
    h, recs = synthetic(a.log2, a.load, eng, np.random.default_rng(1))
    n = recs.shape[0]
    eng.restore_records(h, recs, chunk=1 << 20)
    del recs
    slots = 6 * (1 << a.log2) + 2 * (1 << 12)

    def slots_of(lg):
        return 2 * sum(1 << x for x in lg)

    def resize_case(up):
        new = [x or b for x, b in zip(up, base)]
        ups, backs = [], []
        for k in range(a.repeats + 1):
            t0 = time.perf_counter()
            eng.resize(up)
            t1 = time.perf_counter()
            eng.resize(base)
            t2 = time.perf_counter()
            assert sum(eng.occupancy()["live"]) == n
            if k:
                ups.append(t1 - t0)
                backs.append(t2 - t1)
        ms = memset_ms(32 * slots_of(new), a.repeats)
        return {
            "log2_slots": new, "new_table_GiB": round(32 * slots_of(new) / 2**30, 3),
            "pause_ms": {"median": med([t * 1e3 for t in ups]), "all": [round(t * 1e3, 3) for t in ups]},
            "records_per_s": round(statistics.median([n / t for t in ups]), 1),
            "source_GBps": med([32 * slots / t / 1e9 for t in ups]),
            "memset_new_table_ms": {"median": med(ms), "all": [round(x, 3) for x in ms]} if ms else None,
            "resize_back_ms": {"median": med([t * 1e3 for t in backs])},
        }

    res = {
        "tool": "tools/resize_probe.py", "log2_slots": list(base), "table_slots": slots,
        "table_GiB": round(slots * 32 / 2**30, 3), "records": n, "load": a.load, "repeats": a.repeats,
        "prefill": "synthetic uniform keys, regions 0-5, restored",
        "resize_one_unit": resize_case((a.log2 + 1, 0, 0, 0)),
        "resize_all_units": resize_case((a.log2 + 1, a.log2 + 1, a.log2 + 1, 13)),
    }

    # the path before rl_resize: the live records to the host and into a second engine
    grown = (a.log2 + 1, a.log2 + 1, a.log2 + 1, 13)
    host, create = [], []
    for k in range(a.repeats + 1):
        t0 = time.perf_counter()
        b = hiprl.Engine(log2_slots=grown, local_cache=True, max_batch_desc=4096)
        t1 = time.perf_counter()
        hh, rr = eng.snapshot_records(cap=1 << 20)
        t2 = time.perf_counter()
        b.restore_records(hh, rr, chunk=1 << 20)
        t3 = time.perf_counter()
        assert sum(b.occupancy()["live"]) == n
        b.close()
        del rr
        if k:
            create.append(t1 - t0)
            host.append((t2 - t1, t3 - t2))
    tot = [s + r for s, r in host]
    res["host_path_all_units"] = {
        "what": "snapshot_records() to pageable host memory + restore_records() into a second engine "
                "of the new size; the second engine's creation is not counted",
        "pause_ms": {"median": med([t * 1e3 for t in tot]), "all": [round(t * 1e3, 3) for t in tot]},
        "snapshot_ms": med([s * 1e3 for s, _ in host]), "restore_ms": med([r * 1e3 for _, r in host]),
        "second_engine_create_ms": med([t * 1e3 for t in create]),
    }
    res["host_path_over_resize"] = round(res["host_path_all_units"]["pause_ms"]["median"] /
                                         res["resize_all_units"]["pause_ms"]["median"], 2)
    eng.close()
    lp = ROOT / "tools" / "microbench" / "libroofline_probe.so"
    if lp.exists():  # the same probe bench.py --full runs: copy bandwidth, random 32-B slot RMW rate
        plib = C.CDLL(str(lp))
        plib.rl_probe_roofline.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]
        plib.rl_probe_roofline.restype = C.c_int
        gbs, rate, rus = C.c_double(), C.c_double(), C.c_double()
        if plib.rl_probe_roofline(slots, 1 << 20, C.byref(gbs), C.byref(rate), C.byref(rus)) == 0:
            res["bounds_same_box"] = {
                "copy_GBps": round(gbs.value, 1), "slot_rmw_per_s": round(rate.value, 1),
                "resize_frac_of_rmw": round(res["resize_all_units"]["records_per_s"] / rate.value, 4)}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
