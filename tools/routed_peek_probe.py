#!/usr/bin/env python3
"""rl_peek_routed rate of one engine beside rl_peek_device on this box, and one Router.peek end to
end ("Routed peek").

Kernel part: the table of tools/peek_probe.py (an HOUR region of 2^LOG2 slots prefilled with N
keys through one submit). The N keys' routed records come from the engine's own pack
(rl_route_pack_strided, one owner), so both kernels look the same key strings up: k_peek from
descriptors (offsets, rule, request index, time, 16 prefix bytes hashed), k_peek_routed from 32-B
records (no prefix to hash). Each is timed as BURST calls queued back to back before one
synchronise, REPEATS times, the two kernels alternating inside every repeat, for

  found    the N prefilled keys      absent   N keys never inserted

beside the random slot read-modify-write rate of the same box (tools/microbench, as peek_probe).

Router part: 4 logical shards on the local transport, each owner's table prefilled by one routed
step of the same N keys from origin 0; then Router.peek of those N descriptors from origin 0 (the
others pass empty batches), host clock around the whole call: staging, pack, exchanges by device
copies, four owner lookups, unpack, copy out.

  python tools/routed_peek_probe.py --n 1000000 --out profiles/routed_peek_probe.json
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="records per lookup (and prefilled keys)")
    ap.add_argument("--log2", type=int, default=22, help="log2 slots of each HOUR region")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--shards", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n
    dev = torch.device("cuda", 0)
    now = 1_700_000_000
    log2 = (12, 12, a.log2, 12)
    rules = [(1 << 30, hiprl.HOUR)]
    present, absent = keys(n, "k", now), keys(n, "x", now + 1)

    def new_engine():
        e = hiprl.Engine(log2_slots=log2, local_cache=True, max_batch_desc=max(n, 4096), max_blob_bytes=16 * max(n, 4096))
        e.load_rules(rules)
        return e

    # ---- the two kernels on one table ----
    eng = new_engine()
    eng.submit(present)
    assert sum(eng.occupancy()["live"]) == n
    out_a = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    out_b = torch.zeros(n * 16, dtype=torch.uint8, device=dev)

    def both(b, want_found):
        db = router.DeviceBatch.from_host(b, dev)
        send = torch.zeros(n * hiprl.ROUTE_RECORD_BYTES, dtype=torch.uint8, device=dev)
        x = torch.zeros(16, dtype=torch.int32, device=dev)
        perm = torch.zeros(n, dtype=torch.int32, device=dev)
        eng.route_pack_strided(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), 0, 1, n, send.data_ptr(), x.data_ptr(),
                               perm.data_ptr())
        torch.cuda.synchronize()
        assert x.cpu().tolist()[:2] == [n, 0]
        a_args = (db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), out_a.data_ptr())
        b_args = (send.data_ptr(), n, out_b.data_ptr())

        def timed(fn, args):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.burst):
                fn(*args)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.burst

        timed(eng.peek_device, a_args)
        timed(eng.peek_routed, b_args)
        ra = out_a.cpu().numpy().view(hiprl.PEEK_DTYPE)
        rb = out_b.cpu().numpy().view(hiprl.PEEK_DTYPE)[perm.cpu().numpy().view(np.uint32)]
        assert int((ra["flags"] & hiprl.PEEK_FOUND != 0).sum()) == (n if want_found else 0)
        assert ra.tobytes() == rb.tobytes(), "the two kernels disagree"
        ta, tb = [], []
        for _ in range(a.repeats):  # interleaved: each repeat times one kernel, then the other
            ta.append(timed(eng.peek_device, a_args))
            tb.append(timed(eng.peek_routed, b_args))

        def side(ts):
            return {"burst_call_us": round(statistics.median(ts) * 1e6, 1),
                    "lookups_per_s_burst": round(n / statistics.median(ts), 1),
                    "all_burst_us": [round(t * 1e6, 1) for t in ts]}
        return {"k_peek": side(ta), "k_peek_routed": side(tb),
                "routed_over_k_peek_time": round(statistics.median(tb) / statistics.median(ta), 3)}

    res = {"tool": "tools/routed_peek_probe.py", "records": n, "prefix_bytes": 16, "log2_slots": list(log2),
           "region_load": round(n / (1 << a.log2), 3), "repeats": a.repeats, "burst": a.burst,
           "prefill": "N keys of one HOUR window, one submit",
           "timing": "host clock around a burst of calls and a device synchronise; the two kernels alternate",
           "found": both(present, True), "absent": both(absent, False)}
    eng.close()
    del eng

    # ---- one Router.peek end to end ----
    G = a.shards
    engines = [new_engine() for _ in range(G)]
    rt = hiprl.Router(engines, max_desc=n, host=True, max_blob_bytes=16 * n)
    empty = hiprl.build_batch([])
    row = [present] + [empty] * (G - 1)
    rt.submit_host(row)
    rt.wait_into([(b.n_desc, b.n_req) for b in row])
    assert sum(sum(e.occupancy()["live"]) for e in engines) == n
    rep = rt.peek(row)  # untimed: allocates the call's buffers
    assert int((rep[0]["flags"] & hiprl.PEEK_FOUND != 0).sum()) == n
    ts = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt.peek(row)
        ts.append(time.perf_counter() - t0)
    res["router_peek"] = {"shards": G, "transport": "local", "descriptors": n, "origins_with_descriptors": 1,
                          "call_ms": round(statistics.median(ts) * 1e3, 2),
                          "lookups_per_s": round(n / statistics.median(ts), 1),
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
                "routed_found_burst_frac_of_rmw": round(res["found"]["k_peek_routed"]["lookups_per_s_burst"] / rmw.value, 3)}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
