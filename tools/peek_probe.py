#!/usr/bin/env python3
"""rl_peek_device rate of one engine on this box ("Peek").

Prefills an HOUR region (2^LOG2 slots) with N keys through one submit, then measures
rl_peek_device over N descriptors resident in device memory, REPEATS times each after one untimed
pass, in lookups/s:

  found    the N prefilled keys (every probe chain ends at the key's slot)
  absent   N keys never inserted (every chain ends at a free slot)

each as one call followed by a synchronise, and as BURST calls queued back to back before one
synchronise (the launch and the synchronise amortised). Beside them, what bounds a kernel of
random 32-B table reads on the same box: the random slot read-modify-write rate of bench.py
--full's probe (tools/microbench).

  python tools/peek_probe.py --n 1000000 --out profiles/peek_probe.json
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
import router  # noqa: E402


def keys(n, tag, now):
    """N one-entry descriptors of 16-byte prefixes under rule 0, one request."""
    blob = np.frombuffer("".join(f"pk_{tag}_{i:010d}_" for i in range(n)).encode(), np.uint8).copy()
    assert blob.shape[0] == 16 * n
    return hiprl.Batch(blob, (np.arange(n + 1, dtype=np.uint32) * 16).astype(np.uint32), np.zeros(n, np.uint32),
                       np.zeros(n, np.uint32), np.array([now], np.int64), np.ones(1, np.uint32))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="descriptors per peek (and prefilled keys)")
    ap.add_argument("--log2", type=int, default=22, help="log2 slots of each HOUR region")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    dev = torch.device("cuda", 0)
    now = 1_700_000_000
    eng = hiprl.Engine(log2_slots=(12, 12, a.log2, 12), local_cache=True, max_batch_desc=max(a.n, 4096),
                       max_blob_bytes=16 * max(a.n, 4096))
    eng.load_rules([(1 << 30, hiprl.HOUR)])
    present, absent = keys(a.n, "k", now), keys(a.n, "x", now + 1)
    eng.submit(present)
    occ = eng.occupancy()
    assert sum(occ["live"]) == a.n, occ
    out = torch.zeros(a.n * 16, dtype=torch.uint8, device=dev)

    def rate(b, want_found):
        db = router.DeviceBatch.from_host(b, dev)
        args = (db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), out.data_ptr())
        torch.cuda.synchronize()

        def timed(calls):
            t0 = time.perf_counter()
            for _ in range(calls):
                eng.peek_device(*args)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / calls

        timed(1)
        rep = out.cpu().numpy().view(hiprl.PEEK_DTYPE)
        assert int((rep["flags"] & hiprl.PEEK_FOUND != 0).sum()) == (a.n if want_found else 0)
        one = [timed(1) for _ in range(a.repeats)]
        burst = [timed(a.burst) for _ in range(a.repeats)]
        return {"one_call_us": round(statistics.median(one) * 1e6, 1),
                "burst_call_us": round(statistics.median(burst) * 1e6, 1),
                "lookups_per_s_one_call": round(a.n / statistics.median(one), 1),
                "lookups_per_s_burst": round(a.n / statistics.median(burst), 1),
                "all_burst_us": [round(x * 1e6, 1) for x in burst]}

    slots = 2 * (1 << a.log2) + 6 * (1 << 12)
    res = {"tool": "tools/peek_probe.py", "descriptors": a.n, "prefix_bytes": 16, "log2_slots": [12, 12, a.log2, 12],
           "region_load": round(a.n / (1 << a.log2), 3), "repeats": a.repeats, "burst": a.burst,
           "prefill": "N keys of one HOUR window, one submit", "timing": "host clock around the calls and a device synchronise",
           "found": rate(present, True), "absent": rate(absent, False)}
    del eng
    lp = ROOT / "tools" / "microbench" / "libroofline_probe.so"
    if lp.exists():  # the same probe bench.py --full runs: random 32-B slot RMW rate
        plib = C.CDLL(str(lp))
        plib.rl_probe_roofline.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]
        plib.rl_probe_roofline.restype = C.c_int
        gbs, rmw, rus = C.c_double(), C.c_double(), C.c_double()
        if plib.rl_probe_roofline(slots, 1 << 20, C.byref(gbs), C.byref(rmw), C.byref(rus)) == 0:
            res["bounds_same_box"] = {"slot_rmw_per_s": round(rmw.value, 1), "copy_GBps": round(gbs.value, 1),
                                      "found_burst_frac_of_rmw": round(res["found"]["lookups_per_s_burst"] / rmw.value, 3)}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
