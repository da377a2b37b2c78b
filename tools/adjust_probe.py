#!/usr/bin/env python3
"""rl_adjust cost of one engine on this box ("Adjust").

rl_adjust of N descriptors (host call: staging, k_adjust_index with its replies, k_adjust_apply, the
control block's and the replies' read-back) on a table prefilled by rl_set, in three cases, each
REPEATS times after one untimed round, interleaved in every round with rl_peek and rl_set of the
same batch:

  found      every counter is found
  half       every other string is absent from the table
  dup50      the second half of the call repeats the first half's keys

as wall-clock µs per call and keys/s, then one round with the engine's kernel timing on for the two
kernels' shares. The yardstick is rl_set of the same batch over the same table in the same round
(every string found: the same index and apply work, plus planning). Beside them the random 32-B
slot read-modify-write rate of bench.py --full's probe (tools/microbench).

  python tools/adjust_probe.py --n 1000000 --out profiles/adjust_probe.json
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

ADJUST_KERNELS = ["k_adjust_index", "k_adjust_apply"]


def keys(n, now, distinct=None, tag="ak"):
    """N one-entry descriptors of 16-byte prefixes under rule 0, one request; the keys repeat
    after `distinct`."""
    distinct = distinct or n
    blob = np.frombuffer("".join(f"{tag}_k_{i % distinct:010d}_" for i in range(n)).encode(), np.uint8).copy()
    assert blob.shape[0] == 16 * n
    return hiprl.Batch(blob, (np.arange(n + 1, dtype=np.uint32) * 16).astype(np.uint32), np.zeros(n, np.uint32),
                       np.zeros(n, np.uint32), np.array([now], np.int64), np.ones(1, np.uint32))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="descriptors per call")
    ap.add_argument("--log2", type=int, default=22, help="log2 slots of each HOUR region")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    now = 1_700_000_000
    rules = [(1 << 30, hiprl.HOUR)]
    eng = hiprl.Engine(log2_slots=(12, 12, a.log2, 12), local_cache=True, max_batch_desc=max(a.n, 4096),
                       max_blob_bytes=16 * max(a.n, 4096))
    eng.load_rules(rules)
    b, bdup = keys(a.n, now), keys(a.n, now, a.n // 2)
    # every other string of bhalf is one the table never held
    bhalf = keys(a.n, now)
    blob = bhalf.blob.reshape(a.n, 16).copy()
    blob[1::2, 0] = ord("z")
    bhalf = hiprl.Batch(blob.reshape(-1), bhalf.off, bhalf.rule, bhalf.req_of, bhalf.now, bhalf.hits)
    v = np.zeros(a.n, hiprl.PEEK_DTYPE)
    v["count"], v["ttl_s"], v["flags"] = 1000, 3000, hiprl.PEEK_FOUND
    rng = np.random.default_rng(1)
    up, down = rng.integers(1, 100, a.n).astype(np.int32), -rng.integers(1, 100, a.n).astype(np.int32)

    def timed(f, *args, **kw):
        t0 = time.perf_counter()
        r = f(*args, **kw)
        return time.perf_counter() - t0, r

    eng.set(b, v, want_out=False)
    assert sum(eng.occupancy()["live"]) == a.n

    def round_():
        out = {}
        out["set_overwrite"], _ = timed(eng.set, b, v)
        out["adjust_found"], (_, rep) = timed(eng.adjust, b, down)
        assert rep["applied"] == a.n and rep["floored"] == 0
        out["peek"], _ = timed(eng.peek, b)
        out["adjust_found_no_out"], _ = timed(eng.adjust, b, up, want_out=False)
        out["adjust_half"], (_, rep) = timed(eng.adjust, bhalf, down)
        assert (rep["applied"], rep["absent"]) == (a.n - a.n // 2, a.n // 2)
        out["set_overwrite_no_out"], _ = timed(eng.set, b, v, want_out=False)
        out["adjust_dup50"], (_, rep) = timed(eng.adjust, bdup, down)
        assert rep["applied"] == a.n
        assert sum(eng.occupancy()["live"]) == a.n
        return out

    round_()
    rounds = [round_() for _ in range(a.repeats)]
    calls = {}
    for k in rounds[0]:
        med = statistics.median(r[k] for r in rounds)
        calls[k] = {"us": round(med * 1e6, 1), "keys_per_s": round(a.n / med, 1),
                    "all_us": [round(r[k] * 1e6, 1) for r in rounds]}

    # one round with the kernels timed (events around each launch)
    eng.set_timing(True)
    kernels = {}

    def shares(name, f):
        t0 = {k: eng.kernel_times()[k][0] for k in ADJUST_KERNELS}
        f()
        ms = {k: eng.kernel_times()[k][0] - t0[k] for k in ADJUST_KERNELS}
        tot = sum(ms.values())
        kernels[name] = {k: {"us": round(ms[k] * 1e3, 1), "share": round(ms[k] / tot, 3)} for k in ADJUST_KERNELS}
        kernels[name]["kernels_us"] = round(tot * 1e3, 1)

    eng.set(b, v, want_out=False)
    shares("adjust_found", lambda: eng.adjust(b, down, want_out=False))
    shares("adjust_half", lambda: eng.adjust(bhalf, down, want_out=False))
    shares("adjust_dup50", lambda: eng.adjust(bdup, down, want_out=False))
    eng.set_timing(False)

    slots = 2 * (1 << a.log2) + 6 * (1 << 12)
    res = {"tool": "tools/adjust_probe.py", "descriptors": a.n, "prefix_bytes": 16, "log2_slots": [12, 12, a.log2, 12],
           "region_load": round(a.n / (1 << a.log2), 3), "repeats": a.repeats,
           "timing": "host clock around each synchronous host call (staging and read-backs included); kernels: "
                     "events around each launch, one round",
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
