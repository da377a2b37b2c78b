#!/usr/bin/env python3
"""rl_census and k_cache_stats on this box ("Census and lookup counters").

  census        on a table of 2^LOG2 slots per SECOND / MINUTE / HOUR region, prefilled to LOAD as
                tools/snapshot_probe.py prefills it: the pause of rl_census and of
                rl_snapshot_begin (host clock around the synchronous call), REPEATS times each,
                alternating, after one untimed pass of both; k_census alone from rl_kernel_times;
                and the box's copy rate (tools/microbench's probe) for the bytes the pass reads
  kernel_us     k_cache_stats and k_rule_stats microseconds from rl_kernel_times at N descriptors
                on the statuses of a decided config-3 batch, alternating, and the floor of 8 B per
                descriptor at the copy rate
  step_us       the depth-2 rl_submit_pipelined step on config-3 batches (local cache on) with
                RL_CFG_CACHE_STATS off and on, two engines interleaved in rounds, host clock

  python tools/census_probe.py --log2 24 --out profiles/census_probe.json
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
import workload  # noqa: E402
from snapshot_probe import synthetic  # noqa: E402


def spread(xs, nd=3):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd),
            "all": [round(x, nd) for x in xs]}


def copy_rate(slots):
    lp = ROOT / "tools" / "microbench" / "libroofline_probe.so"
    if not lp.exists():
        return None
    plib = C.CDLL(str(lp))
    plib.rl_probe_roofline.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double)]
    plib.rl_probe_roofline.restype = C.c_int
    gbs, rate, rus = C.c_double(), C.c_double(), C.c_double()
    if plib.rl_probe_roofline(slots, 1 << 20, C.byref(gbs), C.byref(rate), C.byref(rus)):
        return None
    return gbs.value


def probe_census(a):
    eng = hiprl.Engine(log2_slots=(a.log2, a.log2, a.log2, 12), local_cache=True, max_batch_desc=4096)
    h, recs = synthetic(a.log2, a.load, eng, np.random.default_rng(1))
    recs["frz"][::3] = 1_700_000_000  # a third of the strings frozen until their expiry
    eng.restore_records(h, recs, chunk=1 << 20)
    n = recs.shape[0]
    slots = 6 * (1 << a.log2) + 2 * (1 << 12)
    now = 1_699_999_990

    def snap():
        t0 = time.perf_counter()
        hh = eng.snapshot_begin()
        dt = time.perf_counter() - t0
        eng.snapshot_end()
        assert hh.n_records == n
        return dt * 1e3

    def census():
        t0 = time.perf_counter()
        rep = eng.census(now)
        dt = time.perf_counter() - t0
        assert int(rep["live"].sum()) == int(rep["keys_main"].sum()) == n, (rep["live"], n)
        assert int(rep["cached"].sum()) == (n + 2) // 3
        return dt * 1e3

    snap(), census()
    s_ms, c_ms = [], []
    for _ in range(a.repeats):
        s_ms.append(snap())
        c_ms.append(census())
    eng.set_timing(True)
    census()
    base = eng.kernel_times()["k_census"]
    for _ in range(a.repeats):
        census()
    ms, cnt = eng.kernel_times()["k_census"]
    k_ms = (ms - base[0]) / (cnt - base[1])
    eng.close()
    res = {"log2_slots": [a.log2, a.log2, a.log2, 12], "table_slots": slots, "table_GiB": round(slots * 32 / 2**30, 3),
           "records": n, "load": a.load, "repeats": a.repeats, "order": "snapshot_begin, census, alternating",
           "census_pause_ms": spread(c_ms), "snapshot_begin_pause_ms": spread(s_ms),
           "k_census_ms": round(k_ms, 3), "k_census_read_GBps": round(slots * 32 / k_ms / 1e6, 1),
           "census_minus_snapshot_median_ms": round(statistics.median(c_ms) - statistics.median(s_ms), 3),
           "snapshot_min_max_spread_ms": round(max(s_ms) - min(s_ms), 3)}
    gbs = copy_rate(slots)
    if gbs:
        res["copy_GBps"] = round(gbs, 1)
        res["table_read_at_copy_rate_ms"] = round(slots * 32 / (gbs * 1e9) * 1e3, 3)
    return res


def probe_kernels_and_step(a):
    dev = torch.device("cuda", 0)
    n = a.n
    hbs = [workload.config3_batch(b, d=n, batches_per_s=4) for b in range(4)]
    dbs = [router.DeviceBatch.from_host(hb, dev) for hb in hbs]
    outs = [torch.zeros(n * 20, dtype=torch.uint8, device=dev) for _ in range(hiprl.MAX_IN_FLIGHT)]
    thrs = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(hiprl.MAX_IN_FLIGHT)]

    def engine(**kw):
        e = hiprl.Engine(log2_slots=(22, 22, 22, 16), max_batch_desc=n, max_batch_req=n, max_blob_bytes=n * 32 + 64,
                         local_cache=True, **kw)
        e.load_rules(workload.CONFIG3_RULES)
        return e

    # ---- the two counting kernels alone, alternating ----
    e = engine()
    db = dbs[0]
    torch.cuda.synchronize()
    e.submit_device_async(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), outs[0].data_ptr(), thrs[0].data_ptr())
    e.wait()
    e.set_timing(True)
    us = {"k_cache_stats": [], "k_rule_stats": []}
    calls = {"k_cache_stats": e.cache_stats_add_device, "k_rule_stats": e.rule_stats_add_device}
    for rep in range(a.repeats + 1):
        for name, call in calls.items():
            base = e.kernel_times()[name]
            call(db.n_desc, db.n_req, 0, db.ptrs(), outs[0].data_ptr())
            ms, cnt = e.kernel_times()[name]
            assert cnt - base[1] == 1
            if rep:  # the first pass is untimed
                us[name].append((ms - base[0]) * 1e3)
    cs = e.cache_stats()
    assert cs["lookups"] == (a.repeats + 1) * n, cs
    e.close()
    res = {"descriptors": n, "statuses": "a decided config-3 batch (workload.config3_batch(0)), local cache on",
           "local_cache_hits_per_batch": cs["hits"] // (a.repeats + 1),
           "kernel_us": {k: spread(v, 2) for k, v in us.items()}}
    gbs = copy_rate(1 << 22)
    if gbs:
        res["copy_GBps"] = round(gbs, 1)
        res["floor_us_8B_per_descriptor"] = round(8.0 * n / (gbs * 1e9) * 1e6, 2)

    # ---- the depth-2 pipelined step, flag off and on, interleaved ----
    engs = {flag: engine(cache_stats=flag) for flag in (False, True)}
    sbs = [hiprl.Engine.device_batch(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs()) for db in dbs]

    def run(e, steps):
        pend = 0
        for j in range(steps):
            e.submit_pipelined_batch(sbs[j % len(sbs)], outs[j % 3].data_ptr(), thrs[j % 3].data_ptr())
            pend += 1
            if pend == 2:
                e.wait()
                pend -= 1
        for _ in range(pend):
            e.wait()

    torch.cuda.synchronize()
    for e in engs.values():
        run(e, 16)  # the hot set forms, the first batch's fallback is behind
    step = {False: [], True: []}
    for _ in range(a.rounds):
        for flag in (False, True):
            t0 = time.perf_counter()
            run(engs[flag], a.steps)
            step[flag].append((time.perf_counter() - t0) / a.steps * 1e6)
    res["step_us"] = {"depth": 2, "rounds": a.rounds, "steps_per_round": a.steps,
                      "flag_off": spread(step[False], 1), "flag_on": spread(step[True], 1),
                      "fallbacks": {str(f): engs[f].stats()["lsd_fallbacks"] for f in engs}}
    assert engs[True].cache_stats()["lookups"] == (16 + a.rounds * a.steps) * n
    assert engs[False].cache_stats()["lookups"] == 0 and engs[False].kernel_times()["k_cache_stats"][1] == 0
    for e in engs.values():
        e.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, default=24, help="log2 slots of each SECOND/MINUTE/HOUR region")
    ap.add_argument("--load", type=float, default=0.23)
    ap.add_argument("--n", type=int, default=1_000_000, help="descriptors per batch")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=6, help="interleaved rounds per engine of the step A/B")
    ap.add_argument("--steps", type=int, default=24, help="steps per round")
    ap.add_argument("--census-only", action="store_true", help="skip the counter kernels and the step A/B")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "tools/census_probe.py", "census": probe_census(a)}
    if not a.census_only:
        res["counters"] = probe_kernels_and_step(a)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
