#!/usr/bin/env python3
"""k_rule_stats on this box ("Rule stats").

At N descriptors resident in device memory, with the statuses of a decided config-3 batch:

  kernel_us     k_rule_stats microseconds from rl_kernel_times (event pairs around each launch of
                rl_rule_stats_add_device, REPEATS launches after one untimed) for four rule mixes —
                one rule, config 3's three rules, 10^4 and 10^5 rules uniform — for each reduction
                variant (RL_DIAG_RULE_STATS_VARIANT: 0 = rule ids below 1024 summed in LDS, 1 =
                global adds only) and grid bound (RL_DIAG_RULE_STATS_BLOCKS)
  floor_us      28 B per descriptor at the box's copy rate (tools/microbench's probe)
  step_us       the depth-2 rl_submit_pipelined step on config-3 batches with RL_CFG_RULE_STATS off
                and on, two engines interleaved in rounds in one run, host clock per round

  python tools/rule_stats_probe.py --out profiles/rule_stats_probe.json
"""
import argparse
import ctypes as C
import json
import os
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
import workload  # noqa: E402

N_RULES = 100_000


def engine(n, rule_stats=False, variant=None, blocks=None):
    for k, v in (("RL_DIAG_RULE_STATS_VARIANT", variant), ("RL_DIAG_RULE_STATS_BLOCKS", blocks)):
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = str(v)  # read by rl_create
    return hiprl.Engine(log2_slots=(22, 22, 22, 16), max_batch_desc=n, max_batch_req=n, max_blob_bytes=n * 32 + 64,
                        rule_stats=rule_stats)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="descriptors per batch")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6, help="interleaved rounds per engine of the step A/B")
    ap.add_argument("--steps", type=int, default=24, help="steps per round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = a.n
    hbs = [workload.config3_batch(b, d=n, batches_per_s=4) for b in range(4)]
    dbs = [router.DeviceBatch.from_host(hb, dev) for hb in hbs]
    outs = [torch.zeros(n * 20, dtype=torch.uint8, device=dev) for _ in range(hiprl.MAX_IN_FLIGHT)]
    thrs = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(hiprl.MAX_IN_FLIGHT)]
    rng = np.random.default_rng(1)
    mixes = {"one_rule": np.zeros(n, np.uint32), "config3_three_rules": hbs[0].rule,
             "1e4_rules_uniform": rng.integers(0, 10_000, n).astype(np.uint32),
             "1e5_rules_uniform": rng.integers(0, N_RULES, n).astype(np.uint32)}
    d_mix = {k: torch.from_numpy(v.view(np.int32)).to(dev) for k, v in mixes.items()}
    res = {"tool": "tools/rule_stats_probe.py", "descriptors": n, "repeats": a.repeats,
           "statuses": "a decided config-3 batch (workload.config3_batch(0))", "kernel_us": {}}

    # ---- the kernel alone, per variant and grid bound ----
    for variant, blocks in ((0, 256), (1, 256), (0, 128), (0, 512)):
        e = engine(n, variant=variant, blocks=blocks)
        e.load_rules(workload.CONFIG3_RULES + [(100, hiprl.MINUTE)] * (N_RULES - 3))
        db = dbs[0]
        torch.cuda.synchronize()
        e.submit_device_async(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), outs[0].data_ptr(), thrs[0].data_ptr())
        e.wait()
        e.set_timing(True)
        row = {}
        for name, d_rule in d_mix.items():
            ptrs = [0, 0, d_rule.data_ptr(), db.req_of.data_ptr(), 0, db.hits.data_ptr(), 0]
            e.rule_stats_add_device(n, db.n_req, 0, ptrs, outs[0].data_ptr())  # untimed pass
            base = e.kernel_times()["k_rule_stats"]
            for _ in range(a.repeats):
                e.rule_stats_add_device(n, db.n_req, 0, ptrs, outs[0].data_ptr())
            ms, cnt = e.kernel_times()["k_rule_stats"]
            assert cnt - base[1] == a.repeats
            row[name] = round((ms - base[0]) / a.repeats * 1e3, 2)
        rows = e.rule_stats(0, N_RULES)
        assert int(rows["total_hits"].sum()) == 4 * (a.repeats + 1) * n  # config 3: hits_addend 1
        res["kernel_us"][f"variant{variant}_blocks{blocks}"] = row
        e.close()

    # ---- the box's copy rate: the kernel's floor ----
    lp = ROOT / "tools" / "microbench" / "libroofline_probe.so"
    if lp.exists():
        plib = C.CDLL(str(lp))
        plib.rl_probe_roofline.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]
        plib.rl_probe_roofline.restype = C.c_int
        gbs, rmw, rus = C.c_double(), C.c_double(), C.c_double()
        if plib.rl_probe_roofline(1 << 22, 1 << 20, C.byref(gbs), C.byref(rmw), C.byref(rus)) == 0:
            res["copy_GBps"] = round(gbs.value, 1)
            res["floor_us"] = round(28.0 * n / (gbs.value * 1e9) * 1e6, 2)

    # ---- the depth-2 pipelined step, flag off and on, interleaved ----
    engs = {}
    for flag in (False, True):
        e = engine(n, rule_stats=flag)
        e.load_rules(workload.CONFIG3_RULES)
        engs[flag] = e
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
                      "flag_off": [round(x, 1) for x in step[False]], "flag_on": [round(x, 1) for x in step[True]],
                      "flag_off_median": round(statistics.median(step[False]), 1),
                      "flag_on_median": round(statistics.median(step[True]), 1),
                      "fallbacks": {str(f): engs[f].stats()["lsd_fallbacks"] for f in engs}}
    assert int(engs[True].rule_stats()["total_hits"].sum()) == (16 + a.rounds * a.steps) * n
    assert engs[False].kernel_times()["k_rule_stats"][1] == 0
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
