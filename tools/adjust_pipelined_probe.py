#!/usr/bin/env python3
"""An adjust after every batch: waiting the pipeline out for rl_adjust against rl_adjust_pipelined
("Adjust in flight").

A config-3-like stream of N-descriptor device batches, two decision batches in flight, and after
every batch an adjust of M descriptors of that batch's keys (the refund / true-up of a cost
limiter: about one adjust per decision). In one process, the arms alternating round by round:

  serial     the batch is submitted, the pipeline is waited out (rl_wait until nothing is in flight)
             and the synchronous rl_adjust runs from host memory: what the engine offered before
  pipelined  the batch is submitted and rl_adjust_pipelined is queued behind it from device
             memory; the oldest flight is waited for only when RL_MAX_IN_FLIGHT are in flight
  plain      the same stream with no adjusts

as wall-clock ms per batch-plus-adjust pair (per batch for plain), then one timed round of the
pipelined arm for the two adjust kernels' shares of the kernel time (rl_kernel_times).

  python tools/adjust_pipelined_probe.py --out profiles/adjust_pipelined_probe.json
"""
import argparse
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
import workload  # noqa: E402

ADJUST_KERNELS = ["k_adjust_index", "k_adjust_apply"]


def head(b, m):
    """The first m descriptors of a one-descriptor-per-request batch."""
    return hiprl.Batch(b.blob[:int(b.off[m])].copy(), b.off[:m + 1].copy(), b.rule[:m].copy(),
                       np.arange(m, dtype=np.uint32), b.now[:m].copy(), b.hits[:m].copy())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="descriptors per batch")
    ap.add_argument("--m", type=int, default=100_000, help="descriptors per adjust")
    ap.add_argument("--batches", type=int, default=6, help="distinct batches, cycled")
    ap.add_argument("--steps", type=int, default=60, help="pairs per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    dev = torch.device("cuda", 0)
    # one time for every batch: the stream is cycled, and time must not run backwards
    hbs = [workload.config3_batch(k, d=a.n, batches_per_s=1 << 30) for k in range(a.batches)]
    habs = [head(hb, a.m) for hb in hbs]
    eng = hiprl.Engine(log2_slots=(22, 22, 23, 12), max_batch_desc=a.n, max_batch_req=a.n,
                       max_blob_bytes=max(int(hb.blob.shape[0]) for hb in hbs) + 64, pipeline="v4")
    eng.load_rules(workload.CONFIG3_RULES)
    dbs = [router.DeviceBatch.from_host(hb, dev) for hb in hbs]
    dabs = [router.DeviceBatch.from_host(hb, dev) for hb in habs]
    delta = np.full(a.m, -1, np.int32)
    d_delta = torch.from_numpy(delta).to(dev)
    outs = [torch.zeros(a.n * 20, dtype=torch.uint8, device=dev) for _ in range(3)]
    thrs = [torch.zeros(a.n, dtype=torch.int32, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    seq = [0]

    def submit(k):
        db, s = dbs[k % a.batches], seq[0] % 3
        seq[0] += 1
        eng.submit_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), outs[s].data_ptr(), thrs[s].data_ptr())

    def arm_plain(steps):
        fl = 0
        for k in range(steps):
            submit(k)
            fl += 1
            if fl == 2:
                eng.wait()
                fl -= 1
        for _ in range(fl):
            eng.wait()

    def arm_serial(steps):
        fl = 0
        for k in range(steps):
            submit(k)
            fl += 1
            while fl:  # rl_adjust needs nothing in flight
                eng.wait()
                fl -= 1
            eng.adjust(habs[k % a.batches], delta, want_out=False)

    def arm_pipelined(steps):
        fl = 0

        def room():
            nonlocal fl
            if fl == hiprl.MAX_IN_FLIGHT:
                eng.wait()
                fl -= 1

        for k in range(steps):
            room()
            submit(k)
            fl += 1
            room()
            ab = dabs[k % a.batches]
            eng.adjust_pipelined(ab.n_desc, ab.n_req, ab.blob_bytes(), ab.ptrs(), d_delta.data_ptr())
            fl += 1
        for _ in range(fl):
            eng.wait()

    arms = {"serial": arm_serial, "pipelined": arm_pipelined, "plain": arm_plain}

    def timed(f, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    for f in arms.values():  # untimed: the hot set forms, the scratch is allocated
        f(2 * a.batches)
    rounds = [{name: timed(f, a.steps) for name, f in arms.items()} for _ in range(a.rounds)]
    ms = {name: {"ms": round(statistics.median(r[name] for r in rounds), 4),
                 "all_ms": [round(r[name], 4) for r in rounds]} for name in arms}

    eng.set_timing(True)
    t0 = eng.kernel_times()
    arm_pipelined(a.batches)
    t1 = eng.kernel_times()
    eng.set_timing(False)
    kms = {k: t1[k][0] - t0.get(k, (0.0, 0))[0] for k in t1}
    tot = sum(kms.values())
    kernels = {k: {"us_per_pair": round(kms[k] / a.batches * 1e3, 1), "share": round(kms[k] / tot, 4)}
               for k in ADJUST_KERNELS}
    kernels["all_kernels_us_per_pair"] = round(tot / a.batches * 1e3, 1)

    res = {"tool": "tools/adjust_pipelined_probe.py", "descriptors_per_batch": a.n, "descriptors_per_adjust": a.m,
           "distinct_batches": a.batches, "steps_per_round": a.steps, "rounds": a.rounds, "batches_in_flight": 2,
           "timing": "host clock around each round, arms alternating in one process, device idle at both ends; "
                     "kernels: events around each launch (nothing overlaps while timed), one round of the pipelined arm",
           "ms_per_pair": ms,
           "pipelined_over_serial": round(ms["pipelined"]["ms"] / ms["serial"]["ms"], 3),
           "adjust_cost_ms": {"serial": round(ms["serial"]["ms"] - ms["plain"]["ms"], 4),
                              "pipelined": round(ms["pipelined"]["ms"] - ms["plain"]["ms"], 4)},
           "kernels": kernels, "stats": eng.stats()}
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
