#!/usr/bin/env python3
"""A refund behind every batch: rl_refund_pipelined against what it replaces.

A config-3-like stream of N-descriptor device batches, two decision batches in flight. The ranks
of RATES get rules of limit 1, so after the first batch every request on them is rejected: the
hot keys over their limit, at a rate the stream's history does not move. In one process, the arms
alternating round by round:

  a  no refund
  b  rl_refund_pipelined behind each batch
  c  the host path: the batch is waited for, its statuses are read back, the amounts are made on the
     host (numpy), and the deltas go down again as an rl_adjust_pipelined flight

as wall-clock ms per batch, at each rejection rate; then one timed round of b and of c for the
kernels' times (rl_kernel_times), and the box's device-to-device copy rate for the two streaming
passes' bytes.

  python tools/refund_probe.py --out profiles/refund_probe.json
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

# Zipf(1.1) over 1e8 keys: rank 1 alone holds about 5 % of the descriptors, ranks 0-9 about 30 %
RATES = {"0": [], "5": [1], "30": list(range(10))}
# bytes the two passes stream per descriptor: the status (20 B, of which the code word is used) in
# both; rule id, req_of, prefix offset, the request's time, hits and rej word in the second
STREAM_BYTES = 20 + 4 + 20 + 4 + 4 + 4 + 8 + 4 + 4


def batch_of(k, n, hot):
    """config3_batch(k) with the descriptors of the ranks in `hot` under rules 3-5 (limit 1)."""
    hb = workload.config3_batch(k, d=n, batches_per_s=1 << 30)
    if hot:
        rank = workload.Zipf(100_000_000, 1.1).sample(3, k, n) - 1
        sel = np.isin(rank, hot)
        hb.rule[sel] += 3
    return hb


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="descriptors per batch")
    ap.add_argument("--batches", type=int, default=4, help="distinct batches, cycled")
    ap.add_argument("--steps", type=int, default=40, help="batches per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    # the stream is cycled at one time, so config 3's own limits would soon reject every repeated
    # key: rules 0-2 never reject, rules 3-5 (the ranks of RATES) always do after their first hit
    rules = [(1 << 31, u) for _, u in workload.CONFIG3_RULES] + [(1, u) for _, u in workload.CONFIG3_RULES]

    # the box's copy rate: a device-to-device copy of 256 MiB, read + written bytes over its time
    src = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        dst.copy_(src)
    torch.cuda.synchronize()
    copy_gbs = 20 * 2 * (1 << 28) / (time.perf_counter() - t0) / 1e9
    del src, dst

    res = {"tool": "tools/refund_probe.py", "descriptors_per_batch": a.n, "distinct_batches": a.batches,
           "steps_per_round": a.steps, "rounds": a.rounds, "batches_in_flight": 2,
           "timing": "host clock around each round, arms alternating in one process, device idle at both ends; "
                     "kernels: events around each launch (nothing overlaps while timed), one round of the arm",
           "copy_rate_GBps": round(copy_gbs, 1), "streamed_bytes_per_descriptor": STREAM_BYTES,
           "streaming_passes_at_copy_rate_us": round(a.n * STREAM_BYTES / copy_gbs / 1e3, 1), "rates": {}}

    for name, hot in RATES.items():
        hbs = [batch_of(k, a.n, hot) for k in range(a.batches)]
        eng = hiprl.Engine(log2_slots=(22, 22, 23, 12), max_batch_desc=a.n, max_batch_req=a.n,
                           max_blob_bytes=max(int(hb.blob.shape[0]) for hb in hbs) + 64, pipeline="v4")
        eng.load_rules(rules)
        dbs = [router.DeviceBatch.from_host(hb, dev) for hb in hbs]
        outs = [torch.zeros(a.n * 20, dtype=torch.uint8, device=dev) for _ in range(3)]
        thrs = [torch.zeros(a.n, dtype=torch.int32, device=dev) for _ in range(3)]
        d_delta = torch.zeros(a.n, dtype=torch.int32, device=dev)
        h_st = torch.zeros(a.n * 20, dtype=torch.uint8).pin_memory()
        h_delta = torch.zeros(a.n, dtype=torch.int32).pin_memory()
        torch.cuda.synchronize()
        seq = [0]
        reports = []

        def submit(k):
            db, s = dbs[k % a.batches], seq[0] % 3
            seq[0] += 1
            eng.submit_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), outs[s].data_ptr(), thrs[s].data_ptr())
            return db, outs[s]

        def arm_a(steps):
            fl = 0
            for k in range(steps):
                submit(k)
                fl += 1
                if fl == 2:
                    eng.wait()
                    fl -= 1
            for _ in range(fl):
                eng.wait()

        def arm_b(steps):
            kinds = []

            def room():
                if len(kinds) == hiprl.MAX_IN_FLIGHT:
                    if kinds.pop(0) == "r":
                        reports.append(eng.wait_refund())
                    else:
                        eng.wait()

            for k in range(steps):
                room()
                db, out = submit(k)
                kinds.append("b")
                room()
                eng.refund_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), out.data_ptr())
                kinds.append("r")
            while kinds:
                if kinds.pop(0) == "r":
                    reports.append(eng.wait_refund())
                else:
                    eng.wait()

        def arm_c(steps):
            adj = False
            for k in range(steps):
                db, out = submit(k)
                if adj:
                    eng.wait()  # the previous batch's adjust
                eng.wait()
                hb = hbs[k % a.batches]
                h_st.copy_(out)  # 20 B per descriptor back; the copy synchronises
                st = h_st.numpy().view(hiprl.STATUS_DTYPE)
                cf = st["code_flags"]
                rej = np.zeros(hb.n_req, bool)
                rej[hb.req_of[(cf & 0xFF) == 2]] = True
                owed = rej[hb.req_of] & (hb.rule != hiprl.NIL_RULE) & ((cf >> 8) & 2 == 0)
                h_delta.numpy()[:] = -(np.maximum(hb.hits[hb.req_of], 1).astype(np.int64) * owed).astype(np.int32)
                d_delta.copy_(h_delta, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                eng.adjust_pipelined(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs(), d_delta.data_ptr())
                adj = True
            if adj:
                eng.wait()

        arms = {"a": arm_a, "b": arm_b, "c": arm_c}

        def timed(f, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(steps)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        for f in arms.values():  # untimed: the hot set forms, the scratch is allocated
            f(2 * a.batches)
        reports.clear()
        rounds = [{n_: timed(f, a.steps) for n_, f in arms.items()} for _ in range(a.rounds)]
        ms = {n_: {"ms": round(statistics.median(r[n_] for r in rounds), 4), "all_ms": [round(r[n_], 4) for r in rounds]}
              for n_ in arms}
        rate = sum(r["rejected_req"] for r in reports) / max(1, sum(r["descriptors"] for r in reports))

        kernels = {}
        for n_, f, names in (("b", arm_b, ["k_refund_mark", "k_refund_index", "k_adjust_apply"]),
                             ("c", arm_c, ["k_adjust_index", "k_adjust_apply"])):
            eng.set_timing(True)
            k0 = eng.kernel_times()
            f(a.batches)
            k1 = eng.kernel_times()
            eng.set_timing(False)
            kms = {k: k1[k][0] - k0.get(k, (0.0, 0))[0] for k in k1}
            tot = sum(kms.values())
            kernels[n_] = {k: {"us_per_batch": round(kms.get(k, 0.0) / a.batches * 1e3, 1),
                               "share": round(kms.get(k, 0.0) / tot, 4)} for k in names}
            kernels[n_]["refund_kernels_us_per_batch"] = round(sum(kms.get(k, 0.0) for k in names) / a.batches * 1e3, 1)
            kernels[n_]["all_kernels_us_per_batch"] = round(tot / a.batches * 1e3, 1)
        # The batcher's path: host batches (rl_submit: the H2D copy of one batch under the kernels of
        # the one before, statuses copied back), two decision batches in flight. `compact` is the
        # format the batcher sends without the option, `full` the one it must send with it (the
        # statuses stay on the device), `full_refund` that with rl_refund_behind behind each batch.
        cbs = [hiprl.compact_batch(hb) for hb in hbs]

        def host_arm(mode):
            def run(steps):
                kinds = []
                for k in range(steps):
                    while len(kinds) >= (2 if mode != "full_refund" else hiprl.MAX_IN_FLIGHT):
                        kinds.pop(0)
                        eng.wait()
                    if mode == "compact":
                        eng.submit_c(cbs[k % a.batches])
                    else:
                        eng.submit_host_async(hbs[k % a.batches])
                    kinds.append("b")
                    if mode == "full_refund":
                        if len(kinds) == hiprl.MAX_IN_FLIGHT:
                            kinds.pop(0)
                            eng.wait()
                        eng.refund_behind()
                        kinds.append("r")
                for _ in kinds:
                    eng.wait()
            return run

        harms = {m_: host_arm(m_) for m_ in ("compact", "full", "full_refund")}
        for f in harms.values():
            f(2 * a.batches)
        hrounds = [{n_: timed(f, a.steps) for n_, f in harms.items()} for _ in range(a.rounds)]
        host_ms = {n_: {"ms": round(statistics.median(r[n_] for r in hrounds), 4),
                        "all_ms": [round(r[n_], 4) for r in hrounds]} for n_ in harms}
        res["rates"][name] = {"rejected_share": round(rate, 4), "ms_per_batch": ms, "host_path_ms_per_batch": host_ms,
                              "refund_cost_ms": {"b": round(ms["b"]["ms"] - ms["a"]["ms"], 4),
                                                 "c": round(ms["c"]["ms"] - ms["a"]["ms"], 4)},
                              "kernels": kernels, "stats": eng.stats()}
        eng.close()
        del dbs, outs, thrs
        print(json.dumps({name: res["rates"][name]}), flush=True)

    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
