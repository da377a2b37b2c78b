#!/usr/bin/env python3
"""What a hot set that is one probe chain of the LDS tag table costs k4_hist.

hot_home / hot_tag (rl_common.h) read bits 0..10 and 41..63 of the prefix lane a, and a
difference confined to byte 6 of a prefix's last 8-byte word moves only bits 17..24 of it: the
256 prefixes stem6 + bytes([v]) + b"_" share one home and one tag, so a set made of them is a
chain of 256 equal tag words and a member's lookup walks to its own place in it, confirming
every word on the way on the full (a, b).

The workload is config-3-like: N descriptors per batch, one per request, h = 1, local cache on,
rules by key % 3 (SECOND 10 / MINUTE 600 / HOUR 36000), --hot-share of the descriptors on 256
hot prefixes with Zipf(1.1) weights among themselves (the least frequent still has > 128 per
batch), the rest uniform over 1e7 cold keys, four batches per second. Two engines, one fed
`spread` hot prefixes (the id outside the last word: 256 places in the table), one `clustered`
ones, each warmed until its set holds the 256; then, alternating between the two in one process:

  step_us   the depth-2 rl_submit_pipelined step, host clock, ROUNDS rounds of STEPS steps
  kernel_us per-kernel microseconds per batch from rl_kernel_times (rl_set_timing on, one batch
            in flight), REPEATS rounds of 4 batches

  python tools/hot_cluster_probe.py --out profiles/hot_cluster_probe.json
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

HOT = 256
FAMILIES = {
    "spread": [b"hs_k_%d_tail_" % i for i in range(HOT)],
    "clustered": [b"hsclu_" + bytes([v]) + b"_" for v in range(HOT)],
}


def spread_of(xs, nd=2):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd),
            "all": [round(x, nd) for x in xs]}


def batch(family, b, n, hot_share, seed=11, n_cold=10_000_000, t0=1_700_000_000):
    """Batch b of the workload: the same draw for both families, only the hot prefixes' bytes differ."""
    rng = np.random.default_rng(seed * 1000 + b)
    w = np.arange(1, HOT + 1, dtype=np.float64) ** -1.1
    is_hot = rng.random(n) < hot_share
    hot_id = rng.choice(HOT, n, p=w / w.sum())
    cold_id = rng.integers(0, n_cold, n).astype(np.uint64)
    cblob, coff = workload.prefix_blob([b"bench_k_", cold_id, b"_"])
    hp = FAMILIES[family]
    width = max(len(p) for p in hp)
    table = np.zeros((HOT, width), np.uint8)
    for i, p in enumerate(hp):
        table[i, :len(p)] = np.frombuffer(p, np.uint8)
    hlen = np.array([len(p) for p in hp], np.int64)
    coff = coff.astype(np.int64)
    lens = np.where(is_hot, hlen[hot_id], coff[1:] - coff[:-1])
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    row = np.repeat(np.arange(n), lens)
    pos = np.arange(int(off[-1])) - off[row]
    blob = np.zeros(int(off[-1]) + hiprl.BLOB_SLACK, np.uint8)
    hot_b = is_hot[row]
    blob[:int(off[-1])] = np.where(hot_b, table[hot_id[row], np.minimum(pos, width - 1)],
                                   cblob[np.minimum(coff[row] + pos, len(cblob) - 1)])
    key = np.where(is_hot, hot_id, cold_id.astype(np.int64))
    return hiprl.Batch(blob, off.astype(np.uint32), (key % 3).astype(np.uint32), np.arange(n, dtype=np.uint32),
                       np.full(n, t0 + b // 4, np.int64), np.ones(n, np.uint32)), int(is_hot.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000, help="descriptors per batch")
    ap.add_argument("--hot-share", type=float, default=0.55)
    ap.add_argument("--warm", type=int, default=24, help="warm-up steps per engine")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=24, help="steps per round of the step timing")
    ap.add_argument("--repeats", type=int, default=6, help="rounds of 4 batches of the kernel timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hot_cluster_probe: no GPU (the probe measures; it has no CPU fall-back)")
    dev = torch.device("cuda", 0)
    n = a.n
    NB = 4
    names = list(FAMILIES)
    dbs, sbs, hot_desc = {}, {}, {}
    for f in names:
        hb = [batch(f, b, n, a.hot_share) for b in range(NB)]
        hot_desc[f] = [h for _, h in hb]
        dbs[f] = [router.DeviceBatch.from_host(x, dev) for x, _ in hb]
        sbs[f] = [hiprl.Engine.device_batch(db.n_desc, db.n_req, db.blob_bytes(), db.ptrs()) for db in dbs[f]]
    outs = [torch.zeros(n * 20, dtype=torch.uint8, device=dev) for _ in range(hiprl.MAX_IN_FLIGHT)]
    thrs = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(hiprl.MAX_IN_FLIGHT)]
    engs = {}
    for f in names:
        e = hiprl.Engine(log2_slots=(22, 22, 22, 16), max_batch_desc=n, max_batch_req=n, max_blob_bytes=n * 32 + 64,
                         local_cache=True)
        e.load_rules(workload.CONFIG3_RULES)
        engs[f] = e

    def run(f, steps, depth=2):
        e, pend = engs[f], 0
        for j in range(steps):
            e.submit_pipelined_batch(sbs[f][j % NB], outs[j % 3].data_ptr(), thrs[j % 3].data_ptr())
            pend += 1
            if pend == depth:
                e.wait()
                pend -= 1
        for _ in range(pend):
            e.wait()

    torch.cuda.synchronize()
    for f in names:
        run(f, a.warm)
    warm_stats = {f: engs[f].stats() for f in names}
    for f in names:
        assert warm_stats[f]["hot_keys"] == HOT, (f, warm_stats[f])
    # the same decisions either way: the two engines' last outputs of one batch index agree
    same = []
    for f in names:
        run(f, 1, depth=1)
        torch.cuda.synchronize()
        same.append(outs[0].cpu().numpy().copy())
    assert np.array_equal(same[0], same[1]), "spread and clustered hot prefixes gave different statuses"

    step = {f: [] for f in names}
    for _ in range(a.rounds):
        for f in names:
            t0 = time.perf_counter()
            run(f, a.steps)
            step[f].append((time.perf_counter() - t0) / a.steps * 1e6)

    kern = {f: {} for f in names}
    for f in names:
        engs[f].set_timing(True)
        run(f, NB, depth=1)  # untimed pass with the marks on
    for _ in range(a.repeats):
        for f in names:
            base = engs[f].kernel_times()
            run(f, NB, depth=1)
            for k, (ms, cnt) in engs[f].kernel_times().items():
                b_ms, b_cnt = base.get(k, (0.0, 0))
                if cnt > b_cnt:
                    kern[f].setdefault(k, []).append((ms - b_ms) / (cnt - b_cnt) * 1e3)
    end_stats = {f: engs[f].stats() for f in names}
    for f in names:
        assert end_stats[f]["hot_keys"] == HOT and end_stats[f]["lsd_fallbacks"] == warm_stats[f]["lsd_fallbacks"], end_stats
        engs[f].close()

    res = {"tool": "tools/hot_cluster_probe.py", "descriptors": n, "hot_share": a.hot_share, "hot_prefixes": HOT,
           "hot_descriptors_per_batch": hot_desc["spread"], "batches": NB, "local_cache": True,
           "order": "spread, clustered, alternating in one process",
           "same_statuses": True,
           "fallbacks": {f: end_stats[f]["lsd_fallbacks"] for f in names},
           "step_us": {"depth": 2, "rounds": a.rounds, "steps_per_round": a.steps,
                       **{f: spread_of(step[f], 1) for f in names}},
           "kernel_us": {f: {k: spread_of(v) for k, v in sorted(kern[f].items())} for f in names}}
    hs, hc_ = (statistics.median(kern[f]["k4_hist"]) for f in names)
    res["k4_hist_us"] = {"spread": round(hs, 2), "clustered": round(hc_, 2), "ratio": round(hc_ / hs, 3)}
    ss, sc = (statistics.median(step[f]) for f in names)
    res["step_ratio"] = round(sc / ss, 3)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
