"""An independent model of the decision and of serial DoLimit at the numeric-range edges.

Plain Python ints and numpy.float32, none of the project's C code: the second opinion that pins
the oracle (oracle/rl_oracle.cpp) where counters wrap at 2^32, limits pass 2^24 (float32 near
threshold) and times approach MAX_NOW. Restated from the reference:
  decide  src/limiter/base_limiter.go:70-177 (GetResponseDescriptorStatus, checkOverLimitThreshold,
          checkNearLimitThreshold) and utils.CalculateReset
  serial  src/redis/fixed_cache_impl.go:39-117 (every lookup of a request before its Sets, uint32
          INCRBY replies, EXPIRE div + jitter) with freecache TTL = div (base_limiter.go:102)
Also the shared edge vectors and streams of test_numeric_edges_cpu.py / test_gpu_numeric_edges.py.
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
MAX_NOW = 0xFFFD0000
SECOND, MINUTE, HOUR, DAY = 1, 2, 3, 4
DIV = {SECOND: 1, MINUTE: 60, HOUR: 3600, DAY: 86400}
NIL = 0xFFFFFFFF
OK, OVER = 1, 2
HAS_LIMIT, LOCAL_HIT = 1, 2
STATUS_DTYPE = np.dtype([("code_flags", "<u4"), ("limit_remaining", "<u4"), ("reset_s", "<u4"),
                         ("over_limit_delta", "<u4"), ("near_limit_delta", "<u4")])


def near_threshold(L, ratio):
    """uint32(math.Floor(float64(float32(L) * nearLimitRatio))), base_limiter.go:86; None when the
    float32 product does not fit uint32 (the conversion is then implementation-defined)."""
    p = float(np.float32(L) * np.float32(ratio))
    return int(p // 1) if p < 2.0 ** 32 else None


def decide(L, unit, ratio, now, h, after, local_hit):
    """-> (code_flags, limit_remaining, reset_s, over_limit_delta, near_limit_delta, throttle_ms)
    of a descriptor with a limit whose INCRBY replied `after` (uint32) for `h` hits."""
    div = DIV[unit]
    reset = div - now % div
    if local_hit:  # :76-81
        return (OVER | (HAS_LIMIT | LOCAL_HIT) << 8, 0, reset, h, 0, 0)
    near = near_threshold(L, ratio)
    before = (after - h) & M32  # fixed_cache_impl.go:110, uint32
    if after > L:  # :88
        if before >= L:  # :135
            over, nr = h, 0
        else:
            over, nr = after - L, (L - max(near, before)) & M32  # uint32: near > L once float32(L) rounds up
        return (OVER | HAS_LIMIT << 8, 0, reset, over, nr, 0)
    thr = nr = 0
    if after > near:  # :155
        end = now // div * div + div
        millis = ((end - now) & M32) * 1000 & M32
        thr = millis // max(L - after, 1)
        nr = h if before >= near else after - near
    return (OK | HAS_LIMIT << 8, L - after, reset, 0, nr, thr)


def prefix(domain, entries):
    return domain + "_" + "".join(f"{k}_{v}_" for k, v in entries)


def serial(reqs, rules, ratio, local_cache, jit=None):
    """reqs: hiprl.build_batch's tuples (domain, [entries...], [rule id | NIL...], hits_addend, now)
    in serial order; jit: EXPIRE jitter per descriptor (flat) or None. -> (statuses, throttles)."""
    redis, cache = {}, {}
    st = np.zeros(sum(len(r[1]) for r in reqs), STATUS_DTYPE)
    thr = np.zeros(len(reqs), np.uint32)
    d0 = 0
    for q, (dom, descs, rids, ha, now) in enumerate(reqs):
        h = max(1, ha)
        keys = [None if r == NIL else prefix(dom, e) + str(now // DIV[rules[r][1]] * DIV[rules[r][1]])
                for e, r in zip(descs, rids)]
        hit = [k is not None and local_cache and cache.get(k, 0) > now for k in keys]
        after = [0] * len(keys)
        for i, k in enumerate(keys):
            if k is None or hit[i]:
                continue
            c = redis.get(k)
            n = (c[0] if c and now < c[1] else 0) + h
            redis[k] = (n, now + DIV[rules[rids[i]][1]] + (int(jit[d0 + i]) if jit is not None else 0))
            after[i] = n & M32
        t = 0
        for i, k in enumerate(keys):
            if k is None:
                st[d0 + i] = (OK, 0, 0, 0, 0)
                continue
            L, unit = rules[rids[i]][:2]
            s = decide(L, unit, ratio, now, h, after[i], hit[i])
            st[d0 + i] = s[:5]
            t = max(t, s[5])
            if local_cache and not hit[i] and after[i] > L:
                cache[k] = now + DIV[unit]
        thr[q] = t
        d0 += len(keys)
    return st, thr


# ---- the shared edge vectors and streams -----------------------------------------------------------
GRID_L = [0, 1, 2, 5, 10, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2,
          2 ** 32 - 1]
GRID_RATIO = [0.0, 0.5, 0.8, 0.999, 1.0]
# every unit, at times up to MAX_NOW: a window's first and last second, both sides of 2^31
GRID_UNIT_NOW = [(SECOND, 0), (MINUTE, 59), (HOUR, 3600), (DAY, 86399), (SECOND, 0x7FFFFFFF), (MINUTE, 0x80000000),
                 (HOUR, MAX_NOW - 1), (DAY, MAX_NOW), (SECOND, MAX_NOW), (DAY, 1_700_000_000)]
PALETTE = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFF0, 0xFFFFFFFF]
EDGE_TIMES = [0, 1, 59, 60, 61, 3599, 3600, 3601, 86399, 86400, 86401, 0x7FFFFFFF, 0x80000000, MAX_NOW - 1, MAX_NOW]
EDGE_RULES = [(2 ** 32 - 1, SECOND), (0xFFFFFFF0, SECOND), (40, SECOND), (0, SECOND), (2 ** 24 + 1, MINUTE),
              (2 ** 31, HOUR), (2 ** 32 - 1, DAY), (2 ** 32 - 1, MINUTE)]


def grid(ratios=GRID_RATIO):
    """The decide vectors: dicts of L, unit, ratio, now, hits, after, local_hit. The (L, ratio)
    pairs whose near threshold does not fit uint32 are left out."""
    out = []
    for ratio in ratios:
        for L in GRID_L:
            near = near_threshold(L, ratio)
            if near is None:
                continue
            afters = sorted({a for a in (0, 1, 2, near - 1, near, near + 1, L - 1, L, L + 1, M32 - 1, M32)
                             if 0 <= a <= M32})
            hs = sorted({max(1, x) for x in (1, 2, 3, L, 2 ** 31, M32)})
            for after in afters:
                for h in hs:
                    for unit, now in GRID_UNIT_NOW:
                        out.append(dict(L=L, unit=unit, ratio=ratio, now=now, hits=h, after=after, local_hit=False))
            for h in hs:
                for unit, now in GRID_UNIT_NOW:
                    out.append(dict(L=L, unit=unit, ratio=ratio, now=now, hits=h, after=0, local_hit=True))
    return out


def day_stream(seed=7, n=4000, t0=86400 * 19676 - 40):
    """n requests over 12 prefixes under EDGE_RULES, hits from the palette and 16, 1-3 descriptors
    each (a string under two units among them), ~80 s across a day boundary."""
    rng = np.random.default_rng(seed)
    pal = PALETTE + [16]
    reqs, t = [], t0
    for i in range(n):
        t += int(rng.random() < 0.02)
        nd = 1 + int(rng.integers(0, 3))
        descs, rids = [], []
        for _ in range(nd):
            k = int(rng.integers(0, 12))
            descs.append([("k", str(k))])
            rids.append(NIL if rng.random() < 0.03 else (k + (7 if rng.random() < 0.1 else 0)) % len(EDGE_RULES))
        reqs.append(("edge", descs, rids, pal[i % len(pal)], t))
    return reqs


def time_batches():
    """One batch per edge time: 12 requests of two descriptors over the four units."""
    rules = [(3, SECOND), (5, MINUTE), (2 ** 32 - 1, HOUR), (7, DAY)]
    out = []
    for t in EDGE_TIMES:
        out.append([("tm", [[("a", str(i % 5))], [("b", str(i % 3))]], [i % 4, (i + 1 + i // 4) % 4],
                     PALETTE[i % 6] if i % 4 == 2 else i % 3, t) for i in range(12)])
    return rules, out


def jitter_stream():
    """-> (rules, batches, jitter per batch): the largest EXPIRE jitter on a DAY rule in the last
    admissible hour. exp = MAX_NOW + 86400 + 65535 = 0xFFFF517F still fits uint32 (what MAX_NOW is
    for). A MINUTE rule's string of the hour's first minute, kept alive by its jitter, is found
    65 s later by the HOUR rule that shares it; the last batch, at MAX_NOW, finds the DAY key."""
    rules = [(2 ** 32 - 1, DAY), (5, MINUTE), (5, HOUR)]
    th = MAX_NOW // 3600 * 3600
    assert MAX_NOW + 86400 + 65535 < 2 ** 32 and th // 86400 == MAX_NOW // 86400
    batches = [[("j", [[("k", "d")], [("k", "m")]], [0, 1], 0xFFFFFFFF, th)],
               [("j", [[("k", "d")], [("k", "m")]], [0, 2], 3, th + 65)],
               [("j", [[("k", "d")]], [0], 2, MAX_NOW)]]
    return rules, batches, [[65535, 65535], [65535, 0], [65535]]


def wrapped(st, rules, rule_ids, keys):
    """Proof of a wrap from reference outputs alone: for some key under a limit of 2^32 - 1,
    after = L - limit_remaining decreases somewhere along its arrival order. keys: a hashable per
    descriptor naming its counter."""
    last = {}
    for i, (r, k) in enumerate(zip(rule_ids, keys)):
        if r == NIL or rules[r][0] != M32 or (int(st["code_flags"][i]) >> 8) & LOCAL_HIT:
            continue
        after = M32 - int(st["limit_remaining"][i])
        if k in last and after < last[k]:
            return True
        last[k] = after
    return False
