"""A dict model of rl_adjust (rl_hip.h "Adjust"): from what rl_peek answered just before the call,
the deltas and the rules, what rl_peek answers just after it and the call's report. The oracle has
no such command; this is the contract restated in a few lines of Python, checked by hand-written
cases in test_adjust_cpu.py and held against the device in test_gpu_adjust.py.

A descriptor's key string is named by any hashable value (`string_of` below gives the string
itself); its store is read off the reply's PER_SECOND flag. The model sees deadlines only through
LOCAL_CACHED, so `unfrozen` is exact when no string of the call carries an expired, non-zero
deadline (none does after a forget, a set to "no entry" or before the first freeze)."""
import numpy as np

import hiprl

F, LC, NILF, PS = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND
U32 = 0xFFFFFFFF


def string_of(prefix: bytes, unit: int, t: int) -> bytes:
    """GenerateCacheKey: prefix || decimal window start of t under the unit."""
    d = hiprl.UNIT_DIVIDER[unit]
    return prefix + str(t // d * d).encode()


def adjust_model(strings, before, deltas, limits, local_cache=False, keep_cache=False):
    """strings[i]: descriptor i's key string (None: a nil descriptor); before: rl_peek's replies just
    before the call (PEEK_DTYPE); deltas[i]: its int32 correction; limits[i]: its rule's
    requests_per_unit. -> (rl_peek's replies just after the call, the report as a dict)."""
    n = len(strings)
    assert len(before) == len(deltas) == len(limits) == n
    rep = dict.fromkeys(hiprl.ADJUST_REPORT_FIELDS, 0)
    rep["descriptors"] = n
    pairs = {}  # (string, per-second) -> [count before, net, smallest limit]
    for i in range(n):
        fl = int(before[i]["flags"])
        if strings[i] is None:
            assert fl & NILF
            rep["nil"] += 1
        elif not fl & F:
            rep["absent"] += 1
        else:
            rep["applied"] += 1
            p = pairs.setdefault((strings[i], bool(fl & PS)), [int(before[i]["count"]), 0, U32])
            assert p[0] == int(before[i]["count"]), "duplicates of a pair read one counter"
            p[1] += int(deltas[i])
            p[2] = min(p[2], int(limits[i]))
    new, released = {}, set()
    for key, (count, net, lim) in pairs.items():
        s = count + net
        rep["floored"] += s < 0
        rep["capped"] += s > U32
        new[key] = min(max(s, 0), U32)
        if local_cache and not keep_cache and net < 0 and new[key] <= lim:
            released.add(key[0])
    was_cached = {strings[i] for i in range(n) if strings[i] is not None and int(before[i]["flags"]) & LC}
    rep["unfrozen"] = len(released & was_cached)
    after = np.array(before, hiprl.PEEK_DTYPE).copy()
    for i in range(n):
        fl = int(before[i]["flags"])
        if strings[i] is None:
            continue
        if fl & F:
            c = new[(strings[i], bool(fl & PS))]
            after[i]["count"] = c
            if fl & PS and c == 0:  # 0 is the per-second store's "absent"
                after[i]["flags"] = fl & ~F
        if strings[i] in released:
            after[i]["flags"] = int(after[i]["flags"]) & ~LC
            after[i]["cached_s"] = 0
    return after, rep
