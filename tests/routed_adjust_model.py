"""A dict model of rl_router_adjust (rl_hip.h "Routed adjust"): rl_adjust's contract (adjust_model.py)
over the concatenation of all origins' descriptors, with one keep flag per descriptor. From what
Router.peek answered just before the call, the deltas, the rules and the keep flags: what
Router.peek answers just after it, and the call's totals (the owners' reports summed over the
ranks, plus the nil descriptors, which never leave their origin).

The one rule adjust_model does not have: a pair's cache part runs when at least one of its found
descriptors came without keep, and never when all carry it. With one flag on every descriptor the
two models agree (checked in test_routed_adjust_cpu.py)."""
import numpy as np

import hiprl

F, LC, NILF, PS = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND
U32 = 0xFFFFFFFF


def routed_adjust_model(strings, before, deltas, limits, keeps, local_cache=False):
    """strings / before / deltas / limits: adjust_model's, per origin (lists of equal length, one
    entry per origin); keeps[o][i]: descriptor i of origin o carries KEEP_CACHE (or one bool per
    origin). -> (the replies after the call, per origin; the totals as a dict)."""
    G = len(strings)
    assert len(before) == len(deltas) == len(limits) == len(keeps) == G
    cat_s, cat_b, cat_d, cat_l, cat_k = [], [], [], [], []
    for o in range(G):
        n = len(strings[o])
        assert len(before[o]) == len(deltas[o]) == len(limits[o]) == n
        k = [bool(keeps[o])] * n if isinstance(keeps[o], (bool, np.bool_)) else [bool(x) for x in keeps[o]]
        assert len(k) == n
        cat_s += list(strings[o])
        cat_b += [tuple(r) for r in np.asarray(before[o], hiprl.PEEK_DTYPE).tolist()]
        cat_d += [int(x) for x in deltas[o]]
        cat_l += [int(x) for x in limits[o]]
        cat_k += k
    n = len(cat_s)
    rep = dict.fromkeys(hiprl.ADJUST_REPORT_FIELDS, 0)
    rep["descriptors"] = n
    pairs = {}  # (string, per-second) -> [count before, net, smallest limit, some found descriptor without keep]
    for i in range(n):
        fl = cat_b[i][3]
        if cat_s[i] is None:
            assert fl & NILF
            rep["nil"] += 1
        elif not fl & F:
            rep["absent"] += 1
        else:
            rep["applied"] += 1
            p = pairs.setdefault((cat_s[i], bool(fl & PS)), [cat_b[i][0], 0, U32, False])
            assert p[0] == cat_b[i][0], "duplicates of a pair read one counter"
            p[1] += cat_d[i]
            p[2] = min(p[2], cat_l[i])
            p[3] = p[3] or not cat_k[i]
    new, released = {}, set()
    for key, (count, net, lim, nokeep) in pairs.items():
        s = count + net
        rep["floored"] += s < 0
        rep["capped"] += s > U32
        new[key] = min(max(s, 0), U32)
        if local_cache and nokeep and net < 0 and new[key] <= lim:
            released.add(key[0])
    was_cached = {cat_s[i] for i in range(n) if cat_s[i] is not None and cat_b[i][3] & LC}
    rep["unfrozen"] = len(released & was_cached)
    after = np.array(cat_b, hiprl.PEEK_DTYPE).reshape(n).copy()
    for i in range(n):
        fl = cat_b[i][3]
        if cat_s[i] is None:
            continue
        if fl & F:
            c = new[(cat_s[i], bool(fl & PS))]
            after[i]["count"] = c
            if fl & PS and c == 0:  # 0 is the per-second store's "absent"
                after[i]["flags"] = fl & ~F
        if cat_s[i] in released:
            after[i]["flags"] = int(after[i]["flags"]) & ~LC
            after[i]["cached_s"] = 0
    outs, o0 = [], 0
    for o in range(G):
        outs.append(after[o0:o0 + len(strings[o])])
        o0 += len(strings[o])
    return outs, rep
