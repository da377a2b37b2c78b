"""A model of the refund (rl_hip.h "Refund"): statuses + batch -> amounts, and amounts -> adjust_model
with Python-int deltas. RefundOracle holds the state the refund is applied to: the oracle's DoLimit
(oracle/rl_oracle.cpp do_limit) restated over Python dicts, one request at a time, with the oracle's
own GetResponseDescriptorStatus (oracle.decide) for every status. The C++ oracle cannot be written
to, so this is the oracle a refund can be applied to; test_refund_cpu.py pins it to the C++ one on
streams without refunds."""
import numpy as np

import hiprl
import oracle
from adjust_model import adjust_model

NIL = hiprl.NIL_RULE
OVER, OK = 2, 1
FLAG_LOCAL_HIT, FLAG_SHADOW = 2, 4
F, LC, PS = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_PER_SECOND
U32 = 0xFFFFFFFF


def refund_amounts(code_flags, rule, req_of, hits, n_req):
    """-> (amount per descriptor as Python ints, 0: skipped; the number of rejected requests)."""
    rej = [False] * n_req
    for cf, q in zip(code_flags, req_of):
        if int(cf) & 0xFF == OVER:
            rej[int(q)] = True
    out = []
    for cf, r, q in zip(code_flags, rule, req_of):
        owed = rej[int(q)] and int(r) != NIL and not (int(cf) >> 8) & FLAG_LOCAL_HIT
        out.append(max(1, int(hits[int(q)])) if owed else 0)
    return out, sum(rej)


class RefundOracle:
    def __init__(self, rules, near_limit_ratio=0.8, local_cache=False, per_second_split=False):
        self.rules = [(r[0], r[1], len(r) > 2 and bool(r[2])) for r in rules]
        self.ratio, self.local_cache, self.split = near_limit_ratio, local_cache, per_second_split
        self.redis = ({}, {})  # store -> key string -> [count, expiry]
        self.lcache = {}  # key string -> deadline

    def _key(self, b, i):
        r = int(b.rule[i])
        if r == NIL:
            return None, 0
        unit = self.rules[r][1]
        t = int(b.now[b.req_of[i]])
        d = hiprl.UNIT_DIVIDER[unit]
        return b.prefix(i) + str(t // d * d).encode(), int(self.split and unit == hiprl.SECOND)

    def submit(self, b):
        out = np.zeros(b.n_desc, hiprl.STATUS_DTYPE)
        thr = np.zeros(b.n_req, np.uint32)
        jit = getattr(b, "jit", None)
        i = 0
        while i < b.n_desc:
            q = int(b.req_of[i])
            j = i
            while j < b.n_desc and int(b.req_of[j]) == q:
                j += 1
            now, h = int(b.now[q]), max(1, int(b.hits[q]))
            keys = [self._key(b, k) for k in range(i, j)]
            hit = [self.local_cache and key is not None and now < self.lcache.get(key, 0) for key, _ in keys]
            res = [0] * len(keys)
            for store in (0, 1):
                for k, (key, st) in enumerate(keys):
                    if key is None or hit[k] or st != store:
                        continue
                    c = self.redis[store].setdefault(key, [0, 0])
                    if now >= c[1]:
                        c[0] = 0
                    c[0] += h
                    unit = self.rules[int(b.rule[i + k])][1]
                    c[1] = now + hiprl.UNIT_DIVIDER[unit] + (int(jit[i + k]) if jit is not None else 0)
                    res[k] = c[0] & U32
            tmax = 0
            for k, (key, _) in enumerate(keys):
                has = key is not None
                L, unit, shadow = self.rules[int(b.rule[i + k])] if has else (0, hiprl.SECOND, False)
                st, t = oracle.decide(L, unit, self.ratio, now, h, res[k], local_hit=hit[k], has_limit=has,
                                      before=(res[k] - h) & U32)
                cf = int(st["code_flags"])
                if has and shadow and cf & 0xFF == OVER:
                    cf = (cf & ~0xFF) | OK | (FLAG_SHADOW << 8)
                out[i + k] = st
                out[i + k]["code_flags"] = cf
                tmax = max(tmax, t)
                if has and not hit[k] and self.local_cache and res[k] > L:
                    self.lcache[key] = now + hiprl.UNIT_DIVIDER[unit]
            thr[q] = tmax
            i = j
        return out, thr

    def peek(self, key, store, t):
        """-> rl_peek's (count, ttl_s, cached_s, flags) of a key string in a store at time t."""
        c = self.redis[store].get(key)
        count = ttl = cached = 0
        flags = PS if store else 0
        if c is not None and (c[0] != 0 if store else t < c[1]):
            flags |= F
            count = c[0]
            ttl = 0 if store else c[1] - t
        if self.local_cache and t < self.lcache.get(key, 0):
            flags |= LC
            cached = self.lcache[key] - t
        return count, ttl, cached, flags

    def refund(self, b, status, keep_cache=False):
        """Apply the refund of batch b with the given statuses. -> (amounts, report)."""
        amounts, n_rej = refund_amounts(status["code_flags"], b.rule, b.req_of, b.hits, b.n_req)
        owed = [i for i in range(b.n_desc) if amounts[i]]
        keys = [self._key(b, i) for i in owed]
        rows = []
        for (key, store), i in zip(keys, owed):
            count, ttl, cached, flags = self.peek(key, store, int(b.now[b.req_of[i]]))
            # a deadline word that is not 0 counts in `unfrozen` when it is cleared, expired or not:
            # the model sees deadlines through LOCAL_CACHED, so that flag stands for "not 0" here
            if self.lcache.get(key, 0):
                flags |= LC
            rows.append((count, ttl, cached, flags))
        before = np.array(rows, hiprl.PEEK_DTYPE).reshape(len(rows))
        limits = [self.rules[int(b.rule[i])][0] for i in owed]
        after, rep = adjust_model([k for k, _ in keys], before, [-amounts[i] for i in owed], limits, self.local_cache,
                                  keep_cache)
        for (key, store), a, bf in zip(keys, after, before):
            if int(bf["flags"]) & F:
                self.redis[store][key][0] = int(a["count"])
            if int(bf["flags"]) & LC and not int(a["flags"]) & LC:
                self.lcache.pop(key, None)
        assert rep["capped"] == 0 and rep["nil"] == 0
        return amounts, dict(descriptors=b.n_desc, rejected_req=n_rej, skipped=b.n_desc - len(owed),
                             absent=rep["absent"], refunded=rep["applied"], floored=rep["floored"],
                             unfrozen=rep["unfrozen"])
