"""A NumPy / dict model of rl_merge (rl_hip.h "Merge"), written from the contract's words: the
table as {(ctrl, key): [count, exp, pcount, frz]} with the newest window generation per region.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import hiprl
import oracle

M32 = 0xFFFFFFFF
SEED = 0x5EE7AB1E5EED  # hiprl.Engine's default hash_seed
FIELDS = ("records", "folded", "claimed", "dropped_over", "dropped_empty")


def sorted_set(recs):
    return np.sort(recs, order=["key", "ctrl"])


def ident(prefix: bytes, unit: int, now: int, seed: int = SEED):
    """(ctrl, key) of the key string prefix || window start of `now` under `unit`."""
    div = hiprl.UNIT_DIVIDER[unit]
    ws = now // div * div
    hi, lo = oracle.fingerprint(prefix, ws, seed)
    region, gen = oracle.place(ws)
    return gen | (lo << 32), (region << 61) | (hi >> 3)


class TableModel:
    def __init__(self, lag=False, local_cache=False):
        self.lag, self.local_cache = lag, local_cache
        self.gen = [0] * 8
        self.slots = {}

    @classmethod
    def of(cls, engine, lag=False, local_cache=False):
        """The live content of an engine's table (its snapshot)."""
        m = cls(lag, local_cache)
        h, recs = engine.snapshot_records()
        m.gen = list(h.gen)
        for r in recs:
            m.slots[(int(r["ctrl"]), int(r["key"]))] = [int(r["count"]), int(r["exp"]), int(r["pcount"]), int(r["frz"])]
        return m

    def lazy(self, region):
        return self.lag and region < 2

    def live(self, region, g):
        G = self.gen[region]
        return g != 0 and (g == G or (self.lazy(region) and g + 2 == G))

    def leaves(self, st, now):
        return now < st[1] or st[2] != 0 or (self.local_cache and now < st[3])

    def merge(self, recs, now):
        """One rl_merge call of `recs` at `now`: the report it must return."""
        items = [((int(r["ctrl"]), int(r["key"])), [int(r["count"]), int(r["exp"]), int(r["pcount"]), int(r["frz"])])
                 for r in recs]
        T = list(self.gen)
        for (ctrl, key), st in items:
            region, g = key >> 61, ctrl & M32
            if g > T[region] and self.leaves(st, now):
                T[region] = g
        self.gen = T  # a target above the region's generation comes with a claim of it
        self.slots = {k: v for k, v in self.slots.items() if self.live(k[1] >> 61, k[0] & M32)}
        rep = dict.fromkeys(FIELDS, 0)
        rep["records"] = len(items)
        for k, R in items:
            region, g = k[1] >> 61, k[0] & M32
            if not self.live(region, g):
                rep["dropped_over"] += 1
            elif not self.leaves(R, now):
                rep["dropped_empty"] += 1
            else:
                S = self.slots.get(k)
                found = S is not None
                o = list(S) if found else [0, 0, 0, 0]
                alive_r, alive_s = now < R[1], found and now < S[1]
                if alive_r and alive_s:
                    o[0], o[1] = (S[0] + R[0]) & M32, max(S[1], R[1])
                elif alive_r:
                    o[0], o[1] = R[0], R[1]
                o[2] = (o[2] + R[2]) & M32
                o[3] = max(o[3], R[3])
                self.slots[k] = o
                rep["folded" if found else "claimed"] += 1
        return rep

    def records(self):
        out = np.zeros(len(self.slots), hiprl.SNAP_DTYPE)
        for i, ((ctrl, key), st) in enumerate(self.slots.items()):
            out[i] = (ctrl, key, st[0], st[1], st[2], st[3])
        return sorted_set(out)

    def counts(self):
        """(live[8], prev[8]) as a snapshot header of the table would carry them."""
        live, prev = [0] * 8, [0] * 8
        for ctrl, key in self.slots:
            region = key >> 61
            (live if (ctrl & M32) == self.gen[region] else prev)[region] += 1
        return live, prev
