"""A model of rl_router_refund (rl_hip.h "Routed refund") over RefundOracle's state (refund_model.py):
a G-origin call is refund_amounts per origin, then one adjust over all origins' owed descriptors in
origin order, with one keep flag per origin (routed_adjust_model.py: adjust_model's contract plus the
rule that a pair's cache part runs when some found descriptor of it came without keep; its deltas
are Python ints, so an amount of 2^32 - 1 passes whole). With one flag on every origin it equals
RefundOracle.refund on the concatenated batch (test_routed_refund_cpu.py)."""
import numpy as np

import hiprl
from refund_model import RefundOracle, refund_amounts
from routed_adjust_model import routed_adjust_model

F, LC, NILF = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL
OWNER_FIELDS = ("absent", "refunded", "floored", "unfrozen")


class RoutedRefundOracle(RefundOracle):
    def refund_routed(self, batches, statuses, keeps=False):
        """Apply one routed refund: batches[o] with statuses[o] from origin o, keeps a bool or one per
        origin. -> (amounts per origin (Python ints, 0: skipped); the replies per origin: rl_peek's
        state before the call for an owed descriptor, NIL for any other; per origin its origin fields
        {descriptors, rejected_req, skipped}; the owners' fields summed over the world)."""
        G = len(batches)
        ks = [bool(keeps)] * G if isinstance(keeps, (bool, np.bool_)) else [bool(k) for k in keeps]
        assert len(statuses) == len(ks) == G
        amounts, origin, owed, keys, before, limits = [], [], [], [], [], []
        for b, st in zip(batches, statuses):
            am, n_rej = refund_amounts(st["code_flags"], b.rule, b.req_of, b.hits, b.n_req)
            ow = [i for i in range(b.n_desc) if am[i]]
            amounts.append(am)
            origin.append(dict(descriptors=b.n_desc, rejected_req=n_rej, skipped=b.n_desc - len(ow)))
            owed.append(ow)
            keys.append([self._key(b, i) for i in ow])
            before.append([self.peek(key, store, int(b.now[b.req_of[i]])) for (key, store), i in zip(keys[-1], ow)])
            limits.append([self.rules[int(b.rule[i])][0] for i in ow])
        # RefundOracle.refund's rule for `unfrozen`: a deadline word that is not 0 counts when it is
        # cleared, expired or not; the adjust model sees deadlines through LOCAL_CACHED
        seen = [[(c, t, s, fl | (LC if self.lcache.get(key, 0) else 0)) for (c, t, s, fl), (key, _) in zip(bf, ky)]
                for bf, ky in zip(before, keys)]
        arr = [np.array(rows, hiprl.PEEK_DTYPE).reshape(len(rows)) for rows in seen]
        after, rep = routed_adjust_model([[k for k, _ in ky] for ky in keys], arr,
                                         [[-amounts[o][i] for i in owed[o]] for o in range(G)], limits, ks,
                                         self.local_cache)
        for o in range(G):
            for (key, store), a, bf in zip(keys[o], after[o], arr[o]):
                if int(bf["flags"]) & F:
                    self.redis[store][key][0] = int(a["count"])
                if int(bf["flags"]) & LC and not int(a["flags"]) & LC:
                    self.lcache.pop(key, None)
        assert rep["capped"] == 0 and rep["nil"] == 0
        outs = []
        for o, b in enumerate(batches):
            out = np.zeros(b.n_desc, hiprl.PEEK_DTYPE)
            out["flags"] = NILF
            for i, row in zip(owed[o], before[o]):
                out[i] = row
            outs.append(out)
        owner = dict(absent=rep["absent"], refunded=rep["applied"], floored=rep["floored"], unfrozen=rep["unfrozen"])
        return amounts, outs, origin, owner
