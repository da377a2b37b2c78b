"""The router's copy of the hot-set table (rl_route.hip route_hot_lookup, rl_router::refresh_hot)
at capacity: 300 hot prefixes, so the route set is cut at 256 groups and group index 255 of the
8-bit perm field is in use; spread keys, and a mix in which half the set is one probe chain of
the tag table (hot_cases.py). Local transport, combining on, every step bit-exact against one
oracle replaying the origins' batches in shard order."""
import numpy as np
import pytest

import hiprl
import hot_cases as hc
import oracle
from hot_cases import HOT_MAX, HOT_MIN_SEG, T
from test_gpu_combining import engines, run_steps

pytestmark = pytest.mark.gpu

N_HOT, STEPS = 300, 18


def hot_prefixes(kind):
    if kind == "spread":
        return hc.spread(N_HOT)
    return hc.clustered(N_HOT // 2) + hc.spread(N_HOT - N_HOT // 2)


def routed_steps(kind, G):
    """Per step and origin: `per` descriptors of every hot prefix (G * per >= HOT_MIN_SEG, so the
    owner's engine sees each of its keys often enough to make it hot, and each origin's hits of a
    group sum past the route set's keep threshold of 64) and a cold tail; one request time per
    step."""
    per = max(-(-(HOT_MIN_SEG + 4) // G), 48)
    keys = hc.keys_of(hot_prefixes(kind) + hc.cold(400))
    steps = []
    for s in range(STEPS):
        row = []
        for g in range(G):
            c = np.full(len(keys), 1)
            c[:N_HOT] = per
            row.append(hc.make_batch(keys, hc.mix(c, np.random.default_rng(7000 + s * 16 + g)), T + 300 + s))
        steps.append(row)
    return steps


@pytest.mark.parametrize("kind", ["spread", "clustered+spread"])
@pytest.mark.parametrize("G", [2, 4])
def test_route_hot_set_at_capacity(G, kind):
    steps = routed_steps(kind, G)
    cap = max(b.n_desc for row in steps for b in row)
    r = hiprl.Router(engines(G, cap * G, rules=hc.RULES), max_desc=cap)
    o = oracle.Oracle()
    o.load_rules(hc.RULES)
    groups = []
    for s0 in (0, 9, 17):  # the route set is refreshed at steps 8 and 16
        s1 = {0: 9, 9: 17, 17: STEPS}[s0]
        run_steps(r, steps[s0:s1], o, "sync", f"routed {kind} G={G} from step {s0}")
        groups.append(r.stats()["hot_groups"])
    st = r.stats()
    print(f"hot_groups after steps 9, 17, 18: {groups}; combined_steps {st['combined_steps']}")
    assert groups == [HOT_MAX] * 3, (groups, st)  # cut at 256 by the first refresh, kept by the second
    assert st["combined_steps"] >= 6 and st["steps"] == STEPS, st
    assert st["status"] == [0] * G, st
    r.close()
