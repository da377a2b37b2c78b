"""The oracle against an independent model (tests/edge_model.py) at the numeric-range edges:
limits up to 2^32 - 1 and past 2^24 (float32 near threshold), INCRBY replies that wrap at 2^32,
times up to MAX_NOW, a day boundary, the largest EXPIRE jitter. The GPU suite's reference
(test_gpu_numeric_edges.py) is pinned here in the regime it is used in.
Reference: src/limiter/base_limiter.go:70-177, src/redis/fixed_cache_impl.go:39-117."""
import numpy as np
import pytest

import edge_model as em
import hiprl
import oracle
import streams


def submit_all(o, batches):
    outs = [o.submit(hiprl.build_batch(reqs)) for reqs in batches]
    return np.concatenate([s for s, _ in outs]), np.concatenate([t for _, t in outs])


def test_units_and_codes_are_the_bindings():
    assert (em.SECOND, em.MINUTE, em.HOUR, em.DAY) == (hiprl.SECOND, hiprl.MINUTE, hiprl.HOUR, hiprl.DAY)
    assert em.DIV == hiprl.UNIT_DIVIDER and em.NIL == hiprl.NIL_RULE and em.STATUS_DTYPE == oracle.STATUS_DTYPE
    assert (em.OK, em.OVER, em.HAS_LIMIT, em.LOCAL_HIT) == (hiprl.CODE_OK, hiprl.CODE_OVER_LIMIT, hiprl.FLAG_HAS_LIMIT,
                                                            hiprl.FLAG_LOCAL_CACHE_HIT)


def test_decide_grid():
    vs = em.grid()
    assert len(vs) > 30000
    # the grid holds what it is for: wraps (before > after), the float32-inexact limits, MAX_NOW
    assert sum((v["after"] - v["hits"]) < 0 for v in vs) > 1000
    assert em.near_threshold(2 ** 24 + 1, 1.0) == 2 ** 24 and em.near_threshold(2 ** 24 + 3, 1.0) == 2 ** 24 + 4
    assert any(v["now"] == em.MAX_NOW for v in vs)
    for v in vs:
        want = em.decide(v["L"], v["unit"], v["ratio"], v["now"], v["hits"], v["after"], v["local_hit"])
        st, thr = oracle.decide(v["L"], v["unit"], v["ratio"], v["now"], v["hits"], v["after"], v["local_hit"])
        assert tuple(int(x) for x in st) + (thr,) == want, v


@pytest.mark.parametrize("local_cache", [False, True])
def test_day_boundary_stream_with_wrapping_hits(local_cache):
    reqs = em.day_stream()
    assert reqs[0][4] // 86400 + 1 == reqs[-1][4] // 86400  # crosses the day boundary
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(em.EDGE_RULES)
    sizes = streams.batch_sizes(reqs, np.random.default_rng(3), 700)
    got = streams.replay(o, reqs, sizes)
    want = em.serial(reqs, em.EDGE_RULES, np.float32(0.8), local_cache)
    streams.assert_same(*want, *got, f"day stream local={local_cache}")
    rid = [r for q in reqs for r in q[2]]
    keys = [(str(e), q[4] // em.DIV[em.EDGE_RULES[r][1]]) if r != em.NIL else None
            for q in reqs for e, r in zip(q[1], q[2])]
    assert em.wrapped(want[0], em.EDGE_RULES, rid, keys)
    if local_cache:
        assert np.any((want[0]["code_flags"] >> 8) & em.LOCAL_HIT)


@pytest.mark.parametrize("local_cache", [False, True])
def test_batches_at_edge_times(local_cache):
    rules, batches = em.time_batches()
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(rules)
    got = submit_all(o, batches)
    want = em.serial([r for b in batches for r in b], rules, np.float32(0.8), local_cache)
    streams.assert_same(*want, *got, f"edge times local={local_cache}")
    assert np.any(want[0]["code_flags"] & 0xFF == em.OVER) and np.any(want[1] > 0)


def test_largest_jitter_on_a_day_rule_at_max_now():
    """EXPIRE 86400 + 65535 in the last admissible hour (edge_model.jitter_stream)."""
    rules, batches, jits = em.jitter_stream()
    o = oracle.Oracle(local_cache=False)
    o.load_rules(rules)
    outs = [o.submit(hiprl.build_batch(reqs, jit=j)) for reqs, j in zip(batches, jits)]
    want = em.serial([r for b in batches for r in b], rules, np.float32(0.8), False, jit=[x for j in jits for x in j])
    streams.assert_same(*want, np.concatenate([s for s, _ in outs]), np.concatenate([t for _, t in outs]),
                        "jitter at MAX_NOW")
    # the shared string survived 65 s (2^32 - 1 + 3 wraps to 2), and the DAY counter wrapped
    assert int(want[0]["limit_remaining"][3]) == 5 - 2 and int(want[0]["limit_remaining"][4]) == 2 ** 32 - 1 - 4
