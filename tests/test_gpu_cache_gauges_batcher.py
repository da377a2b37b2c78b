"""HipRateLimitCache::local_cache_stats with the device's local cache (rl_cache.hpp; INTEGRATION.md
§4e), through the existing test shim: hits / misses against the reference-pinned fixture
(tests/golden/local_cache_gauges.json) after every request of the integration stream, entries /
expired against the oracle's local cache at the shim's time source."""
import ctypes as C
import json
from pathlib import Path

import pytest

import hiprl
import oracle
import streams
from test_gpu_cache_mirror import Mirror
from test_gpu_freecache_batcher import FcMirror

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GAUGES = json.loads((ROOT / "tests" / "golden" / "local_cache_gauges.json").read_text())["streams"]


def cache_stats(m):
    """hits, misses, lookups, entries, evicted, expired"""
    m.lib.rlc_local_cache_stats.argtypes = [C.c_void_p, C.c_void_p]
    o = (C.c_uint64 * 6)()
    m.lib.rlc_local_cache_stats(m.h, o)
    return list(o)


def run_stream(m, s, check):
    ids = [m.add_rule(L, u, s["stat_keys"][k]) for k, (L, u) in enumerate(s["rules"])]
    for k, req in enumerate(s["requests"]):
        m.lib.rlc_set_time(m.h, req["now"])
        descs = [[tuple(e) for e in d] for d in req["descriptors"]]
        m.do_limit(req["domain"], descs, [None if r is None else ids[r] for r in req["rules"]], req["hits"])
        check(k, cache_stats(m))


def oracle_cache(s, now):
    """(entries, expired) of the oracle's local cache after the whole stream, at `now`: the strings
    rlo_local_cached holds at `now`, and the ones it held (asked at time 0) whose deadline has
    passed and whose window generation is still its table region's newest."""
    o = oracle.Oracle(local_cache=s["local_cache"])
    rules = [tuple(x) for x in s["rules"]]
    o.load_rules(rules)
    reqs = streams.fixture_requests(s)
    o.submit(hiprl.build_batch(reqs))
    strings = {}
    for dom, descs, rids, _, t in reqs:
        for entries, rid in zip(descs, rids):
            if rid != streams.NIL:
                div = hiprl.UNIT_DIVIDER[rules[rid][1]]
                strings[oracle.cache_key(hiprl.cache_key_prefix(dom, entries), rules[rid][1], t)] = t // div * div
    placed = {k: oracle.place(ws) for k, ws in strings.items()}
    newest = {}
    for r, g in placed.values():
        newest[r] = max(newest.get(r, 0), g)
    entries = sum(o.local_cached(k, now) for k in strings)
    expired = sum(1 for k, (r, g) in placed.items()
                  if g == newest[r] and o.local_cached(k, 0) and not o.local_cached(k, now))
    return entries, expired


def test_device_cache_gauges_on_the_integration_stream(golden):
    s = next(x for x in golden["streams"] if x["name"] == "integration_basic_local1")
    want = GAUGES[s["name"]]
    m = Mirror(True)

    def check(k, got):
        assert got[:3] == [want[k][0], want[k][1], want[k][0] + want[k][1]], (k, got)
        assert got[4] == 0  # the device cache never evicts

    run_stream(m, s, check)
    t = s["requests"][-1]["now"]
    ent, exp = oracle_cache(s, t)
    assert (ent, exp) == (2, 0)  # guard: the oracle's own figures
    got = cache_stats(m)
    assert got == [8, 48, 56, ent, 0, exp], got
    # past the MINUTE rule's deadline: its string leaves the cache and shows as expired
    div = 60 - t % 60 + 60
    m.lib.rlc_set_time(m.h, t + div)
    ent2, exp2 = oracle_cache(s, t + div)
    assert (ent2, exp2) == (1, 1), (ent2, exp2)
    assert cache_stats(m) == [8, 48, 56, ent2, 0, exp2]
    m.close()


def test_gauges_stay_zero_without_the_local_cache(golden):
    s = next(x for x in golden["streams"] if x["name"] == "integration_basic_local0")
    m = Mirror(False)
    run_stream(m, s, lambda k, got: got == [0] * 6 or pytest.fail(f"request {k}: {got}"))
    assert all(p == [0, 0] for p in GAUGES[s["name"]])
    m.close()


def test_the_freecache_model_path_is_unchanged(golden):
    """HIP_LOCAL_CACHE=freecache keeps reporting the host model's own counters: on this stream
    (nothing is evicted) the same reference-pinned hits and misses."""
    s = next(x for x in golden["streams"] if x["name"] == "integration_basic_local1")
    want = GAUGES[s["name"]]
    m = FcMirror(1 << 30)
    run_stream(m, s, lambda k, got: got[:3] == [want[k][0], want[k][1], sum(want[k])] or pytest.fail(f"request {k}: {got}"))
    assert m.cache_stats() == [8, 48, 56, 2, 0, 0]
    m.close()
