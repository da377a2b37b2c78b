"""Local-cache gauges and the table census (rl_hip.h "Local-cache gauges and the table census")
without a GPU: struct sizes, field offsets and flag values of the header against the Python
binding, the calls that must fail before they touch the device, and the reference-pinned
hitCount / missCount fixture (tests/golden/local_cache_gauges.json) against an oracle replay."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import hiprl
import oracle
import streams

ROOT = Path(__file__).resolve().parents[1]
EINVAL = -1
CS_FIELDS = ("hits", "misses", "lookups", "reserved")
CE_FIELDS = ("struct_size", "reserved0") + hiprl.CENSUS_REGION_FIELDS + ("count_log2", "reserved")


def test_struct_layouts_and_flags_match_the_header(tmp_path):
    src = tmp_path / "cg.c"
    offs = ",".join([f"offsetof(rl_cache_stats,{f})" for f in CS_FIELDS] +
                    [f"offsetof(rl_census_report,{f})" for f in CE_FIELDS])
    n = len(CS_FIELDS) + len(CE_FIELDS)
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf('
                   '"%zu %zu %u %u %u %u' + " %zu" * n + '\\n",sizeof(rl_cache_stats),sizeof(rl_census_report),'
                   '(unsigned)RL_CFG_CACHE_STATS,(unsigned)RL_CACHE_STATS_CLEAR,(unsigned)RL_CENSUS_LOG2_BINS,'
                   '(unsigned)RL_ABI_VERSION,' + offs + ');return 0;}\n')
    exe = tmp_path / "cg"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:6] == [64, 832, 8, 1, 33, 7]
    assert (C.sizeof(hiprl.RlCacheStats), C.sizeof(hiprl.RlCensusReport), hiprl.CFG_CACHE_STATS, hiprl.CACHE_STATS_CLEAR,
            hiprl.CENSUS_LOG2_BINS, hiprl.ABI_VERSION) == (64, 832, 8, 1, 33, 7)
    assert got[6:6 + len(CS_FIELDS)] == [getattr(hiprl.RlCacheStats, f).offset for f in CS_FIELDS]
    assert got[6 + len(CS_FIELDS):] == [getattr(hiprl.RlCensusReport, f).offset for f in CE_FIELDS]
    assert [f for f, _ in hiprl.RlCensusReport._fields_] == list(CE_FIELDS)
    # every count is a uint64, eight per region field
    for f in hiprl.CENSUS_REGION_FIELDS:
        assert getattr(hiprl.RlCensusReport, f).size == 64, f
    assert hiprl.RlCensusReport.count_log2.size == 8 * 33
    # the flag shares rl_config.flags with the pipeline, lag-window and rule-stats bits
    assert hiprl.CFG_CACHE_STATS not in (hiprl.CFG_LAG_WINDOW, hiprl.CFG_RULE_STATS, *hiprl.PIPELINE_FLAGS.values())


def test_null_arguments_fail_before_the_device():
    """No engine exists (and no GPU need): the calls return RL_EINVAL on their null checks."""
    lib = hiprl.load_library()
    rep = hiprl.RlCensusReport()
    rep.struct_size = C.sizeof(hiprl.RlCensusReport)
    cs = hiprl.RlCacheStats()
    b = hiprl.RlBatch()
    assert lib.rl_census(None, 0, C.byref(rep)) == EINVAL
    assert lib.rl_cache_stats_read(None, C.byref(cs), 0) == EINVAL
    assert lib.rl_cache_stats_add_device(None, C.byref(b), None) == EINVAL
    assert lib.rl_cache_stats_add_device(None, None, None) == EINVAL


def test_fixture_equals_an_oracle_replay(golden):
    fx = json.loads((ROOT / "tests" / "golden" / "local_cache_gauges.json").read_text())
    assert "integration_test.go:295-473" in fx["src"]
    assert sorted(fx["streams"]) == sorted(s["name"] for s in golden["streams"])
    for s in golden["streams"]:
        want = fx["streams"][s["name"]]
        assert len(want) == len(s["requests"]) == 42
        o = oracle.Oracle(local_cache=s["local_cache"])
        o.load_rules([tuple(x) for x in s["rules"]])
        for k, req in enumerate(streams.fixture_requests(s)):
            o.submit(hiprl.build_batch([req]))
            st = o.local_cache_stats()
            assert [st["hit"], st["miss"]] == want[k], (s["name"], k, st)
            assert st["lookup"] == st["hit"] + st["miss"]
    assert fx["streams"]["integration_basic_local1"][-1] == [8, 48]
    assert all(p == [0, 0] for p in fx["streams"]["integration_basic_local0"])
