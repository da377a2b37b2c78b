"""Rule stats (rl_hip.h "Rule stats") without a GPU: the struct layout and flag value of the
header against the Python binding, and RateLimitConfig.stats' folding of rule ids into the
reference's stat names (config_impl.go:64-70, 286-296)."""
import subprocess
from pathlib import Path

import numpy as np

import hiprl
import rl_config

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("total_hits", "over_limit", "near_limit", "over_limit_with_local_cache", "shadow_mode", "reserved")


def test_rule_stat_layout_and_flag_match_the_header(tmp_path):
    src = tmp_path / "rs.c"
    offs = ",".join(f"offsetof(rl_rule_stat,{f})" for f in FIELDS)
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf('
                   '"%zu %u %u %u' + " %zu" * len(FIELDS) + '\\n",sizeof(rl_rule_stat),(unsigned)RL_CFG_RULE_STATS,'
                   '(unsigned)RL_RULE_STATS_CLEAR,(unsigned)RL_ABI_VERSION,' + offs + ');return 0;}\n')
    exe = tmp_path / "rs"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    dt = hiprl.RULE_STAT_DTYPE
    assert got[:4] == [64, 4, 1, 7]
    assert (dt.itemsize, hiprl.CFG_RULE_STATS, hiprl.RULE_STATS_CLEAR, hiprl.ABI_VERSION) == (64, 4, 1, 7)
    assert got[4:] == [dt.fields[f][1] for f in FIELDS]
    assert dt.names == FIELDS and hiprl.RULE_STAT_FIELDS == FIELDS[:5]
    assert all(dt.fields[f][0] == np.dtype("<u8") for f in FIELDS[:5]) and dt.fields["reserved"][0].shape == (3,)
    # the flag shares rl_config.flags with the pipeline and lag-window bits
    assert hiprl.CFG_RULE_STATS not in (hiprl.CFG_LAG_WINDOW, *hiprl.PIPELINE_FLAGS.values())


class FakeEngine:
    """What RateLimitConfig.stats needs of an engine: rule_stats(first, n, clear)."""

    def __init__(self, rows):
        self.rows, self.calls = rows, []

    def rule_stats(self, first=0, n=None, clear=False):
        self.calls.append((first, n, clear))
        return self.rows[first:first + n]


YAML = """
domain: shop
descriptors:
  - key: user
    rate_limit: {unit: minute, requests_per_unit: 10}
    descriptors:
      - key: path
        value: /buy
        rate_limit: {unit: second, requests_per_unit: 2}
  - key: plain
"""


def test_stats_fold_rule_ids_into_stat_names():
    cfg = rl_config.RateLimitConfig([("shop.yaml", YAML)])
    assert [r.full_key for r in cfg.rules] == ["shop.user", "shop.user.path_/buy"]
    # two overrides of one key: two rule ids, one stats key (config_impl.go:286-296)
    a = cfg.override_rule("shop", [("user", "u7")], 5, hiprl.MINUTE)
    b = cfg.override_rule("shop", [("user", "u7")], 9, hiprl.HOUR)
    assert (a, b) == (2, 3) and cfg.rules[a].full_key == cfg.rules[b].full_key == "shop.user_u7"
    rows = np.zeros(4, hiprl.RULE_STAT_DTYPE)
    for i in range(4):
        for k, f in enumerate(hiprl.RULE_STAT_FIELDS):
            rows[f][i] = 1000 * (i + 1) + k
    rows["total_hits"][2] = 2 ** 64 - 1  # sums wrap like the device's
    eng = FakeEngine(rows)
    got = cfg.stats(eng, clear=True)
    assert eng.calls == [(0, 4, True)]
    want = {}
    for k, f in enumerate(hiprl.RULE_STAT_FIELDS):
        want[f"shop.user.{f}"] = 1000 + k
        want[f"shop.user.path_/buy.{f}"] = 2000 + k
        want[f"shop.user_u7.{f}"] = 3000 + k + 4000 + k
    want["shop.user_u7.total_hits"] = (2 ** 64 - 1 + 4000) % 2 ** 64
    assert got == want
    assert "shop.user.shadow_mode" in got and all(type(v) is int for v in got.values())
    eng2 = FakeEngine(rows)
    assert cfg.stats(eng2) == want and eng2.calls == [(0, 4, False)]


def test_stats_of_a_tree_without_limits_is_empty():
    cfg = rl_config.RateLimitConfig([("nil.yaml", "domain: nil\ndescriptors:\n  - key: a\n    descriptors:\n      - key: b\n")])
    assert cfg.rules == []
    eng = FakeEngine(np.zeros(0, hiprl.RULE_STAT_DTYPE))
    assert cfg.stats(eng) == {} and eng.calls == [(0, 0, False)]
