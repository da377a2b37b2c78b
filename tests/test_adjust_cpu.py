"""Adjust (rl_hip.h "Adjust"), CPU only: the report's layout, the flag value and the prototype
against the header, the library's entry point, the Python entry points, and the dict model
(adjust_model.py) against hand-written cases."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import hiprl
from adjust_model import adjust_model, string_of

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ["descriptors", "nil", "absent", "applied", "floored", "capped", "unfrozen", "reserved"]
F, LC, NILF, PS = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND


def test_report_layout_flag_and_prototype_match_the_header(tmp_path):
    offs = ",".join(f"offsetof(rl_adjust_report,{f})" for f in FIELDS)
    src = tmp_path / "adjust.c"
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int (*fn)(rl_engine*, const rl_batch*, const int32_t*, uint32_t, rl_peek_reply*, rl_adjust_report*)'
                   ' = rl_adjust;\n'
                   'int main(){size_t v[]={'
                   f'sizeof(rl_adjust_report),RL_ADJUST_KEEP_CACHE,RL_ABI_VERSION,{offs}}};'
                   'for(unsigned i=0;i<sizeof v/sizeof v[0];++i)printf("%zu ",v[i]);return 0;}\n')
    obj = tmp_path / "adjust.o"
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(obj)], check=True)
    exe = tmp_path / "adjust"
    subprocess.run(["gcc", str(obj), "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [64, 1, 7] + [8 * k for k in range(8)]
    R = hiprl.RlAdjustReport
    assert C.sizeof(R) == 64 and [getattr(R, f).offset for f in FIELDS] == [8 * k for k in range(8)]
    assert hiprl.ADJUST_KEEP_CACHE == 1 and hiprl.ABI_VERSION == 7
    assert list(hiprl.ADJUST_REPORT_FIELDS) == FIELDS[:-1]


def test_library_exports_adjust():
    lib = hiprl.load_library()
    assert hasattr(lib, "rl_adjust") and "rl_adjust" in {n for n, _, _ in hiprl.ABI}
    assert lib.rl_abi_version() == 7
    # null arguments are refused before anything touches the GPU
    assert lib.rl_adjust(None, None, None, 0, None, None) == -1
    assert hasattr(hiprl.Engine, "adjust") and hasattr(hiprl.HipRateLimitCache, "adjust")


# ---- the model against hand-written cases --------------------------------------------------------
def replies(rows):
    return np.array([tuple(r) for r in rows], hiprl.PEEK_DTYPE).reshape(len(rows))


def report(n, **kw):
    return dict(dict.fromkeys(hiprl.ADJUST_REPORT_FIELDS, 0), descriptors=n, **kw)


def test_model_sums_once_per_pair():
    # counter 5 with (-10, +3) ends at 0, not 3, in either order: one INCRBY of the net, clamped once
    before = replies([(5, 40, 0, F), (5, 40, 0, F)])
    for deltas in ([-10, 3], [3, -10]):
        after, rep = adjust_model(["k", "k"], before, deltas, [9, 9])
        assert after.tolist() == [(0, 40, 0, F)] * 2 and rep == report(2, applied=2, floored=1)
    # a zero net: nothing moves, and a sum of exactly 0 is not floored
    after, rep = adjust_model(["k", "k"], before, [-4, 4], [9, 9])
    assert np.array_equal(after, before) and rep == report(2, applied=2)
    after, rep = adjust_model(["k"], before[:1], [-5], [9])
    assert after.tolist() == [(0, 40, 0, F)] and rep == report(1, applied=1)


def test_model_clamps_at_both_ends():
    before = replies([(7, 9, 0, F), (0xFFFFFFF0, 9, 0, F), (0xFFFFFFF0, 9, 0, F)])
    after, rep = adjust_model(["a", "b", "c"], before, [-2**31, 2**31 - 1, 0xF], [1, 1, 1])
    assert after["count"].tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFF] and rep == report(3, applied=3, floored=1, capped=1)
    assert after["ttl_s"].tolist() == [9, 9, 9] and after["flags"].tolist() == [F, F, F]  # a floored counter keeps its TTL


def test_model_nil_absent_and_the_two_stores():
    before = replies([(0, 0, 0, NILF), (0, 0, 0, 0), (0, 0, 0, PS), (4, 0, 0, F | PS), (4, 30, 0, F), (2, 0, 0, F | PS)])
    strings = [None, "gone", "gone_s", "two", "two", "s"]
    after, rep = adjust_model(strings, before, [5, 5, 5, -1, 2, -2], [3] * 6)
    assert rep == report(6, nil=1, absent=2, applied=3)
    # absent stays absent (nothing is claimed); one string's two stores move apart; per-second 0 is "absent"
    assert after.tolist() == [(0, 0, 0, NILF), (0, 0, 0, 0), (0, 0, 0, PS), (3, 0, 0, F | PS), (6, 30, 0, F), (0, 0, 0, PS)]


def test_model_cache_part_and_the_min_limit_rule():
    frozen = (12, 50, 60, F | LC)
    # released: net < 0 and the result is not above the smallest limit among the pair's descriptors
    after, rep = adjust_model(["k"], replies([frozen]), [-2], [10], local_cache=True)
    assert after.tolist() == [(10, 50, 0, F)] and rep == report(1, applied=1, unfrozen=1)
    # ... still above it: stays frozen
    after, rep = adjust_model(["k"], replies([frozen]), [-1], [10], local_cache=True)
    assert after.tolist() == [(11, 50, 60, F | LC)] and rep == report(1, applied=1)
    # the smallest limit decides: 10 under limits (10, 8) is still over the 8
    after, rep = adjust_model(["k", "k"], replies([frozen, frozen]), [-1, -1], [10, 8], local_cache=True)
    assert after.tolist() == [(10, 50, 60, F | LC)] * 2 and rep["unfrozen"] == 0
    after, rep = adjust_model(["k", "k"], replies([frozen, frozen]), [-1, -3], [10, 8], local_cache=True)
    assert after.tolist() == [(8, 50, 0, F)] * 2 and rep["unfrozen"] == 1
    # KEEP_CACHE, a cache that is off, a positive and a zero net never touch the deadline
    for kw, d in ((dict(local_cache=True, keep_cache=True), -5), (dict(local_cache=False), -5),
                  (dict(local_cache=True), 5), (dict(local_cache=True), 0)):
        after, rep = adjust_model(["k"], replies([frozen]), [d], [10], **kw)
        assert after.tolist() == [(12 + d, 50, 60, F | LC)] and rep["unfrozen"] == 0
    # a positive net freezes nothing; a release of a string that was not cached counts nothing
    after, rep = adjust_model(["k", "j"], replies([(9, 50, 0, F), (9, 50, 0, F)]), [5, -5], [10, 10], local_cache=True)
    assert after.tolist() == [(14, 50, 0, F), (4, 50, 0, F)] and rep["unfrozen"] == 0
    # one string, two stores, both qualify: one deadline, counted once
    two = replies([(5, 0, 1, F | PS | LC), (5, 30, 1, F | LC)])
    after, rep = adjust_model(["s", "s"], two, [-1, -1], [4, 4], local_cache=True)
    assert after.tolist() == [(4, 0, 0, F | PS), (4, 30, 0, F)] and rep["unfrozen"] == 1
    # ... one qualifies: the string is released all the same, the other store's reply loses the flag too
    after, rep = adjust_model(["s", "s"], two, [-1, 0], [4, 4], local_cache=True)
    assert after.tolist() == [(4, 0, 0, F | PS), (5, 30, 0, F)] and rep["unfrozen"] == 1


def test_string_of():
    assert string_of(b"d_k_v_", hiprl.MINUTE, 1_700_000_007) == b"d_k_v_1699999980"
    assert string_of(b"p_", hiprl.SECOND, 7) == b"p_7" and string_of(b"p_", hiprl.DAY, 0xFFFD0000) == b"p_4294684800"  # 49707 days
