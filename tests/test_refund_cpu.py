"""Refund (rl_hip.h "Refund"), CPU only: the report's layout, the flag value and the prototypes
against the header, the library's entry points, and the model (refund_model.py) against hand-worked
cases and, without refunds, against the C++ oracle."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import hiprl
import oracle
import streams
from refund_model import RefundOracle, refund_amounts

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ["descriptors", "rejected_req", "skipped", "absent", "refunded", "floored", "unfrozen", "reserved"]
NIL = hiprl.NIL_RULE
T = 1_700_000_007


def test_report_layout_flag_and_prototypes_match_the_header(tmp_path):
    offs = ",".join(f"offsetof(rl_refund_report,{f})" for f in FIELDS)
    src = tmp_path / "refund.c"
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int (*f0)(rl_engine*, const rl_batch*, const rl_status*, uint32_t, uint32_t*) = rl_refund_pipelined;\n'
                   'int (*f1)(rl_engine*, uint32_t) = rl_refund_behind;\n'
                   'int (*f2)(rl_engine*, rl_refund_report*) = rl_wait_refund;\n'
                   'int main(){size_t v[]={'
                   f'sizeof(rl_refund_report),RL_REFUND_KEEP_CACHE,RL_ADJUST_KEEP_CACHE,RL_ABI_VERSION,{offs}}};'
                   'for(unsigned i=0;i<sizeof v/sizeof v[0];++i)printf("%zu ",v[i]);return 0;}\n')
    obj = tmp_path / "refund.o"
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(obj)], check=True)
    exe = tmp_path / "refund"
    subprocess.run(["gcc", str(obj), "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [64, 1, 1, 7] + [8 * k for k in range(8)]
    R = hiprl.RlRefundReport
    assert C.sizeof(R) == 64 and [getattr(R, f).offset for f in FIELDS] == [8 * k for k in range(8)]
    assert hiprl.REFUND_KEEP_CACHE == 1 and hiprl.ABI_VERSION == 7
    assert list(hiprl.REFUND_REPORT_FIELDS) == FIELDS[:-1]


def test_library_exports_refund():
    lib = hiprl.load_library()
    names = {n for n, _, _ in hiprl.ABI}
    for fn in ("rl_refund_pipelined", "rl_refund_behind", "rl_wait_refund"):
        assert hasattr(lib, fn) and fn in names
    assert lib.rl_abi_version() == 7
    # null arguments are refused before anything touches the GPU
    assert lib.rl_refund_pipelined(None, None, None, 0, None) == -1
    assert lib.rl_refund_behind(None, 0) == -1 and lib.rl_wait_refund(None, None) == -1
    for m in ("refund_pipelined", "refund_behind", "wait_refund"):
        assert hasattr(hiprl.Engine, m)


# ---- the model against hand-worked cases ---------------------------------------------------------
def one_request(domain, keys, rules, hits, t=T):
    return (domain, [[("k", k)] for k in keys], rules, hits, t)


def run(o, reqs, keep=False):
    b = hiprl.build_batch(reqs)
    st, _ = o.submit(b)
    amounts, rep = o.refund(b, st, keep)
    return b, st, amounts, rep


def count(o, b, i):
    key, store = o._key(b, i)
    return o.peek(key, store, int(b.now[b.req_of[i]]))[0]


def test_model_cost_limiter_case():
    """9000 / 10000, a request of 1500 is rejected and refunded; 100 behind it passes."""
    o = RefundOracle([(10000, hiprl.HOUR)])
    b, st, amounts, rep = run(o, [one_request("c", ["a"], [0], 9000)])
    assert amounts == [0] and rep["rejected_req"] == 0 and rep["skipped"] == 1 and count(o, b, 0) == 9000
    b, st, amounts, rep = run(o, [one_request("c", ["a"], [0], 1500)])
    assert int(st["code_flags"][0]) & 0xFF == 2 and amounts == [1500]
    assert rep == dict(descriptors=1, rejected_req=1, skipped=0, absent=0, refunded=1, floored=0, unfrozen=0)
    assert count(o, b, 0) == 9000
    b, st, amounts, rep = run(o, [one_request("c", ["a"], [0], 100)])
    assert int(st["code_flags"][0]) & 0xFF == 1 and amounts == [0] and count(o, b, 0) == 9100
    # without the refund the reference refuses it
    o = RefundOracle([(10000, hiprl.HOUR)])
    for h in (9000, 1500):
        o.submit(hiprl.build_batch([one_request("c", ["a"], [0], h)]))
    st, _ = o.submit(hiprl.build_batch([one_request("c", ["a"], [0], 100)]))
    assert int(st["code_flags"][0]) & 0xFF == 2


def test_model_per_user_and_global():
    """Rejected by the global descriptor: the per-user descriptor's quota comes back too, and the
    over-limit descriptor itself is owed (it was counted)."""
    o = RefundOracle([(100, hiprl.HOUR), (5, hiprl.HOUR)])
    b, st, amounts, rep = run(o, [one_request("u", ["user1", "global"], [0, 1], 5)])
    assert amounts == [0, 0] and [count(o, b, i) for i in (0, 1)] == [5, 5]
    b, st, amounts, rep = run(o, [one_request("u", ["user1", "global"], [0, 1], 3)])
    assert [int(c) & 0xFF for c in st["code_flags"]] == [1, 2] and amounts == [3, 3]
    assert rep["rejected_req"] == 1 and rep["refunded"] == 2 and [count(o, b, i) for i in (0, 1)] == [5, 5]
    # two requests of one batch: the second was decided on the counters before the refund
    o = RefundOracle([(100, hiprl.HOUR), (5, hiprl.HOUR)])
    b, st, amounts, rep = run(o, [one_request("u", ["user1", "global"], [0, 1], 6),
                                   one_request("u", ["user2", "global"], [0, 1], 1)])
    assert [int(c) & 0xFF for c in st["code_flags"]] == [1, 2, 1, 2] and amounts == [6, 6, 1, 1]
    assert rep["rejected_req"] == 2 and [count(o, b, i) for i in range(4)] == [0, 0, 0, 0]


def test_model_shadow_local_cache_hit_and_nil():
    # a shadowed over-limit descriptor rejects nothing
    o = RefundOracle([(2, hiprl.HOUR, True), (100, hiprl.HOUR)])
    b, st, amounts, rep = run(o, [one_request("s", ["a", "b"], [0, 1], 5)])
    assert int(st["code_flags"][0]) == 1 | (4 | 1) << 8 and amounts == [0, 0] and rep["rejected_req"] == 0
    assert [count(o, b, i) for i in (0, 1)] == [5, 5]
    # a nil rule is owed nothing; a local-cache hit is owed nothing (no INCRBY happened), the
    # request's other descriptor is
    o = RefundOracle([(2, hiprl.HOUR), (100, hiprl.HOUR)], local_cache=True)
    b, st, amounts, rep = run(o, [one_request("l", ["a", "b", "n"], [0, 1, NIL], 5)], keep=True)
    assert amounts == [5, 5, 0] and rep["skipped"] == 1 and rep["unfrozen"] == 0
    assert [count(o, b, i) for i in (0, 1)] == [0, 0]
    b, st, amounts, rep = run(o, [one_request("l", ["a", "b", "n"], [0, 1, NIL], 1)], keep=True)
    assert int(st["code_flags"][0]) >> 8 & 2 and amounts == [0, 1, 0]
    assert rep == dict(descriptors=3, rejected_req=1, skipped=2, absent=0, refunded=1, floored=0, unfrozen=0)
    # without KEEP_CACHE the first refund (to 0 <= 2) clears the deadline: the key counts again
    o = RefundOracle([(2, hiprl.HOUR), (100, hiprl.HOUR)], local_cache=True)
    b, st, amounts, rep = run(o, [one_request("l", ["a", "b"], [0, 1], 5)])
    assert rep["unfrozen"] == 1
    b, st, amounts, rep = run(o, [one_request("l", ["a", "b"], [0, 1], 1)])
    assert [int(c) & 0xFF for c in st["code_flags"]] == [1, 1] and amounts == [0, 0]


def test_model_amounts_are_full_uint32():
    for h in (0, 1, 7, 2**31 - 1, 2**31, 2**32 - 1):
        amounts, n = refund_amounts([2, 1, 1 | 2 << 8, 1], [0, 0, 0, NIL], [0, 0, 0, 0], [h], 1)
        assert amounts == [max(1, h), max(1, h), 0, 0] and n == 1


@pytest.mark.parametrize("local_cache,split", [(False, False), (True, False), (False, True), (True, True)])
def test_model_is_the_oracle_without_refunds(local_cache, split):
    reqs = streams.make_stream(3, 1500, 1_700_000_000)
    o = oracle.Oracle(local_cache=local_cache, per_second_split=split)
    o.load_rules(streams.RULES)
    m = RefundOracle(streams.RULES, local_cache=local_cache, per_second_split=split)
    for i in range(0, len(reqs), 500):
        b = hiprl.build_batch(reqs[i:i + 500])
        streams.assert_same(*o.submit(b), *m.submit(b), f"batch at {i}")
