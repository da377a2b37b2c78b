"""Routed adjust (rl_hip.h "Routed adjust"), CPU only: the library's four entry points, their
prototypes in the header against the Python binding, the ABI version the change left alone, and the
dict model (routed_adjust_model.py) against hand-written cases."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import hiprl
from adjust_model import adjust_model
from routed_adjust_model import routed_adjust_model

ROOT = Path(__file__).resolve().parents[1]
NEW = ("rl_route_pack_adjust", "rl_adjust_routed_plan", "rl_adjust_routed_commit", "rl_router_adjust")
F, LC, NILF, PS = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND


def test_library_exports_the_routed_adjust_entry_points():
    lib = hiprl.load_library()
    names = {n for n, _, _ in hiprl.ABI}
    for f in NEW:
        assert hasattr(lib, f), f
        assert f in names
    # null arguments are refused before anything touches the GPU
    assert lib.rl_route_pack_adjust(None, None, None, None, 0, None) == -1
    assert lib.rl_adjust_routed_plan(None, None, 0, None) == -1
    assert lib.rl_adjust_routed_commit(None, 1, None) == -1
    assert lib.rl_router_adjust(None, None, None, None, None, None) == -1
    assert lib.rl_abi_version() == 7
    for m in ("route_pack_adjust", "adjust_routed_plan", "adjust_routed_commit"):
        assert hasattr(hiprl.Engine, m), m
    assert hasattr(hiprl.Router, "adjust")


def test_prototypes_and_abi_version_match_header(tmp_path):
    # the header's prototypes are assignable to the shapes its "Routed adjust" section documents (a
    # mismatch is a compile error under -Werror), and the version did not move
    src = tmp_path / "ra.c"
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n'
                   'int (*f_pack)(rl_engine*, const rl_batch*, const uint32_t*, const int32_t*, uint32_t, void*) = '
                   'rl_route_pack_adjust;\n'
                   'int (*f_plan)(rl_engine*, const void*, uint32_t, rl_peek_reply*) = rl_adjust_routed_plan;\n'
                   'int (*f_commit)(rl_engine*, int, rl_adjust_report*) = rl_adjust_routed_commit;\n'
                   'int (*f_adj)(rl_router*, const rl_batch*, const int32_t* const*, const uint32_t*, '
                   'rl_peek_reply* const*, rl_adjust_report* const*) = rl_router_adjust;\n'
                   'int main(){printf("%u %u %u %u", (unsigned)RL_ABI_VERSION, (unsigned)RL_ROUTE_RECORD_BYTES, '
                   '(unsigned)RL_ADJUST_KEEP_CACHE, (unsigned)sizeof(rl_adjust_report)); return 0;}\n')
    obj = tmp_path / "ra.o"
    subprocess.run(["gcc", "-Wall", "-Werror", "-c", "-I", str(ROOT / "include"), str(src), "-o", str(obj)], check=True)
    exe = tmp_path / "ra"
    subprocess.run(["gcc", str(obj), "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [hiprl.ABI_VERSION, hiprl.ROUTE_RECORD_BYTES, hiprl.ADJUST_KEEP_CACHE, C.sizeof(hiprl.RlAdjustReport)]
    assert hiprl.ABI_VERSION == 7 and hiprl.load_library().rl_abi_version() == 7
    abi = {n: (a, r) for n, a, r in hiprl.ABI}
    assert abi["rl_route_pack_adjust"] == ([C.c_void_p, C.POINTER(hiprl.RlBatch), C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_void_p], C.c_int)
    assert abi["rl_adjust_routed_plan"] == ([C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p], C.c_int)
    assert abi["rl_adjust_routed_commit"] == ([C.c_void_p, C.c_int, C.POINTER(hiprl.RlAdjustReport)], C.c_int)
    assert len(abi["rl_router_adjust"][0]) == 6


# ---- the model against hand-written cases --------------------------------------------------------
def replies(rows):
    return np.array([tuple(r) for r in rows], hiprl.PEEK_DTYPE).reshape(len(rows))


def report(n, **kw):
    return dict(dict.fromkeys(hiprl.ADJUST_REPORT_FIELDS, 0), descriptors=n, **kw)


def test_model_sums_across_origins_once():
    # a counter of 5 given -10 by origin 0 and +3 by origin 1 ends at 0 with floored == 1, in either order
    five = replies([(5, 40, 0, F)])
    for d in ([[-10], [3]], [[3], [-10]]):
        outs, rep = routed_adjust_model([["k"], ["k"]], [five, five], d, [[9], [9]], [False, False])
        assert [o.tolist() for o in outs] == [[(0, 40, 0, F)]] * 2
        assert rep == report(2, applied=2, floored=1)
    # an origin with nothing, nil and absent descriptors beside a found one
    outs, rep = routed_adjust_model([[], [None, "gone", "k"], ["k"]],
                                    [replies([]), replies([(0, 0, 0, NILF), (0, 0, 0, 0), (5, 40, 0, F)]), five],
                                    [[], [7, 7, 1], [1]], [[], [9, 9, 9], [9]], [False, False, False])
    assert [len(o) for o in outs] == [0, 3, 1]
    assert outs[1].tolist() == [(0, 0, 0, NILF), (0, 0, 0, 0), (7, 40, 0, F)] and outs[2].tolist() == [(7, 40, 0, F)]
    assert rep == report(4, nil=1, absent=1, applied=2)


def test_model_mixed_keep_rule():
    frozen = (12, 50, 60, F | LC)
    one = replies([frozen])
    # released if any found descriptor of the pair comes without keep ...
    for keeps in ([True, False], [False, True], [False, False]):
        outs, rep = routed_adjust_model([["k"], ["k"]], [one, one], [[-1], [-1]], [[10], [10]], keeps, local_cache=True)
        assert [o.tolist() for o in outs] == [[(10, 50, 0, F)]] * 2 and rep["unfrozen"] == 1, keeps
    # ... and never if all carry it
    outs, rep = routed_adjust_model([["k"], ["k"]], [one, one], [[-1], [-1]], [[10], [10]], [True, True], local_cache=True)
    assert [o.tolist() for o in outs] == [[(10, 50, 60, F | LC)]] * 2 and rep["unfrozen"] == 0
    # per descriptor inside one origin; an absent descriptor without keep releases nothing
    outs, rep = routed_adjust_model([["k", "gone"], ["k"]], [replies([frozen, (0, 0, 0, 0)]), one], [[-1, -1], [-1]],
                                    [[10, 10], [10]], [[True, False], [True]], local_cache=True)
    assert outs[0].tolist() == [(10, 50, 60, F | LC), (0, 0, 0, 0)] and rep["unfrozen"] == 0 and rep["absent"] == 1
    # the no-keep descriptor's own delta need not be negative: the pair's net and the pair's flag decide
    outs, rep = routed_adjust_model([["k"], ["k"]], [one, one], [[-3], [1]], [[10], [10]], [True, False], local_cache=True)
    assert [o.tolist() for o in outs] == [[(10, 50, 0, F)]] * 2 and rep["unfrozen"] == 1
    # a cache that is off releases nothing
    outs, rep = routed_adjust_model([["k"]], [one], [[-5]], [[10]], [False], local_cache=False)
    assert outs[0].tolist() == [(7, 50, 60, F | LC)] and rep["unfrozen"] == 0


def test_model_equals_adjust_model_with_one_flag():
    before = replies([(0, 0, 0, NILF), (0, 0, 0, PS), (4, 0, 1, F | PS | LC), (4, 30, 1, F | LC), (0xFFFFFFF0, 9, 0, F),
                      (7, 9, 0, F)])
    strings = [None, "gone", "two", "two", "top", "low"]
    deltas, limits = [5, 5, -1, -2, 2**31 - 1, -2**31], [3, 3, 3, 3, 1, 1]
    for keep in (False, True):
        want_after, want_rep = adjust_model(strings, before, deltas, limits, local_cache=True, keep_cache=keep)
        # one origin, and the same descriptors split over two
        outs, rep = routed_adjust_model([strings], [before], [deltas], [limits], [keep], local_cache=True)
        assert np.array_equal(outs[0], want_after) and rep == want_rep
        outs, rep = routed_adjust_model([strings[:3], strings[3:]], [before[:3], before[3:]], [deltas[:3], deltas[3:]],
                                        [limits[:3], limits[3:]], [keep, keep], local_cache=True)
        assert np.array_equal(np.concatenate(outs), want_after) and rep == want_rep
