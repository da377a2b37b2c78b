"""Routed set (rl_hip.h "Routed set"), CPU only: the library's three entry points, their
prototypes in the header against the Python binding, and the ABI version the change left alone."""
import ctypes as C
import subprocess
from pathlib import Path

import hiprl

ROOT = Path(__file__).resolve().parents[1]
NEW = ("rl_set_routed_plan", "rl_set_routed_commit", "rl_router_set")


def test_library_exports_the_routed_set_entry_points():
    lib = hiprl.load_library()
    names = {n for n, _, _ in hiprl.ABI}
    for f in NEW:
        assert hasattr(lib, f), f
        assert f in names
    # null arguments are refused before anything touches the GPU
    assert lib.rl_set_routed_plan(None, None, None, 0, None) == -1
    assert lib.rl_set_routed_commit(None, 1) == -1
    assert lib.rl_router_set(None, None, None, None) == -1
    for m in ("set_routed_plan", "set_routed_commit"):
        assert hasattr(hiprl.Engine, m), m
    assert hasattr(hiprl.Router, "set")


def test_prototypes_and_abi_version_match_header(tmp_path):
    # the header's prototypes are assignable to the shapes the binding declares (a mismatch is a
    # compile error under -Werror), and the version did not move
    src = tmp_path / "rs.c"
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n'
                   'int (*f_plan)(rl_engine*, const void*, const rl_peek_reply*, uint32_t, rl_peek_reply*) = '
                   'rl_set_routed_plan;\n'
                   'int (*f_commit)(rl_engine*, int) = rl_set_routed_commit;\n'
                   'int (*f_set)(rl_router*, const rl_batch*, const rl_peek_reply* const*, rl_peek_reply* const*) = '
                   'rl_router_set;\n'
                   'int main(){printf("%u %u %u", (unsigned)RL_ABI_VERSION, (unsigned)RL_ROUTE_RECORD_BYTES, '
                   '(unsigned)sizeof(rl_peek_reply)); return 0;}\n')
    obj = tmp_path / "rs.o"
    subprocess.run(["gcc", "-Werror", "-c", "-I", str(ROOT / "include"), str(src), "-o", str(obj)], check=True)
    exe = tmp_path / "rs"
    subprocess.run(["gcc", str(obj), "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [hiprl.ABI_VERSION, hiprl.ROUTE_RECORD_BYTES, hiprl.PEEK_DTYPE.itemsize]
    # a value is half a record: the record exchange's count vectors carry the values scaled 16 / 32
    assert hiprl.ROUTE_RECORD_BYTES == 2 * hiprl.PEEK_DTYPE.itemsize
    assert hiprl.ABI_VERSION == 7 and hiprl.load_library().rl_abi_version() == 7
    abi = {n: (a, r) for n, a, r in hiprl.ABI}
    assert abi["rl_set_routed_plan"] == ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p], C.c_int)
    assert abi["rl_set_routed_commit"] == ([C.c_void_p, C.c_int], C.c_int)
    assert len(abi["rl_router_set"][0]) == 4
