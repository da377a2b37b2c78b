"""Adjust in flight (rl_hip.h "Adjust in flight"), CPU only: the three prototypes against the header
and against the ctypes declarations, the ABI version, and the library's entry points."""
import ctypes as C
import subprocess
from pathlib import Path

import hiprl

ROOT = Path(__file__).resolve().parents[1]

PROTOS = {
    "rl_adjust_pipelined": "int (*f0)(rl_engine*, const rl_batch*, const int32_t*, uint32_t, rl_peek_reply*)",
    "rl_adjust_submit": "int (*f1)(rl_engine*, const rl_batch*, const int32_t*, uint32_t, int)",
    "rl_wait_adjust": "int (*f2)(rl_engine*, rl_peek_reply*, rl_adjust_report*)",
}
# the ctypes declaration of each, argument by argument: pointers are c_void_p or a typed pointer
CTYPES = {
    "rl_adjust_pipelined": [C.c_void_p, C.POINTER(hiprl.RlBatch), C.c_void_p, C.c_uint32, C.c_void_p],
    "rl_adjust_submit": [C.c_void_p, C.POINTER(hiprl.RlBatch), C.c_void_p, C.c_uint32, C.c_int],
    "rl_wait_adjust": [C.c_void_p, C.c_void_p, C.POINTER(hiprl.RlAdjustReport)],
}


def test_prototypes_match_the_header_and_ctypes(tmp_path):
    src = tmp_path / "adjp.c"
    body = "".join(f"{decl} = {name};\n" for name, decl in PROTOS.items())
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n' + body +
                   'int main(){printf("%u %d", (unsigned)RL_ABI_VERSION, RL_MAX_IN_FLIGHT);return 0;}\n')
    obj = tmp_path / "adjp.o"
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(obj)], check=True)
    exe = tmp_path / "adjp"
    subprocess.run(["gcc", str(obj), "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all"], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert got == ["7", "3"]
    abi = {n: (a, r) for n, a, r in hiprl.ABI}
    for name, want in CTYPES.items():
        assert name in abi, name
        argt, rest = abi[name]
        assert argt == want and rest is C.c_int, name


def test_library_exports_the_entry_points():
    lib = hiprl.load_library()
    assert lib.rl_abi_version() == 7 and hiprl.ABI_VERSION == 7
    for name in PROTOS:
        assert hasattr(lib, name), name
    # null arguments are refused before anything touches the GPU
    assert lib.rl_adjust_pipelined(None, None, None, 0, None) == -1
    assert lib.rl_adjust_submit(None, None, None, 0, 0) == -1
    assert lib.rl_wait_adjust(None, None, None) == -1
    for m in ("adjust_pipelined", "adjust_submit", "wait_adjust"):
        assert hasattr(hiprl.Engine, m), m
