"""Routed peek / forget (rl_hip.h "Routed peek / forget"), CPU only: the library's four entry
points, the header's flag against the Python binding, and the ABI version the change left alone."""
import subprocess
from pathlib import Path

import hiprl

ROOT = Path(__file__).resolve().parents[1]
NEW = ("rl_peek_routed", "rl_route_unpack_peek", "rl_router_peek", "rl_router_forget")


def test_library_exports_the_routed_entry_points():
    lib = hiprl.load_library()
    names = {n for n, _, _ in hiprl.ABI}
    for f in NEW:
        assert hasattr(lib, f), f
        assert f in names
    # null arguments are refused before anything touches the GPU
    assert lib.rl_peek_routed(None, None, 0, None, 0) == -1
    assert lib.rl_route_unpack_peek(None, None, None, None, None) == -1
    assert lib.rl_router_peek(None, None, None) == -1
    assert lib.rl_router_forget(None, None, None) == -1


def test_forget_flag_and_abi_version_match_header(tmp_path):
    src = tmp_path / "rp.c"
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\nint main(){'
                   'printf("%u %u %u %u", (unsigned)RL_PEEK_ROUTED_FORGET, (unsigned)RL_ABI_VERSION, '
                   '(unsigned)RL_ROUTE_RECORD_BYTES, (unsigned)sizeof(rl_peek_reply));'
                   'return 0;}\n')
    exe = tmp_path / "rp"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [hiprl.PEEK_ROUTED_FORGET, hiprl.ABI_VERSION, hiprl.ROUTE_RECORD_BYTES, hiprl.PEEK_DTYPE.itemsize]
    assert hiprl.PEEK_ROUTED_FORGET == 1 and hiprl.ABI_VERSION == 7
    assert hiprl.load_library().rl_abi_version() == 7
