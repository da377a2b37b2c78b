"""Peek / forget (rl_hip.h "Peek / forget"), CPU only: rl_peek_reply's layout and flag values
against the Python binding, and the library's entry points."""
import subprocess
from pathlib import Path

import hiprl

ROOT = Path(__file__).resolve().parents[1]

FIELDS = ["count", "ttl_s", "cached_s", "flags"]


def test_reply_layout_and_flags_match_header(tmp_path):
    offs = ",".join(f"offsetof(rl_peek_reply,{f})" for f in FIELDS)
    src = tmp_path / "peek.c"
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){size_t v[]={'
                   f'sizeof(rl_peek_reply),RL_PEEK_FOUND,RL_PEEK_LOCAL_CACHED,RL_PEEK_NIL,RL_PEEK_PER_SECOND,'
                   f'RL_PEEK_BAD,RL_ABI_VERSION,{offs}}};'
                   'for(unsigned i=0;i<sizeof v/sizeof v[0];++i)printf("%zu ",v[i]);return 0;}\n')
    exe = tmp_path / "peek"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = hiprl.PEEK_DTYPE
    want = [D.itemsize, hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND,
            hiprl.PEEK_BAD, hiprl.ABI_VERSION] + [D.fields[f][1] for f in FIELDS]
    assert got == want
    assert D.itemsize == 16 and list(D.names) == FIELDS
    assert [hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED, hiprl.PEEK_NIL, hiprl.PEEK_PER_SECOND, hiprl.PEEK_BAD] == [
        1, 2, 4, 8, 16]


def test_library_exports_peek_and_forget():
    lib = hiprl.load_library()
    names = {n for n, _, _ in hiprl.ABI}
    for f in ("rl_peek", "rl_peek_device", "rl_forget"):
        assert hasattr(lib, f), f
        assert f in names
    # null arguments are refused before anything touches the GPU
    assert lib.rl_peek(None, None, None) == -1
    assert lib.rl_peek_device(None, None, None) == -1
    assert lib.rl_forget(None, None, None) == -1
