"""Resize (rl_hip.h "Resize"), CPU only: the header declares rl_resize, the library exports it,
the Python binding binds it, and the ABI version is the one tests/test_abi.py pins."""
import re
from pathlib import Path

import hiprl

ROOT = Path(__file__).resolve().parents[1]


def test_header_declares_and_library_exports_resize():
    header = (ROOT / "include" / "rl_hip.h").read_text()
    assert re.search(r"\bint\s+rl_resize\s*\(\s*rl_engine\s*\*\s*e\s*,\s*const\s+uint32_t\s+log2_slots\[4\]\s*\)\s*;",
                     header)
    lib = hiprl.load_library()
    assert hasattr(lib, "rl_resize")
    assert "rl_resize" in {n for n, _, _ in hiprl.ABI}
    assert callable(getattr(hiprl.Engine, "resize", None))
    assert callable(getattr(hiprl.HipRateLimitCache, "resize", None))
    # null arguments are refused before anything touches the GPU
    assert lib.rl_resize(None, None) == -1


def test_abi_version_is_unchanged():
    assert hiprl.load_library().rl_abi_version() == hiprl.ABI_VERSION == 7
