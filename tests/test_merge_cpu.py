"""rl_merge without a GPU: rl_merge_report's layout against the ctypes struct, the exported
symbols, and the rule of the merge (rl_merge.h merge_fold / merge_class / merge_leaves, which the
kernels and the engine's host pass share) against an independent Python model."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import pytest

import hiprl

ROOT = Path(__file__).resolve().parents[1]
M32 = (1 << 32) - 1


def test_report_layout_matches_ctypes(tmp_path):
    fields = list(hiprl.MERGE_REPORT_FIELDS) + ["reserved"]
    offs = ",".join(f"offsetof(rl_merge_report,{f})" for f in fields)
    src = tmp_path / "merge.c"
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){size_t v[]={'
                   f'sizeof(rl_merge_report),{offs}}};'
                   'for(unsigned i=0;i<sizeof v/sizeof v[0];++i)printf("%zu ",v[i]);return 0;}\n')
    exe = tmp_path / "merge"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = hiprl.RlMergeReport
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f in fields]
    assert C.sizeof(R) == 64
    assert [f for f, _ in R._fields_] == fields == ["records", "folded", "claimed", "dropped_over", "dropped_empty",
                                                    "reserved"]


def test_library_exports_merge():
    lib = hiprl.load_library()
    assert hasattr(lib, "rl_merge")
    assert "rl_merge" in [n for n, _, _ in hiprl.ABI]
    assert lib.rl_abi_version() == hiprl.ABI_VERSION == 7
    assert lib.rl_merge(None, None, None, 0, 0, None) == -1  # RL_EINVAL before any device call


def host_rule():
    lib = hiprl.load_library()
    U4 = C.c_uint32 * 4
    lib.rlx_merge_fold_host.argtypes = [U4, C.c_int, U4, C.c_uint32, U4]
    lib.rlx_merge_fold_host.restype = None
    lib.rlx_merge_class_host.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    lib.rlx_merge_class_host.restype = C.c_uint32
    lib.rlx_merge_leaves_host.argtypes = [U4, C.c_uint32, C.c_int]
    lib.rlx_merge_leaves_host.restype = C.c_int

    def fold(S, found, R, now):
        out = U4()
        lib.rlx_merge_fold_host(U4(*S), int(found), U4(*R), now, out)
        return tuple(out)

    return lib, fold, U4


def model_fold(S, found, R, now):
    """The contract of rl_hip.h "Merge", from its words. States are (count, exp, pcount, frz)."""
    sc, se, sp, sf = S if found else (0, 0, 0, 0)
    rc, re_, rp, rf = R
    alive_r, alive_s = now < re_, found and now < se
    if alive_r and alive_s:
        count, exp = (sc + rc) & M32, max(se, re_)
    elif alive_r:
        count, exp = rc, re_
    else:
        count, exp = sc, se
    return (count, exp, (sp + rp) & M32, max(sf, rf))


def test_fold_rule_matches_the_model():
    _, fold, _ = host_rule()
    now = 1_700_000_000
    exps = [0, now - 1, now, now + 1]
    counts = [(0, 0), (5, 9), (M32 - 1, 1), (M32, 1), (M32, 2), (1 << 31, 1 << 31), (3, M32)]  # sums 2^32-1, 2^32, 2^32+1
    pcs = [(0, 0), (7, 0), (0, 7), (M32, 1), (M32, M32)]
    frzs = [(0, 0), (now - 1, now + 1), (now + 1, now - 1), (now, now), (now + 5, now + 9)]
    n = 0
    for es, er, (cs, cr), found in itertools.product(exps, exps, counts, (False, True)):
        for (ps, pr), (fs, fr) in zip(itertools.cycle(pcs), frzs + frzs[::-1] + frzs):
            S, R = (cs, es, ps, fs), (cr, er, pr, fr)
            assert fold(S, found, R, now) == model_fold(S, found, R, now), (S, found, R)
            n += 1
    for (ps, pr), (fs, fr) in itertools.product(pcs, frzs):  # the two side words on their own grid
        for found in (False, True):
            S, R = (1, now + 1, ps, fs), (2, now + 2, pr, fr)
            assert fold(S, found, R, now) == model_fold(S, found, R, now), (S, found, R)
            n += 1
    assert n > 3000
    # spelled out: both alive add in 32 bits and take the later expiry; a dead slot is replaced;
    # a dead record changes only the side words; a fresh claim starts from zeros
    assert fold((M32, now + 3, 1, 0), True, (2, now + 1, M32, now + 9), now) == (1, now + 3, 0, now + 9)
    assert fold((40, now, 0, 0), True, (2, now + 1, 0, 0), now) == (2, now + 1, 0, 0)
    assert fold((40, now + 7, 0, 50), True, (2, now, 3, 20), now) == (40, now + 7, 3, 50)
    assert fold((40, now + 7, 9, 50), False, (2, now, 3, 20), now) == (0, 0, 3, 20)


def test_class_rule():
    lib, _, _ = host_rule()
    NEWEST, PREVIOUS, OVER = 0, 1, 2
    for T in (5, 6, 472_222_223, M32 - 2):
        for lazy in (0, 1):
            for g in range(T - 4, T + 3):
                want = NEWEST if g == T else PREVIOUS if lazy and g + 2 == T else OVER
                assert lib.rlx_merge_class_host(g, T, lazy) == want, (g, T, lazy)
    for lazy in (0, 1):  # generation 0 is a never-used slot, whatever the target
        assert lib.rlx_merge_class_host(0, 0, lazy) == OVER and lib.rlx_merge_class_host(0, 2, lazy) == OVER


@pytest.mark.parametrize("local_cache", [0, 1])
def test_leaves_rule(local_cache):
    lib, _, U4 = host_rule()
    now = 1000
    for exp, pc, frz in itertools.product([0, now - 1, now, now + 1], [0, 1, M32], [0, now - 1, now, now + 1]):
        want = now < exp or pc != 0 or (bool(local_cache) and now < frz)
        assert lib.rlx_merge_leaves_host(U4(77, exp, pc, frz), now, local_cache) == int(want), (exp, pc, frz)
