"""HipRateLimitCache::Resize / Occupancy and auto-grow (rl_cache.hpp) on the GPU, through the
batcher's queue: the C++ mirror answers as one oracle that never stopped across a resize, and
with HIP_TABLE_AUTOGROW set it grows its table before a region fills instead of refusing."""
import ctypes as C
from pathlib import Path

import pytest

import hiprl
import oracle

pytestmark = pytest.mark.gpu

T = 1_700_000_000


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(str(Path(__file__).resolve().parent / "cshim_resize" / "librl_resize_shim.so"))
    lib.rlz_create.restype = C.c_void_p
    lib.rlz_create.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    lib.rlz_error.restype = C.c_char_p
    lib.rlz_destroy.restype = None
    lib.rlz_batcher_stats.restype = None
    for f in (lib.rlz_destroy, lib.rlz_error):
        f.argtypes = [C.c_void_p]
    lib.rlz_set_time.argtypes = [C.c_void_p, C.c_int64]
    lib.rlz_add_rule.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.rlz_do_limit.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.rlz_resize.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    lib.rlz_occupancy.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    lib.rlz_batcher_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    return lib


def create(lib, log2, rules, autogrow=0, max_log2=(31, 31, 31, 31)):
    p = lib.rlz_create(1, (C.c_uint32 * 4)(*log2), autogrow, (C.c_uint32 * 4)(*max_log2))
    assert p
    for L, u in rules:
        lib.rlz_add_rule(p, L, u)
    return p


def occupancy(lib, p):
    w = (C.c_uint32 * 32)()
    assert lib.rlz_occupancy(p, w) == 0, lib.rlz_error(p)
    return {k: list(w[8 * i:8 * i + 8]) for i, k in enumerate(("gen", "live", "limit", "slots"))}


def batcher_stats(lib, p):
    w = (C.c_uint64 * 4)()
    lib.rlz_batcher_stats(p, w)
    return dict(zip(("batches", "drains", "resizes", "resize_failures"), list(w)))


def call(lib, p, o, domain_value, rule, hits, t):
    """One DoLimit; on success the oracle decides the same request and both must agree. Returns
    False when the cache threw RedisError (the oracle, which has no capacity bound, is not asked)."""
    out = (C.c_uint32 * 3)()
    if lib.rlz_do_limit(p, domain_value.encode(), rule, hits, out):
        return False
    st, thr = o.submit(hiprl.build_batch([("grow", [[("k", domain_value)]], [rule], hits, t)]))
    want = [int(st[0]["code_flags"]) & 0xFF, int(st[0]["limit_remaining"]), int(thr[0])]
    assert list(out) == want, (domain_value, list(out), want)
    return True


def test_resize_and_occupancy_through_the_queue(lib):
    rules = [(3, hiprl.MINUTE), (5, hiprl.HOUR), (2, hiprl.DAY)]
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)
    p = create(lib, (12, 12, 12, 12), rules)

    def calls(t, n, ctx):
        lib.rlz_set_time(p, t)
        for i in range(n):  # 13 values x 3 rules: 13 key strings per home unit
            assert call(lib, p, o, f"v{i % 13}", i % 3, 1 + i % 2, t), (ctx, i, lib.rlz_error(p))

    calls(T, 40, "before the resize")
    occ = occupancy(lib, p)
    assert occ["slots"] == [4096] * 8 and sum(occ["live"]) == 39 and max(occ["live"]) == 13
    assert lib.rlz_resize(p, (C.c_uint32 * 4)(8, 9, 10, 8)) == 0, lib.rlz_error(p)
    occ2 = occupancy(lib, p)
    assert occ2["slots"] == [256, 256, 512, 512, 1024, 1024, 256, 256]
    assert occ2["limit"] == [s * 750 // 1000 for s in occ2["slots"]]
    assert occ2["live"] == occ["live"] and occ2["gen"] == occ["gen"]
    calls(T + 5, 40, "after the resize")
    # a refused resize (16 slots, load limit 12, below the 13 live) throws and changes nothing
    occ3 = occupancy(lib, p)
    assert lib.rlz_resize(p, (C.c_uint32 * 4)(4, 4, 4, 4)) == -1
    assert b"load limit" in lib.rlz_error(p)
    assert occupancy(lib, p) == occ3
    calls(T + 6, 40, "after the refused resize")
    assert batcher_stats(lib, p)["resizes"] == 0  # auto-grow is off: Resize calls are not counted there
    lib.rlz_destroy(p)


def test_autogrow(lib):
    """HOUR regions of 256 slots, watermark 500 permille: live 129 -> 512 slots, 257 -> 1024,
    513 -> 2048, and 1000 <= 1024 ends it. The load limit of 192 is never reached: no refusal."""
    rules = [(4, hiprl.HOUR)]
    assert oracle.place(T // 3600 * 3600)[0] == 4
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)
    p = create(lib, (12, 12, 8, 12), rules, autogrow=500, max_log2=(12, 12, 12, 12))
    lib.rlz_set_time(p, T)
    for i in range(1000):
        assert call(lib, p, o, f"n{i}", 0, 1, T), (i, lib.rlz_error(p))
    bs = batcher_stats(lib, p)
    occ = occupancy(lib, p)
    assert bs["resizes"] == 3 and bs["resize_failures"] == 0, bs
    assert occ["slots"][4] == 2048 and occ["slots"][5] == 2048 and occ["live"][4] == 1000, occ
    assert occ["slots"][:4] == [4096] * 4 and occ["slots"][6:] == [4096] * 2
    # every counter was kept: a second hit of early, middle and late keys counts on
    for i in (0, 128, 129, 256, 257, 512, 513, 999):
        assert call(lib, p, o, f"n{i}", 0, 4, T), i
    lib.rlz_destroy(p)


def test_autogrow_off_refuses_as_before(lib):
    """The control arm: without auto-grow the same calls hit the 192-slot load limit."""
    rules = [(4, hiprl.HOUR)]
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)
    p = create(lib, (12, 12, 8, 12), rules, autogrow=0)
    lib.rlz_set_time(p, T)
    failed = None
    for i in range(200):
        if not call(lib, p, o, f"n{i}", 0, 1, T):
            failed = i
            break
    assert failed is not None and failed < 199, failed
    assert b"load limit" in lib.rlz_error(p)
    bs = batcher_stats(lib, p)
    assert bs["resizes"] == 0 and occupancy(lib, p)["slots"][4] == 256
    lib.rlz_destroy(p)


def test_autogrow_is_bounded(lib):
    """max_log2_slots 9: one growth to 512 slots, then the 384-slot load limit refuses as today."""
    rules = [(4, hiprl.HOUR)]
    o = oracle.Oracle(local_cache=True)
    o.load_rules(rules)
    p = create(lib, (12, 12, 8, 12), rules, autogrow=500, max_log2=(12, 12, 9, 12))
    lib.rlz_set_time(p, T)
    failed = None
    for i in range(400):
        if not call(lib, p, o, f"n{i}", 0, 1, T):
            failed = i
            break
    assert failed is not None and 192 < failed < 399, failed
    bs = batcher_stats(lib, p)
    occ = occupancy(lib, p)
    assert bs["resizes"] == 1 and bs["resize_failures"] == 0 and occ["slots"][4] == 512, (bs, occ)
    lib.rlz_destroy(p)
