"""HipRateLimitCache::Merge (rl_cache.hpp) through the batcher's queue (tests/cshim_merge): a
snapshot file is folded in one control call per chunk while client threads keep calling DoLimit —
the trace hook shows their batches between the chunks — a merge over the auto-grow watermark grows
the table, and a refused chunk says how many records are merged, so the caller resizes and resumes."""
import ctypes as C
import threading
from pathlib import Path

import pytest

import hiprl

pytestmark = pytest.mark.gpu
SHIM = Path(__file__).resolve().parent / "cshim_merge" / "librl_merge_shim.so"
OK = 1
T0 = 1_700_000_000
NAMES = ["Found", "LocalCached", "Count", "TtlSeconds", "CachedSeconds"]
REPORT = ["Records", "Folded", "Claimed", "DroppedOver", "DroppedEmpty"]
L = 100_000


def _lib():
    if not SHIM.exists():
        raise RuntimeError(f"{SHIM} missing (built by __graft_entry__.build())")
    lib = C.CDLL(str(SHIM))
    vp, u32, u64, cp, pu32, pu64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    lib.rlm_create.argtypes, lib.rlm_create.restype = [C.c_int, u32, pu32, u32, pu32, u32], vp
    lib.rlm_destroy.argtypes = [vp]
    lib.rlm_set_time.argtypes = [vp, C.c_int64]
    lib.rlm_add_rule.argtypes, lib.rlm_add_rule.restype = [vp, u32, u32], C.c_int
    lib.rlm_do_limit.argtypes = [vp, cp, cp, cp, C.c_int, u32, pu32, pu64, pu32]
    lib.rlm_peek.argtypes = [vp, cp, cp, cp, C.c_int, pu32]
    lib.rlm_merge.argtypes = [vp, cp, u64, pu64, pu64]
    lib.rlm_control_seqs.argtypes, lib.rlm_control_seqs.restype = [vp, pu64, u32], u32
    lib.rlm_resize.argtypes = [vp, pu32]
    lib.rlm_occupancy.argtypes = [vp, pu32]
    lib.rlm_resizes.argtypes, lib.rlm_resizes.restype = [vp], u64
    lib.rlm_error.argtypes, lib.rlm_error.restype = [vp], cp
    return lib


class Cache:
    def __init__(self, batch_limit, window_us=0, log2_slots=(12, 12, 12, 12), autogrow_permille=0,
                 max_log2_slots=(31, 31, 31, 31)):
        self.lib = _lib()
        self.h = self.lib.rlm_create(0, window_us, (C.c_uint32 * 4)(*log2_slots), autogrow_permille,
                                     (C.c_uint32 * 4)(*max_log2_slots), batch_limit)
        assert self.h, "HipRateLimitCache construction failed"
        self.rule = self.lib.rlm_add_rule(self.h, L, hiprl.HOUR)
        self.lib.rlm_set_time(self.h, T0)

    def error(self):
        return self.lib.rlm_error(self.h).decode()

    def do_limit(self, value, hits):
        out, seq, pos = (C.c_uint32 * 3)(), C.c_uint64(), C.c_uint32()
        assert self.lib.rlm_do_limit(self.h, b"mc", b"k", value.encode(), self.rule, hits, out, C.byref(seq),
                                     C.byref(pos)) == 0, self.error()
        return tuple(out), (seq.value, pos.value)

    def peek(self, value):
        out = (C.c_uint32 * 5)()
        assert self.lib.rlm_peek(self.h, b"mc", b"k", value.encode(), self.rule, out) == 0, self.error()
        return dict(zip(NAMES, out))

    def merge(self, path, first_record=0):
        """-> (report dict, None) or (None, records merged before the refusal)"""
        rep, merged = (C.c_uint64 * 5)(), C.c_uint64()
        if self.lib.rlm_merge(self.h, str(path).encode(), first_record, rep, C.byref(merged)):
            return None, merged.value
        return dict(zip(REPORT, rep)), None

    def control_seqs(self):
        out = (C.c_uint64 * 256)()
        n = self.lib.rlm_control_seqs(self.h, out, 256)
        return list(out[:n])

    def occupancy(self):
        out = (C.c_uint32 * 16)()
        assert self.lib.rlm_occupancy(self.h, out) == 0, self.error()
        return list(out[:8]), list(out[8:])

    def close(self):
        self.lib.rlm_destroy(self.h)


def snapshot_file(path, n):
    """A snapshot of n key strings "mc_k_v<i>_" of T0's HOUR window, string i counted 1 + i % 5."""
    e = hiprl.Engine(max_batch_desc=1 << 12)
    e.load_rules([(L, hiprl.HOUR)])
    e.submit(hiprl.build_batch([("mc", [[("k", f"v{i}")]], [0], 1 + i % 5, T0 - 5) for i in range(n)]))
    h, recs = e.snapshot_records()
    assert recs.shape[0] == n
    hiprl.write_snapshot(path, h, recs)
    e.close()
    return h


def test_merge_runs_between_the_callers_batches(tmp_path):
    n, T = 640, 4
    path = tmp_path / "old.rlsnap"
    snapshot_file(path, n)
    m = Cache(batch_limit=64, window_us=200)  # 64 records a chunk: ten control calls
    done = threading.Event()
    calls = [[] for _ in range(T)]

    def run(t):
        i = 0
        while i < 4000 and not (done.is_set() and i >= 50):
            v = (7 * t + i) % 20
            hits = 1 + (t + i) % 3
            (code, _, _), (seq, pos) = m.do_limit(f"v{v}", hits)
            calls[t].append((seq, pos, v, hits, code))
            i += 1

    th = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    while sum(len(c) for c in calls) < 40:  # the callers are under way
        pass
    rep, _ = m.merge(path)
    done.set()
    for x in th:
        x.join()
    assert rep == dict(Records=n, Folded=rep["Folded"], Claimed=n - rep["Folded"], DroppedOver=0, DroppedEmpty=0), rep
    assert rep["Folded"] <= 20  # only strings a caller had touched before their chunk
    ctl = m.control_seqs()
    assert len(ctl) == 10 and ctl == sorted(ctl), ctl
    flat = [c for per in calls for c in per]
    assert all(c[4] == OK and c[1] != 0xFFFFFFFF for c in flat)
    between = [c for c in flat if ctl[0] <= c[0] < ctl[-1]]
    assert ctl[-1] > ctl[0] and between, "no DoLimit batch was decided between the merge's chunks"
    spent = [0] * 20
    for _, _, v, hits, _ in flat:
        spent[v] += hits
    for i in list(range(25)) + [n - 1]:
        st = m.peek(f"v{i}")
        assert (st["Found"], st["Count"]) == (1, 1 + i % 5 + (spent[i] if i < 20 else 0)), (i, st)
    m.close()


def test_merge_over_the_watermark_is_followed_by_a_grow(tmp_path):
    path = tmp_path / "grow.rlsnap"
    snapshot_file(path, 40)
    m = Cache(batch_limit=16, log2_slots=(6, 6, 6, 6), autogrow_permille=500, max_log2_slots=(8, 8, 8, 8))
    assert m.occupancy()[1] == [64] * 8 and m.lib.rlm_resizes(m.h) == 0
    rep, _ = m.merge(path)  # chunks of 16, 16, 8: 40 live slots of 64 pass the watermark of 32
    assert rep == dict(Records=40, Folded=0, Claimed=40, DroppedOver=0, DroppedEmpty=0), rep
    live, slots = m.occupancy()
    assert m.lib.rlm_resizes(m.h) == 1 and sorted(slots) == [64] * 6 + [128] * 2 and max(live) == 40
    for i in range(40):
        st = m.peek(f"v{i}")
        assert (st["Found"], st["Count"], st["TtlSeconds"]) == (1, 1 + i % 5, 3595), (i, st)
    m.close()


def test_refused_chunk_names_the_merged_count_and_resumes_after_a_resize(tmp_path):
    path = tmp_path / "full.rlsnap"
    snapshot_file(path, 60)
    m = Cache(batch_limit=16, log2_slots=(6, 6, 6, 6))  # 64 slots, load limit 48
    rep, merged = m.merge(path)
    assert rep is None and merged == 48, (rep, merged, m.error())
    assert "48 records" in m.error() and "first_record = 48" in m.error(), m.error()
    assert max(m.occupancy()[0]) == 48
    assert m.lib.rlm_resize(m.h, (C.c_uint32 * 4)(0, 0, 7, 0)) == 0, m.error()
    rep, _ = m.merge(path, 48)
    assert rep == dict(Records=12, Folded=0, Claimed=12, DroppedOver=0, DroppedEmpty=0), rep
    assert max(m.occupancy()[0]) == 60
    for i in range(60):
        assert m.peek(f"v{i}")["Count"] == 1 + i % 5, i
    # a file that is no snapshot, and a start past its end, are refused before anything is merged
    bad = tmp_path / "cut.rlsnap"
    bad.write_bytes(path.read_bytes()[:-32])
    assert m.merge(bad) == (None, 2**64 - 1) and "n_records" in m.error()
    assert m.merge(path, 61) == (None, 2**64 - 1)
    assert m.merge(path, 60)[0] == dict.fromkeys(REPORT, 0)
    m.close()
