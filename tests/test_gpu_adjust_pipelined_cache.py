"""HipRateLimitCache::AdjustQueued (rl_cache.hpp) through the batcher's queue
(tests/cshim_adjust_pipelined): queued adjusts are gathered beside the DoLimit calls and go to the
engine as rl_adjust_submit flights behind the gather's decision batch, with nothing drained. Every
call's place in the serial order is the one the trace hook reports; replayed in that order, the
DoLimit calls through the oracle and each gathered adjust group through the dict model of
adjust_model.py, it gives every answer."""
import ctypes as C
import threading
from pathlib import Path

import numpy as np
import pytest

import hiprl
import oracle
from adjust_model import adjust_model

pytestmark = pytest.mark.gpu
SHIM = Path(__file__).resolve().parent / "cshim_adjust_pipelined" / "librl_adjust_pipelined_shim.so"
OK, OVER_LIMIT = 1, 2
NAMES = ["Found", "LocalCached", "Count", "TtlSeconds", "CachedSeconds"]
PEEK, ADJUST, QUEUED = 0, 1, 2
F, LC = hiprl.PEEK_FOUND, hiprl.PEEK_LOCAL_CACHED
T0 = 1_700_000_000


def _lib():
    if not SHIM.exists():
        raise RuntimeError(f"{SHIM} missing (built by __graft_entry__.build())")
    lib = C.CDLL(str(SHIM))
    vp, u32, u64, cp, pu32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint32)
    lib.rlq_create.argtypes, lib.rlq_create.restype = [C.c_int, u32, pu32, u32], vp
    lib.rlq_destroy.argtypes = [vp]
    lib.rlq_set_time.argtypes = [vp, C.c_int64]
    lib.rlq_add_rule.argtypes, lib.rlq_add_rule.restype = [vp, u32, u32], C.c_int
    lib.rlq_do_limit.argtypes = [vp, cp, cp, cp, C.c_int, u32, pu32, C.POINTER(u64), pu32]
    lib.rlq_by_key.argtypes = [vp, C.c_int, cp, cp, cp, C.c_int, C.POINTER(C.c_int32), u32, C.c_int, pu32,
                               C.POINTER(u64), pu32]
    lib.rlq_drains.argtypes, lib.rlq_drains.restype = [vp], u64
    lib.rlq_batches.argtypes, lib.rlq_batches.restype = [vp], u64
    for f in (lib.rlq_trace_control, lib.rlq_trace_adjust, lib.rlq_trace_adjust_keep):
        f.restype = u32
    lib.rlq_error.argtypes, lib.rlq_error.restype = [vp], cp
    return lib


class Cache:
    def __init__(self, local_cache, window_us=0, log2_slots=(12, 12, 12, 12), batch_limit=1 << 12):
        self.lib = _lib()
        self.h = self.lib.rlq_create(int(local_cache), window_us, (C.c_uint32 * 4)(*log2_slots), batch_limit)
        assert self.h, "HipRateLimitCache construction failed"
        self.ctl, self.adj, self.adj_keep = (self.lib.rlq_trace_control(), self.lib.rlq_trace_adjust(),
                                             self.lib.rlq_trace_adjust_keep())

    def _ok(self, rc):
        if rc:
            raise hiprl.RedisError(self.lib.rlq_error(self.h).decode())

    def do_limit(self, key, rule, hits):
        """-> (code, remaining, throttle), (seq, pos)"""
        out, seq, pos = (C.c_uint32 * 3)(), C.c_uint64(), C.c_uint32()
        self._ok(self.lib.rlq_do_limit(self.h, b"q", b"k", key.encode(), rule, hits, out, C.byref(seq), C.byref(pos)))
        return tuple(out), (seq.value, pos.value)

    def by_key(self, how, key, rule, deltas=0, keep_cache=False):
        """Peek / Adjust / AdjustQueued of one descriptor per delta, all the same key -> the first
        one's status before, (seq, pos)"""
        deltas = [deltas] if isinstance(deltas, int) else list(deltas)
        out, seq, pos = (C.c_uint32 * 5)(), C.c_uint64(), C.c_uint32()
        self._ok(self.lib.rlq_by_key(self.h, how, b"q", b"k", key.encode(), rule, (C.c_int32 * len(deltas))(*deltas),
                                     len(deltas), int(keep_cache), out, C.byref(seq), C.byref(pos)))
        return dict(zip(NAMES, out)), (seq.value, pos.value)

    def close(self):
        self.lib.rlq_destroy(self.h)


def test_queued_adjust_alone_and_beside_the_control_call():
    m = Cache(True)
    rule = m.lib.rlq_add_rule(m.h, 5, hiprl.MINUTE)
    m.lib.rlq_set_time(m.h, T0 + 7)
    # a rule first seen by AdjustQueued is registered; an absent key stays absent; the call is
    # traced as a queued adjust, in a gather of its own
    before, (seq0, pos) = m.by_key(QUEUED, "v", rule, 4)
    assert before == dict.fromkeys(NAMES, 0) and pos == m.adj and seq0 != 2**64 - 1
    assert m.by_key(PEEK, "v", rule)[0] == dict.fromkeys(NAMES, 0)
    assert m.do_limit("v", rule, 6)[0][:2] == (OVER_LIMIT, 0)  # 6 > 5: over, and frozen
    st, _ = m.by_key(PEEK, "v", rule)
    assert (st["Found"], st["Count"], st["LocalCached"]) == (1, 6, 1)
    # keep_cache: the quota comes back, the key stays frozen; its trace position carries the keep bit
    before, (_, pos) = m.by_key(QUEUED, "v", rule, -1, keep_cache=True)
    assert before == st and pos == m.adj | m.adj_keep
    assert m.do_limit("v", rule, 1)[0][:2] == (OVER_LIMIT, 0)
    # two refunds of one key in one call add up, and release the key
    before, (seq1, pos) = m.by_key(QUEUED, "v", rule, [-1, -2])
    assert (before["Count"], before["LocalCached"]) == (5, 1) and pos == m.adj
    st, _ = m.by_key(PEEK, "v", rule)
    assert (st["Found"], st["LocalCached"], st["Count"], st["CachedSeconds"]) == (1, 0, 2, 0)
    (code, rem, _), (seq2, pos2) = m.do_limit("v", rule, 1)
    assert (code, rem) == (OK, 2) and seq2 > seq1 and pos2 < m.adj
    # Adjust, the control call, still traces as a control call
    before, (_, pos) = m.by_key(ADJUST, "v", rule, -1)
    assert pos == m.ctl and before["Count"] == 3
    # a nil limit: nothing
    assert m.by_key(QUEUED, "v", -1, -3)[0] == dict.fromkeys(NAMES, 0)
    assert m.by_key(PEEK, "v", rule)[0]["Count"] == 2
    assert m.lib.rlq_drains(m.h) == 0
    m.close()


def test_callers_and_queued_adjusts_replay_in_the_traced_order():
    """8 threads call DoLimit and 4 call AdjustQueued on 16 shared keys, 200 calls each."""
    TD, TA, n, L, K = 8, 4, 200, 40, 16
    m = Cache(True, window_us=200)
    rule = m.lib.rlq_add_rule(m.h, L, hiprl.HOUR)
    m.lib.rlq_set_time(m.h, T0)
    keys = [f"s{j}" for j in range(K)]
    # one call before the race, so that registering the rule is not part of it
    assert m.do_limit("warm", rule, 1)[0][:2] == (OK, L - 1)
    drains0 = m.lib.rlq_drains(m.h)
    events = [[] for _ in range(TD + TA)]

    def caller(t):
        rng = np.random.default_rng(t)
        for i in range(n):
            key, hits = keys[int(rng.integers(0, K))], 1 + int(rng.integers(0, 3))
            (code, rem, _), (seq, pos) = m.do_limit(key, rule, hits)
            events[t].append((seq, pos, "call", key, hits, (code, rem)))

    def adjuster(t):
        rng = np.random.default_rng(100 + t)
        keep = t == TD + TA - 1  # one thread's adjusts keep the cache entry
        for i in range(n):
            key, d = keys[int(rng.integers(0, K))], int(rng.integers(-6, 2))
            before, (seq, pos) = m.by_key(QUEUED, key, rule, d, keep_cache=keep)
            assert pos & m.adj and bool(pos & m.adj_keep) == keep and pos != m.ctl
            events[t].append((seq, pos, "adjust", key, d, before))

    th = [threading.Thread(target=caller if t < TD else adjuster, args=(t,)) for t in range(TD + TA)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert m.lib.rlq_drains(m.h) == drains0, "the drain count does not grow"
    ev = sorted((e for per in events for e in per), key=lambda e: (e[0], e[1]))
    assert len({(e[0], e[1]) for e in ev}) == (TD + TA) * n, "every call has a place of its own"

    # The replay. state: key -> [count, exists, frozen]. DoLimit through the oracle: a key whose
    # counter an adjust moved continues there under a fresh name charged its new count at once
    # (the oracle has no command that lowers a counter); where that charge cannot give the key's
    # cache state (frozen at or under the limit after a keep_cache refund, or over the limit and not
    # frozen after a true-up) the one-key DoLimit rules of test_gpu_adjust_cache.py decide alone.
    o = oracle.Oracle(local_cache=True)
    o.load_rules([(L, hiprl.HOUR)])
    state = {k: [0, False, False] for k in keys}
    alias = {k: (k, True) for k in keys}  # name in the oracle, in step with the model
    epoch = [0]

    def oracle_call(name, hits):
        st, _ = o.submit(hiprl.build_batch([("q", [[("k", name)]], [0], hits, T0)]))
        return int(st[0]["code_flags"]) & 0xFF, int(st[0]["limit_remaining"])

    checked = mid_adjusts = released = groups = 0
    i = 0
    while i < len(ev):
        seq, pos, kind = ev[i][:3]
        if kind == "call":
            _, _, _, key, hits, got = ev[i]
            s = state[key]
            if s[2]:  # a local-cache hit: no INCRBY
                want = (OVER_LIMIT, 0)
            else:
                s[0] += hits
                s[1] = True
                want = (OVER_LIMIT, 0) if s[0] > L else (OK, L - s[0])
                s[2] = s[0] > L
            assert got == want, (ev[i], s)
            name, in_step = alias[key]
            if in_step:
                assert oracle_call(name, hits) == got, (ev[i], s)
                checked += 1
            i += 1
            continue
        # one gathered group: the queued adjusts of this gather with this keep flag are one engine call
        grp = pos & (m.adj | m.adj_keep)
        j = i
        while j < len(ev) and ev[j][0] == seq and ev[j][2] == "adjust" and ev[j][1] & (m.adj | m.adj_keep) == grp:
            j += 1
        group = ev[i:j]
        assert [e[1] & 0x3FFFFFFF for e in group] == list(range(len(group))), "positions count the group's calls"
        groups += 1
        before = np.zeros(len(group), hiprl.PEEK_DTYPE)
        for r, e in enumerate(group):
            c, ex, fr = state[e[3]]
            before[r] = (c, 0, 0, (F if ex else 0) | (LC if fr else 0))
            got = e[5]
            assert (bool(got["Found"]), got["Count"], bool(got["LocalCached"])) == (ex, c, fr), (e, state[e[3]])
        after, rep = adjust_model([e[3] for e in group], before, [e[4] for e in group], [L] * len(group),
                                  local_cache=True, keep_cache=bool(grp & m.adj_keep))
        released += rep["unfrozen"]
        mid_adjusts += rep["applied"]
        for r, e in enumerate(group):
            s = state[e[3]]
            new = [int(after[r]["count"]), s[1], bool(int(after[r]["flags"]) & LC)]
            if new != s:
                state[e[3]] = new
                epoch[0] += 1
                name = f"{e[3]}#{epoch[0]}"
                if new[0]:
                    oracle_call(name, new[0])
                alias[e[3]] = (name, new[2] == (new[0] > L))
        i = j
    for k in keys:
        st, _ = m.by_key(PEEK, k, rule)
        assert (st["Count"], bool(st["Found"]), bool(st["LocalCached"])) == tuple(state[k]), (k, st, state[k])
    assert mid_adjusts > 100 and released > 0 and groups > 10, (mid_adjusts, released, groups)
    assert checked > TD * n // 2, f"guard: the oracle decided {checked} of {TD * n} calls"
    m.close()


def test_a_failing_adjust_batch_fails_exactly_its_calls():
    m = Cache(True, window_us=500, batch_limit=1 << 12)
    rule = m.lib.rlq_add_rule(m.h, 1000, hiprl.HOUR)
    m.lib.rlq_set_time(m.h, T0)
    for j in range(4):
        assert m.do_limit(f"f{j}", rule, 10)[0][0] == OK
    errors, fine = [], []

    def big():
        try:  # one descriptor more than the engine takes: the flight is refused
            m.by_key(QUEUED, "f0", rule, [-1] * ((1 << 12) + 4096 + 1))
        except hiprl.RedisError as e:
            errors.append(str(e))

    def small(t):
        for i in range(30):
            before, _ = m.by_key(QUEUED, f"f{t}", rule, -1 if t else 0)
            fine.append((t, before["Found"], before["Count"]))
            assert m.do_limit(f"d{t}", rule, 1)[0][0] == OK

    th = [threading.Thread(target=big)] + [threading.Thread(target=small, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert len(errors) == 1 and "capacity" in errors[0], errors
    assert len(fine) == 120 and all(found for _, found, _ in fine)
    # nothing of the refused call was applied, every other call was; the cache goes on serving
    assert m.by_key(PEEK, "f0", rule)[0]["Count"] == 10
    for t in range(1, 4):
        assert m.by_key(PEEK, f"f{t}", rule)[0]["Count"] == 0  # 10 - 30, floored
    assert m.do_limit("f0", rule, 1)[0][:2] == (OK, 1000 - 11)
    m.close()
