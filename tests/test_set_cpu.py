"""Set (rl_hip.h "Set"), CPU only: the flag values and the unchanged reply layout against the
header, the library's entry point, the Redis import (resp.import_batch) and the clocked RespStore
against the oracle."""
import subprocess
from pathlib import Path

import numpy as np

import hiprl
import oracle
import resp
from streams import RULES, UNITS, make_stream

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ["count", "ttl_s", "cached_s", "flags"]
S, M, H, D = hiprl.SECOND, hiprl.MINUTE, hiprl.HOUR, hiprl.DAY
UNIT_RULE = {S: 10, M: 11, H: 12, D: 13}


def test_flags_match_header_and_layout_is_unchanged(tmp_path):
    offs = ",".join(f"offsetof(rl_peek_reply,{f})" for f in FIELDS)
    src = tmp_path / "set.c"
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int (*fn)(rl_engine*, const rl_batch*, const rl_peek_reply*, rl_peek_reply*) = rl_set;\n'
                   'int main(){size_t v[]={'
                   f'sizeof(rl_peek_reply),RL_SET_KEEP_COUNTER,RL_SET_KEEP_CACHE,RL_ABI_VERSION,{offs}}};'
                   'for(unsigned i=0;i<sizeof v/sizeof v[0];++i)printf("%zu ",v[i]);return 0;}\n')
    obj = tmp_path / "set.o"
    subprocess.run(["gcc", "-c", "-I", str(ROOT / "include"), str(src), "-o", str(obj)], check=True)
    exe = tmp_path / "set"
    subprocess.run(["gcc", str(obj), "-o", str(exe), "-Wl,--unresolved-symbols=ignore-all"], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = hiprl.PEEK_DTYPE
    assert got == [16, hiprl.SET_KEEP_COUNTER, hiprl.SET_KEEP_CACHE, 7] + [P.fields[f][1] for f in FIELDS]
    assert (hiprl.SET_KEEP_COUNTER, hiprl.SET_KEEP_CACHE) == (32, 64) and hiprl.ABI_VERSION == 7
    peek_bits = hiprl.PEEK_FOUND | hiprl.PEEK_LOCAL_CACHED | hiprl.PEEK_NIL | hiprl.PEEK_PER_SECOND | hiprl.PEEK_BAD
    assert not peek_bits & (hiprl.SET_KEEP_COUNTER | hiprl.SET_KEEP_CACHE)


def test_library_exports_set():
    lib = hiprl.load_library()
    assert hasattr(lib, "rl_set") and "rl_set" in {n for n, _, _ in hiprl.ABI}
    assert lib.rl_abi_version() == 7
    # null arguments are refused before anything touches the GPU
    assert lib.rl_set(None, None, None, None) == -1
    assert hasattr(hiprl.Engine, "set") and hasattr(hiprl.HipRateLimitCache, "set")


# ---- resp.import_batch ---------------------------------------------------------------------------
def one(b, v, i=0):
    return b.prefix(i), int(b.rule[i]), tuple(int(x) for x in v[i])


def test_import_splits_prefix_and_window():
    now = 1_700_000_007
    m = now // 60 * 60
    # a value that contains '_' and digits: the window start is what follows the last '_'
    ents = [(f"dom_k_v_12_34_{m}", 5, 40), (f"dom_k__{now}".encode(), 2, 1), (f"a_b_c_{now // 3600 * 3600}", 9, 1000)]
    b, v, skipped = resp.import_batch(ents, now, UNIT_RULE)
    assert not skipped and b.n_desc == 3 and b.n_req == 1 and int(b.now[0]) == now
    assert one(b, v, 0) == (b"dom_k_v_12_34_", UNIT_RULE[M], (5, 40, 0, hiprl.PEEK_FOUND))
    assert one(b, v, 1) == (b"dom_k__", UNIT_RULE[S], (2, 1, 0, hiprl.PEEK_FOUND))
    assert one(b, v, 2) == (b"a_b_c_", UNIT_RULE[H], (9, 1000, 0, hiprl.PEEK_FOUND))
    assert v.dtype == hiprl.PEEK_DTYPE and list(b.req_of) == [0, 0, 0] and int(b.off[-1]) == b.blob.shape[0]
    # the key string is rebuilt exactly: prefix || decimal(window start)
    for i, (k, _, _) in enumerate(ents):
        k = k.encode() if isinstance(k, str) else k
        assert resp.cache_key(b.prefix(i), {10: S, 11: M, 12: H, 13: D}[int(b.rule[i])], now) == k
    # strings that are no cache keys
    _, _, skipped = resp.import_batch([("nounderscore", 1, 5), ("p_", 1, 5), ("p_12x", 1, 5), (f"p_0{m}", 1, 5)], now,
                                      UNIT_RULE)
    assert [k for k, _ in skipped] == [b"nounderscore", b"p_", b"p_12x", f"p_0{m}".encode()]


def test_import_chooses_the_smallest_unit_whose_window_is_current():
    day = 1_700_000_000 // 86400 * 86400 + 86400
    for now, ws, want in [
        (day, day, S),                # a day's first second: SECOND, MINUTE, HOUR and DAY keys are one string
        (day + 59, day, M),           # the minute's window, still also the hour's and the day's
        (day + 60, day, H),
        (day + 3600, day, D),
        (day + 3600, day + 3600, S),  # an hour's first second
        (day + 3661, day + 3660, M),
        (day + 3661, day + 3600, H),
        (day + 7, day + 7, S),
    ]:
        b, v, skipped = resp.import_batch([(f"p_{ws}", 1, 10)], now, UNIT_RULE)
        assert not skipped and int(b.rule[0]) == UNIT_RULE[want], (now - day, ws - day)
    # only the loaded units are candidates
    b, _, skipped = resp.import_batch([(f"p_{day}", 1, 10)], day, {H: 2, D: 3})
    assert int(b.rule[0]) == 2 and not skipped
    b, _, skipped = resp.import_batch([(f"p_{day + 7}", 1, 10)], day + 7, {H: 2, D: 3})
    assert b.n_desc == 0 and skipped == [(f"p_{day + 7}".encode(), "window is not current")]


def test_import_skips_dead_keys_and_wraps_values():
    now = 1_700_000_007
    m = now // 60 * 60
    ents = [(f"p_{m - 60}", 3, 5),    # the minute before: no current window
            (f"p_{m}", 3, 0),         # TTL 0
            (f"q_{m}", 3, -1),        # no expiry
            (f"r_{m}", 3, -2),        # gone
            (f"s_{now + 1}", 3, 5),   # a second ahead
            (f"t_{m}", 2**32 + 5, 5), (f"u_{m}", 2**32 - 1, 5), (f"w_{m}", 2**40 + 2**32 - 2, 5)]
    b, v, skipped = resp.import_batch(ents, now, UNIT_RULE)
    assert [k for k, _ in skipped] == [f"p_{m - 60}".encode(), f"p_{m}".encode(), f"q_{m}".encode(),
                                       f"r_{m}".encode(), f"s_{now + 1}".encode()]
    assert [b.prefix(i) for i in range(b.n_desc)] == [b"t_", b"u_", b"w_"]
    assert [int(x) for x in v["count"]] == [5, 2**32 - 1, 2**32 - 2]
    assert b.blob.dtype == np.uint8 and b.off.dtype == np.uint32 and b.rule.dtype == np.uint32
    # nothing to import: an empty batch, which rl_set accepts
    b, v, _ = resp.import_batch([], now, UNIT_RULE)
    assert b.n_desc == 0 and v.shape == (0,) and b.n_req == 1


def test_import_per_second_list_takes_second_keys_only():
    now = 1_700_000_040 // 60 * 60 + 60  # a minute's first second: the SECOND and the MINUTE key are one string
    b, v, skipped = resp.import_batch([(f"p_{now}", 4, 1), (f"p_{now - 1}", 4, 1)], now, UNIT_RULE, per_second=True)
    assert b.n_desc == 1 and int(b.rule[0]) == UNIT_RULE[S] and [k for k, _ in skipped] == [f"p_{now - 1}".encode()]
    b, _, _ = resp.import_batch([(f"p_{now}", 4, 1)], now + 1, UNIT_RULE, per_second=True)
    assert b.n_desc == 0  # the main list would read it as the MINUTE key
    b, _, _ = resp.import_batch([(f"p_{now}", 4, 1)], now + 1, UNIT_RULE)
    assert int(b.rule[0]) == UNIT_RULE[M]
    b, _, skipped = resp.import_batch([(f"p_{now}", 4, 1)], now, {M: 1}, per_second=True)
    assert b.n_desc == 0 and len(skipped) == 1


# ---- the clocked RespStore against the oracle ----------------------------------------------------
def test_clocked_store_dump_equals_the_oracle():
    for split in (False, True):
        reqs = make_stream(5, 1500, t0=(1_700_000_000 // 3600 + 1) * 3600 - 25, dt_max=2)
        times = sorted({r[4] for r in reqs})
        o = oracle.Oracle(per_second_split=split)
        o.load_rules(RULES)
        clock = {"t": 0}
        main, ps = resp.RespStore(lambda: clock["t"]), resp.RespStore()
        keys = set()
        for t in times:
            b = hiprl.build_batch([r for r in reqs if r[4] == t])
            st, _ = o.submit(b)
            clock["t"] = t
            cmds = resp.commands(b, RULES, st, split)
            m_bytes, p_bytes = resp.encode(cmds)
            main.execute(m_bytes)
            ps.execute(p_bytes, now=t)  # the per-call clock
            keys |= {(c.key, c.per_second) for c in cmds}
        assert len(keys) > 300 and any(p for _, p in keys) == split
        for now in (times[-1], times[-1] + 1, times[-1] + 45, times[-1] + 4000):
            for store, is_ps in ((main, False), (ps, True)):
                dump = store.dump(now)
                seen = {k for k, _, _ in dump}
                assert len(seen) == len(dump)
                for k, v, ttl in dump:
                    assert ttl > 0 and o.counter(k, now, per_second=is_ps) == v, (k, v, ttl)
                    assert o.counter(k, now + ttl - 1, per_second=is_ps) == v  # the oracle's expiry is now + ttl
                    assert o.counter(k, now + ttl, per_second=is_ps) == -1
                for k, p in keys:
                    if p == is_ps and k not in seen:
                        assert o.counter(k, now, per_second=is_ps) == -1, k
        assert len(main.dump(times[-1])) > 50 and (not split or ps.dump(times[-1]))
    # the default store keeps its old behaviour: no clock, no deadlines, EXPIRE's argument in ttl
    s = resp.RespStore()
    s.execute(resp.flat_cmd("INCRBY", b"k_1", 3) + resp.flat_cmd("EXPIRE", b"k_1", 60))
    assert s.counters == {b"k_1": 3} and s.ttl == {b"k_1": 60} and s.dump(10**9) == [(b"k_1", 3, -1)]
    # a clocked one forgets a key at its deadline, as Redis does
    s = resp.RespStore()
    s.execute(resp.flat_cmd("INCRBY", b"k_1", 3) + resp.flat_cmd("EXPIRE", b"k_1", 60), now=100)
    assert s.dump(159) == [(b"k_1", 3, 1)] and s.dump(160) == []
    assert resp.parse_replies(s.execute(resp.flat_cmd("INCRBY", b"k_1", 2), now=160)) == [2]
    assert UNITS == [S, M, H, D]
