"""Key families and batch builders of the hot-set tests (test_hot_cases_cpu.py,
test_gpu_hot_set.py, test_gpu_hot_set_routed.py).

A hot prefix is found through the LDS tag table of rl_common.h: home = hot_home(a), the low 11
bits of the prefix lane a; tag = hot_tag(a), its bits 41..63. The lane is rotl((a ^ w) * M, 31)
per 8-byte word with no final mix, so a difference confined to bytes 5..7 of a prefix's last
8-byte word never reaches the tag and reaches at most four bits of the home:

  spread(K)     the varying id lies in the first word: homes and tags all over the table
  clustered(K)  stem6 + bytes([v]) + b"_": ONE (home, tag), so the set is one probe chain of K
                equal tag words, each confirmed on the full (a, b)
  wrapping(K)   clustered, with a stem whose home lies in [2048 - K/2, 2047]: the chain runs
                over the end of the tag table
  two_lane(K)   bytes 5 and 6 vary: 16 homes, one tag

Prefixes are raw bytes put into hiprl.Batch directly; the engine does not parse them. The rule
of a key is a function of its id: every unit, with a tiny limit (the key freezes in the first
teaching batch, so a MINUTE / HOUR / DAY key is frozen before the checked batch: HB_FROZEN_PRE),
a small one (the key freezes inside the checked batch) and a large one (never over).
"""
from __future__ import annotations

import functools

import numpy as np

import hiprl
import oracle
import streams

SEED = 0x5EE7AB1E5EED          # hiprl.Engine's default hash_seed
HOT_MAX = 256                  # rl_common.h
HOT_TAGS = 2048
HOT_TAG_MASK = 0xFFFFFE00
HOT_MIN_SEG = 128
HOT_CAND_MIN = 64
CAND_MAX = 1024
T = 1_700_006_400              # the first second of a day, an hour and a minute
assert T % 86400 == 0

UNITS = [hiprl.SECOND, hiprl.MINUTE, hiprl.HOUR, hiprl.DAY]
TINY, SMALL, LARGE = 5, 30, 1 << 20
LIMITS = [TINY, SMALL, LARGE]
RULES = [(L, u) for u in UNITS for L in LIMITS]  # rule id = unit index * 3 + limit class


def rule_of(i: int) -> int:
    """Rule of key id i: the unit cycles fastest, then the limit class."""
    return (i % 4) * 3 + (i // 4) % 3


def is_tiny(i: int) -> bool:
    return (i // 4) % 3 == 0


# ---- the tag table's view of a prefix ------------------------------------------------------------
def lanes(p: bytes, seed: int = SEED):
    return oracle.prefix_lanes(p, seed)


def hot_home(a: int) -> int:
    return a & (HOT_TAGS - 1)


def hot_tag(a: int) -> int:
    return (a >> 32) & HOT_TAG_MASK


def home_tag(p: bytes, seed: int = SEED):
    a, _ = lanes(p, seed)
    return hot_home(a), hot_tag(a)


# ---- families ------------------------------------------------------------------------------------
CLU_STEM = b"hsclu_"
TWO_STEM = b"hstwo"


def spread(K: int):
    return [b"hs_k_%d_tail_" % i for i in range(K)]


def clustered(K: int, stem: bytes = CLU_STEM):
    assert K <= 256 and len(stem) == 6
    return [stem + bytes([v]) + b"_" for v in range(K)]


@functools.lru_cache(maxsize=None)
def _stem_homes():
    return [(b"h%04d_" % i, home_tag(b"h%04d_" % i + b"\0_")[0]) for i in range(10000)]


def wrap_interval(K: int):
    return HOT_TAGS - max(1, K // 2), HOT_TAGS - 1


@functools.lru_cache(maxsize=None)
def wrap_stem(K: int) -> bytes:
    """The first stem b"hNNNN_" whose chain of K tag words runs over the table's end (engine's
    default seed)."""
    lo, hi = wrap_interval(K)
    return next(s for s, h in _stem_homes() if lo <= h <= hi)


def wrapping(K: int):
    return clustered(K, wrap_stem(K))


def two_lane(K: int):
    assert K <= 256
    return [TWO_STEM + bytes([48 + i % 16, 64 + i // 16]) + b"_" for i in range(K)]


FAMILIES = {"spread": spread, "clustered": clustered, "wrapping": wrapping, "two_lane": two_lane}


def unused_values(keys):
    """A clustered family's byte values that are not in `keys` (same home, same tag)."""
    stem = keys[0][:6]
    have = set(keys)
    return [p for p in (stem + bytes([v]) + b"_" for v in range(256)) if p not in have]


def chain_mates(keys, n: int, seed: int = SEED):
    """Up to n non-members that land in the family's chain: keys[0] with bytes 5 and 6 varied,
    kept where (home, tag) is one of the family's."""
    have = set(keys)
    want = {home_tag(p, seed) for p in keys}
    base = keys[0]
    out = []
    for u in range(256):
        for v in range(0, 256, 5):
            p = base[:5] + bytes([u, v]) + base[7:]
            if p not in have and home_tag(p, seed) in want:
                out.append(p)
                if len(out) == n:
                    return out
    return out


@functools.lru_cache(maxsize=None)
def same_home_other_tag(home: int, tag: int, n: int, seed: int = SEED):
    """n prefixes whose home is `home` and whose tag is not `tag`."""
    out = []
    i = 0
    while len(out) < n:
        p = b"hs_sh_%d_" % i
        h, t = home_tag(p, seed)
        if h == home and t != tag:
            out.append(p)
        i += 1
        assert i < 2_000_000
    return tuple(out)


def cold(n: int, stem: bytes = b"hs_cold_"):
    return [stem + b"%d_x_" % i for i in range(n)]


# ---- batches -------------------------------------------------------------------------------------
class Keys:
    """Prefixes with their rule ids."""

    def __init__(self, prefixes, rules):
        self.prefixes = list(prefixes)
        self.rules = np.asarray(rules, np.uint32)
        assert len(self.prefixes) == len(self.rules)

    def __len__(self):
        return len(self.prefixes)

    def __add__(self, other):
        return Keys(self.prefixes + other.prefixes, np.concatenate([self.rules, other.rules]))


def keys_of(prefixes, id0: int = 0) -> Keys:
    return Keys(prefixes, [rule_of(id0 + i) for i in range(len(prefixes))])


def mix(counts, rng) -> np.ndarray:
    """Key ids, counts[i] of id i, in a seeded random order."""
    ids = np.repeat(np.arange(len(counts), dtype=np.int64), np.asarray(counts, np.int64))
    rng.shuffle(ids)
    return ids


def straddle(n_req: int, t: int, frac: float = 0.5) -> np.ndarray:
    """Request times t - 1 for the first `frac` of the requests, t for the rest."""
    now = np.full(n_req, t, np.int64)
    now[:int(n_req * frac)] = t - 1
    return now


def n_requests(n_desc: int, per_req: int) -> int:
    return (n_desc + per_req - 1) // per_req


def make_batch(keys: Keys, ids, times, per_req: int = 3, jitter=None) -> hiprl.Batch:
    """One batch: descriptor d carries key ids[d] and belongs to request d // per_req (so requests
    straddle tiles); `times` is one time or the non-decreasing per-request times (at most two
    adjacent seconds); hits_addend cycles 1..3 over the requests; jitter: None or the EXPIRE
    jitter per descriptor."""
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    nr = n_requests(n, per_req)
    now = np.full(nr, times, np.int64) if np.ndim(times) == 0 else np.asarray(times, np.int64)
    assert now.shape == (nr,) and (nr == 0 or (np.all(np.diff(now) >= 0) and now[-1] - now[0] <= 1))
    lens = np.array([len(p) for p in keys.prefixes], np.int64)[ids]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    raw = b"".join([keys.prefixes[i] for i in ids.tolist()])
    blob = np.zeros(len(raw) + hiprl.BLOB_SLACK, np.uint8)
    blob[:len(raw)] = np.frombuffer(raw, np.uint8)
    return hiprl.Batch(blob, off.astype(np.uint32), keys.rules[ids].astype(np.uint32),
                       (np.arange(n) // per_req).astype(np.uint32), now, (1 + np.arange(nr) % 3).astype(np.uint32),
                       None if jitter is None else np.asarray(jitter, np.uint16))


def checked_batch(keys: Keys, n_hot: int, t: int = T, per_key: int = 40, seed: int = 0, jitter: bool = False,
                  extra=None) -> hiprl.Batch:
    """The batch a test checks: per_key descriptors of each of the first n_hot keys and a quarter
    as many of the other keys of `keys` (the cold tail), times t - 1 -> t. extra: ids appended to
    the mix (each once)."""
    rng = np.random.default_rng(1000 + seed)
    counts = np.zeros(len(keys), np.int64)
    counts[:n_hot] = per_key
    n_cold = len(keys) - n_hot
    if n_cold:
        counts[n_hot:] = np.bincount(rng.integers(0, n_cold, n_hot * per_key // 4), minlength=n_cold)
    if extra is not None:
        counts[np.asarray(extra, np.int64)] += 1
    ids = mix(counts, rng)
    jit = rng.integers(0, 300, len(ids)).astype(np.uint16) if jitter else None
    return make_batch(keys, ids, straddle(n_requests(len(ids), 3), t), 3, jit)


def teaching_batch(keys: Keys, n_hot: int, t: int, j: int, per_key: int = HOT_MIN_SEG + 2) -> hiprl.Batch:
    """per_key descriptors of each of the first n_hot keys, all at one time (so each key is one
    segment of >= HOT_MIN_SEG), and three of every other key."""
    counts = np.full(len(keys), 3, np.int64)
    counts[:n_hot] = per_key
    return make_batch(keys, mix(counts, np.random.default_rng(2000 + j)), t)


def submit_checked(o, e, b, ctx):
    ref = o.submit(b)
    streams.assert_same(*ref, *e.submit(b), ctx)
    return ref


def teach(o, e, keys: Keys, t: int, n_hot=None, n_batches: int = 3):
    """The batches that make the first n_hot keys (default: all) the hot set: batches at t, t + 1,
    ..., each key with >= HOT_MIN_SEG descriptors, every batch checked against the oracle. A set
    sampled on one batch is applied behind the next submit and uploaded by the one after, so the
    third batch is the first to run on it. Returns the fallbacks since the engine's first batch
    began (the guard of every later assertion)."""
    n_hot = len(keys) if n_hot is None else n_hot
    fb0 = None
    for j in range(n_batches):
        submit_checked(o, e, teaching_batch(keys, n_hot, t + j, j), f"teach {j}")
        if j == 0:
            fb0 = e.stats()["lsd_fallbacks"]
    s = e.stats()
    assert s["hot_keys"] == min(n_hot, HOT_MAX), s
    assert s["lsd_fallbacks"] == fb0, s
    return fb0


# ---- oracle-side figures of a checked batch ----------------------------------------------------------
def figures(st) -> dict:
    cf = st["code_flags"]
    return dict(over=int(((cf & 0xFF) == hiprl.CODE_OVER_LIMIT).sum()),
                local_hits=int((((cf >> 8) & hiprl.FLAG_LOCAL_CACHE_HIT) != 0).sum()),
                ok=int(((cf & 0xFF) == hiprl.CODE_OK).sum()))


def frozen_before(o, keys: Keys, n_hot: int, now: int) -> int:
    """How many of the first n_hot keys' strings of `now` the oracle's local cache holds."""
    n = 0
    for i in range(n_hot):
        unit = RULES[int(keys.rules[i])][1]
        n += o.local_cached(oracle.cache_key(keys.prefixes[i], unit, now), now)
    return n


def last_touch(b: hiprl.Batch, rules=RULES) -> dict:
    """(prefix, window start) -> (time, jitter, rule id) of the string's last descriptor in b."""
    out = {}
    blob = b.blob.tobytes()
    for i in range(b.n_desc):
        r = int(b.rule[i])
        now = int(b.now[b.req_of[i]])
        div = hiprl.UNIT_DIVIDER[rules[r][1]]
        out[(blob[int(b.off[i]):int(b.off[i + 1])], now // div * div)] = (now, 0 if b.jit is None else int(b.jit[i]), r)
    return out
