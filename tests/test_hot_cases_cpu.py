"""What the hot-set GPU tests assume, checked without a GPU: the key families' places in the tag
table (oracle.prefix_lanes), a Python restatement of build_hot_table (rl_internal.h) and
hot_lookup (rl_tile.h) on every family, and the oracle's own figures on the test streams."""
import numpy as np
import pytest

import hiprl
import hot_cases as hc
import oracle
import routing
from hot_cases import HOT_MAX, HOT_TAG_MASK, HOT_TAGS, SEED, T

SEEDS = [SEED, 7, 0x123456789ABCDEF]
MISS = 0xFFFFFFFF


# ---- 1. family properties ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_family_places(seed):
    for fam in (hc.clustered, hc.wrapping):
        assert len({hc.home_tag(p, seed) for p in fam(256)}) == 1, fam.__name__
    two = [hc.home_tag(p, seed) for p in hc.two_lane(256)]
    assert len({t for _, t in two}) == 1 and 1 < len({h for h, _ in two}) <= 16
    assert len({hc.home_tag(p, seed)[0] for p in hc.spread(256)}) >= 200
    # ... and 16 constant bytes in front change nothing, while a varying byte outside the last
    # word gives 256 places
    assert len({hc.home_tag(b"0123456789abcdef" + p, seed) for p in hc.clustered(256)}) == 1
    assert len({hc.home_tag(b"hs" + bytes([v]) + b"clu__", seed) for v in range(256)}) == 256
    for name, fam in hc.FAMILIES.items():
        assert len(set(fam(256))) == 256, name


@pytest.mark.parametrize("K", [1, 2, 255, 256])
def test_wrapping_home_interval(K):
    lo, hi = hc.wrap_interval(K)
    home = hc.home_tag(hc.wrapping(K)[0])[0]
    assert lo <= home <= hi and hi == HOT_TAGS - 1
    assert lo == HOT_TAGS - max(1, K // 2)
    if K >= 2:
        assert home + K > HOT_TAGS  # the chain's last word lies before its first


def test_wrap_stem_census():
    """The figures the family was chosen by."""
    homes = dict(hc._stem_homes()[:2000])
    assert sum(1850 <= h <= 2040 for h in homes.values()) == 185
    assert homes[b"h0010_"] == 2023


# ---- 2. build_hot_table / hot_lookup, line for line ------------------------------------------------
def build_hot_table(hot):
    """rl_internal.h build_hot_table: hot = [(a, b, rule)] in index order -> (tag words, entries)."""
    tags = [0] * HOT_TAGS
    ents = []
    for i, (a, b, rule) in enumerate(hot[:HOT_MAX]):
        s = hc.hot_home(a)
        while tags[s]:
            s = (s + 1) & (HOT_TAGS - 1)
        tags[s] = hc.hot_tag(a) | (i + 1)
        ents.append((a, b, rule, i))
    return tags, ents


def hot_lookup(tags, ents, a, b, confirm=True):
    """rl_tile.h hot_lookup -> (hot index or MISS, rule, probes)."""
    t = hc.hot_tag(a)
    s = hc.hot_home(a)
    for probe in range(HOT_TAGS):
        w = tags[s]
        if w == 0:
            return MISS, None, probe + 1
        if (w & HOT_TAG_MASK) == t:
            ea, eb, rule, idx = ents[(w & ~HOT_TAG_MASK & 0xFFFFFFFF) - 1]
            if not confirm or (ea == a and eb == b):
                return idx, rule, probe + 1
        s = (s + 1) & (HOT_TAGS - 1)
    return MISS, None, HOT_TAGS


def non_members(keys, seed):
    """2000 prefixes outside `keys`: same home / other tag, the chain's own non-members (for a
    clustered family its unused byte values among them), and plain cold keys."""
    home, tag = hc.home_tag(keys[0], seed)
    out = list(hc.same_home_other_tag(home, tag, 8, seed))
    if keys[0][:6] in (hc.CLU_STEM, hc.wrap_stem(len(keys))):
        out += hc.unused_values(keys)
    out += hc.chain_mates(keys, 400, seed)
    have = set(keys)
    out = [p for p in out if p not in have]
    out += hc.cold(2000 - len(out))
    assert len(out) == 2000 and not have & set(out)
    return out


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K", [1, 255, 256])
@pytest.mark.parametrize("family", list(hc.FAMILIES))
def test_lookup_restatement(family, K, seed):
    keys = hc.FAMILIES[family](K)
    hot = [hc.lanes(p, seed) + (hc.rule_of(i),) for i, p in enumerate(keys)]
    tags, ents = build_hot_table(hot)
    assert sum(1 for w in tags if w) == K
    probes = []
    for i, (a, b, rule) in enumerate(hot):
        idx, r, n = hot_lookup(tags, ents, a, b)
        assert (idx, r) == (i, rule), (family, K, i)
        probes.append(n)
    misses = non_members(keys, seed)
    walked = []
    for p in misses:
        a, b = hc.lanes(p, seed)
        idx, _, n = hot_lookup(tags, ents, a, b)
        assert idx == MISS, (family, K, p)
        walked.append(n)
    assert max(walked) <= K + 1 <= HOT_TAGS
    if family in ("clustered", "wrapping"):
        # where the chain lies: K equal tag words from the family's home on (over the table's end
        # for `wrapping`), member i at its i-th word, a chain-mate's miss walks all of it
        home, tag = hc.home_tag(keys[0], seed)
        assert [tags[(home + i) & (HOT_TAGS - 1)] for i in range(K)] == [tag | (i + 1) for i in range(K)]
        assert probes == list(range(1, K + 1)) and max(walked) == K + 1
        if family == "wrapping" and K >= 2 and seed == SEED:
            assert home + K > HOT_TAGS and tags[0] != 0
        # without the (a, b) confirmation every member but the first is taken for index 0
        if K > 1:
            a, b = hc.lanes(keys[K - 1], seed)
            assert hot_lookup(tags, ents, a, b, confirm=False)[0] == 0
    if family == "spread" and K == 256:
        assert np.mean(probes) < 1.2  # rl_tile.h's "~1.1 probes" holds for such a set


# ---- 3. the oracle on the test streams --------------------------------------------------------------
def _stream(family, K, local_cache, jitter=False):
    hot = hc.FAMILIES[family](K)
    keys = hc.keys_of(hot + hc.cold(300))
    bs = [hc.teaching_batch(keys, K, T - 4 + j, j) for j in range(3)]
    bs.append(hc.checked_batch(keys, K, jitter=jitter))
    return keys, bs


def _oracle(local_cache):
    o = oracle.Oracle(local_cache=local_cache)
    o.load_rules(hc.RULES)
    return o


@pytest.mark.parametrize("local_cache", [False, True])
@pytest.mark.parametrize("family,K", [("spread", 17), ("spread", 256), ("clustered", 256), ("two_lane", 256)])
def test_oracle_invariant_under_recutting(family, K, local_cache):
    keys, bs = _stream(family, K, local_cache, jitter=True)
    o = _oracle(local_cache)
    outs = [o.submit(b) for b in bs[:3]]
    frozen = hc.frozen_before(o, keys, K, T - 1)
    outs.append(o.submit(bs[3]))
    st = np.concatenate([s for s, _ in outs])
    thr = np.concatenate([t for _, t in outs])
    # the same requests in other cuts: one batch, and cuts at request indices that are no
    # multiple of anything the builders use
    whole = routing.concat_batches(bs)
    o1 = _oracle(local_cache)
    st1, thr1 = o1.submit(whole)
    assert np.array_equal(st, st1) and np.array_equal(thr, thr1)
    o2 = _oracle(local_cache)
    cuts = [0, 1, 777, whole.n_req // 3 + 1, whole.n_req - 5, whole.n_req]
    parts = [o2.submit(whole.slice_requests(a, b)) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(st, np.concatenate([s for s, _ in parts]))
    assert np.array_equal(thr, np.concatenate([t for _, t in parts]))
    assert o.num_strings() == o1.num_strings() == o2.num_strings()
    # the guards the GPU tests rely on, on the oracle alone
    f = hc.figures(outs[3][0])
    assert f["over"] >= K and f["ok"] >= K, f
    if local_cache:
        assert f["local_hits"] >= K // 4, f
        # tiny-limit MINUTE / HOUR / DAY keys froze while teaching
        want = sum(1 for i in range(K) if hc.is_tiny(i) and i % 4 != 0)
        assert frozen >= want and (K < 8 or want > 0), (frozen, want)
    else:
        assert f["local_hits"] == 0 and frozen == 0


def test_rules_cover_every_unit_and_limit():
    seen = {hc.rule_of(i) for i in range(12)}
    assert seen == set(range(len(hc.RULES)))
    assert {hc.RULES[hc.rule_of(i)] for i in range(256) if hc.is_tiny(i)} == {(hc.TINY, u) for u in hc.UNITS}


def test_batch_builder_layout():
    keys = hc.keys_of(hc.spread(5) + hc.cold(2))
    ids = [0, 1, 2, 3, 4, 5, 6, 0]
    b = hc.make_batch(keys, ids, hc.straddle(3, T, 0.34), 3, jitter=np.arange(8))
    assert b.n_desc == 8 and b.n_req == 3
    assert [b.prefix(i) for i in range(8)] == [keys.prefixes[i] for i in ids]
    assert list(b.req_of) == [0, 0, 0, 1, 1, 1, 2, 2] and list(b.hits) == [1, 2, 3]
    assert list(b.now) == [T - 1, T, T] and list(b.rule) == [hc.rule_of(i) for i in ids]
    assert b.blob.shape[0] == int(b.off[-1]) + hiprl.BLOB_SLACK
    lt = hc.last_touch(b)
    assert lt[(keys.prefixes[0], T)] == (T, 7, hc.rule_of(0))  # SECOND key: one string per second
    assert lt[(keys.prefixes[0], T - 1)] == (T - 1, 0, hc.rule_of(0))
    assert lt[(keys.prefixes[1], T - 60)] == (T - 1, 1, hc.rule_of(1))
