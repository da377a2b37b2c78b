"""The case sets of tests/resolve_cases.py through the host build of the device GetLimit walk
(tests/cshim/librl_resolve_shim.so: rl_resolve.hip's resolve_fast, then resolve_one for what it
leaves) against the config oracle (oracle/config_oracle.py, GetLimit config_impl.go:274-323).
CPU only. It validates the generator, keeps the host walk pinned at the same edges as
tests/test_gpu_resolve_edges.py pins the device, and asserts the guards: which pass decides
what (the shim's classification) and how varied the expected answers are (the oracle's), so the
sets keep reaching the boundaries they were built for."""
import numpy as np
import pytest

import resolve_cases as rc


def _check(cs, shift=0):
    got, ex = rc.shim_resolve(cs.cfg, cs.batch, shift)
    bad = rc.mismatches(cs, got)
    assert not bad, bad
    return ex


def test_generator_layout():
    """What the sets promise about their own blobs: every offset residue in both layouts, joined
    values right behind their key's separator, a pad byte after every separate string."""
    a = rc.set_a()
    b, raw = a.batch, a.batch.bytes
    e = b.entry.reshape(-1, 4).astype(np.int64)
    joined = e[:, 2] == e[:, 0] + e[:, 1] + 1
    assert 0.4 < joined.mean() < 0.6
    for sel in (joined, ~joined):
        assert set((e[sel, 0] % 4).tolist()) == {0, 1, 2, 3} and set((e[sel, 2] % 4).tolist()) == {0, 1, 2, 3}
    assert (raw[e[~joined, 0] + e[~joined, 1]] == ord("P")).all() and (raw[e[~joined, 2] + e[~joined, 3]] == ord("P")).all()
    assert (raw[e[joined, 0] + e[joined, 1]] == ord("_")).all() and (raw[e[joined, 2] + e[joined, 3]] == ord("_")).all()
    assert set((b.domain.reshape(-1, 2)[:, 0] % 4).tolist()) == {0, 1, 2, 3}
    assert b.bytes_len == b.last_string_end(b.n_desc) + 2 + rc.PAD_TAIL and (raw[-rc.PAD_TAIL:] == ord("P")).all()
    lens = set((e[:, 1] + 1 + e[:, 3]).tolist())
    assert {15, 16, 17, 31, 32, 33, 34, 41} <= lens and {15, 16, 17, 31, 32, 33, 40} <= set(e[:, 1].tolist())


def test_set_a_as_built():
    a = rc.set_a()
    ex = _check(a)
    want = a.want
    print(f"set A: {len(want)} descriptors, first pass {1 - ex.mean():.2f}, exact {ex.mean():.2f}, "
          f"non-nil {np.mean([w is not None for w in want]):.2f}, distinct {len(set(want))}")
    assert 1 - ex.mean() >= 0.25
    assert ex.mean() >= 0.25
    assert np.mean([w is not None for w in want]) >= 0.50
    assert len(set(want)) >= 100


def test_set_a_reads_no_byte_too_many():
    """The planted extensions are live: the value of a TRAPS cell followed by "P" or "_" as part of
    the value resolves to another node than the value alone, in every length class."""
    a = rc.set_a()
    for kl, vl in rc.TRAPS:
        k, v = rc.name("k", kl), rc.name("v", vl)
        got = {s: a.orc.get_limit(rc.GRID, [(k, v + s)]).requests_per_unit for s in ("", "P", "_")}
        assert len(set(got.values())) == 3, (kl, vl, got)
    assert {kl + 1 + vl <= 16 for kl, vl in rc.TRAPS} == {True, False}
    assert any(16 < kl + 1 + vl <= 32 for kl, vl in rc.TRAPS) and any(kl + 1 + vl > 32 for kl, vl in rc.TRAPS)


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_set_a_bytes_len_at_the_last_byte(residue):
    a, cut = rc.set_a(), rc.set_a_cut(residue)
    assert cut.batch.bytes_len % 4 == residue and a.batch.n_desc - cut.batch.n_desc <= 3
    assert cut.batch.bytes_len == cut.batch.last_string_end(cut.batch.n_desc)
    _, ex_a = rc.shim_resolve(a.cfg, a.batch)
    # past bytes_len: "P", then bytes that go on as a longer name (the tail value + "P" is a node)
    assert bytes(cut.batch.bytes[cut.batch.bytes_len:cut.batch.bytes_len + 4]) == rc.beyond_the_end(4) == b"Phij"
    ex = _check(cut)
    moved = ex & ~ex_a[:cut.batch.n_desc]
    assert moved.any()  # a 20-byte window past the blob's end sends a first-pass descriptor to the exact walk
    assert moved[-1]


@pytest.mark.parametrize("shift", [1, 3])
def test_set_a_unaligned_blob(shift):
    ex = _check(rc.set_a(), shift)
    assert ex.all()  # everything goes down the byte path


def test_set_b_overrides():
    b = rc.set_b()
    ex = _check(b)
    want, ov = b.want, b.batch.override
    assert any(w is not None and o != rc.hiprl.NIL_RULE for w, o in zip(want, ov))       # an override applied
    assert any(w is None and o != rc.hiprl.NIL_RULE for w, o in zip(want, ov))           # an unknown domain's ignored
    long_ov = [j for j, d in enumerate(b.descs) if d[2] is not None and len(d[0]) in (17, 32, 33, 40) and want[j]]
    assert long_ov and ex[long_ov].all()  # overridden descriptors of long domains take the exact walk
    assert {len(d[1]) for d in b.descs if d[2] is not None} == {0, 1, 3}


def test_set_c_fanout():
    c = rc.set_c_fanout()
    ex = _check(c)
    assert not ex.any()  # short names: the first pass walks inline children and the edge table itself
    assert np.mean([w is not None for w in c.want]) > 0.5 and None in c.want


@pytest.mark.parametrize("walk", ["fast", "exact"])
def test_set_c_collisions(walk):
    c = rc.set_c_collide(walk)
    ex = _check(c)
    if walk == "fast":
        assert ex.any()


def test_set_c_many_domains():
    c = rc.set_c_domains()
    _check(c)
    assert sum(w is not None for w in c.want) == 40 and sum(w is None for w in c.want) == 40


@pytest.mark.parametrize("long_at", [1, 5, 9])
def test_set_d_depth(long_at):
    d = rc.set_d(long_at)
    ex = _check(d)
    n_ent = np.diff(d.batch.entry_first.astype(np.int64))
    assert {0, 1, 2, 3, 5, 8, 9, 10} <= set(n_ent.tolist())
    # the hand-off happens exactly where a walk reaches the 20-byte key
    reach = np.array([len(q[1]) >= long_at and all(e[0] != "zz" for e in q[1][:long_at - 1]) for q in d.descs])
    assert ex[reach].any() and not ex[n_ent < long_at].any()
    assert len({w for w in d.want if w}) >= 5 and None in d.want


def _e_cases():
    return [(n, v) for n in rc.E_SIZES for v in rc.E_VARIANTS] + [(rc.E_BIG, "big")]


@pytest.mark.parametrize("n,variant", _e_cases())
def test_set_e_blocks(n, variant):
    e = rc.set_e(n, variant)
    assert e.batch.n_desc == n
    ex = _check(e)
    assert np.flatnonzero(ex).tolist() == rc.e_positions(n, variant)  # exactly the planted descriptors
    assert all(e.want[p] is not None for p in rc.e_positions(n, variant))
    if variant == "big":
        assert sorted({p // 256 for p in rc.e_positions(n, variant)}) == [0, 2047, 2048, 2049] == sorted(
            {0, 2047, 2048, (n - 1) // 256})


def test_set_f_sequence():
    assert len(rc.F_SIZES) >= 9 and max(rc.F_SIZES) > rc.F_MAX_BATCH_DESC
    for call, n in enumerate(rc.F_SIZES):
        f = rc.set_f(call)
        assert f.batch.n_desc == n
        ex = _check(f)
        variant = rc.F_VARIANTS[call % 3]
        assert ex.all() if variant == "all" else np.flatnonzero(ex).tolist() == ([n - 1] if variant == "one" else [])
