"""Device GetLimit (rl_resolve.hip: k_resolve's first pass and k_resolve_exact) at the edges of
its string handling and its two-pass hand-off, on an MI355X, against the config oracle
(oracle/config_oracle.py, GetLimit config_impl.go:274-323). The case sets are those of
tests/resolve_cases.py, which tests/test_resolve_edges_cpu.py runs through the host build of the
same walk and whose guards (which pass decides what) it asserts:

  A  names of 15/16/17 bytes (the first pass's 16 held in registers) and 31/32/33 bytes (the exact
     walk's 32), every string offset mod 4, key "_" value joined in one load window and apart,
     bytes_len ending at the last string's last byte (the 20-byte load window at the blob's
     end), the blob 1 and 3 bytes past a 16-B boundary (the byte path throughout);
  B  overrides over known, unknown, short and long domains;
  C  nodes with 0/1/7/8/9/20 children (8 hashes inline, more in the fast edge table), sibling
     names with equal edge hashes, 40 domains;
  D  a 9-level chain with the hand-off to the exact walk at level 1, 5 or 9;
  E  the descriptor left to the exact walk alone in its 256-thread block, at block edges, and
     past k_resolve_exact's 2048 blocks;
  F  nine calls of different sizes on one engine: the ring of four flag sets wraps twice, a
     small call reuses the set of a large one, and the flag buffer regrows.

Every descriptor of every set is compared, through Engine.resolve (host arrays) and
Engine.resolve_device (torch device buffers)."""
import numpy as np
import pytest
import torch  # (initialised before the engines, as in the other GPU test modules)

import hiprl
import resolve_cases as rc

pytestmark = pytest.mark.gpu


def _engine(cs, max_batch_desc=rc.F_MAX_BATCH_DESC):
    eng = hiprl.Engine(log2_slots=(10, 10, 10, 10), max_batch_desc=max_batch_desc)
    cs.cfg.install(eng)
    return eng


@pytest.fixture(scope="module")
def grid_engine():
    """One engine with set A's tree (sets A and E share it, so their calls also follow each
    other through the flag ring in whatever order they run)."""
    eng = _engine(rc.set_a())
    yield eng
    eng.close()


def _host(eng, cs):
    bad = rc.mismatches(cs, eng.resolve(cs.batch))
    assert not bad, "rl_resolve: " + bad


def _device(eng, cs, shift=0):
    """rl_resolve_device: the batch's arrays in torch device buffers, its blob (every byte of it,
    those past bytes_len too) `shift` bytes past a 16-B boundary."""
    b = cs.batch
    dev = torch.device("cuda", 0)
    words = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)
    raw = torch.full((b.bytes.size + 64,), ord("P"), dtype=torch.uint8, device=dev)
    base = (-raw.data_ptr()) % 16 + 16 + shift
    raw[base:base + b.bytes.size] = torch.from_numpy(b.bytes.copy()).to(dev)
    keep = [words(b.domain), words(b.entry_first), words(b.entry if b.entry.size else np.zeros(4, np.uint32)),
            words(b.override)]
    s = hiprl.RlResolveBatch()
    s.n_desc, s.n_entries, s.bytes_len, s.reserved = b.n_desc, b.n_entries, b.bytes_len, 0
    s.bytes, s.domain, s.entry_first, s.entry = raw.data_ptr() + base, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
    s.override_rule = keep[3].data_ptr() if b.has_override else None
    out = torch.full((b.n_desc,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.resolve_device(s, out.data_ptr())
    torch.cuda.synchronize()
    bad = rc.mismatches(cs, out.cpu().numpy().view(np.uint32))
    assert not bad, f"rl_resolve_device (blob + {shift}): " + bad


def _both(eng, cs):
    _host(eng, cs)
    _device(eng, cs)


def test_set_a_name_lengths_alignments_layouts_gpu(grid_engine):
    """Set A as built: 32 pad bytes after the last string, bytes_len counting them."""
    _both(grid_engine, rc.set_a())


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_set_a_bytes_len_at_the_last_byte_gpu(grid_engine, residue):
    """bytes_len ends at the last string's last byte, = residue mod 4; the buffer goes on with "P"
    and a longer name's bytes, and the tree holds the last value extended by "P"."""
    _both(grid_engine, rc.set_a_cut(residue))


@pytest.mark.parametrize("shift", [1, 3])
def test_set_a_unaligned_blob_gpu(grid_engine, shift):
    _device(grid_engine, rc.set_a(), shift)


def test_set_b_overrides_gpu():
    b = rc.set_b()
    _both(_engine(b), b)


def test_set_c_fanout_gpu():
    c = rc.set_c_fanout()
    _both(_engine(c), c)


@pytest.mark.parametrize("walk", ["fast", "exact"])
def test_set_c_collisions_gpu(walk):
    c = rc.set_c_collide(walk)
    _both(_engine(c), c)


def test_set_c_many_domains_gpu():
    c = rc.set_c_domains()
    _both(_engine(c), c)


@pytest.mark.parametrize("long_at", [1, 5, 9])
def test_set_d_depth_gpu(long_at):
    d = rc.set_d(long_at)
    _both(_engine(d), d)


@pytest.mark.parametrize("n", rc.E_SIZES)
def test_set_e_block_edges_gpu(grid_engine, n):
    """One descriptor for the exact walk at position 0, then at 255 / 256 / n-1, then none."""
    for variant in rc.E_VARIANTS:
        _both(grid_engine, rc.set_e(n, variant))


def test_set_e_past_the_exact_grid_gpu(grid_engine):
    """2050 blocks of descriptors, the exact walk's in blocks 0, 2047, 2048 and 2049: the second
    pass's 2048 blocks stride over the flags, and the "any" word sits at flags[2050]."""
    _both(grid_engine, rc.set_e(rc.E_BIG, "big"))


def test_set_f_flag_ring_sequence_gpu():
    """Calls of 70,000, 300, 257, 256, 1, 513, 70,001, 255 and 4097 descriptors on one engine
    (max_batch_desc 4096): all, none, or just the last of a call's descriptors need the exact
    walk. Each call is checked; once through rl_resolve, once more through rl_resolve_device."""
    f0 = rc.set_f(0)
    eng = _engine(f0)
    for form in (_host, _device):
        for call in range(len(rc.F_SIZES)):
            form(eng, rc.set_f(call))
    # a larger call still: the flag buffer regrows in mid-sequence, then small calls again
    cs, _, slow, _ = rc.pool()
    _host(eng, cs.take(slow[np.arange(150_001) % slow.size]))
    for call in (4, 3, 7, 1):
        _host(eng, rc.set_f(call))
