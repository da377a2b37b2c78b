"""Snapshot file format (CPU only): rl_snapshot_header's layout against the ctypes struct, the
file round trip of hiprl.write_snapshot / read_snapshot, and every malformed-file error."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import hiprl

ROOT = Path(__file__).resolve().parents[1]

FIELDS = ["magic", "header_bytes", "record_bytes", "flags", "reserved0", "seed_check", "n_records", "gen", "live",
          "prev", "src_log2", "reserved"]


def test_header_layout_matches_ctypes(tmp_path):
    offs = ",".join(f"offsetof(rl_snapshot_header,{f})" for f in FIELDS)
    src = tmp_path / "snap.c"
    src.write_text('#include "rl_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){size_t v[]={'
                   f'sizeof(rl_snapshot_header),RL_SNAP_HEADER_BYTES,RL_SNAP_RECORD_BYTES,RL_SNAP_SPLIT,RL_SNAP_LAG,'
                   f'RL_SNAP_LOCAL_CACHE,{offs}}};'
                   'for(unsigned i=0;i<sizeof v/sizeof v[0];++i)printf("%zu ",v[i]);return 0;}\n')
    exe = tmp_path / "snap"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    H = hiprl.RlSnapshotHeader
    want = [C.sizeof(H), hiprl.SNAP_HEADER_BYTES, hiprl.SNAP_RECORD_BYTES, hiprl.SNAP_SPLIT, hiprl.SNAP_LAG,
            hiprl.SNAP_LOCAL_CACHE] + [getattr(H, f).offset for f in FIELDS]
    assert got == want
    assert C.sizeof(H) == 256
    assert [f for f, _ in H._fields_] == FIELDS
    assert hiprl.SNAP_DTYPE.itemsize == 32
    assert [hiprl.SNAP_DTYPE.fields[f][1] for f in ("ctrl", "key", "count", "exp", "pcount", "frz")] == [0, 8, 16, 20,
                                                                                                          24, 28]


def synthetic(n, seed=5):
    rng = np.random.default_rng(seed)
    recs = np.zeros(n, hiprl.SNAP_DTYPE)
    for f in recs.dtype.names:
        recs[f] = rng.integers(0, np.iinfo(recs.dtype[f]).max, n, dtype=recs.dtype[f], endpoint=True)
    h = hiprl.RlSnapshotHeader()
    h.magic[:] = hiprl.SNAP_MAGIC
    h.header_bytes, h.record_bytes = hiprl.SNAP_HEADER_BYTES, hiprl.SNAP_RECORD_BYTES
    h.flags = hiprl.SNAP_SPLIT | hiprl.SNAP_LOCAL_CACHE
    h.seed_check = 0x0123456789ABCDEF
    h.n_records = n
    for r in range(8):
        h.gen[r], h.src_log2[r] = 1000 + r, 10 + r
    h.live[4] = n
    return h, recs


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_file_round_trip(tmp_path, n):
    h, recs = synthetic(n)
    p = tmp_path / "t.rlsnap"
    hiprl.write_snapshot(p, h, recs)
    raw = p.read_bytes()
    assert len(raw) == 256 + 32 * n
    assert raw[:8] == b"RLSNAP01" and raw[:256] == bytes(h) and raw[256:] == recs.tobytes()
    h2, recs2 = hiprl.read_snapshot(p)
    assert bytes(h2) == bytes(h)
    assert recs2.dtype == hiprl.SNAP_DTYPE and np.array_equal(recs2, recs)
    assert list(h2.gen) == [1000 + r for r in range(8)] and h2.n_records == n and h2.seed_check == 0x0123456789ABCDEF


def test_malformed_files(tmp_path):
    h, recs = synthetic(10)
    good = tmp_path / "good"
    hiprl.write_snapshot(good, h, recs)
    raw = good.read_bytes()

    def bad(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(ValueError):
            hiprl.read_snapshot(p)

    bad("magic", b"RLSNAP02" + raw[8:])
    bad("hbytes", raw[:8] + (128).to_bytes(4, "little") + raw[12:])
    bad("rbytes", raw[:12] + (64).to_bytes(4, "little") + raw[16:])
    bad("short", raw[:-1])
    bad("record_short", raw[:-32])
    bad("long", raw + b"\0" * 32)
    bad("header_only_part", raw[:100])
    bad("empty", b"")
    # write side: a header that is no snapshot header, a count that is not len(records), odd items
    h3, _ = synthetic(10)
    h3.magic[0] = 0
    with pytest.raises(ValueError):
        hiprl.write_snapshot(tmp_path / "w1", h3, recs)
    with pytest.raises(ValueError):
        hiprl.write_snapshot(tmp_path / "w2", h, recs[:9])
    with pytest.raises(ValueError):
        hiprl.write_snapshot(tmp_path / "w3", h, np.zeros(10, np.uint32))
    assert hiprl.read_snapshot(good)[0].n_records == 10
