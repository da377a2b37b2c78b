"""Case sets for the device GetLimit (rl_resolve.hip: k_resolve's first pass, k_resolve_exact)
at its name-length, layout, fan-out, depth, block and flag-ring edges. TEST INFRASTRUCTURE ONLY.

Each case set is one descriptor tree (YAML, loaded by rl_config.RateLimitConfig for the device
and by config_oracle.Config for the expected answers) and one resolve batch whose arrays are
built here directly, so every string's offset in the blob is chosen: rl_config.ResolveBatch lays
strings out incidentally. tests/test_resolve_edges_cpu.py runs the sets through the host build
of the walk (tests/cshim/librl_resolve_shim.so), tests/test_gpu_resolve_edges.py through the
engine on the device; both compare against config_oracle (GetLimit, config_impl.go:274-323).
The shim only classifies which pass decides a descriptor; no expected value comes from it.

Conventions: every limit of a tree has its own requests_per_unit, so (requests_per_unit, unit)
names the node a lookup landed on. The byte after every string is the pad character "P"; names
use lower-case letters and digits, so a walk that reads one byte too many meets a byte no
name ends with unless the tree plants that name (the "P" / "_" extended nodes below).
"""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

import config_oracle
import hiprl
import rl_config

SHIM = Path(__file__).resolve().parent / "cshim" / "librl_resolve_shim.so"
PAD = b"P"
PAD_TAIL = 32                    # pad bytes after the last string of a blob as built
FIRST_PASS_BYTES = 16            # rl_resolve.hip FB: names the first pass holds in registers
UNITS = ("second", "minute", "hour", "day")
ALPHA = "abcdefghijklmnopqrstuvwxyz0123456789"


def name(first, n):
    """A name of n bytes starting with `first`; name(c, a) is a prefix of name(c, b) for a < b,
    so a walk that drops or adds trailing bytes lands on another node of the tree."""
    return (first + ALPHA * 2)[:n]


# ---- trees ----
class Tree:
    """A YAML descriptor tree under construction: nodes get distinct limits in creation order."""

    def __init__(self, domain, first_limit=1):
        self.domain = domain
        self.top = []
        self.next_limit = first_limit

    def node(self, parent, key, value=None, limit=True):
        """Add key[_value] under parent (None: the domain) and return it."""
        n = {"key": key, "value": value, "limit": None, "children": []}
        if limit:
            n["limit"] = (self.next_limit, UNITS[self.next_limit % 4])
            self.next_limit += 1
        (self.top if parent is None else parent["children"]).append(n)
        return n

    def yaml(self):
        lines = [f'domain: "{self.domain}"']

        def emit(nodes, ind):
            if not nodes:
                return
            lines.append(" " * ind + "descriptors:")
            for n in nodes:
                lines.append(" " * ind + f'  - key: "{n["key"]}"')
                if n["value"] is not None:
                    lines.append(" " * ind + f'    value: "{n["value"]}"')
                if n["limit"]:
                    lines.append(" " * ind + f'    rate_limit: {{unit: {n["limit"][1]}, requests_per_unit: {n["limit"][0]}}}')
                emit(n["children"], ind + 4)

        emit(self.top, 0)
        return "\n".join(lines) + "\n"


# ---- batches ----
class Batch:
    """The fields of rl_config.ResolveBatch and its struct(), over arrays given directly.
    blob: every byte a device buffer holds (pad included); bytes_len: what the batch declares."""

    def __init__(self, blob, bytes_len, domain, entry_first, entry, override=None):
        self.bytes = np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else blob
        self.bytes_len = int(bytes_len)
        self.domain = np.ascontiguousarray(domain, np.uint32).reshape(-1)
        self.entry_first = np.ascontiguousarray(entry_first, np.uint32)
        self.entry = np.ascontiguousarray(entry, np.uint32).reshape(-1)
        self.n_desc = self.entry_first.size - 1
        self.n_entries = self.entry.size // 4
        assert self.domain.size == 2 * self.n_desc and int(self.entry_first[-1]) == self.n_entries
        self.has_override = override is not None
        self.override = (np.ascontiguousarray(override, np.uint32) if self.has_override
                         else np.full(self.n_desc, hiprl.NIL_RULE, np.uint32))

    def struct(self):
        s = hiprl.RlResolveBatch()
        s.n_desc, s.n_entries, s.bytes_len, s.reserved = self.n_desc, self.n_entries, self.bytes_len, 0
        p = lambda a: a.ctypes.data if a.size else None
        s.bytes, s.domain, s.entry_first, s.entry = p(self.bytes), p(self.domain), p(self.entry_first), p(self.entry)
        s.override_rule = p(self.override) if self.has_override else None
        return s

    def last_string_end(self, n_desc):
        """One past the last byte of any string of descriptors [0, n_desc)."""
        d = self.domain.reshape(-1, 2)[:n_desc].astype(np.int64)
        e = self.entry.reshape(-1, 4)[:int(self.entry_first[n_desc])].astype(np.int64)
        ends = [int((d[:, 0] + d[:, 1]).max())] if n_desc else [0]
        if e.size:
            ends += [int((e[:, 0] + e[:, 1]).max()), int((e[:, 2] + e[:, 3]).max())]
        return max(ends)

    def head(self, n_desc, bytes_len):
        """The first n_desc descriptors over the same blob, declaring bytes_len of it."""
        ne = int(self.entry_first[n_desc])
        return Batch(self.bytes, bytes_len, self.domain[:2 * n_desc], self.entry_first[:n_desc + 1], self.entry[:4 * ne],
                     self.override[:n_desc] if self.has_override else None)

    def take(self, idx):
        """Descriptors idx (repeats allowed) over the same strings: the index arrays tiled."""
        idx = np.asarray(idx, np.int64)
        f0 = self.entry_first.astype(np.int64)
        cnt = (f0[1:] - f0[:-1])[idx]
        first = np.concatenate([[0], np.cumsum(cnt)])
        rows = np.repeat(f0[:-1][idx], cnt) + (np.arange(int(first[-1])) - np.repeat(first[:-1], cnt))
        return Batch(self.bytes, self.bytes_len, self.domain.reshape(-1, 2)[idx], first, self.entry.reshape(-1, 4)[rows],
                     self.override[idx] if self.has_override else None)


class Layout:
    """A blob written string by string. A descriptor goes in at an offset = r mod 4, either
    joined (domain "_" key "_" value "_" ..., the cache key's prefix: each value starts at its
    key's offset + length + 1) or separate (its values, then the domain, then its keys, a pad
    byte after each: no value follows its key)."""

    def __init__(self):
        self.buf = bytearray()
        self.dom, self.first, self.ent = [], [0], []

    def _put(self, s, after=PAD):
        b = s.encode()
        r = (len(self.buf), len(b))
        self.buf += b + after
        return r

    def add(self, domain, entries, r=0, joined=True):
        while len(self.buf) % 4 != r:
            self.buf += PAD
        if joined:
            self.dom += self._put(domain, b"_")
            for k, v in entries:
                kr = self._put(k, b"_")
                self.ent += kr + self._put(v, b"_")
            self.buf += PAD
        else:
            vs = [self._put(v) for _, v in entries]
            self.dom += self._put(domain)
            for (k, _), vr in zip(entries, vs):
                self.ent += self._put(k) + vr
        self.first.append(len(self.ent) // 4)

    def batch(self, override=None):
        n = len(self.buf)
        return Batch(bytes(self.buf) + PAD * PAD_TAIL, n + PAD_TAIL, self.dom, self.first, self.ent, override)


class CaseSet:
    """One tree and one batch. descs[i] = (domain, entries, override (limit, unit) or None) is
    what the oracle gets; batch descriptor j is descs[index[j]] (index None: one to one), so a
    tiled batch costs the oracle its base descriptors only."""

    def __init__(self, files, descs, batch, cfg=None, index=None, of=None):
        self.files = files
        self.descs = descs
        self.batch = batch
        self.index = index
        self._of = of  # the set whose tree, descs and expected answers this one tiles
        self.cfg = cfg or (of.cfg if of else rl_config.RateLimitConfig(files))

    @functools.cached_property
    def orc(self):
        return self._of.orc if self._of else config_oracle.Config(self.files)

    @functools.cached_property
    def base_want(self):
        return self._of.base_want if self._of else expected(self.orc, self.descs)

    @functools.cached_property
    def want(self):
        w = self.base_want
        return w if self.index is None else [w[i] for i in self.index]

    def desc(self, j):
        return self.descs[j if self.index is None else int(self.index[j])]

    def take(self, idx):
        idx = np.asarray(idx, np.int64)
        return CaseSet(self.files, self.descs, self.batch.take(idx), index=idx if self.index is None else self.index[idx],
                       of=self._of or self)

    def head(self, n_desc, bytes_len):
        return CaseSet(self.files, self.descs, self.batch.head(n_desc, bytes_len),
                       index=np.arange(n_desc) if self.index is None else self.index[:n_desc], of=self._of or self)


def expected(orc, descs):
    """(requests_per_unit, unit) or None per descriptor, from config_oracle.Config.get_limit."""
    out = []
    for d in descs:
        w = orc.get_limit(d[0], d[1], override=d[2] if len(d) > 2 else None)
        out.append(None if w is None else (w.requests_per_unit, w.unit))
    return out


def have(cfg, rule_ids):
    """(requests_per_unit, unit) or None per rule id of cfg's rule table (an id outside the
    table, such as the first pass's "left to the exact walk" mark, stays visible as itself)."""
    tab = [(r.requests_per_unit, r.unit) for r in cfg.rules]
    return [None if r == hiprl.NIL_RULE else tab[r] if r < len(tab) else ("no such rule", hex(r))
            for r in np.asarray(rule_ids).astype(np.int64).tolist()]


def mismatches(cs, rule_ids, limit=5):
    """Text for the descriptors whose answer differs from the oracle's ('' when none do)."""
    got, want = have(cs.cfg, rule_ids), cs.want
    assert len(got) == len(want) == cs.batch.n_desc
    bad = [j for j, (a, b) in enumerate(zip(got, want)) if a != b]
    if not bad:
        return ""
    d, e = cs.batch.domain.reshape(-1, 2), cs.batch.entry.reshape(-1, 4)
    rows = []
    for j in bad[:limit]:
        ent = e[int(cs.batch.entry_first[j]):int(cs.batch.entry_first[j + 1])].tolist()
        rows.append(f"#{j} {cs.desc(j)} domain@{d[j].tolist()} entries@{ent}: have {got[j]}, want {want[j]}")
    return f"{len(bad)} of {len(want)} differ: " + "; ".join(rows)


# ---- the host build of the walk ----
@functools.lru_cache(maxsize=None)
def shim():
    if not SHIM.exists():
        subprocess.run(["make", "-C", str(SHIM.parent), SHIM.name], check=True, capture_output=True)
    lib = C.CDLL(str(SHIM))
    lib.rls_resolve2.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(hiprl.RlResolveBatch),
                                 C.c_void_p, C.c_void_p, C.c_int]
    lib.rls_resolve2.restype = C.c_int
    return lib


def shim_resolve(cfg, batch, shift=0, exact_only=False):
    """The shim's rls_resolve2 -> (rules, took_exact_walk). shift: the blob that many bytes past
    a 16-B boundary. exact_only: resolve_one alone (every descriptor counts as exact)."""
    nodes, names = cfg.tree_arrays()
    nodes = np.ascontiguousarray(nodes, np.uint32)
    nb = np.frombuffer(names or b"\0", np.uint8)
    s = batch.struct()
    raw = np.zeros(batch.bytes.size + 32, np.uint8)
    base = (-raw.ctypes.data) % 16 + shift
    raw[base:base + batch.bytes.size] = batch.bytes
    s.bytes = raw.ctypes.data + base
    out = np.zeros(max(1, batch.n_desc), np.uint32)
    ex = np.zeros(max(1, batch.n_desc), np.uint8)
    rc = shim().rls_resolve2(nodes.ctypes.data, nodes.shape[0], nb.ctypes.data, len(names), C.byref(s), out.ctypes.data,
                             ex.ctypes.data, 1 if exact_only else 0)
    assert rc == 0
    return out[:batch.n_desc], ex[:batch.n_desc].astype(bool)


# ---- A: name length x alignment x layout ----
KEY_LENS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 40)
JOINED_LENS = (15, 16, 17, 31, 32, 33, 34, 41)  # key "_" value
DOMAIN_LENS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 40)
# cells (key length, value length) whose value also exists extended by the byte that follows it
# in the blob ("P" in the separate layout, "_" in the joined one), one or more per length class:
# key "_" value of 8, 16 and 17 (first pass), 32 (the exact walk's registers), 34 (the byte path)
TRAPS = ((5, 2), (7, 8), (8, 8), (15, 16), (16, 17))
TAIL_CELL = (7, 8)       # the blob's last descriptors (configuration 2 ends bytes_len inside them)
PLANTED_KEY = name("x", 20)  # a key-only node no first pass can hold: sets E and F plant it
GRID = "grid"


def value_lens(kl):
    return sorted({1, 2} | {t - kl - 1 for t in JOINED_LENS if t - kl - 1 >= 1})


@functools.lru_cache(maxsize=None)
def grid_files():
    t = Tree(GRID)
    for kl in KEY_LENS:
        k = name("k", kl)
        t.node(None, k)
        for vl in value_lens(kl):
            t.node(None, k, name("v", vl))
            if (kl, vl) in TRAPS:
                t.node(None, k, name("v", vl) + "P")
                t.node(None, k, name("v", vl) + "_")
    t.node(None, PLANTED_KEY)
    files = [("grid.yaml", t.yaml())]
    nxt = t.next_limit
    for dl in DOMAIN_LENS:
        d = Tree(name("d", dl), nxt)
        d.node(None, "c")
        nxt = d.next_limit
        files.append((f"d{dl}.yaml", d.yaml()))
    return tuple(files)


def _last_changed(s):
    return s[:-1] + "Z"


def grid_queries():
    """(domain, entries) per query of set A, before layout."""
    q = []
    for kl in KEY_LENS:
        k = name("k", kl)
        for vl in value_lens(kl):
            v = name("v", vl)
            q += [(GRID, [(k, v)]), (GRID, [(k, _last_changed(v))]), (GRID, [(k, v + "Y")]), (GRID, [(k, v[:-1])]),
                  (GRID, [(_last_changed(k), v)]), (GRID, [(k, "")])]
    return q


def domain_queries():
    q = []
    for dl in DOMAIN_LENS:
        d = name("d", dl)
        q += [d, _last_changed(d), d + "Y", d[:-1]]
    return q


@functools.lru_cache(maxsize=None)
def set_a():
    """Every query 8 times (offsets = 0..3 mod 4, joined and separate); the blob ends with the
    TAIL_CELL pair, joined, at the four alignments (their values end at four residues mod 4)."""
    lay, descs = Layout(), []

    def put(d, e):
        for joined in (True, False):
            for r in range(4):
                lay.add(d, e, r, joined)
                descs.append((d, e, None))

    for d, e in grid_queries():
        put(d, e)
    for d in domain_queries():
        put(d, [("c", "1")])
    tail = (GRID, [(name("k", TAIL_CELL[0]), name("v", TAIL_CELL[1]))])
    for r in range(4):
        lay.add(tail[0], tail[1], r, True)
        descs.append(tail + (None,))
    return CaseSet(list(grid_files()), descs, lay.batch())


def beyond_the_end(n):
    """What a device buffer holds past a batch whose bytes_len ends at the TAIL_CELL value's last
    byte: "P" (the tree holds that value extended by "P"), then bytes that go on as a longer name."""
    return (PAD + name("v", 64)[TAIL_CELL[1]:].encode() * 8)[:n]


@functools.lru_cache(maxsize=None)
def set_a_cut(residue):
    """Set A with bytes_len at its last string's last byte, = residue mod 4: the fewest trailing
    descriptors (0-3) dropped that get there."""
    a = set_a()
    for drop in range(4):
        n = a.batch.n_desc - drop
        end = a.batch.last_string_end(n)
        if end % 4 == residue:
            cut = a.head(n, end)
            blob = a.batch.bytes.copy()  # what lies past bytes_len is not the set's own next descriptor
            blob[end:] = np.frombuffer(beyond_the_end(blob.size - end), np.uint8)
            cut.batch.bytes = blob
            return cut
    raise AssertionError(f"no cut with bytes_len = {residue} mod 4")


# ---- B: overrides ----
@functools.lru_cache(maxsize=None)
def set_b():
    """The domain queries with override rules: rows alternate no override / an override, with
    0, 1 or 3 entries; an existing domain gives the override whatever the entries are
    (config_impl.go:286-296), an unknown domain nil (:279-284)."""
    cfg = rl_config.RateLimitConfig(list(grid_files()))
    lay, descs, ov = Layout(), [], []
    shapes = ([], [("c", "1")], [("c", "1"), (name("k", 5), name("v", 2)), ("zz", "")])
    i = 0
    for rep in range(2):                     # every domain query meets both an override and none
        for d in domain_queries():
            for joined in (True, False):
                e = shapes[(i // 2) % 3]
                lim = None if (i + rep) % 2 == 0 else (1000 + i % 13, 1 + i % 4)
                lay.add(d, e, (i + rep) % 4, joined)
                descs.append((d, e, lim))
                ov.append(hiprl.NIL_RULE if lim is None else cfg.override_rule(d, e, *lim))
                i += 1
    return CaseSet(list(grid_files()), descs, lay.batch(ov), cfg=cfg)


# ---- C: fan-out, sibling hash collisions, many domains ----
FAN = (0, 1, 7, 8, 9, 20)  # children: a fast node holds up to 8 hashes inline (FAST_CHILDREN)


def _fan_children(t, parent, n):
    """n children under parent: key/value and key-only forms of the key "c", plus distinct keys."""
    kids = []
    if n == 1:
        return [(t.node(parent, "c", "v0"), ("c", "v0"))]
    if n:
        kids.append((t.node(parent, "c"), ("c", "")))
    for j in range(n // 2):
        kids.append((t.node(parent, "c", f"v{j}"), ("c", f"v{j}")))
    for j in range(n - len(kids)):
        kids.append((t.node(parent, f"d{j}"), (f"d{j}", "q")))
    return kids


@functools.lru_cache(maxsize=None)
def set_c_fanout():
    t = Tree("fan")
    paths = []  # (entries to a parent, its children [(node, entry)])
    for n in FAN:
        p = t.node(None, f"p{n}")
        paths.append(([(f"p{n}", "")], _fan_children(t, p, n)))
    q = t.node(None, "q", "w", limit=False)
    for n in FAN:  # the same shapes one level further down
        r = t.node(q, f"r{n}", limit=n % 2 == 0)
        paths.append(([("q", "w"), (f"r{n}", "any")], _fan_children(t, r, n)))
    lay, descs = Layout(), []
    i = 0

    def put(e):
        nonlocal i
        lay.add("fan", e, i % 4, i % 8 < 4)
        lay.add("fan", e, (i + 1) % 4, i % 8 >= 4)
        descs.extend([("fan", e, None)] * 2)
        i += 1

    for path, kids in paths:
        put(path)                                   # the parent itself
        for _, ent in kids:
            put(path + [ent])                       # every child
        put(path + [("zz", "x")])                   # a miss under the parent
        put(path + [("c", "nope")])                 # the key-only sibling of the "c" values
        put(path + [("d0", "x"), ("c", "v0")])      # past a leaf
    return CaseSet([("fan.yaml", t.yaml())], descs, lay.batch())


@functools.lru_cache(maxsize=None)
def set_c_collide(walk):
    """The two trees and ten descriptors of tests/test_resolve_host.py's
    test_edge_hash_collisions_take_the_exact_walk: sibling names whose 32-bit edge hashes collide
    under the first pass's hash (walk "fast") or the exact walk's (walk "exact")."""
    from test_resolve_host import _colliding, _fast_id, _mix
    lib = shim()
    probe = rl_config.RateLimitConfig([("p.yaml", "domain: dc\ndescriptors:\n  - key: a\n    value: x\n")])
    nodes, _ = probe.tree_arrays()
    dom = int(np.nonzero(nodes[:, 0] == 0xFFFFFFFF)[0][0])
    fn = "rls_fast_hash" if walk == "fast" else "rls_tree_hash"
    par = _fast_id(lib, probe, dom) if walk == "fast" else dom
    ci, cj = _colliding(lib, par, lambda k: f"a_{_mix(k)}", fn=fn)
    cp, cq = _colliding(lib, par, lambda k: f"k{_mix(k)}", fn=fn)
    i, j, p, q = _mix(ci), _mix(cj), _mix(cp), _mix(cq)
    t = Tree("dc")
    a = t.node(None, "a", i)
    t.node(a, "b")
    t.node(None, "a", j)
    t.node(None, "a")
    t.node(None, f"k{p}")
    t.node(None, f"k{q}")
    t2 = Tree("dd", t.next_limit)
    t2.node(None, "a", i)
    t2.node(None, "a")
    files = [("c.yaml", t.yaml()), ("d.yaml", t2.yaml())]
    cfg = rl_config.RateLimitConfig(files)
    nodes2, _ = cfg.tree_arrays()
    assert int(np.nonzero(nodes2[:, 0] == 0xFFFFFFFF)[0][0]) == dom  # the hashes were searched under this parent
    assert walk != "fast" or _fast_id(lib, cfg, dom) == par
    qs = [("dc", [("a", i)]), ("dc", [("a", j)]), ("dc", [("a", "nope")]), ("dc", [(f"k{p}", "v")]),
          ("dc", [(f"k{q}", "v")]), ("dc", [("a", i), ("b", "z")]), ("dc", [("a", j), ("b", "z")]),
          ("dd", [("a", j)]), ("dd", [("a", i)]), ("dc", [(f"k{q}", "v"), ("b", "z")])]
    lay, descs = Layout(), []
    for n, (d, e) in enumerate(qs):
        for joined in (True, False):
            lay.add(d, e, n % 4, joined)
            descs.append((d, e, None))
    return CaseSet(files, descs, lay.batch(), cfg=cfg)


@functools.lru_cache(maxsize=None)
def set_c_domains():
    """40 domains (the domain edge table then has probe chains); each queried, and 40 absent."""
    files, lay, descs = [], Layout(), []
    nxt = 1
    for n in range(40):
        t = Tree(f"dom{n}" + "x" * (n % 11), nxt)
        t.node(None, "c")
        nxt = t.next_limit
        files.append((f"m{n}.yaml", t.yaml()))
    for n in range(40):
        for d in (f"dom{n}" + "x" * (n % 11), f"dom{n}" + "y" * (1 + n % 11)):
            lay.add(d, [("c", "1")], n % 4, n % 2 == 0)
            descs.append((d, [("c", "1")], None))
    return CaseSet(files, descs, lay.batch())


# ---- D: depth ----
DEPTH = 9


@functools.lru_cache(maxsize=None)
def set_d(long_at):
    """A 9-level chain: odd levels key/value nodes, even levels key-only; levels 2, 5 and 8 carry
    no limit; level 3 also has a key-only sibling and level 4 a leaf "b4". The key at level
    long_at has 20 bytes, so the first pass hands off to the exact walk at that depth."""
    key = lambda l: name(f"a{l}", 20) if l == long_at else f"a{l}"
    ent = lambda l: (key(l), f"x{l}") if l % 2 else (key(l), f"any{l}")
    t = Tree("deep")
    p = None
    for l in range(1, DEPTH + 1):
        nxt = t.node(p, key(l), f"x{l}" if l % 2 else None, limit=l not in (2, 5, 8))
        if l == 3:
            t.node(p, key(3))       # the fall-back of a3_<other value>: a leaf
        if l == 4:
            t.node(p, "b4")         # a leaf beside a4
        p = nxt
    chain = [ent(l) for l in range(1, DEPTH + 1)]
    qs = [chain[:n] for n in (0, 1, 2, 3, 5, 8, 9)]
    qs.append(chain + [("a10", "x10")])                         # 10 entries: past the chain's end
    qs += [chain[:3] + [("b4", "")], chain[:3] + [("b4", "")] + chain[4:6], chain[:3] + [("b4", "v"), ("a5", "x5")]]
    qs += [chain[:2] + [(key(3), "other")], chain[:2] + [(key(3), "other")] + chain[3:5]]
    for l in range(1, DEPTH + 1):                               # diverge at level l, then go on along the chain
        qs.append(chain[:l - 1] + [("zz", "q")] + chain[l:])
        qs.append(chain[:l - 1] + [(key(l), "x0")] + chain[l:l + 1])   # (an even level takes any value)
    lay, descs = Layout(), []
    for n, e in enumerate(qs):
        for joined in (True, False):
            lay.add("deep", e, n % 4, joined)
            descs.append(("deep", e, None))
    return CaseSet([("deep.yaml", t.yaml())], descs, lay.batch())


# ---- E and F: block, grid and flag-ring edges ----
def _first_pass_by_rule(d):
    """Names of at most 16 bytes throughout (and the blob has 32 pad bytes): the first pass
    decides the descriptor unless hashes collide; the CPU test checks this with the shim."""
    return len(d[0]) <= FIRST_PASS_BYTES and all(len(k) + 1 + len(v) <= FIRST_PASS_BYTES for k, v in d[1])


def _exact_by_rule(d):
    """A domain over 16 bytes, or the grid domain and a first entry over 16 bytes: the first
    pass leaves the descriptor to the exact walk."""
    return len(d[0]) > FIRST_PASS_BYTES or (d[0] == GRID and len(d[1][0][0]) + 1 + len(d[1][0][1]) > FIRST_PASS_BYTES)


@functools.lru_cache(maxsize=None)
def pool():
    """Set A's descriptors plus the planted one (the 20-byte key-only node, which hits), over one
    blob: (case set, ids the first pass decides (at most 1023), ids the exact walk decides, the
    planted id). Sets E and F tile these."""
    lay, descs = Layout(), []
    a = set_a()
    for j, d in enumerate(a.descs):
        lay.add(d[0], d[1], j % 4, (j // 4) % 2 == 0)
        descs.append(d)
    lay.add(GRID, [(PLANTED_KEY, "")], 1, True)
    descs.append((GRID, [(PLANTED_KEY, "")], None))
    cs = CaseSet(list(grid_files()), descs, lay.batch())
    fast = [j for j, d in enumerate(a.descs) if _first_pass_by_rule(d)]
    step = max(1, len(fast) // 1023 + 1)
    fast = np.array(fast[::step][:1023])
    slow = np.array([j for j, d in enumerate(a.descs) if _exact_by_rule(d)])
    return cs, fast, slow, len(descs) - 1


E_SIZES = (1, 255, 256, 257, 511, 513, 4097)
E_VARIANTS = ("first", "block_edges", "none")
E_BIG = 2049 * 256 + 3  # 2050 blocks: k_resolve_exact's 2048 blocks stride (RS_EXACT_BLOCKS)


def e_positions(n, variant):
    if variant == "first":
        return [0]
    if variant == "block_edges":
        return sorted({p for p in (255, 256, n - 1) if 0 <= p < n})
    if variant == "big":  # blocks 0, 2047, 2048 and 2049 (the last, of 3 descriptors)
        return [5, 2047 * 256 + 100, 2048 * 256, 2049 * 256 + 2]
    return []


@functools.lru_cache(maxsize=None)
def set_e(n, variant):
    """n descriptors the first pass decides, the planted one at e_positions(n, variant)."""
    cs, fast, _, planted = pool()
    idx = fast[np.arange(n) % fast.size]
    idx[e_positions(n, variant)] = planted
    return cs.take(idx)


# F: calls on one engine in this order; all / none / exactly one (in the last block) of a call's
# descriptors need the exact walk. The engine's max_batch_desc stays below the large sizes.
F_SIZES = (70_000, 300, 257, 256, 1, 513, 70_001, 255, 4097)
F_VARIANTS = ("all", "none", "one")
F_MAX_BATCH_DESC = 4096


def set_f(call):
    cs, fast, slow, planted = pool()
    n, variant = F_SIZES[call], F_VARIANTS[call % 3]
    src = slow if variant == "all" else fast
    idx = src[(np.arange(n) + 7 * call) % src.size]
    if variant == "one":
        idx[n - 1] = planted
    return cs.take(idx)
