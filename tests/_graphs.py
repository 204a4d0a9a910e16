"""Shared test graphs (seeded, small enough for the oracle to finish in seconds)."""
from __future__ import annotations

import numpy as np

import oracle as orc
from gala import layout


def to_oracle(g: layout.HostGraph, val=None, heads=1) -> orc.Graph:
    v = g.val if val is None else val
    return orc.Graph(g.n_rows, g.n_cols, g.rowptr, g.col, v, g.n_seg, g.bounds, heads)


def cora_like(seed=42) -> layout.HostGraph:
    # N=2708, 5278 undirected edges + N self loops = 13264 stored edges
    return layout.gen_graph("uniform", 2708, 5278, seed)


def powerlaw(n=4096, m=30000, seed=7) -> layout.HostGraph:
    return layout.gen_graph("rmat", n, m, seed)


def banded(n=3000, width=40, per_row=6, seed=5) -> layout.HostGraph:
    """Symmetric graph with locality: every edge joins vertices at most `width` apart, plus
    self loops (a few vertex ranges touch each row: the sparse vertex-cut exchange)."""
    rng = np.random.default_rng(seed)
    u = np.repeat(np.arange(n, dtype=np.int64), per_row)
    v = np.clip(u + rng.integers(-width, width + 1, u.shape[0]), 0, n - 1)
    src = np.concatenate([u, v, np.arange(n)]).astype(np.int32)
    dst = np.concatenate([v, u, np.arange(n)]).astype(np.int32)
    return layout.csr_build(n, n, src, dst)


def with_empty_rows(n=700, m=3000, seed=3) -> layout.HostGraph:
    """Directed random graph (no self loops) with a block of empty rows + one heavy row."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n // 2, m).astype(np.int32)       # rows >= n/2 empty
    dst = rng.integers(0, n, m).astype(np.int32)
    heavy = np.full(900, 5, np.int32)                        # row 5: >= 900 edges
    src = np.concatenate([src, heavy])
    dst = np.concatenate([dst, rng.integers(0, n, 900).astype(np.int32)])
    return layout.csr_build(n, n, src, dst)


def long_row_graph(seed=3) -> layout.HostGraph:
    """Mean degree ~600 (hub threshold 8 * 600 > 4096): rows of 4 500 edges (above the row
    order's counting-sort cap, below the threshold) beside real hub rows of 9 000-12 000."""
    rng = np.random.default_rng(seed)
    n = 2000
    deg = rng.integers(450, 750, n)
    deg[[5, 700, 1500, 1999]] = 4500
    deg[[3, 900, 1200]] = [9000, 12000, 9000]
    src = np.repeat(np.arange(n), deg).astype(np.int32)
    dst = rng.integers(0, n, src.shape[0]).astype(np.int32)
    return layout.csr_build(n, n, src, dst)


PHASE_N = 8205          # 1026 blocks of 8 rows on a grid of 512: workgroups 0, 1 run three phases
PHASE_STEP = 8 * 512    # with the identity order row r hands off to row r + PHASE_STEP
PHASE_S = (0, 1, 16, 17, 64, 65)
PHASE_SPECIAL = (3, 15, 31, 32, 33, 63, 127, 128, 129)
PHASE_CLASSES = ((0, 0), (1, 15), (16, 16), (17, 63), (64, 64), (65, 1 << 30))


def phase_class(deg):
    """Batch class of a degree: 0, 1-15, 16, 17-63, 64, >= 65 (the 16-edge batch and the
    64-index column window of gat_input.hip's row walk)."""
    deg = np.asarray(deg)
    out = np.full(deg.shape, -1, np.int64)
    for k, (lo, hi) in enumerate(PHASE_CLASSES):
        out[(deg >= lo) & (deg <= hi)] = k
    return out


def phase_degrees(rng) -> np.ndarray:
    """The prescribed degrees of phase_graph (see there)."""
    n, step = PHASE_N, PHASE_STEP
    deg = rng.integers(0, 13, n)                         # every other row: ~6 on average
    deg[3000:3050] = 0                                   # blocks of empty rows in both phases
    deg[7000:7050] = 0
    for i in range(72):                                  # every ordered pair of S, twice, over
        r = 56 * i + i % 8                               # workgroups 0, 7, 14, ... and all 8 wave slots
        deg[r], deg[r + step] = PHASE_S[i % 6], PHASE_S[(i // 6) % 6]
    # the third phase (workgroups 0 and 1: rows 8192..8204) and the rows handing off to it;
    # slots 5..7 of workgroup 1 (rows 4109..4111) hand off to no row
    deg[2 * step:] = [65, 0, 17, 64, 1, 16, 129, 3, 0, 64, 17, 1, 65]
    deg[step + 8:step + 16] = [16, 65, 0, 1, 64, 65, 17, 0]
    # rows at the batch and window edges, as first-phase rows and as rows handed off to
    for k, d in enumerate(PHASE_SPECIAL):
        deg[1001 + 104 * k] = d
        deg[step + 1003 + 104 * k] = d
    deg[2000], deg[2000 + step] = 129, 128               # window refresh on both sides of a hand-off
    deg[1905 + step] = 1024                              # the longest row below the hub-row threshold
    return deg


def phase_graph(symmetric: bool, seed=11) -> layout.HostGraph:
    """8205 rows for the persistent input-space GAT kernels (csrc/gat_input.hip: 8 rows per
    workgroup phase, at most 512 workgroups): every workgroup runs two phases, workgroups 0 and
    1 three, the last block has 5 rows.  With the identity order row r hands off to row r +
    4096; the degrees are prescribed so that every ordered pair of {0, 1, 16, 17, 64, 65} is
    such a hand-off, beside rows of exactly 3, 15, 31, 32, 33, 63, 127, 128, 129 and 1024
    edges, blocks of empty rows and small random rows (0..12 edges).
    Directed: columns drawn uniformly, duplicates kept.  Symmetric: the same degrees kept
    exactly -- row r repeated deg[r] times, the list shuffled and consecutive entries (u, v)
    joined as the edges u -> v and v -> u (a loop (u, u) stored twice) -- so its empty rows are
    isolated vertices.  check_phase_graph asserts what the tests rely on."""
    rng = np.random.default_rng(seed)
    deg = phase_degrees(rng)
    n = PHASE_N
    if not symmetric:
        src = np.repeat(np.arange(n), deg)
        dst = rng.integers(0, n, src.shape[0])
    else:
        if deg.sum() % 2:
            deg[5] += 1                                  # (a small random row)
        stubs = rng.permutation(np.repeat(np.arange(n), deg))
        u, v = stubs[0::2], stubs[1::2]
        src, dst = np.concatenate([u, v]), np.concatenate([v, u])
        o = np.lexsort((dst, src))                       # rows sorted by column: A^T's CSR is A's
        src, dst = src[o], dst[o]
    return layout.csr_build(n, n, src.astype(np.int32), dst.astype(np.int32))


def check_phase_graph(g: layout.HostGraph, symmetric: bool):
    """What the multi-phase tests rely on, from the built rowptr."""
    n, step = g.n_rows, PHASE_STEP
    deg = np.diff(g.rowptr.astype(np.int64))
    assert n == PHASE_N and n % 8 != 0 and n > 2 * step and (n + 7) // 8 == 1026
    cls = phase_class(deg)
    assert (cls >= 0).all()
    pairs = set(zip(cls[:n - step].tolist(), cls[step:].tolist()))
    missing = [(a, b) for a in range(6) for b in range(6) if (a, b) not in pairs]
    assert not missing, f"hand-off class pairs missing: {missing}"
    third = set(zip(cls[step:n - step].tolist(), cls[2 * step:].tolist()))
    assert len(third) >= 6, third                        # second -> third phase hand-offs differ
    assert (deg >= 129).any() and deg.max() == 1024      # window refreshes; no hub-row plan (> 1024)
    assert layout.split_threshold(n, g.nnz) == 1024
    assert (deg == 0).sum() >= 100 and (deg[step:] == 0).any() and (deg[:step] == 0).any()
    for d in PHASE_SPECIAL + (1024,):
        assert (deg == d).any(), d
    assert g.nnz < 150_000
    gT, _ = layout.transpose(g)
    same = np.array_equal(gT.rowptr, g.rowptr) and np.array_equal(gT.col, g.col)
    assert same == symmetric
    if symmetric:                                        # the empty rows are isolated
        assert not np.isin(g.col, np.flatnonzero(deg == 0)).any()


LONG_N = 3000
LONG_DEFAULT = (1023, 1024, 1025, 1536, 1537, 2047, 2048, 2049, 2600)   # threshold 1024, 512-edge chunks
LONG_TEST = (63, 64, 65, 95, 96, 97, 128, 129)                          # threshold 64, chunks of 32 / 16


def long_rows_graph(seed=17) -> layout.HostGraph:
    """3 000 rows, directed and square, for the chunked hub-row paths of the edge / GAT kernels:
    rows of exactly LONG_DEFAULT edges (either side of the default plan's threshold 1024 and of
    its 512-edge chunk boundaries) and of exactly LONG_TEST edges (the same for the tests' plan:
    threshold 64, chunks of 32 or 16), on even and odd rows; a block of empty rows (odd rows
    only), one-edge rows, small random rows (1..12 edges).  Every even row has a self loop
    (counted in its length), no odd row has one: the statistics forward takes a row's own source
    logit from its self loop or from X[row].  Columns drawn uniformly, duplicates kept.
    check_long_rows_graph asserts what the tests rely on."""
    rng = np.random.default_rng(seed)
    n = LONG_N
    deg = rng.integers(1, 13, n)
    deg[1001:1200:2] = 0                                 # empty rows (odd: no self loop to hold)
    deg[1400:1500] = 1                                   # one-edge rows: a self loop / one random edge
    for k, d in enumerate(LONG_DEFAULT + LONG_TEST):
        deg[40 + 172 * k + k % 2] = d                    # rows 40, 213, 384, ...: even and odd
    src = np.repeat(np.arange(n), deg)
    dst = rng.integers(0, n, src.shape[0])
    first = np.concatenate([[0], np.cumsum(deg)])[:-1]
    even = np.flatnonzero((np.arange(n) % 2 == 0) & (deg > 0))
    odd = src % 2 == 1
    dst[odd & (dst == src)] = (src[odd & (dst == src)] + 1) % n     # no self loop on odd rows
    dst[first[even]] = even                                          # one on every even row
    return layout.csr_build(n, n, src.astype(np.int32), dst.astype(np.int32))


def check_long_rows_graph(g: layout.HostGraph):
    """What the long-row tests rely on, from the built rowptr."""
    from gala import _abi
    n = g.n_rows
    deg = np.diff(g.rowptr.astype(np.int64))
    assert n == LONG_N == g.n_cols and g.n_seg == 1 and 30_000 < g.nnz < 60_000
    for d in LONG_DEFAULT + LONG_TEST:
        assert (deg == d).sum() == 1, d
    assert deg.max() == 2600 and (deg == 0).sum() >= 100 and (deg == 1).sum() >= 100
    small = np.setdiff1d(np.arange(n), np.flatnonzero(np.isin(deg, LONG_DEFAULT + LONG_TEST)))
    assert deg[small].max() <= 12
    assert layout.split_threshold(n, g.nnz) == 1024
    rows = np.repeat(np.arange(n), deg)
    loops = np.zeros(n, bool)
    loops[rows[rows == g.col]] = True
    assert loops[0::2].all() and not loops[1::2].any()
    long_ = np.flatnonzero(deg > 64)
    assert (long_ % 2 == 0).any() and (long_ % 2 == 1).any()

    def plan(threshold, chunk):
        nr, nc = np.zeros(1, np.int64), np.zeros(1, np.int64)
        _abi.call("gala_host_split_plan", n, g.rowptr.ctypes.data, threshold, chunk, None, None, None,
                  nr.ctypes.data, nc.ctypes.data)
        return int(nr[0]), int(nc[0])
    hub = [d for d in LONG_DEFAULT if d > 1024]
    mid = [d for d in LONG_DEFAULT + LONG_TEST if d > 64]
    assert len(hub) == 7 and len(mid) == 15              # strictly above the threshold
    assert plan(1024, 512) == (7, sum(-(-d // 512) for d in hub))
    for c in (32, 16):
        assert plan(64, c) == (15, sum(-(-d // c) for d in mid))


_BOUND_GRAPHS = {}


def edge_bound_graph(name) -> layout.HostGraph:
    """The graphs of the per-element bound tests, built once: "long" (long_rows_graph, checked),
    "long_tiled" (by 1000 columns), "empty" (with_empty_rows) and "empty_tiled" (by 300)."""
    if not _BOUND_GRAPHS:
        g = long_rows_graph()
        check_long_rows_graph(g)
        e = with_empty_rows()
        _BOUND_GRAPHS.update(long=g, long_tiled=layout.col_tile(g, 1000), empty=e,
                             empty_tiled=layout.col_tile(e, 300))
    return _BOUND_GRAPHS[name]


def features(n, F, seed=1234, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(-8, 9, (n, F)).astype(np.float32)
    return rng.uniform(-1, 1, (n, F)).astype(np.float32)


def edge_values(nnz, heads=1, seed=99, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, nnz * heads).astype(np.float32)
