"""Grid caps of the grid-stride and persistent kernels, and the graphs that cross them.

Every kernel below caps its grid and loops; a test that stays under the cap runs the loop body
once.  The constants mirror the launch code (file:line beside each); every test that uses one
asserts that its shape is past it, so a changed cap fails that assertion instead of silently
falling back to one round.  tests/test_gat_input_rounds_cpu.py and the test_gpu_*_rounds.py
files use them.
"""
from __future__ import annotations

import numpy as np

from gala import _abi, layout
from _hub_graphs import PlannedCsr

# k_gat_in_chunks: one wave per chunk, chunk_grid() caps the grid at 1024 workgroups of
# kBlock / kWave = 4 waves (csrc/gat_input.hip:918-921; the loop: gat_input.hip:855)
CHUNK_ROUND = 1024 * 4
# k_gat_in_prep: 16 lanes per row, kBlock / 16 = 16 rows per workgroup, at most 4096 workgroups
# (csrc/gat_input.hip:932-933; the loop: gat_input.hip:130)
PREP_ROUND = 4096 * 16
# k_gat_in_q: 8 lanes per row, kBlock / 8 = 32 rows per workgroup, at most 8192 workgroups
# (csrc/gat_input.hip:948-949; the loop: gat_input.hip:768)
Q_ROUND = 8192 * 32
# k_rows: one (row, vector) pair per thread, at most 256 * 16 workgroups of kBlock = 256 threads
# (csrc/spmm.hip:1231-1232; the loop: spmm.hip:1202)
ROWS_ROUND = 256 * 16 * 256
# k_ffn_fwd: 4 row tiles of 32 rows per workgroup, at most 256 * 4 workgroups
# (csrc/dense.hip:618-620; the loop: dense.hip:298)
FFN_ROUND = 256 * 4 * 4 * 32
# k_tn_skinny: U = 4 block steps of RPB = (64 / KL) * 4 rows per pass of the rb loop
# (csrc/dense.hip:355-357; the loop: dense.hip:366)
SKINNY_U = 4
# k_tn_lds: rows per LDS stage, 32 at BM = 128 (WT 2) and 16 at BM = 192 (WT 3)
# (csrc/dense.hip:148; the loop: dense.hip:212); two buffers, so stage 2 reuses buffer 0
LDS_STAGE = {2: 32, 3: 16}


def skinny_kl(K: int) -> int:
    """Lanes per row of k_tn_skinny: the smallest power of two covering K, 8..64
    (csrc/dense.hip:562-575)."""
    kl = 1
    while kl < K and kl < 64:
        kl <<= 1
    return max(kl, 8)


def dense_grad_plan(N: int, K: int, M: int, vec4: bool) -> dict:
    """plan_for's arithmetic (csrc/dense.hip:466-498): the kernel family a dense-gradient shape
    takes, its rows per chunk and the passes of that kernel's row loop over a full chunk."""
    skinny = M <= 4 and K <= 256
    staged = (not skinny) and vec4 and M > 64 and K > 64
    wt = 0
    if staged:
        m128, m192 = -(-M // 128) * 128, -(-M // 192) * 192
        wt = 3 if m192 < m128 else 2
        n_tg = -(-K // 128) * -(-M // (64 * wt))
        target, align = -(-512 // n_tg), 32
    elif skinny:
        n_tg, target, align = 1, 1024, 64
    else:
        wm, wk = (2 if M > 32 else 1), (2 if K > 32 else 1)
        n_tg = -(-K // (32 * wk)) * -(-M // (32 * wm))
        target, align = -(-8192 // n_tg), 16
    rpc = max(-(-(-(-N // target)) // align) * align, align)
    P = max(-(-N // rpc), 1)
    if skinny:
        step = SKINNY_U * (64 // skinny_kl(K)) * 4
        kernel = "skinny"
    elif staged:
        step = LDS_STAGE[wt]
        kernel = f"lds{wt}"
    else:
        step = 2 * (4 if wm * wk < 4 else 8)      # kStep * in_flight (dense.hip:25-30, 90)
        kernel = "mfma"
    return dict(kernel=kernel, rows_per_chunk=rpc, P=P, step=step, passes=-(-rpc // step),
                ragged=rpc % step != 0, n_tg=n_tg)


# ---- hub chunks past one round per wave (k_gat_in_chunks) -----------------------------------
ROUND_PLAN = (64, 64)                      # (threshold, chunk)
ROUND_LEN = (1, 15, 16, 17, 63, 64)        # edges of a chunk: 64 a full chunk, the others a row's tail
ROUND_HUB_STRIDE = 5                       # hub row j is row 5 j + 2
ROUND_CHUNKS = 2 * CHUNK_ROUND + 1100      # the plan's size, about: three rounds for the first 1100 wave slots


def round_hub_degrees(rng) -> np.ndarray:
    """The hub rows' degrees in plan order (ascending row).  Every degree is 64 k + t with t in
    ROUND_LEN, so a row is k full chunks and a tail of t edges (t = 64: k + 1 full chunks).
    Rows 0..2047 have two chunks each (chunks 0..4095: chunk 2 i full, chunk 2 i + 1 the tail
    ROUND_LEN[i % 6]); rows 2048..2083 likewise with the tail ROUND_LEN[(i // 6) % 6], so chunk
    2 i + 1 -> chunk 2 i + 1 + 4096 is every ordered pair of lengths (the pairs with a full
    chunk through the 128-edge rows).  The rows after them have 2..6 chunks, drawn, until the
    plan has ROUND_CHUNKS chunks: the second and third round take a row's chunks at any
    position."""
    S = ROUND_LEN
    deg = [64 + S[i % 6] for i in range(CHUNK_ROUND // 2)]
    deg += [64 + S[(i // 6) % 6] for i in range(36)]
    chunks = 2 * len(deg)
    while chunks < ROUND_CHUNKS:
        k, t = int(rng.integers(1, 6)), S[int(rng.integers(0, 6))]
        deg.append(64 * k + t)
        chunks += k + 1
    return np.asarray(deg, np.int64)


def round_hub_graph(symmetric: bool, seed=29) -> layout.HostGraph:
    """About 3 400 hub rows of 65..384 edges under the plan (64, 64) -- more than 2 * 4096
    chunks, so waves 0..3 of the first workgroups of k_gat_in_chunks live through three chunks
    -- between ordinary rows of 0..6 edges and two blocks of empty rows; hub row j is row
    5 j + 2.  Directed: columns drawn uniformly, duplicates kept (the transposed pattern then
    has no long rows to speak of; the backward's pre-pass walks this graph as the transposed
    pattern of its transpose).  Symmetric: the same degrees kept exactly by stub pairing (as
    _graphs.phase_graph), empty rows isolated.  check_round_hub_graph asserts what the tests
    rely on."""
    rng = np.random.default_rng(seed)
    hub = round_hub_degrees(rng)
    n = ROUND_HUB_STRIDE * len(hub) + 57
    deg = rng.integers(0, 7, n)
    deg[1000:1040] = 0
    deg[n - 45:n - 5] = 0
    deg[ROUND_HUB_STRIDE * np.arange(len(hub)) + 2] = hub
    if not symmetric:
        src = np.repeat(np.arange(n), deg)
        dst = rng.integers(0, n, src.shape[0])
    else:
        if deg.sum() % 2:
            deg[5] += 1                                  # (a small ordinary row)
        stubs = rng.permutation(np.repeat(np.arange(n), deg))
        u, v = stubs[0::2], stubs[1::2]
        src, dst = np.concatenate([u, v]), np.concatenate([v, u])
        o = np.lexsort((dst, src))
        src, dst = src[o], dst[o]
    return layout.csr_build(n, n, src.astype(np.int32), dst.astype(np.int32))


def chunk_table(g: layout.HostGraph, plan=ROUND_PLAN):
    """Per chunk of g's plan, from the plan's own arrays (gala_host_split_plan): the row, the
    edge count and the position in its row (0 first, 1 middle, 2 last)."""
    thr, chunk = plan
    A = PlannedCsr(g, thr, chunk)
    deg = np.diff(g.rowptr.astype(np.int64))
    ri = A.crow[:A.n_chunks].astype(np.int64)
    row = A.rows[ri].astype(np.int64)
    k = np.arange(A.n_chunks) - A.rc0[ri]
    nck = (A.rc0[1:] - A.rc0[:-1])[ri]
    length = np.minimum(chunk, deg[row] - k * chunk)
    pos = np.where(k == 0, 0, np.where(k == nck - 1, 2, 1))
    return A, row, length, pos


def check_round_hub_graph(g: layout.HostGraph, symmetric: bool):
    """What the tests of the chunk pre-pass past one round rely on.  Wave slot s of
    k_gat_in_chunks sums chunks s, s + 4096, s + 8192; while it sums chunk c it requests chunk
    c + 4096's bounds, column window, side values and first batch.  Asserted of the hand-offs
    c -> c + 4096: every ordered pair of the chunk lengths {1, 15, 16, 17, 63, 64}; every
    ordered pair of positions in the row (first, middle, last); a chunk in the third round; a
    chunk whose slot hands off to nothing (every chunk of the last round, and the second-round
    chunks of the slots past it); a slot without a chunk in the last round.
    Not asserted: a hand-off inside one row.  It needs a row of more than 4096 chunks (262 145
    edges, half of the edge budget of these graphs in one row); the hub rows here have 65..384
    edges, at most 6 chunks, so every hand-off goes to another row -- which is asserted."""
    R = CHUNK_ROUND
    thr, chunk = ROUND_PLAN
    deg = np.diff(g.rowptr.astype(np.int64))
    A, row, length, pos = chunk_table(g)
    nc = A.n_chunks
    assert 2 * R < nc < 3 * R, nc                        # a third round, and slots without one
    assert nc == int(sum(-(-d // chunk) for d in deg[deg > thr])) and A.n_rows_split == int((deg > thr).sum())
    hubs = np.flatnonzero(deg > thr)
    assert np.array_equal(hubs, ROUND_HUB_STRIDE * np.arange(len(hubs)) + 2)
    assert deg[hubs].min() == 65 and deg[hubs].max() <= 400 and deg[deg <= thr].max() <= 7
    assert set(np.unique(length).tolist()) == set(ROUND_LEN)
    pairs = set(zip(length[:nc - R].tolist(), length[R:].tolist()))
    missing = [(a, b) for a in ROUND_LEN for b in ROUND_LEN if (a, b) not in pairs]
    assert not missing, f"chunk length hand-offs missing: {missing}"
    third = set(zip(length[R:nc - R].tolist(), length[2 * R:].tolist()))
    assert len(third) >= 12, third                       # second -> third round hand-offs differ
    ppairs = set(zip(pos[:nc - R].tolist(), pos[R:].tolist()))
    assert ppairs == {(a, b) for a in range(3) for b in range(3)}, ppairs
    assert (row[:nc - R] != row[R:]).all()               # (no hand-off inside a row: see above)
    assert (pos[2 * R:] == 1).any() and (pos[nc - R:2 * R] == 1).any()
    # the T-mode workspace stays near 100 MB, the graph small enough for the oracle
    ws = nc * int(_abi.lib().gala_gat_in_split_ws_cols(_abi.GALA_GAT_IN_WS_FWD_T)) * 4
    assert ws < 110e6 and g.nnz < 600_000, (ws, g.nnz)
    assert (deg == 0).sum() >= 80
    gT, _ = layout.transpose(g)
    same = np.array_equal(gT.rowptr, g.rowptr) and np.array_equal(gT.col, g.col)
    assert same == symmetric
    if symmetric:
        assert not np.isin(g.col, np.flatnonzero(deg == 0)).any()
    return nc


# ---- k_gat_in_prep and k_gat_in_q past one round ---------------------------------------------
PREP_Q_N = Q_ROUND + 77
# hub rows under ROUND_PLAN on both sides of row Q_ROUND (and of PREP_ROUND): row -> edges
PREP_Q_HUBS = {900: 65, PREP_ROUND + 3: 129, 200_000: 200, Q_ROUND - 100: 81, Q_ROUND + 50: 128, PREP_Q_N - 3: 191}


def prep_q_graph(seed=37) -> layout.HostGraph:
    """262 221 rows: five rounds of k_gat_in_prep (65 536 rows each), two of k_gat_in_q
    (262 144).  Degrees 0..3, a block of empty rows straddling row 262 144, the hub rows
    PREP_Q_HUBS (plan (64, 64)) in both rounds of k_gat_in_q.  Directed, columns uniform."""
    rng = np.random.default_rng(seed)
    n = PREP_Q_N
    deg = rng.integers(0, 4, n)
    deg[Q_ROUND - 40:Q_ROUND + 40] = 0
    for r, d in PREP_Q_HUBS.items():
        deg[r] = d
    src = np.repeat(np.arange(n), deg)
    dst = rng.integers(0, n, src.shape[0])
    return layout.csr_build(n, n, src.astype(np.int32), dst.astype(np.int32))


def check_prep_q_graph(g: layout.HostGraph):
    n = g.n_rows
    deg = np.diff(g.rowptr.astype(np.int64))
    assert n == PREP_Q_N and 4 * PREP_ROUND < n <= 5 * PREP_ROUND and Q_ROUND < n <= 2 * Q_ROUND
    hubs = np.flatnonzero(deg > ROUND_PLAN[0])
    assert sorted(PREP_Q_HUBS) == hubs.tolist() and all(deg[r] == d for r, d in PREP_Q_HUBS.items())
    assert (hubs < Q_ROUND).sum() >= 2 and (hubs >= Q_ROUND).sum() >= 2
    assert (deg[Q_ROUND - 40:Q_ROUND + 40] == 0).all() and deg[deg <= 64].max() == 3
    for lo in (0, Q_ROUND):                              # every degree class in both rounds of q
        assert set(np.unique(deg[lo:lo + Q_ROUND][deg[lo:lo + Q_ROUND] <= 3]).tolist()) == {0, 1, 2, 3}
