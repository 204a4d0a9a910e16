"""TEST INFRASTRUCTURE: the graph and the mirrored dispatch arithmetic of the bf16 SpMM's tests
(tests/test_bf16_graphs_cpu.py, tests/test_gpu_spmm_bf16_dispatch.py).

bf16_hub_graph() has one hub row of every degree in HUB_DEGREES, chosen so that under the plan
PLAN every tile size of k_spmm_bf16_hub meets rows of 1 .. 5 and more tiles, last tiles of 1,
T - 1 and T edges and every remainder class of the chain's rotation; check_bf16_hub_graph asserts
that.  The constants and functions below mirror the launch code (file:line beside each, paths
under gala-gnn-acceleration-language_amd/); a test asserts the branch it expects from them, so a
changed threshold fails that assertion instead of silently moving the case to another branch.
"""
from __future__ import annotations

import numpy as np

from gala import layout

PLAN = dict(threshold=64, chunk=32, row_order=True)     # tests/test_gpu_spmm_bf16.py's plan
N = 3000
EMPTY_BLOCKS = ((1000, 1040), (2500, 2560))
HUB_DEGREES = (65, 96, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 384, 385, 511, 512, 513, 768, 769, 1024,
               1025, 1537, 2049, 2600)
HUB_ROW0, HUB_STRIDE = 37, 127                          # hub row k is row 37 + 127 k

# ---- csrc/spmm_bf16.hip, csrc/spmm_bf16.h, csrc/spmm.hip ------------------------------------------
MAX_VECS = 256        # kBf16MaxVecs: vectors of a row per launch (csrc/spmm_bf16.h:44)
HUB_BUF_DW = 8192     # kHubBufDw: dwords of X per LDS buffer (csrc/spmm_bf16.hip:283)
HUB_HEADS = 4         # kHubHeads = kHubMaxHeads: edge-weight heads per slice (spmm_bf16.hip:284, spmm.hip:483)
GROUP = 16            # HubLdsB::kGroup: edges per chain group (spmm_bf16.hip:294)
ROTATION = 3 * GROUP  # three groups in rotation (spmm_bf16.hip:432)
TILES = (64, 128, 256, 512)


def hub_fsp(F: int) -> int:
    """Features per hub slice (spmm_bf16.hip:583; spmm.hip:920 for the dispatch's head count)."""
    return 32 if F <= 32 else 64


def hub_tile(xv: int, fsp: int) -> int:
    """HubLdsB::T, edges per tile (spmm_bf16.hip:290)."""
    return 2 * HUB_BUF_DW // fsp // (1 if xv >= 4 else 2 if xv == 2 else 4)


def pick_vec(x_bf16, xoff, ldx, yoff, ldy, y2, F, head_dim, one_head) -> int:
    """bf16_pick_vec (spmm_bf16.hip:600-616) on operands whose allocations are aligned to 16 bytes
    or more: xoff / yoff are the views' first elements, y2 is None or (offset, ld, is_bf16)."""
    def ok(v):
        yv = min(v, 4)
        Fv = -(-F // v) * v
        padded = one_head and ldx >= Fv and ldy >= Fv and (y2 is None or y2[1] >= Fv)
        fits = (F % v == 0 and head_dim % v == 0) or padded
        x_ok = ldx % v == 0 and xoff % v == 0
        y_ok = ldy % yv == 0 and yoff % yv == 0
        y2_ok = y2 is None or (y2[1] % v == 0 and y2[0] % v == 0 if y2[2] else y2[1] % yv == 0 and y2[0] % yv == 0)
        return fits and x_ok and y_ok and y2_ok
    v = 8 if x_bf16 else 4
    while v > 1 and not ok(v):
        v >>= 1
    return v


def rows_shape(F: int, xv: int):
    """(G, CH) of k_spmm_bf16_rows for a launch of F columns (spmm_bf16.hip:535-546)."""
    L = -(-F // xv)
    for top, shape in ((1, (1, 1)), (2, (2, 1)), (4, (4, 1)), (8, (8, 1)), (16, (16, 1)), (32, (32, 1)), (64, (32, 2)),
                       (128, (64, 2)), (MAX_VECS, (64, 4))):
        if L <= top:
            return shape
    raise AssertionError(f"{L} vectors: the dispatch cuts wider rows into column ranges")


def dispatch(x_bf16, xv, F, heads, has_hubs):
    """spmm_bf16()'s launches (spmm.hip:915-926, 964-970): per column range its width, the row
    kernel's (G, CH), and the hub launch's (FSP, T, heads per slice of every slice) -- T is None
    for fp32 X, whose hub rows take k_spmm_hub_exact and k_spmm_bf16_hub_y2 -- or hub None where
    the hub rows stay in the row kernel.  heads: 0 without edge weights."""
    max_cols = MAX_VECS * xv
    head_dim = F // heads if heads else F
    use_hub = has_hubs
    if heads > 1:
        fsp = hub_fsp(F)
        for f0 in range(0, F, fsp):
            f1 = min(f0 + fsp, F) - 1
            if f1 // head_dim - f0 // head_dim + 1 > HUB_HEADS:
                use_hub = False
        if not x_bf16 and F > max_cols:
            use_hub = False
    out = []
    for c0 in range(0, F, max_cols):
        qF = min(F - c0, max_cols)
        hub = None
        if use_hub:
            fsp = hub_fsp(qF)
            hps = tuple((c0 + min(f0 + fsp, qF) - 1) // head_dim - (c0 + f0) // head_dim + 1 for f0 in range(0, qF, fsp))
            hub = (fsp, hub_tile(xv, fsp) if x_bf16 else None, hps if heads else ())
        out.append(dict(F=qF, rows=rows_shape(qF, xv), hub=hub))
    return out


# ---- the graph -----------------------------------------------------------------------------------

def hub_rows() -> np.ndarray:
    return HUB_ROW0 + HUB_STRIDE * np.arange(len(HUB_DEGREES))


def bf16_hub_graph(seed=31) -> layout.HostGraph:
    """3000 rows, directed, square: ordinary rows of 0 .. 12 edges, two blocks of empty rows, one hub
    row of every degree in HUB_DEGREES; uniform columns, duplicates kept."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 13, N)
    for a, b in EMPTY_BLOCKS:
        deg[a:b] = 0
    deg[hub_rows()] = HUB_DEGREES
    src = np.repeat(np.arange(N, dtype=np.int32), deg)
    dst = rng.integers(0, N, src.shape[0]).astype(np.int32)
    return layout.csr_build(N, N, src, dst)


def tile_facts(deg, T):
    """Per hub row (tiles, edges of the last tile) at tile size T (spmm_bf16.hip:318, 408)."""
    nt = -(-deg // T)
    return nt, deg - (nt - 1) * T


def check_bf16_hub_graph(g: layout.HostGraph):
    deg = np.diff(g.rowptr.astype(np.int64))
    assert g.n_rows == g.n_cols == N and g.nnz < 60_000
    rows = hub_rows()
    assert rows.max() < N and not any(((rows >= a) & (rows < b)).any() for a, b in EMPTY_BLOCKS)
    assert np.array_equal(deg[rows], HUB_DEGREES)
    others = np.setdiff1d(np.arange(N), rows)
    assert deg[others].max() == 12 and deg[others].min() == 0
    assert all((deg[a:b] == 0).all() for a, b in EMPTY_BLOCKS)
    hubs = deg[deg > PLAN["threshold"]]
    assert np.array_equal(np.sort(hubs), HUB_DEGREES), "the hub rows are exactly the prescribed ones"
    assert (np.diff(np.sort(g.col[g.rowptr[rows[-1]]:g.rowptr[rows[-1] + 1]])) == 0).any(), "duplicates kept"
    assert {hub_tile(xv, fsp) for xv in (8, 4, 2, 1) for fsp in (32, 64)} == set(TILES)
    for T in TILES:
        nt, cnt = tile_facts(hubs, T)
        for want in (2, 3, 4) + ((1,) if T >= 128 else ()):
            assert (nt == want).any(), (T, want)
        assert (nt >= 5).any(), T                           # the steady state: columns loaded three tiles ahead
        for want in (1, T - 1, T):
            assert (cnt == want).any(), (T, want)           # the last tile's length
        assert (cnt // ROTATION == 0).any() and (cnt // ROTATION > 0).any(), T
        assert {0, 1, 15} <= set((cnt % GROUP).tolist()), T
        tail = cnt % GROUP                                  # the scalar tail: edge j takes the low half of its
        assert (tail == 1).any() and (tail >= 2).any(), T   # dword when j is even, the high half when odd
        assert (tail[tail > 0] % 2 == 0).any() and (tail % 2 == 1).any(), T
