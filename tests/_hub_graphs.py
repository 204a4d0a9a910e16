"""Graphs and plans of the input-space GAT layer's hub-row tests (gala_gat_in_* on graphs whose
split plan has hub rows: tests/test_gat_input_hub_cpu.py, tests/test_gpu_gat_input_hub.py)."""
from __future__ import annotations

import ctypes

import numpy as np

from gala import _abi, layout
from _graphs import PHASE_N, PHASE_STEP

# (threshold, chunk): the tests' small plan and the default one (DeviceGraph.from_host)
PLANS = ((64, 64), (1024, 512))

# Prescribed rows of hub_sym_graph.  With the identity order row r hands off to row r + 4096
# (8 rows per phase on a grid of 512 workgroups), so under both plans there is a hand-off
# hub -> hub, hub -> ordinary, ordinary -> hub and hub -> empty row, a hub row in the third
# phase (rows >= 8192) and one in a slot that hands off to no row (rows 4109..4111).
HUB_SYM_ROWS = {
    # hubs under both plans
    100: 2600, 4196: 1025,          # hub -> hub (2600 edges: 41 chunks of 64, more than a workgroup's 8 waves)
    300: 1537, 4396: 5,             # hub -> ordinary
    400: 7, 4496: 2049,             # ordinary -> hub
    500: 1025, 4596: 0,             # hub -> empty
    3: 4, 4099: 3, 8195: 1025,      # ordinary -> ordinary -> hub in the third phase
    4110: 1537,                     # hands off to no row
    # hubs under (64, 64) only
    200: 65, 4296: 128,             # hub -> hub
    600: 129, 4696: 0,              # hub -> empty
    700: 6, 4796: 65,               # ordinary -> hub
    800: 128, 4896: 4,              # hub -> ordinary
    8: 2, 4104: 65, 8200: 129,      # ordinary -> hub -> hub in the third phase
    4111: 128,                      # hands off to no row
}
HUB_SYM_PLAN_SIZES = {(64, 64): (15, 193), (1024, 512): (7, 28)}   # (n_rows_split, n_chunks)


def plan_sizes(g: layout.HostGraph, threshold: int, chunk: int):
    nr, nc = ctypes.c_int64(0), ctypes.c_int64(0)
    _abi.call("gala_host_split_plan", g.n_rows, g.rowptr.ctypes.data, threshold, chunk, None, None, None,
              ctypes.byref(nr), ctypes.byref(nc))
    return nr.value, nc.value


def hub_sym_graph(seed=23) -> layout.HostGraph:
    """8205 rows, symmetric, degrees kept exactly by stub pairing (as _graphs.phase_graph): the
    rows of HUB_SYM_ROWS, blocks of empty rows, every other row 0..12 edges.  Row r repeated
    deg[r] times, the list shuffled, consecutive entries (u, v) joined as u -> v and v -> u (a
    loop stored twice): empty rows are isolated.  check_hub_sym_graph asserts what the tests
    rely on."""
    rng = np.random.default_rng(seed)
    n = PHASE_N
    deg = rng.integers(0, 13, n)
    deg[3000:3050] = 0
    deg[7000:7050] = 0
    for r, d in HUB_SYM_ROWS.items():
        deg[r] = d
    if deg.sum() % 2:
        deg[5] += 1                                      # (a small random row)
    stubs = rng.permutation(np.repeat(np.arange(n), deg))
    u, v = stubs[0::2], stubs[1::2]
    src, dst = np.concatenate([u, v]), np.concatenate([v, u])
    o = np.lexsort((dst, src))
    return layout.csr_build(n, n, src[o].astype(np.int32), dst[o].astype(np.int32))


def handoff_kinds(deg, threshold):
    kind = np.where(deg > threshold, 2, np.where(deg == 0, 0, 1))   # 2 hub, 1 ordinary, 0 empty
    n = deg.shape[0]
    return set(zip(kind[:n - PHASE_STEP].tolist(), kind[PHASE_STEP:].tolist()))


def check_hub_sym_graph(g: layout.HostGraph):
    n, step = g.n_rows, PHASE_STEP
    deg = np.diff(g.rowptr.astype(np.int64))
    assert n == PHASE_N and (n + 7) // 8 == 1026 and n > 2 * step
    for r, d in HUB_SYM_ROWS.items():
        assert deg[r] == d, (r, deg[r], d)
    others = np.setdiff1d(np.arange(n), list(HUB_SYM_ROWS))
    assert deg[others].max() <= 13 and (deg[3000:3050] == 0).all() and (deg[7000:7050] == 0).all()
    for thr, chunk in PLANS:
        kinds = handoff_kinds(deg, thr)
        for pair in ((2, 2), (2, 1), (1, 2), (2, 0)):
            assert pair in kinds, (thr, pair)
        assert (deg[2 * step:] > thr).any(), "a hub row in the third phase"
        assert (deg[4109:4112] > thr).any(), "a hub row handing off to no row"
        assert plan_sizes(g, thr, chunk) == HUB_SYM_PLAN_SIZES[(thr, chunk)]
    assert -(-deg.max() // 64) == 41 > 8
    assert layout.split_threshold(n, g.nnz) == 1024 and g.nnz < 150_000
    gT, _ = layout.transpose(g)
    assert np.array_equal(gT.rowptr, g.rowptr) and np.array_equal(gT.col, g.col)
    assert not np.isin(g.col, np.flatnonzero(deg == 0)).any()


class PlannedCsr:
    """gala_csr_t over a host graph's numpy arrays with a hub-row plan (threshold, chunk): host
    index arrays and no workspace (the host twins need none)."""

    def __init__(self, g: layout.HostGraph, threshold: int, chunk: int):
        self.g = g
        nr, nc = plan_sizes(g, threshold, chunk)
        self.rows, self.rc0 = np.zeros(max(nr, 1), np.int32), np.zeros(nr + 1, np.int32)
        self.crow = np.zeros(max(nc, 1), np.int32)
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        if nr:
            _abi.call("gala_host_split_plan", g.n_rows, g.rowptr.ctypes.data, threshold, chunk, self.rows.ctypes.data,
                      self.rc0.ctypes.data, self.crow.ctypes.data, ctypes.byref(a), ctypes.byref(b))
        plan = _abi.gala_split_plan_t()
        plan.threshold, plan.chunk, plan.n_rows_split, plan.n_chunks = threshold, chunk, nr, nc
        plan.rows, plan.row_chunk0, plan.chunk_row = self.rows.ctypes.data, self.rc0.ctypes.data, self.crow.ctypes.data
        plan.workspace, plan.ws_cols = None, 0
        plan.row_order = None
        self.plan = plan
        c = _abi.gala_csr_t()
        c.n_rows, c.n_cols, c.nnz = g.n_rows, g.n_cols, g.nnz
        c.rowptr, c.col, c.val = g.rowptr.ctypes.data, g.col.ctypes.data, None
        c.val_heads, c.n_seg, c.seg_bounds = 1, 1, None
        c.split = ctypes.addressof(plan)
        self.c = c
        self.n_rows_split, self.n_chunks = nr, nc

    @property
    def ref(self):
        return ctypes.byref(self.c)
