"""The bf16 SpMM tests' graph with prescribed hub rows (tests/_bf16_graphs.py): what the GPU tests
rely on, and the host twin (gala_cpu_spmm_ex_f32 on bf16 X) against the oracle's CSR-order fp32
sums on it -- widening bf16 is exact, so the two are equal bit for bit, with and without the plan.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _bf16_graphs as B
import oracle as orc
from gala import _abi
from gala.backend import CpuGraph
from _graphs import to_oracle


@functools.lru_cache(None)
def graph():
    return B.bf16_hub_graph()


def test_graph_has_the_prescribed_hub_rows():
    check = B.check_bf16_hub_graph
    check(graph())
    assert np.array_equal(B.bf16_hub_graph().col, graph().col), "the graph is a function of its seed"


def test_mirrored_dispatch_arithmetic():
    """The shapes the issue of these tests names, by hand."""
    assert [B.hub_tile(xv, 32) for xv in (8, 4, 2, 1)] == [512, 512, 256, 128]
    assert [B.hub_tile(xv, 64) for xv in (8, 4, 2, 1)] == [256, 256, 128, 64]
    assert [B.rows_shape(F, 8) for F in (8, 16, 32, 64, 128, 256, 512, 1024, 1032, 2048)] == \
        [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (32, 2), (64, 2), (64, 4), (64, 4)]
    # 2-byte aligned base -> scalar loads; 4-byte -> pairs; contiguous rows of 8 k -> 16-byte loads
    assert B.pick_vec(True, 1, 266, 0, 264, None, 264, 264, True) == 1
    assert B.pick_vec(True, 0, 514, 0, 514, None, 514, 514, True) == 2
    assert B.pick_vec(True, 0, 2056, 0, 2056, None, 2056, 2056, True) == 8
    assert B.pick_vec(True, 0, 2048, 0, 2048, None, 2042, 2042, True) == 8      # padded rows, one head
    assert B.pick_vec(True, 0, 2048, 0, 2048, None, 2044, 1022, False) == 2     # not with several heads
    assert B.pick_vec(False, 0, 265, 0, 264, (0, 264, True), 264, 264, True) == 1
    d = B.dispatch(True, 1, 264, 4, True)                                       # head_dim 66: column 256 is head 3's
    assert [r["F"] for r in d] == [256, 8] and [r["rows"] for r in d] == [(64, 4), (8, 1)]
    assert d[0]["hub"] == (64, 64, (1, 2, 2, 2)) and d[1]["hub"] == (32, 128, (1,))
    assert [r["F"] for r in B.dispatch(True, 1, 513, 0, True)] == [256, 256, 1]
    assert all(r["hub"] is None for r in B.dispatch(True, 4, 32, 8, True))      # 8 heads in one slice
    assert all(r["hub"] is None for r in B.dispatch(False, 1, 264, 4, True))    # fp32 X past one range, 4 heads
    assert B.dispatch(False, 1, 264, 1, True)[1]["hub"] == (32, None, (1,))


def cpu_spmm(g, X, src=None, dst=None):
    P = lambda t: None if t is None else t.data_ptr()
    Y = torch.empty(g.n_rows, X.shape[1])
    _abi.call_cpu("gala_spmm_ex_f32", g.csr(), P(X), X.stride(0), P(Y), Y.stride(0), X.shape[1], P(src), P(dst),
                  _abi.spmm_storage_flags(X), 0, 5, 7, None, None)
    return Y.numpy()


@pytest.mark.parametrize("plan", [True, False], ids=["plan", "noplan"])
@pytest.mark.parametrize("F,heads", [(47, 0), (264, 4)], ids=["plain47", "weighted264h4"])
def test_host_twin_equals_the_oracle(F, heads, plan):
    hg = graph()
    g = CpuGraph(hg)
    if plan:
        g.set_split_plan(B.PLAN["threshold"], B.PLAN["chunk"])
        assert g.c.split and g._plan.n_rows_split == len(B.HUB_DEGREES)
    gen = torch.Generator().manual_seed(F)
    Xb = torch.randn(hg.n_cols, F, generator=gen).to(torch.bfloat16)
    src, dst = torch.rand(hg.n_cols, generator=gen) + 0.5, torch.rand(hg.n_rows, generator=gen) + 0.5
    val = rs = None
    if heads:
        val, rs = torch.randn(hg.nnz, heads, generator=gen), torch.rand(hg.n_rows, heads, generator=gen) + 0.5
        g.c.val, g.c.val_heads, g.c.val_row_scale = val.data_ptr(), heads, rs.data_ptr()
    got = cpu_spmm(g, Xb, src, dst)
    eff = None
    if heads:       # the factored weight is the rounded fp32 product val * row_scale
        eff = (val * rs[np.repeat(np.arange(hg.n_rows), np.diff(hg.rowptr))]).numpy().ravel()
    want = orc.spmm(to_oracle(hg, eff, max(heads, 1)), Xb.float().numpy(), src_scale=src.numpy(), dst_scale=dst.numpy())
    np.testing.assert_array_equal(got, want)
    assert np.isfinite(got).all() and np.abs(got[B.hub_rows()]).max() > 1.0
