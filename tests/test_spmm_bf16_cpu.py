"""bf16 storage of the SpMM's gathered operand on the host-CPU backend (GALA_SPMM_X_BF16 /
GALA_SPMM_Y2_BF16 of gala_cpu_spmm_ex_f32).

Widening bf16 to fp32 is exact and the sums stay fp32 in CSR order, so the call on bf16 X must
equal the fp32 call on X.float() bit for bit; integer features with unit weights make every sum
exact, so it must also equal a float64 gather exactly; a bf16 Y2 is the fp32 Y2 rounded to
nearest even (torch's conversion).
"""
import ctypes

import numpy as np
import pytest
import torch

from gala import _abi
from gala.backend import CpuGraph
from _graphs import cora_like, powerlaw

GRAPHS = {"cora": cora_like, "powerlaw": powerlaw}


def cpu_spmm(g, X, src=None, dst=None, dst_deg=False, out2=None):
    P = lambda t: None if t is None else t.data_ptr()
    Y = torch.empty(g.n_rows, X.shape[1])
    epi = _abi.gala_spmm_epilogue_t()
    epi.dst_deg_rsqrt = int(dst_deg)
    epi.Y2, epi.ldy2 = P(out2), (out2.stride(0) if out2 is not None else 0)
    _abi.call_cpu("gala_spmm_ex_f32", g.csr(), P(X), X.stride(0), P(Y), Y.stride(0), X.shape[1], P(src), P(dst),
                  _abi.spmm_storage_flags(X, out2), 0, 5, 7, ctypes.byref(epi), None)
    return Y


@pytest.mark.parametrize("scales", ["none", "src_dst", "deg_out2"])
@pytest.mark.parametrize("F", [1, 32, 47])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_bf16_x_equals_the_fp32_call_on_the_widened_input(graph, F, scales):
    g = CpuGraph(GRAPHS[graph]())
    gen = torch.Generator().manual_seed(F)
    Xb = torch.randn(g.n_cols, F, generator=gen).to(torch.bfloat16)
    kw = {}
    if scales == "src_dst":
        kw = dict(src=torch.rand(g.n_cols, generator=gen) + 0.5, dst=torch.rand(g.n_rows, generator=gen) + 0.5)
    outs = [torch.empty(g.n_rows, F) for _ in range(2)] if scales == "deg_out2" else [None, None]
    got = cpu_spmm(g, Xb, dst_deg=scales == "deg_out2", out2=outs[0], **kw)
    want = cpu_spmm(g, Xb.float(), dst_deg=scales == "deg_out2", out2=outs[1], **kw)
    assert torch.equal(got, want)
    if outs[0] is not None:
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("F", [32, 47])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_integer_features_sum_exactly(graph, F):
    hg = GRAPHS[graph]()
    X = torch.randint(-128, 129, (hg.n_cols, F), generator=torch.Generator().manual_seed(1)).float()
    got = cpu_spmm(CpuGraph(hg), X.to(torch.bfloat16))
    # float64 row sums as differences of the running sum over the edges: integers, exact
    cs = np.concatenate([np.zeros((1, F)), np.cumsum(X.numpy().astype(np.float64)[hg.col], axis=0)])
    want = cs[hg.rowptr[1:]] - cs[hg.rowptr[:-1]]
    assert np.array_equal(got.numpy().astype(np.float64), want)


@pytest.mark.parametrize("x_bf16", [False, True])
def test_bf16_out2_is_the_fp32_out2_rounded_to_nearest_even(x_bf16):
    g = CpuGraph(cora_like())
    X = torch.randn(g.n_cols, 47, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    X[3, 5], X[4, 6], X[5, 7] = float("inf"), float("-inf"), float("nan")
    X = X if x_bf16 else X.float()
    o16, o32 = torch.empty(g.n_rows, 47, dtype=torch.bfloat16), torch.empty(g.n_rows, 47)
    y16 = cpu_spmm(g, X, dst_deg=True, out2=o16)
    y32 = cpu_spmm(g, X, dst_deg=True, out2=o32)
    assert torch.equal(y16.view(torch.int32), y32.view(torch.int32))
    num = ~o32.isnan()   # (torch's own conversions disagree on a NaN's sign and payload bits)
    assert torch.equal(o16.view(torch.int16)[num], o32.to(torch.bfloat16).view(torch.int16)[num])
    assert torch.equal(o16.isnan(), o32.isnan()) and torch.equal(o16.isinf(), o32.isinf())
    assert o32.isnan().any() and o32.isinf().any()
