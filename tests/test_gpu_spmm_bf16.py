"""GPU: bf16 storage of the SpMM's gathered operand (GALA_SPMM_X_BF16 / GALA_SPMM_Y2_BF16).

Widening bf16 to fp32 is exact and the sums stay fp32 in CSR order, so ops.spmm on a bf16 X must
equal the fp32 kernels on X.float() bit for bit (those are pinned to the oracle by the rest of the
suite), on a plain graph (row kernel) and under a hub plan (the bf16 hub kernel on the side
stream).  Integer features with unit weights sum exactly: there the result equals float64.
"""
import functools

import numpy as np
import pytest
import torch

from gala import _abi, layout, ops
from _graphs import cora_like, powerlaw

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16


@functools.lru_cache(None)
def graph(name):
    """(host graph, device graph): cora without a plan; powerlaw under the plan (threshold 64,
    row order), whose hub rows run in the hub kernel."""
    if name == "cora":
        hg = cora_like()
        return hg, ops.DeviceGraph.from_host(hg, split=False)
    hg = powerlaw()
    dg = ops.DeviceGraph.from_host(hg, split=False)
    dg.set_split_plan(hg.rowptr, 64, chunk=32, row_order=True)
    assert dg.split_rows > 0
    return hg, dg


def rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def scale_args(dg, scales, F, dtype2=torch.float32):
    if scales == "src_dst":
        return dict(src_scale=rand(dg.n_cols, seed=1).abs() + 0.5, dst_scale=rand(dg.n_rows, seed=2).abs() + 0.5)
    if scales == "deg_out2":
        return dict(dst_deg=True, out2=torch.empty(dg.n_rows, F, device="cuda", dtype=dtype2))
    return {}


# F: scalar loads; 4-B loads; 8-B loads; one 64-B row; odd and row-padded to 48; past one chunk of a row group
@pytest.mark.parametrize("scales", ["none", "src_dst", "deg_out2"])
@pytest.mark.parametrize("F", [1, 6, 12, 32, 47, 264])
@pytest.mark.parametrize("name", ["cora", "powerlaw"])
def test_bf16_x_equals_the_fp32_path_on_the_widened_input(name, F, scales):
    _, dg = graph(name)
    Xb = rand(dg.n_cols, F, seed=F).to(bf16)
    got_kw, want_kw = scale_args(dg, scales, F), scale_args(dg, scales, F)
    got = ops.spmm(dg, ops.pad_rows(Xb, 8) if F == 47 else Xb, **got_kw)
    want = ops.spmm(dg, Xb.float(), **want_kw)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    if scales == "deg_out2":
        assert torch.equal(got_kw["out2"], want_kw["out2"])


@pytest.mark.parametrize("name", ["cora", "powerlaw"])
def test_weighted_heads_and_accum(name):
    _, dg = graph(name)
    Xb = rand(dg.n_cols, 32, seed=3).to(bf16)
    wg = dg.with_values(rand(dg.nnz, 4, seed=4), val_heads=4, row_scale=rand(dg.n_rows, 4, seed=5))
    assert torch.equal(ops.spmm(wg, Xb), ops.spmm(wg, Xb.float()))
    base = rand(dg.n_rows, 32, seed=6)
    got = ops.spmm(dg, Xb, out=base.clone(), accum=True)
    assert torch.equal(got, ops.spmm(dg, Xb.float(), out=base.clone(), accum=True))


@pytest.mark.parametrize("F", [32, 47])
@pytest.mark.parametrize("name", ["cora", "powerlaw"])
def test_integer_features_sum_exactly(name, F):
    hg, dg = graph(name)
    X = torch.randint(-128, 129, (hg.n_cols, F), generator=torch.Generator().manual_seed(1)).float()
    got = ops.spmm(dg, X.to(bf16).cuda()).cpu().numpy().astype(np.float64)
    # float64 row sums as differences of the running sum over the edges: integers, exact
    cs = np.concatenate([np.zeros((1, F)), np.cumsum(X.numpy().astype(np.float64)[hg.col], axis=0)])
    assert np.array_equal(got, cs[hg.rowptr[1:]] - cs[hg.rowptr[:-1]])


@pytest.mark.parametrize("name", ["cora", "powerlaw"])
def test_two_byte_aligned_slice_and_strided_out(name):
    _, dg = graph(name)
    Xs = rand(dg.n_cols, 40, seed=7).to(bf16)[:, 1:33]      # base 2-byte aligned, ldx = 40
    assert Xs.data_ptr() % 4 == 2 and Xs.stride(0) == 40
    buf = torch.full((dg.n_rows, 40), -7.0, device="cuda")
    ops.spmm(dg, Xs, out=buf[:, 3:35])
    assert torch.equal(buf[:, 3:35], ops.spmm(dg, Xs.float().contiguous()))
    assert (buf[:, :3] == -7.0).all() and (buf[:, 35:] == -7.0).all()


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("x_dtype", [torch.float32, bf16])
@pytest.mark.parametrize("name", ["cora", "powerlaw"])
def test_bf16_out2_is_the_fp32_out2_rounded_to_nearest_even(name, x_dtype, special):
    _, dg = graph(name)
    X = rand(dg.n_cols, 32, seed=8).to(bf16)
    if special:
        X[3, :8], X[3, 8:16], X[3, 16:24] = float("inf"), float("-inf"), float("nan")
    X = X.to(x_dtype)
    o16, o32 = scale_args(dg, "deg_out2", 32, bf16), scale_args(dg, "deg_out2", 32)
    assert torch.equal(ops.spmm(dg, X, **o16).view(torch.int32), ops.spmm(dg, X, **o32).view(torch.int32))
    o16, o32 = o16["out2"], o32["out2"]
    num = ~o32.isnan()   # (torch's own conversions disagree on a NaN's sign and payload bits)
    assert torch.equal(o16.view(torch.int16)[num], o32.to(bf16).view(torch.int16)[num])
    assert torch.equal(o16.isnan(), o32.isnan()) and torch.equal(o16.isinf(), o32.isinf())
    assert bool(o32.isnan().any()) == special


@pytest.mark.parametrize("case", ["col_tiled", "sampled", "hub_chunked", "src_relu"])
def test_refused_before_any_launch(case):
    dg = graph("powerlaw")[1]
    if case == "col_tiled":
        dg = ops.DeviceGraph.from_host(layout.col_tile(cora_like(), 1000), split=False)
    kw = {"col_tiled": {}, "sampled": dict(nsamp=4), "hub_chunked": dict(hub="chunked"), "src_relu": dict(src_relu=True)}
    out = torch.full((dg.n_rows, 32), -7.0, device="cuda")
    with pytest.raises(_abi.GalaError) as e:
        ops.spmm(dg, rand(dg.n_cols, 32).to(bf16), out=out, **kw[case])
    assert e.value.status == _abi.GALA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == -7.0).all()


def test_mirror_call_takes_bf16_features():
    import gala
    E = gala.torch_ext()
    hg = cora_like()
    off, cols = torch.from_numpy(hg.rowptr).cuda(), torch.from_numpy(hg.col).cuda()
    vals = torch.ones(hg.nnz, device="cuda")
    Xb = rand(hg.n_cols, 32, seed=9).to(bf16)
    got = E.aggregate_node_mul_sum_call(Xb, off, cols, vals, None, 1)
    assert got.dtype == torch.float32
    assert torch.equal(got, E.aggregate_node_mul_sum_call(Xb.float(), off, cols, vals, None, 1))
