"""GPU: the row ops of csrc/spmm.hip (k_rows<VEC, Op>) past one round of their grid.

launch_rows caps the grid at 4096 workgroups of 256 threads; a thread then steps its (row,
vector) pair by 1 048 576 pairs incrementally (r += dr; c += dc; carry when c >= L).  The
shapes here have between two and three rounds of pairs and hit each stepping case: L = 1
(dc = 0), L = 47 (dc = 6), L = 12 with a padded last vector (nv = 3), L = 25 (dc = 1) and
L = 3 at VEC 2.  All four entry points -- row_broadcast, row_broadcast_deg, row_scale_relu,
relu_scale_backward -- against the references of the existing row-op tests
(tests/test_gpu_kernels.py): the torch chain bit for bit with the sign bit compared, the numpy
product, the oracle's degree^-0.5 times X.  -0, exact zeros and NaN sit in rows that only the
second and the third round reach; padding holds a sentinel and comes back unchanged.
"""
import numpy as np
import pytest
import torch

import oracle as orc
from gala import layout, ops
from _graphs import to_oracle
from _rounds import ROWS_ROUND

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 5.0

# name: (rows, F, row stride, float offset of the first element in its buffer, VEC, L)
CASES = {
    "L1": (2_200_000, 1, 1, 0, 1, 1),
    "L47": (50_000, 47, 47, 0, 1, 47),
    "L12_padded": (200_000, 47, 48, 0, 4, 12),
    "L25": (100_000, 100, 100, 0, 4, 25),
    "L3_vec2": (800_000, 6, 6, 2, 2, 3),
}


def rows_vec(F, lds, ptrs):
    """rows_vec of csrc/spmm.hip:1216-1225: the widest vector that divides every stride and
    base, with F a multiple of it or the rows padded to it."""
    for v in (4, 2):
        Fv = -(-F // v) * v
        if all(ld % v == 0 and (F % v == 0 or ld >= Fv) for ld in lds) and all(p % (4 * v) == 0 for p in ptrs):
            return v
    return 1


def placed(a, ld, off):
    """a [n, F] as a view with row stride ld, off floats into a buffer otherwise full of FILL."""
    n, F = a.shape
    buf = torch.full((off + n * ld + 4,), FILL, device=DEV)
    view = buf[off:off + n * ld].view(n, ld)[:, :F]
    view.copy_(torch.from_numpy(a).to(DEV))
    return buf, view


def untouched(buf, n, F, ld, off):
    """The buffer outside the view's [n, F] elements still holds FILL."""
    body = buf[off:off + n * ld].view(n, ld)
    return bool(torch.all(buf[:off] == FILL)) and bool(torch.all(buf[off + n * ld:] == FILL)) and \
        bool(torch.all(body[:, F:] == FILL))


def same_bits(got, want):
    return torch.equal(torch.nan_to_num(got, nan=123.0), torch.nan_to_num(want, nan=123.0)) and \
        torch.equal(torch.signbit(got), torch.signbit(want))


def case_inputs(name):
    n, F, ld, off, vec, L = CASES[name]
    assert L == -(-F // vec) and 2 * ROWS_ROUND < n * L < 3 * ROWS_ROUND      # threads run two and three rounds
    rng = np.random.default_rng(F + n)
    X = rng.uniform(-1, 1, (n, F)).astype(np.float32)
    X[::7, 0] = 0.0
    X[1::11, -1] = -0.0
    r2, r3 = -(-ROWS_ROUND // L) + 5, -(-2 * ROWS_ROUND // L) + 5             # rows of the second and third round
    assert r2 * L >= ROWS_ROUND and r3 * L >= 2 * ROWS_ROUND and r3 + 3 < n
    for r in (r2, r3):
        X[r, 0], X[r + 1, -1], X[r + 2, 0], X[r + 3, -1] = np.nan, -0.0, 0.0, np.nan
    G = rng.uniform(-1, 1, (n, F)).astype(np.float32)
    act = rng.uniform(0.1, 2, n).astype(np.float32)
    pre = rng.uniform(0.1, 2, n).astype(np.float32)
    act[r3 + 1] = -1.5                                                        # -0 * a negative factor: +0
    return X, G, act, pre


def check_vec(vec, F, *views):
    assert rows_vec(F, [v.stride(0) for v in views], [v.data_ptr() for v in views]) == vec


@pytest.mark.parametrize("name", list(CASES))
def test_row_scale_relu_and_backward_past_one_round(name):
    """pre * relu(act * X) and its backward against the torch ops they replace, bit for bit,
    with every combination of the optional factors."""
    n, F, ld, off, vec, L = CASES[name]
    X, G, act, pre = case_inputs(name)
    xb, Xd = placed(X, ld, off)
    gb, Gd = placed(G, ld, off)
    a, p = torch.from_numpy(act).to(DEV), torch.from_numpy(pre).to(DEV)
    for A, Pf in ((a, p), (None, p), (a, None), (None, None)):
        ob, out = placed(np.zeros((n, F), np.float32), ld, off)
        check_vec(vec, F, Xd, out)
        t = Xd if A is None else A[:, None] * Xd
        want = torch.relu(t) if Pf is None else Pf[:, None] * torch.relu(t)
        assert ops.row_scale_relu(Xd, A, Pf, out=out) is out
        assert same_bits(out, want)
        assert untouched(ob, n, F, ld, off)
        db, dX = placed(np.zeros((n, F), np.float32), ld, off)
        check_vec(vec, F, Xd, Gd, dX)
        dt = torch.where(torch.relu(t) <= 0, torch.zeros_like(Gd), Gd)
        want_dx = dt if A is None else dt * A[:, None]
        ops.relu_scale_backward(Xd, Gd, A, out=dX)
        assert same_bits(dX, want_dx)
        assert untouched(db, n, F, ld, off)
    assert untouched(xb, n, F, ld, off) and untouched(gb, n, F, ld, off)


@pytest.mark.parametrize("name", list(CASES))
def test_row_broadcast_past_one_round(name):
    """scale[r] * X[r, :] against the numpy product, bit for bit (NaN in the same places)."""
    n, F, ld, off, vec, L = CASES[name]
    X, _, act, _ = case_inputs(name)
    _, Xd = placed(X, ld, off)
    ob, out = placed(np.zeros((n, F), np.float32), ld, off)
    check_vec(vec, F, Xd, out)
    ops.row_broadcast(torch.from_numpy(act).to(DEV), Xd, out=out)
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), act[:, None] * X
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 4
    assert untouched(ob, n, F, ld, off)


@pytest.mark.parametrize("name", list(CASES))
def test_row_broadcast_deg_past_one_round(name):
    """deg(r)^-0.5 * X[r, :] with the degrees of a uniform graph of that many rows, against the
    oracle's degree pass times X."""
    n, F, ld, off, vec, L = CASES[name]
    X, _, _, _ = case_inputs(name)
    g = layout.gen_graph("uniform", n, n // 2, seed=F)
    assert g.n_rows == n and len(np.unique(np.diff(g.rowptr))) >= 3
    norm = orc.degree(to_oracle(g), power=-0.5)
    _, Xd = placed(X, ld, off)
    ob, out = placed(np.zeros((n, F), np.float32), ld, off)
    check_vec(vec, F, Xd, out)
    ops.row_broadcast_deg(ops.DeviceGraph.from_host(g, split=False), Xd, out=out)
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), norm[:, None] * X
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert untouched(ob, n, F, ld, off)
