"""GPU: the dense kernels of csrc/dense.hip past the first pass of their row loops.

k_ffn_fwd walks 4-tile groups of 32 rows on a grid capped at 1024 workgroups: past 131 072 rows
a workgroup refills its LDS X tiles after the trailing barrier and reuses bv[].  N here is
2 * 131 072 + 4 * 32 * 3 + 5: three rounds for the first workgroups, a ragged last tile, and a
last 4-tile group whose waves 1..3 lie past N.  The dense gradients' k_tn_skinny takes a second
pass of its rb loop once a chunk is longer than U * RPB rows, and k_tn_lds<3> reuses LDS buffer
0 from its third 16-row stage on; the shapes below reach both, as the asserted arithmetic of
plan_for (_rounds.dense_grad_plan) shows.

Beside the existing float64 bounds (1e-5 of the mass, which at these N absorbs a dropped or
doubled row), integer-valued inputs: every product and partial sum is an integer far below
2^24, so float32 holds each exactly whatever the order or chunking, and the result must EQUAL
the exact one (formed in float64, which holds these integers exactly too, so it is the int64
result).  A row taken from another round's stale tile, dropped or counted twice cannot pass.
"""
import numpy as np
import pytest
import torch

from gala import ops
from _rounds import FFN_ROUND, LDS_STAGE, SKINNY_U, dense_grad_plan, skinny_kl

pytestmark = pytest.mark.gpu
DEV = "cuda"

FFN_N = 2 * FFN_ROUND + 4 * 32 * 3 + 5
# (K, M): (the X vector width V, the 32-column tiles WM) of k_ffn_fwd<WM, V>
FFN_CASES = {(5, 3): (1, 1), (8, 40): (4, 2), (47, 32): (1, 1), (48, 128): (4, 4)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ffn_shape_is_past_one_round(N):
    tiles = -(-N // 32)
    assert N > 2 * FFN_ROUND and N % 32 == 5              # three rounds, a ragged last tile
    assert tiles % 4 == 1                                  # the last group: one live wave, three past N
    assert -(-tiles // 4) > 2 * (FFN_ROUND // 128)


def ffn_kernel(K, M, X):
    """(V, WM) as gala_ffn_fwd_f32 selects them (csrc/dense.hip:615, 624)."""
    v4 = K % 4 == 0 and X.stride(0) % 4 == 0 and X.data_ptr() % 16 == 0
    return (4 if v4 else 1), -(-M // 32)


def first_bad_row(Y, want):
    bad = np.flatnonzero((Y != want).any(1))
    return "" if bad.size == 0 else (f"{bad.size} rows differ, the first row {bad[0]} (round {bad[0] // FFN_ROUND}, "
                                     f"tile {bad[0] // 32}): got {Y[bad[0]][:4]}, want {want[bad[0]][:4]}")


@pytest.mark.parametrize("K,M", list(FFN_CASES))
def test_ffn_fwd_integers_exact_past_one_round(K, M):
    N = FFN_N
    ffn_shape_is_past_one_round(N)
    rng = np.random.default_rng(K + M)
    X = rng.integers(-3, 4, (N, K)).astype(np.float32)
    W = rng.integers(-3, 4, (M, K)).astype(np.float32)
    b = rng.integers(-3, 4, M).astype(np.float32)
    Xd = dev(X)
    assert ffn_kernel(K, M, Xd) == FFN_CASES[(K, M)]
    want = X.astype(np.float64) @ W.astype(np.float64).T
    assert np.abs(want).max() + 3 < 2 ** 24
    msg = first_bad_row(host(ops.ffn_fwd(Xd, dev(W), dev(b))), want + b)
    assert not msg, msg
    msg = first_bad_row(host(ops.ffn_fwd(Xd, dev(W), None)), want)
    assert not msg, msg


@pytest.mark.parametrize("K,M", list(FFN_CASES))
def test_ffn_fwd_matches_float64_past_one_round(K, M):
    """tests/test_gpu_kernels.py's test_ffn_fwd_matches_float64 at this N: |err| <= 1e-5 *
    sum_k |x w| + 1e-6, with and without bias."""
    N = FFN_N
    ffn_shape_is_past_one_round(N)
    rng = np.random.default_rng(N + 7 * K + M)
    X = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    W = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    b = rng.uniform(-1, 1, M).astype(np.float32)
    Xd = dev(X)
    assert ffn_kernel(K, M, Xd) == FFN_CASES[(K, M)]
    Y = host(ops.ffn_fwd(Xd, dev(W), dev(b)))
    want = X.astype(np.float64) @ W.astype(np.float64).T + b
    mass = np.abs(X.astype(np.float64)) @ np.abs(W.astype(np.float64)).T + np.abs(b)
    over = np.abs(Y - want) / (1e-5 * mass + 1e-6)
    print(f"ffn_fwd K={K} M={M} bias: worst |err| / bound {over.max():.3g}")
    assert over.max() <= 1, np.unravel_index(over.argmax(), over.shape)
    Y2 = host(ops.ffn_fwd(Xd, dev(W), None))
    over = np.abs(Y2 - (want - b)) / (1e-5 * mass + 1e-6)
    print(f"ffn_fwd K={K} M={M} no bias: worst |err| / bound {over.max():.3g}")
    assert over.max() <= 1, np.unravel_index(over.argmax(), over.shape)


def test_ffn_fwd_strided_past_one_round():
    """ldx = K + 1 with NaN in the skipped column, ldy > M with a sentinel; integers, exact."""
    N, K, M = FFN_N, 47, 40
    ffn_shape_is_past_one_round(N)
    rng = np.random.default_rng(3)
    X = rng.integers(-3, 4, (N, K)).astype(np.float32)
    W = rng.integers(-3, 4, (M, K)).astype(np.float32)
    b = rng.integers(-3, 4, M).astype(np.float32)
    Xb = torch.full((N, K + 1), float("nan"), device=DEV)
    Xb[:, :K] = dev(X)
    Yb = torch.full((N, M + 4), 7.0, device=DEV)
    assert ffn_kernel(K, M, Xb[:, :K]) == (1, 2)
    ops.ffn_fwd(Xb[:, :K], dev(W), dev(b), out=Yb[:, :M])
    msg = first_bad_row(host(Yb[:, :M]), X.astype(np.float64) @ W.astype(np.float64).T + b)
    assert not msg, msg
    assert bool(torch.all(Yb[:, M:] == 7.0))


# ---- the dense gradients -----------------------------------------------------------------------
# (N, K, M): (kernel, passes of its row loop over a full chunk, the last pass ragged)
GRAD_NEW = {
    (140000, 5, 2): ("skinny", 2, True),       # KL = 8: 128 rows per pass, chunks of 192
    (70000, 16, 3): ("skinny", 2, False),      # KL = 16: 64 rows per pass, chunks of 128
    (16500, 68, 180): ("lds3", 4, False),      # one 192 x 128 tile with a partial k tile, chunks of 64 rows
    # three m tiles (the last partial) by two k tiles: 86 chunks of 384 rows, 24 stages each
    (33000, 132, 540): ("lds3", 24, False),
}
GRAD_OLD = {(50000, 32, 47): "mfma", (70001, 5, 2): "skinny", (3000, 100, 180): "lds3"}


def grad_shape_reaches(N, K, M):
    """The kernel and the passes of its loop, from plan_for's arithmetic (csrc/dense.hip:466-498
    through _rounds.dense_grad_plan); float4 rows: contiguous operands, 16-B aligned."""
    pl = dense_grad_plan(N, K, M, K % 4 == 0 and M % 4 == 0)
    want = GRAD_NEW.get((N, K, M))
    if want is None:
        assert pl["kernel"] == GRAD_OLD[(N, K, M)]
        return pl
    assert (pl["kernel"], pl["passes"], pl["ragged"]) == want, pl
    if pl["kernel"] == "skinny":    # a second pass of the rb loop
        assert pl["step"] == SKINNY_U * (64 // skinny_kl(K)) * 4 and pl["rows_per_chunk"] > pl["step"]
    else:                           # a third stage: LDS buffer 0 written again
        assert pl["step"] == LDS_STAGE[3] and pl["rows_per_chunk"] >= 3 * pl["step"]
    assert pl["P"] > 1 and N % pl["rows_per_chunk"] != 0   # and a shorter last chunk
    return pl


@pytest.mark.parametrize("N,K,M", list(GRAD_NEW))
def test_dense_grad_matches_float64_past_one_pass(N, K, M):
    """tests/test_gpu_kernels.py's test_dense_grad_matches_float64 on the shapes whose row loops
    take a second pass (k_tn_skinny) or a third stage (k_tn_lds<3>)."""
    grad_shape_reaches(N, K, M)
    rng = np.random.default_rng(N + K + M)
    X = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    dY = rng.uniform(-1, 1, (N, M)).astype(np.float32)
    dW, db = ops.dense_grad(dev(X), dev(dY))
    X64, Y64 = X.astype(np.float64), dY.astype(np.float64)
    want = Y64.T @ X64
    mass = np.abs(Y64).T @ np.abs(X64)
    over = np.abs(host(dW) - want) / (1e-5 * mass + 1e-6)
    print(f"dense_grad N={N} K={K} M={M}: worst |err| / bound {over.max():.3g}")
    assert over.max() <= 1, np.unravel_index(over.argmax(), over.shape)
    np.testing.assert_allclose(host(db), Y64.sum(0), atol=1e-5 * max(N, 1), rtol=1e-5)
    dW2, db2 = ops.dense_grad(dev(X), dev(dY))
    np.testing.assert_array_equal(host(dW2), host(dW))
    np.testing.assert_array_equal(host(db2), host(db))


@pytest.mark.parametrize("N,K,M", list(GRAD_OLD) + list(GRAD_NEW))
def test_dense_grad_integers_exact(N, K, M):
    """X in {-2..2}, dY in {-1, 0, 1}: every partial is an integer of magnitude <= 2 N < 2^24, so
    dW and db equal dY^T X and the column sums exactly, whatever the chunking; also accumulated
    onto an integer dW0 / db0."""
    grad_shape_reaches(N, K, M)
    assert 2 * N + 8 < 2 ** 24
    rng = np.random.default_rng(N + K + M)
    X = rng.integers(-2, 3, (N, K)).astype(np.float32)
    dY = rng.integers(-1, 2, (N, M)).astype(np.float32)
    want = dY.astype(np.float64).T @ X.astype(np.float64)
    wantb = dY.astype(np.float64).sum(0)
    dW, db = ops.dense_grad(dev(X), dev(dY))
    got, gotb = host(dW), host(db)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(gotb, wantb), (gotb - wantb)
    W0 = rng.integers(-4, 5, (M, K)).astype(np.float32)
    b0 = rng.integers(-4, 5, M).astype(np.float32)
    dW, db = dev(W0), dev(b0)
    ops.dense_grad(dev(X), dev(dY), dW=dW, db=db, accumulate=True)
    assert np.array_equal(host(dW), W0 + want) and np.array_equal(host(db), b0 + wantb)
