"""The exact GAT layer on a directed pattern, on the host (gala_cpu_gat_bwd_stats_exact_t_f32 and
gala_cpu_csr_is_transpose_i32, the twins of the HIP kernels): the float64 reference against
torch.autograd, the twins against the float64 reference per element, the constants of the bounds
(tests/_gat_exact_directed_ref.py), the symmetric pair as the special case (g, g), and the
transpose test's positive and negative cases."""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _edge_ref as E
import _gat_exact_directed_ref as D
import _gat_exact_ref as X
from gala import _abi, backend, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
t = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def test_abi_has_the_directed_pair():
    for lib in (_abi.lib(), _abi.cpu_lib()):
        pre = "gala_cpu_" if lib is _abi.cpu_lib() else "gala_"
        assert hasattr(lib, pre + "gat_bwd_stats_exact_t_f32") and hasattr(lib, pre + "csr_is_transpose_i32")


def test_reference_is_the_derivative():
    """directed_layer's gradients are torch.autograd's of the dense float64 layer: 41 rows of a
    directed graph with empty rows and empty columns, 3 heads, logits on a grid of 1/64 (their
    fp32 sum is exact, so both see the same branch)."""
    rng = np.random.default_rng(2)
    n, H, Dh = 41, 3, 5
    src, dst = rng.integers(0, 33, 260), rng.integers(4, 37, 260)    # rows 33.. empty, columns 0..3 and 37.. empty
    g = D.simple(n, src, dst)
    gT = D.transposed(g)
    assert not np.array_equal(gT.col, g.col) and g.nnz > 150
    aL = (rng.integers(-192, 193, (n, H)) / 64.0).astype(np.float32)
    aR = (rng.integers(-192, 193, (n, H)) / 64.0 + 1.0 / 128).astype(np.float32)     # no logit is 0
    Xf, dY = E._u(rng, -1, 1, n, H * Dh), E._u(rng, -1, 1, n, H * Dh)
    ref = D.directed_layer(g, aL, aR, Xf, dY, H)
    R = ref.R
    mask = torch.zeros((n, n), dtype=torch.bool)
    mask[torch.from_numpy(R.row), torch.from_numpy(R.col)] = True
    taL, taR, tX = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (aL, aR, Xf))
    z = torch.nn.functional.leaky_relu(taL[:, None, :] + taR[None, :, :], float(np.float32(D.SLOPE)))   # [r, c, h]
    z = z.masked_fill(~mask[:, :, None], -float("inf"))
    nonempty = torch.from_numpy(R.deg > 0)
    a = torch.zeros_like(z)
    a[nonempty] = torch.softmax(z[nonempty], dim=1)
    Y = torch.einsum("rch,chd->rhd", a, tX.view(n, H, Dh)).reshape(n, H * Dh)
    Y.backward(torch.tensor(dY, dtype=torch.float64))
    assert (R.deg == 0).sum() >= 8 and (ref.RT.deg == 0).sum() >= 8
    for name, got, want in (("Y", ref.Y, Y.detach()), ("dX", ref.dX, tX.grad), ("daL", ref.daL, taL.grad),
                            ("daR", ref.daR, taR.grad)):
        err = np.abs(got - want.numpy()).max()
        assert err < 1e-12, (name, err)
    # the symmetric reference's backward walk (row c's stored neighbours) is far from it here
    sym = X.exact_layer(g, aL, aR, Xf, dY, H)
    assert np.abs(sym.dX - ref.dX).max() > 1e-2 and np.abs(sym.daR - ref.daR).max() > 1e-2


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_twins_against_float64(case):
    """Every output of the twins within c * mass of the float64 layer; the worst ratios go to
    GALA_GAT_EXACT_RECORD (a JSON-lines file) when set -- profiles/gat_exact_directed_bounds_cpu.jsonl
    holds them, and _gat_exact_directed_ref.MEASURED their maxima."""
    g, i, ref, got, aR = D.twin_case(case)
    if i.rc:
        ar64, arm = X.source_logits(i.X, i.wR, i.bR, case[1])
        E.assert_bounded("aR_out", aR, ar64, arm, X.C_AR, g=g, per="row", record=False)
    if case[4]:
        z = i.aL.reshape(-1, case[1])[ref.R.row] + aR[ref.R.col]
        assert (z > 30).sum() > 100, "logits where the REF softmax's clamp would matter"
    worst = D.check(D.case_id(case), got, ref)
    path = os.environ.get("GALA_GAT_EXACT_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": D.case_id(case), "backend": "cpu", **worst}) + "\n")
    # the symmetric backward's walk over A cannot pass on these graphs
    sym = X.exact_layer(g, i.aL, aR, i.X, i.dY, case[1])
    far = lambda a, b, mass, c: float(np.max(np.abs(a - b) / (c * mass + 1e-12)))
    assert far(sym.dX, ref.dX, ref.dX_mass, D.C["dX"]) > 100


def test_constants_are_the_measured_ones():
    """MEASURED holds the committed profile's maxima; C is 8 x that, or the symmetric pair's
    constant where the directed worst is no larger than the symmetric one."""
    rows = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", "gat_exact_directed_bounds_cpu.jsonl"))]
    assert {r["case"] for r in rows} == {D.case_id(c) for c in D.CASES}
    for q in D.QUANTITIES:
        worst = max(r[q] for r in rows)
        assert worst <= D.MEASURED[q] <= 1.05 * worst + 1e-12, (q, worst, D.MEASURED[q])
        assert D.C[q] == (X.C[q] if D.MEASURED[q] <= X.MEASURED[q] else E.c_from(D.MEASURED[q]))


@pytest.mark.parametrize("name,H,F", [("cora", 1, 47), ("long", 8, 64), ("hub", 8, 256)])
def test_symmetric_pair_is_the_special_case(name, H, F):
    """On a symmetric graph passed as (g, g) the directed backward's twin is array-equal to the
    symmetric backward's (hub rows under the plan included)."""
    g = X.graph(name)
    i = X.inputs(g, H, F, False, True)
    be = backend.CpuBackend()
    cg = be.graph(g)
    cg.set_split_plan(*X.PLAN)
    f = be.gat_stats_exact(cg, t(i.aL), t(i.aR), t(i.X), H, X.SLOPE)
    a = be.gat_bwd_stats_exact(cg, t(i.aL), f[4], t(i.X), t(i.dY), f[1], f[0], f[2], f[3], H, X.SLOPE)
    b = be.gat_bwd_stats_exact_t(cg, cg, t(i.aL), f[4], t(i.X), t(i.dY), f[1], f[0], f[2], f[3], H, X.SLOPE)
    for u, v in zip(a, b):
        assert np.array_equal(u.numpy(), v.numpy())


def test_plan_of_the_transpose_changes_only_its_hub_rows():
    """dX and d_aR of rows of A^T at or below the threshold are bit-identical with and without a
    plan on A^T (A's plan fixed: the forward and the side lines are the same); its hub rows are
    summed as chunk partials, a different association."""
    name, H, F = "split", 8, 256
    g = D.graph(name)
    gT = D.transposed(g)
    i = D.inputs(g, H, F, False, False)
    be = backend.CpuBackend()
    cg = be.graph(g)
    cg.set_split_plan(*D.PLAN)
    out = []
    for plan in (None, D.PLAN):
        cgT = be.graph(gT)
        if plan:
            cgT.set_split_plan(*plan)
        out.append([a.reshape(g.n_rows, -1) for a in D.twin_layer(be, cg, cgT, i, H)[0].values()])
    hub = np.diff(gT.rowptr) > D.PLAN[0]
    assert hub.sum() == 1 and hub[11]
    for a, b in zip(*out):
        assert np.array_equal(a[~hub], b[~hub])
    assert any(not np.array_equal(a[hub], b[hub]) for a, b in zip(*out))


def test_compiled_directed_fixed_program_on_the_host(tmp_path):
    """tests/dsl/gat_directed_fixed.txt's program with --device cpu (the mirror over the host twins)
    on a directed graph with distinct edges: with GALA_GAT_EXACT_DIRECTED=1 it meets the float64
    executor of its IR and its gradients are not the alpha-storing path's bits."""
    D.check_directed_fixed_program(tmp_path, "--device", "cpu")


# ---- the transpose test -----------------------------------------------------------------------

def test_round_constant_is_the_launch_codes():
    """CHECK_ROUND, which the GPU test of the second round relies on, is kCheckMaxBlocks * kBlock
    of the sources."""
    assert D.CHECK_ROUND == D.check_round_from_source()


def cpu_count(a, at):
    be = backend.CpuBackend()
    count = ctypes.c_int32(-1)
    _abi.call_cpu("gala_csr_is_transpose_i32", be.graph(a).csr(), be.graph(at).csr(), ctypes.addressof(count), None)
    return count.value


@pytest.mark.parametrize("name", ["uni", "rmat", "split"])
def test_is_transpose_twin(name):
    g = D.graph(name)
    gT = D.transposed(g)
    be = backend.CpuBackend()
    assert be.is_transpose(be.graph(g), be.graph(gT)) and be.is_transpose(be.graph(gT), be.graph(g))
    assert cpu_count(g, gT) == 0
    for k, (a, at) in D.negatives(g, gT).items():
        assert cpu_count(a, at) > 0, k
        assert not be.is_transpose(be.graph(a), be.graph(at)), k
    s = X.graph("cora")
    assert cpu_count(s, s) == 0
    # a graph with a duplicated edge has no strictly ascending transpose: no pair
    d = layout.csr_build(4, 4, np.array([0, 0, 1], np.int32), np.array([1, 1, 2], np.int32))
    assert cpu_count(d, layout.transpose(d)[0]) > 0


def test_argument_checks():
    g = D.graph("uni")
    gT = D.transposed(g)
    be = backend.CpuBackend()
    cg, cgT = be.graph(g), be.graph(gT)
    # F = 12 at 2 heads: D / VEC = 3 lanes per head, not a power of two
    with pytest.raises(_abi.GalaError) as e:
        z, v = torch.zeros(g.n_rows, 12), torch.zeros(g.n_rows * 2)
        be.gat_bwd_stats_exact_t(cg, cgT, v, v, z, z, v, z, z, v, 2, D.SLOPE)
    assert e.value.status == _abi.GALA_ERR_UNSUPPORTED
    # a second pattern that is not the transpose is refused before any call, and only tested once
    calls = []
    orig = be.is_transpose
    be.is_transpose = lambda a, b: (calls.append(1), orig(a, b))[1]
    z, v = torch.zeros(g.n_rows, 8), torch.zeros(g.n_rows * 2)
    for _ in range(2):
        with pytest.raises(ValueError):
            be.gat_bwd_stats_exact_t(cg, cg, v, v, z, z, v, z, z, v, 2, D.SLOPE)
    assert len(calls) == 1
    # mismatched n, a tiled pattern: a status from the entry point itself
    small = be.graph(D.simple(g.n_rows - 1, [0, 1], [1, 0]))
    tiled = be.graph(layout.col_tile(g, 100))
    side = torch.zeros(g.n_rows * 2 * 4)
    for a, b in ((cg, small), (small, cgT), (cg, tiled), (tiled, cgT)):
        st = _abi.cpu_lib().gala_cpu_gat_bwd_stats_exact_t_f32(
            a.csr(), b.csr(), v.data_ptr(), v.data_ptr(), z.data_ptr(), 8, z.data_ptr(), 8, 8, 2, D.SLOPE, v.data_ptr(),
            z.data_ptr(), 8, z.data_ptr(), 8, v.data_ptr(), side.data_ptr(), z.data_ptr(), 8, v.data_ptr(), v.data_ptr(), None)
        assert st == _abi.GALA_ERR_INVALID_ARG
        count = ctypes.c_int32(-1)
        st = _abi.cpu_lib().gala_cpu_csr_is_transpose_i32(a.csr(), b.csr(), ctypes.addressof(count), None)
        assert st == _abi.GALA_ERR_INVALID_ARG and count.value == -1
        assert not be.is_transpose(a, b)
