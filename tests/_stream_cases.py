"""TEST INFRASTRUCTURE: one small case per device entry point of the C ABI, for the ordering
tests (tests/test_gpu_stream_order.py) and their completeness check (tests/test_stream_cases_cpu.py).

A device entry point is a key of gala._abi.SIGNATURES that returns a status, takes the stream as
its last argument and is no gala_host_* function (device_entry_points()).  CASES maps each to a
builder; a builder makes the operands on the device and returns a Built:

    run()      issues the op on torch's current stream -- through gala.ops where a wrapper exists,
               through _abi.call (DIRECT below) where none does, where the wrapper allocates a
               workspace or a memset target itself (a buffer the test cannot poison hides a launch
               that ran too early), where it synchronises, or where the op reads no float input.
               The wrappers that allocate their outputs (sddvv, sddmm, edge_softmax, head_attn,
               edge_permute, the gat_fwd family, ...) stay: a launch of theirs on another stream
               shows through the NaN it reads from the poisoned inputs;
    inputs     the float tensors the op reads (in-place operands included): the tests refill them;
    outputs    a list the float (and the one int32) tensors the op wrote, refreshed by every run():
               fixed tensors where the op takes its outputs, the wrapper's fresh ones elsewhere;
    graphs     the DeviceGraphs whose hub-row plan owns a float workspace (an output as well);
    partial    indices into outputs of buffers the op writes only in part (tables, workspaces).

Index and structure operands (rowptr, col, row order, the plan's arrays, rows, perm, self_col,
both graphs of gala_csr_is_transpose_i32) are made once and never rewritten: a poisoned index
would make a correct kernel read out of bounds.

Every op here is deterministic (the one atomic of csrc/ is the int32 counter of
csrc/csr_check.hip), so every case compares bit for bit (MODE).  The numbers themselves are not
checked here: operands of a backward are the matching forward's outputs only so that they are
plausible, and the tests perturb them freely.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from gala import _abi, layout, ops
from gala import dist as gdist
from _graphs import cora_like, powerlaw

MODE = "equal"          # the comparison of every case: torch.equal on the bits
REF, FIXED = _abi.GALA_SOFTMAX_REF, _abi.GALA_SOFTMAX_FIXED
THRESHOLD = 64          # the tests' small hub-row plan (tests/test_gpu_kernels.py's capture test)
IN_SHAPE = (37, 4, 16)  # (fin, heads, D) of the gala_gat_in_* cases
DENSE_N = 2708
DENSE_GRAD_KM = (5, 2)  # the smallest (K, M) of tests/test_gpu_kernels.py::test_dense_grad_matches_float64
FFN_KM = (7, 3)         # the smallest beside (1, 1) of tests/test_gpu_kernels.py::test_ffn_fwd_matches_float64
RECT_BOUNDS = (0, 100, 2101, 4096)   # the middle rank: halo rows below and above its own block

# device entry points without a case, each with its reason
EXCLUDED: dict[str, str] = {}


def device_entry_points() -> set[str]:
    return {name for name, (res, args) in _abi.SIGNATURES.items()
            if res is ctypes.c_int and args and args[-1] is ctypes.c_void_p and not name.startswith("gala_host_")}


class Built:
    def __init__(self, run, inputs, outputs, graphs=(), partial=()):
        self.run, self.inputs, self.outputs = run, list(inputs), outputs
        self.graphs, self.partial = tuple(graphs), frozenset(partial)

    def workspaces(self):
        """The float workspaces of the graphs' hub-row plans (grown by the first run)."""
        return [g._split["ws"] for g in self.graphs if g._split is not None and g._split["ws"] is not None]


# ---- operands ---------------------------------------------------------------------------------

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rnd(seed, *shape, lo=-1.0, hi=1.0):
    return dev(np.random.default_rng(seed).uniform(lo, hi, shape).astype(np.float32))


def empty(*shape):
    return torch.empty(*shape, device="cuda", dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def host_graph(name) -> layout.HostGraph:
    """"cora": cora_like(); "rmat" = "sym": powerlaw(), its own transpose; "dir": powerlaw() without
    the edges (r, c), r < c, 3 | r + c (directed, hub rows kept); "dir_t": the transpose of "dir"."""
    if name == "cora":
        return cora_like()
    g = powerlaw()
    if name in ("rmat", "sym"):
        t = layout.transpose(g)[0]
        assert np.array_equal(t.rowptr, g.rowptr) and np.array_equal(t.col, g.col)
        return g
    src = np.repeat(np.arange(g.n_rows, dtype=np.int32), np.diff(g.rowptr))
    keep = ~((src < g.col) & ((src + g.col) % 3 == 0))
    d = layout.csr_build(g.n_rows, g.n_cols, src[keep], g.col[keep])
    t = layout.transpose(d)[0]
    assert d.nnz < g.nnz and not (np.array_equal(t.rowptr, d.rowptr) and np.array_equal(t.col, d.col))
    return d if name == "dir" else t


def plain(name="cora"):
    return ops.DeviceGraph.from_host(host_graph(name), split=False)


def hub(name="rmat", chunk=32, row_order=True, g=None):
    """The graph under the plan (64, chunk) with hub rows, so the chunk kernels and -- for the ops
    that keep the reference's order on hub rows -- the plan's side stream run."""
    g = host_graph(name) if g is None else g
    dg = ops.DeviceGraph.from_host(g, split=False)
    dg.set_split_plan(g.rowptr, THRESHOLD, chunk=chunk, row_order=row_order)
    assert dg.split_rows > 0
    return dg


def _tensors(r):
    return [t for t in (r if isinstance(r, (tuple, list)) else (r,)) if t is not None]


def wrapped(fn, inputs, graphs=(), partial=()):
    """A case over a gala.ops wrapper: outputs are what the wrapper returns."""
    outs = []

    def run():
        outs[:] = _tensors(fn())
    return Built(run, inputs, outs, graphs, partial)


def direct(fn, inputs, outputs, graphs=(), partial=()):
    """A case over _abi.call on buffers the case owns."""
    return Built(fn, inputs, list(outputs), graphs, partial)


def _sync(*r):
    torch.cuda.synchronize()
    return r[0] if len(r) == 1 else r


def _self_cols(n):
    return torch.arange(n, dtype=torch.int32, device="cuda")


# ---- spmm.hip / dense.hip / attn.hip -----------------------------------------------------------

def spmm():
    dg, F = hub(), 47
    X, ss, ds = rnd(1, dg.n_cols, F), rnd(2, dg.n_cols), rnd(3, dg.n_rows)
    out = empty(dg.n_rows, F)
    return wrapped(lambda: ops.spmm(dg, X, src_scale=ss, dst_scale=ds, out=out), [X, ss, ds], [dg])


def spmm_ex():
    dg, F = hub(), 32
    X, ss = rnd(4, dg.n_cols, F), rnd(5, dg.n_cols)
    out, out2 = empty(dg.n_rows, F), empty(dg.n_rows, F)
    return wrapped(lambda: (ops.spmm(dg, X, src_scale=ss, out=out, dst_deg=True, out2=out2), out2), [X, ss], [dg])


def row_broadcast_deg():
    dg, F = plain(), 47
    X, out = rnd(6, dg.n_rows, F), empty(dg.n_rows, F)
    return wrapped(lambda: ops.row_broadcast_deg(dg, X, out=out), [X])


def degree():
    """DIRECT: no float input to poison, so the output is owned and poisoned instead of ops.degree's
    fresh one."""
    dg = hub()
    out = empty(dg.n_rows)

    def run():
        _abi.call("gala_degree_f32", dg.csr(), out.data_ptr(), -0.5, 0, 0, ops._stream())
    return direct(run, [], [out], [dg])


def row_broadcast():
    s, X = rnd(7, DENSE_N), rnd(8, DENSE_N, 47)
    out = empty(DENSE_N, 47)
    return wrapped(lambda: ops.row_broadcast(s, X, out=out), [s, X])


def ffn_fwd():
    K, M = FFN_KM
    X, W, b, out = rnd(9, DENSE_N, K), rnd(10, M, K), rnd(11, M), empty(DENSE_N, M)
    return wrapped(lambda: ops.ffn_fwd(X, W, b, out=out), [X, W, b])


def row_scale_relu():
    X, act, pre = rnd(12, DENSE_N, 47), rnd(13, DENSE_N, lo=0.1, hi=2), rnd(14, DENSE_N, lo=0.1, hi=2)
    out = empty(DENSE_N, 47)
    return wrapped(lambda: ops.row_scale_relu(X, act, pre, out=out), [X, act, pre])


def relu_scale_backward():
    X, G, act = rnd(15, DENSE_N, 32), rnd(16, DENSE_N, 32), rnd(17, DENSE_N, lo=0.1, hi=2)
    out = empty(DENSE_N, 32)
    return wrapped(lambda: ops.relu_scale_backward(X, G, act, out=out), [X, G, act])


def dense_grad():
    """DIRECT: ops.dense_grad allocates the partials' workspace itself."""
    N, (K, M) = DENSE_N, DENSE_GRAD_KM
    X, dY = rnd(18, N, K), rnd(19, N, M)
    dW, db = empty(M, K), empty(M)
    wsb = _abi.lib().gala_dense_grad_workspace(N, K, M)
    ws = empty(max(wsb // 4, 1))

    def run():
        _abi.call("gala_dense_grad_f32", N, K, M, X.data_ptr(), K, dY.data_ptr(), M, dW.data_ptr(), db.data_ptr(), 0,
                  ws.data_ptr(), wsb, ops._stream())
    return direct(run, [X, dY], [dW, db, ws], partial=[2])


def dense_grad_empty():
    """N = 0: the call is its two hipMemsetAsync (csrc/dense.hip), on owned, poisoned dW and db."""
    K, M = DENSE_GRAD_KM
    dW, db = empty(M, K), empty(M)

    def run():
        _abi.call("gala_dense_grad_f32", 0, K, M, None, K, None, M, dW.data_ptr(), db.data_ptr(), 0, None, 0,
                  ops._stream())
    return direct(run, [], [dW, db])


def head_attn():
    X, w, b = rnd(20, DENSE_N, 32), rnd(21, 32), rnd(22, 4)
    return wrapped(lambda: ops.head_attn(X, w, b, heads=4), [X, w, b])


def head_attn_bwd():
    g, w, dX = rnd(23, DENSE_N, 4), rnd(24, 32), rnd(25, DENSE_N, 32)
    return wrapped(lambda: ops.head_attn_bwd(g, w, heads=4, dX=dX), [g, w, dX])   # accumulates into dX


# ---- edge.hip ---------------------------------------------------------------------------------

def sddvv():
    dg, H = hub(), 4
    a, b = rnd(26, dg.n_rows * H), rnd(27, dg.n_cols * H)
    return wrapped(lambda: ops.sddvv(dg, a, b, op=_abi.GALA_SDDVV_ADD_LRELU, heads=H), [a, b], [dg])


def row_sum():
    """The reference's order on hub rows: k_row_sum_hub on the plan's side stream (HubFork)."""
    dg, H = hub(), 4
    v, out = rnd(28, dg.nnz * H), empty(dg.n_rows * H)
    return wrapped(lambda: ops.row_sum(dg, v, heads=H, out=out), [v], [dg])


def row_scale():
    dg = hub()
    q, v = rnd(29, dg.n_rows), rnd(30, dg.nnz)
    return wrapped(lambda: ops.row_scale_(dg, q, v), [q, v], [dg])               # v in place


def sddmm():
    dg, F, H = hub(), 32, 4
    A, B = rnd(31, dg.n_rows, F), rnd(32, dg.n_cols, F)
    return wrapped(lambda: ops.sddmm(dg, A, B, heads=H), [A, B], [dg])


def edge_softmax_fwd():
    dg, H = hub(), 4
    s = rnd(33, dg.nnz * H, lo=-3, hi=3)
    return wrapped(lambda: ops.edge_softmax(dg, s, heads=H, mode=REF), [s], [dg])


def edge_softmax_bwd():
    dg = hub()
    al = _sync(ops.edge_softmax(dg, rnd(34, dg.nnz, lo=-3, hi=3), mode=FIXED)).clone()
    d = rnd(35, dg.nnz)
    return wrapped(lambda: ops.edge_softmax_bwd(dg, al, d, mode=FIXED), [al, d], [dg])


def edge_permute():
    dg, H = plain(), 4
    perm = dev(np.random.default_rng(36).permutation(dg.nnz).astype(np.int32))
    src = rnd(37, dg.nnz * H)
    return wrapped(lambda: ops.edge_permute(perm, src, heads=H), [src])


# ---- gat.hip / gat_fused.hip ------------------------------------------------------------------

def _gat_operands(dg, F, H, seed):
    return rnd(seed, dg.n_rows * H), rnd(seed + 1, dg.n_cols * H), rnd(seed + 2, dg.n_cols, F), rnd(seed + 3, dg.n_rows, F)


def gat_fwd():
    dg, F, H = hub(), 47, 1
    aL, aR, X, _ = _gat_operands(dg, F, H, 40)
    return wrapped(lambda: ops.gat_fwd(dg, aL, aR, X, heads=H, mode=REF, want_alpha=True), [aL, aR, X], [dg])


def gat_bwd():
    dg, F, H = hub(), 32, 4
    aL, aR, X, dY = _gat_operands(dg, F, H, 44)
    al = _sync(ops.gat_fwd(dg, aL, aR, X, heads=H, mode=FIXED, want_alpha=True))[1].clone()
    return wrapped(lambda: ops.gat_bwd(dg, aL, aR, X, dY, al, heads=H, mode=FIXED), [aL, aR, X, dY, al], [dg])


def gat_fwd_attn():
    dg, F = hub(), 32
    aL, _, X, _ = _gat_operands(dg, F, 1, 48)
    wR, bR = rnd(52, F), rnd(53, 1)
    return wrapped(lambda: ops.gat_fwd_attn(dg, aL, wR, bR, X, want_alpha=True), [aL, wR, bR, X], [dg])


def gat_bwd_attn():
    dg, F = hub(), 47
    aL, _, X, dY = _gat_operands(dg, F, 1, 54)
    wR, bR = rnd(58, F), rnd(59, 1)
    al = _sync(ops.gat_fwd_attn(dg, aL, wR, bR, X, want_alpha=True))[1].clone()
    return wrapped(lambda: ops.gat_bwd_attn(dg, aL, wR, bR, X, dY, al), [aL, wR, bR, X, dY, al], [dg])


def gat_fwd_ex():
    dg, F, H = hub(), 32, 4
    aL, _, X, _ = _gat_operands(dg, F, H, 60)
    wR, bR = rnd(64, F), rnd(65, H)
    return wrapped(lambda: ops.gat_fwd_ex(dg, aL, X, wR=wR, bR=bR, heads=H, factored=True), [aL, wR, bR, X], [dg])


def gat_bwd_ex():
    dg, F, H = hub(), 32, 4
    aL, aR, X, dY = _gat_operands(dg, F, H, 66)
    _, p, q = _sync(ops.gat_fwd_ex(dg, aL, X, aR=aR, heads=H, factored=True))
    p, q = p.clone(), q.clone()
    # (REF: d_aL only; dz per edge is FIXED mode's, gala_gat_bwd_f32's case: the library refuses a
    # d_logit buffer in REF mode, tests/test_gpu_kernels.py::test_gat_bwd_ref_mode_refuses_a_dz_buffer)
    return wrapped(lambda: ops.gat_bwd_ex(dg, aL, X, dY, p, q=q, aR=aR, heads=H), [aL, aR, X, dY, p, q], [dg])


def gat_bwd_fused():
    dg, F, H = hub(), 47, 1
    aL, aR, X, dY = _gat_operands(dg, F, H, 70)
    q = _sync(ops.gat_fwd_ex(dg, aL, X, aR=aR, heads=H, factored="q"))[1].clone()
    return wrapped(lambda: ops.gat_bwd_fused(dg, aL, X, dY, q, aR=aR, heads=H), [aL, aR, X, dY, q], [dg])


def gat_fwd_stats():
    dg, F, H = hub(), 32, 4
    aL, _, X, _ = _gat_operands(dg, F, H, 74)
    wR, bR = rnd(78, F), rnd(79, H)
    return wrapped(lambda: ops.gat_fwd_stats(dg, aL, X, wR=wR, bR=bR, heads=H, want_aR=True, want_p=True),
                   [aL, wR, bR, X], [dg])


def _stats(dg, F, H, seed):
    aL, aR, X, dY = _gat_operands(dg, F, H, seed)
    Y, q, Ym, sma = (t.clone() for t in _sync(ops.gat_fwd_stats(dg, aL, X, aR=aR, heads=H)))
    return aL, aR, dY, q, Y, Ym, sma


def gat_bwd_stats():
    dg, F, H = hub(), 47, 1
    a = _stats(dg, F, H, 80)
    return wrapped(lambda: ops.gat_bwd_stats(dg, *a, heads=H), a, [dg])


def gat_bwd_stats_ex():
    dg, F, H = hub(), 32, 4
    a = _stats(dg, F, H, 84)
    dYr = rnd(88, dg.n_rows, F)
    return wrapped(lambda: ops.gat_bwd_stats(dg, *a, heads=H, dY_rows=dYr), a + (dYr,), [dg])


def gat_bwd_stats_linear():
    dg, F, H = hub(), 32, 4
    a = _stats(dg, F, H, 90)
    dYr, wR = rnd(94, dg.n_rows, F), rnd(95, F)
    return wrapped(lambda: ops.gat_bwd_stats(dg, *a, heads=H, dY_rows=dYr, wR=wR), a + (dYr, wR), [dg])


def gat_fwd_stats_ex():
    dg, F, H = hub(), 47, 1
    aL, _, X, _ = _gat_operands(dg, F, H, 96)
    wR, bR, sc, aRo = rnd(100, F), rnd(101, H), _self_cols(dg.n_rows), empty(dg.n_cols, H)
    return wrapped(lambda: ops.gat_fwd_stats(dg, aL, X, wR=wR, bR=bR, heads=H, self_col=sc, aR_out=aRo) + (aRo,),
                   [aL, wR, bR, X], [dg])


def gat_fwd_partial_stats():
    dg, F, H = hub(), 47, 1
    aL, aR, X, _ = _gat_operands(dg, F, H, 102)
    return wrapped(lambda: ops.gat_fwd_partial_stats(dg, aL, X, aR=aR, heads=H), [aL, aR, X], [dg])


def gat_fwd_partial_stats_ex():
    dg, F, H = hub(), 32, 4
    aL, _, X, _ = _gat_operands(dg, F, H, 106)
    wR, bR, sc, aRo = rnd(110, F), rnd(111, H), _self_cols(dg.n_rows), empty(dg.n_cols, H)
    return wrapped(lambda: ops.gat_fwd_partial_stats(dg, aL, X, wR=wR, bR=bR, heads=H, self_col=sc, aR_out=aRo)
                   + (aRo,), [aL, wR, bR, X], [dg])


def gat_fwd_continue():
    """A second range over the same pattern, in place on the first range's partials."""
    dg, F, H = hub(), 32, 4
    aL, aR, X, _ = _gat_operands(dg, F, H, 112)
    U, S, Um, M = (t.clone() for t in _sync(ops.gat_fwd_partial_stats(dg, aL, X, aR=aR, heads=H)))
    return wrapped(lambda: ops.gat_fwd_continue(dg, aL, X, U, S, aR=aR, heads=H, Um0=Um, M0=M),
                   [aL, aR, X, U, S, Um, M], [dg])


# ---- gat_exact.hip / csr_check.hip -------------------------------------------------------------

def gat_fwd_stats_exact():
    dg, F, H = hub(), 32, 4
    aL, _, X, _ = _gat_operands(dg, F, H, 116)
    wR, bR = rnd(120, F), rnd(121, H)
    return wrapped(lambda: ops.gat_fwd_stats_exact(dg, aL, X, wR=wR, bR=bR, heads=H), [aL, wR, bR, X], [dg])


def _exact(dg, F, H, seed):
    aL, aR, X, dY = _gat_operands(dg, F, H, seed)
    Y, lse, Ym, sma, _ = _sync(ops.gat_fwd_stats_exact(dg, aL, X, aR=aR, heads=H))
    return aL, aR, X, dY, lse.clone(), Y.clone(), Ym.clone(), sma.clone()


def _bwd_exact(name, graphs, walk, F, H, seed):
    """DIRECT: the wrappers allocate the side lines' workspace themselves.  graphs: (g,) or
    (g, gT); walk: the graph whose plan the gather pass takes."""
    aL, aR, X, dY, lse, Y, Ym, sma = a = _exact(graphs[0], F, H, seed)
    n = graphs[0].n_rows
    dX, daL, daR, side = empty(n, F), empty(n * H), empty(n * H), empty(n * H * 4)
    w = 2 * ((F + 3) // 4 * 4) + H

    def run():
        csrs = [g.csr(w if g is walk else 0) for g in graphs]
        _abi.call(name, *csrs, aL.data_ptr(), aR.data_ptr(), X.data_ptr(), X.stride(0), dY.data_ptr(), dY.stride(0),
                  F, H, 0.2, lse.data_ptr(), Y.data_ptr(), Y.stride(0), Ym.data_ptr(), Ym.stride(0), sma.data_ptr(),
                  side.data_ptr(), dX.data_ptr(), dX.stride(0), daL.data_ptr(), daR.data_ptr(), ops._stream())
    return direct(run, a, [dX, daL, daR, side], graphs, partial=[3])


def gat_bwd_stats_exact():
    return _bwd_exact("gala_gat_bwd_stats_exact_f32", (g := hub("sym"),), g, 47, 1, 122)


def gat_bwd_stats_exact_t():
    """A real transpose pair: the directed graph and its transpose, a plan with hub rows on each."""
    g, gT = hub("dir"), hub("dir_t")
    return _bwd_exact("gala_gat_bwd_stats_exact_t_f32", (g, gT), gT, 32, 4, 126)


def csr_is_transpose():
    """DIRECT: ops.is_transpose reads the count back (a host synchronisation, no part of the ABI call)."""
    g, gT = plain("dir"), plain("dir_t")
    count = torch.empty(1, device="cuda", dtype=torch.int32)

    def run():
        _abi.call("gala_csr_is_transpose_i32", g.csr(), gT.csr(), count.data_ptr(), ops._stream())
    return direct(run, [], [count])


def gat_fwd_stats_exact_ex():
    dg, F, H = hub(), 32, 4
    aL, _, X, _ = _gat_operands(dg, F, H, 130)
    wR, bR, sc, aRo = rnd(134, F), rnd(135, H), _self_cols(dg.n_rows), empty(dg.n_cols, H)
    return wrapped(lambda: ops.gat_stats_exact_table(dg, aL, X, sc, wR=wR, bR=bR, aR_out=aRo, heads=H) + (aRo,),
                   [aL, wR, bR, X], [dg])


def gat_bwd_exact_pre_ex():
    dg, F, H = hub(), 47, 1
    aL, aR, X, dY, lse, Y, Ym, sma = _exact(dg, F, H, 136)
    sc, side = _self_cols(dg.n_rows), empty(dg.n_cols, 4 * H)
    return wrapped(lambda: (ops.gat_bwd_exact_pre_table(dg, aL, dY, lse, Y, Ym, sma, sc, side, heads=H), side),
                   [aL, dY, lse, Y, Ym, sma], [dg])


def gat_bwd_exact_gather_ex():
    dg, F, H = hub("sym"), 47, 1
    aL, aR, X, dY, lse, Y, Ym, sma = _exact(dg, F, H, 140)
    sc, side = _self_cols(dg.n_rows), empty(dg.n_cols, 4 * H)
    _sync(ops.gat_bwd_exact_pre_table(dg, aL, dY, lse, Y, Ym, sma, sc, side, heads=H))
    return wrapped(lambda: ops.gat_bwd_exact_gather_table(dg, aR, X, dY, side, sc, heads=H), [aR, X, dY, side], [dg])


# ---- gat_input.hip ----------------------------------------------------------------------------

class _InLayer:
    """The operands of the input-space layer at IN_SHAPE on `g` (own rows [lo, lo + n) of a table
    of g.n_cols rows): the prepared table, and what the forward leaves for the backward."""

    def __init__(self, g, base=None, seed=150):
        fin, H, D = IN_SHAPE
        self.g, self.base, self.n, self.F = g, base, g.n_rows, H * D
        self.X = rnd(seed, g.n_cols, fin)
        self.W, self.b = rnd(seed + 1, H * D, fin, lo=-0.3, hi=0.3), rnd(seed + 2, H * D)
        wL, bL, wR, bR = rnd(seed + 3, H * D), rnd(seed + 4, H), rnd(seed + 5, H * D), rnd(seed + 6, H)
        self.u, self.c = ops.gat_in_compose(self.W, self.b, wL, bL, wR, bR, H)
        self.xext = ops.gat_in_prep(self.X, self.u, self.c, H, xext=torch.zeros(g.n_cols, 128, device="cuda"))
        # q of every table row (the halo rows' would come from their owners): finite, positive
        ops.gat_in_q_scatter(self.xext, torch.ones(g.n_cols, H, device="cuda"), H)
        self.Y, self.Ym = empty(self.n, self.F), empty(self.n, self.F)
        self.dY = rnd(seed + 7, self.n, self.F)
        _sync()

    def fwd(self, T=None):
        fin, H, _ = IN_SHAPE
        return ops.gat_in_fwd(self.g, self.xext, self.W, self.b, H, fin, T=T, Y=self.Y, Ym=self.Ym, row_base=self.base)


def in_graph(rect):
    """The symmetric hub graph under the plan (64, 64) (gala_gat_in_* take chunks of 64 k edges), or
    the middle rank of its partition at RECT_BOUNDS: (graph, row_base)."""
    if not rect:
        return hub("sym", chunk=64), None
    p = gdist.partition_graph(host_graph("sym"), 1, 3, bounds=np.asarray(RECT_BOUNDS, np.int64), halo_mode="p2p")
    assert 0 < p.lo and p.lo + p.n < p.n_cols and p.graph.n_rows == p.n and p.graph.n_cols == p.n_cols
    return hub(g=p.graph, chunk=64, row_order=False), p.lo


def gat_in_prep():
    fin, H, _ = IN_SHAPE
    L = _InLayer(plain("cora"))
    xext = torch.zeros(L.g.n_cols, 128, device="cuda")
    return wrapped(lambda: ops.gat_in_prep(L.X, L.u, L.c, H, xext=xext), [L.X, L.u, L.c], partial=[0])


def _in_fwd(rect, tmode):
    g, base = in_graph(rect)
    L = _InLayer(g, base)
    T = empty(L.n, 896) if tmode else None
    if tmode and rect:   # (the rectangular T-mode forward runs no q pass: q is in the table)
        _sync(ops.gat_in_q(g, L.xext, IN_SHAPE[1], row_base=base))
    return wrapped(lambda: L.fwd(T) + (L.xext,) + ((T,) if tmode else ()), [L.xext, L.W, L.b], [g],
                   partial=[4, 5] if tmode else [4])


def _in_bwd(name, rect, tmode):
    """DIRECT: ops.gat_in_bwd allocates M (the target of the call's memset) and the workspace itself."""
    fin, H, D = IN_SHAPE
    g, base = in_graph(rect)
    L = _InLayer(g, base)
    T = empty(L.n, 896) if tmode else None
    if tmode and rect:
        _sync(ops.gat_in_q(g, L.xext, H, row_base=base))
    sma = _sync(L.fwd(T))[3].clone()
    daL, M = empty(L.n, H), empty(H, D, fin + 1)
    wsb = _abi.lib().gala_gat_in_bwd_workspace(H)
    ws = empty(max(wsb // 4, 1))
    tail = (L.dY.data_ptr(), L.Y.data_ptr(), L.Ym.data_ptr(), L.F, sma.data_ptr(), daL.data_ptr(), M.data_ptr(),
            ws.data_ptr(), wsb, 0)

    def run():
        if tmode:
            _abi.call(name, L.n, None, fin, H, D, T.data_ptr(), *tail, ops._stream())
        else:
            csr = g.csr(ops._gat_in_ws_cols(g, _abi.GALA_GAT_IN_WS_BWD))
            b = () if base is None else (int(base),)
            _abi.call(name, csr, *b, None, fin, H, D, 0.2, L.xext.data_ptr(), *tail, ops._stream())
    ins = [L.dY, L.Y, L.Ym, sma] + ([T] if tmode else [L.xext])
    return direct(run, ins, [daL, M, ws], [] if tmode else [g], partial=[2])


def gat_in_q_rect():
    g, base = in_graph(True)
    L = _InLayer(g, base)
    scratch = empty(8 * g.n_cols)
    return wrapped(lambda: (ops.gat_in_q(g, L.xext, IN_SHAPE[1], row_base=base, scratch=scratch), scratch),
                   [L.xext], [g], partial=[0, 1])


def gat_in_q_gather():
    H = IN_SHAPE[1]
    L = _InLayer(plain("cora"))
    rows = dev(np.random.default_rng(160).integers(0, L.g.n_cols, 777).astype(np.int32))
    out = empty(777, H)
    return wrapped(lambda: ops.gat_in_q_gather(L.xext, rows, H, out=out), [L.xext])


def gat_in_q_scatter():
    H = IN_SHAPE[1]
    L = _InLayer(plain("cora"))
    rows = dev(np.random.default_rng(161).permutation(L.g.n_cols)[:777].astype(np.int32))   # distinct rows
    src = rnd(162, 777, H, lo=0.5, hi=2)
    return wrapped(lambda: ops.gat_in_q_scatter(L.xext, src, H, rows=rows), [L.xext, src])


CASES = {
    "gala_spmm_f32": spmm,
    "gala_spmm_ex_f32": spmm_ex,
    "gala_row_broadcast_deg_f32": row_broadcast_deg,
    "gala_degree_f32": degree,
    "gala_row_broadcast_f32": row_broadcast,
    "gala_ffn_fwd_f32": ffn_fwd,
    "gala_row_scale_relu_f32": row_scale_relu,
    "gala_relu_scale_backward_f32": relu_scale_backward,
    "gala_dense_grad_f32": dense_grad,
    "gala_head_attn_f32": head_attn,
    "gala_head_attn_bwd_f32": head_attn_bwd,
    "gala_sddvv_f32": sddvv,
    "gala_row_sum_f32": row_sum,
    "gala_row_scale_f32": row_scale,
    "gala_sddmm_dot_f32": sddmm,
    "gala_edge_softmax_fwd_f32": edge_softmax_fwd,
    "gala_edge_softmax_bwd_f32": edge_softmax_bwd,
    "gala_edge_permute_f32": edge_permute,
    "gala_gat_fwd_f32": gat_fwd,
    "gala_gat_bwd_f32": gat_bwd,
    "gala_gat_fwd_attn_f32": gat_fwd_attn,
    "gala_gat_bwd_attn_f32": gat_bwd_attn,
    "gala_gat_fwd_ex_f32": gat_fwd_ex,
    "gala_gat_bwd_ex_f32": gat_bwd_ex,
    "gala_gat_bwd_fused_f32": gat_bwd_fused,
    "gala_gat_fwd_stats_f32": gat_fwd_stats,
    "gala_gat_bwd_stats_f32": gat_bwd_stats,
    "gala_gat_fwd_stats_ex_f32": gat_fwd_stats_ex,
    "gala_gat_bwd_stats_ex_f32": gat_bwd_stats_ex,
    "gala_gat_bwd_stats_linear_f32": gat_bwd_stats_linear,
    "gala_gat_fwd_partial_stats_f32": gat_fwd_partial_stats,
    "gala_gat_fwd_partial_stats_ex_f32": gat_fwd_partial_stats_ex,
    "gala_gat_fwd_continue_f32": gat_fwd_continue,
    "gala_gat_fwd_stats_exact_f32": gat_fwd_stats_exact,
    "gala_gat_bwd_stats_exact_f32": gat_bwd_stats_exact,
    "gala_gat_bwd_stats_exact_t_f32": gat_bwd_stats_exact_t,
    "gala_csr_is_transpose_i32": csr_is_transpose,
    "gala_gat_fwd_stats_exact_ex_f32": gat_fwd_stats_exact_ex,
    "gala_gat_bwd_exact_pre_ex_f32": gat_bwd_exact_pre_ex,
    "gala_gat_bwd_exact_gather_ex_f32": gat_bwd_exact_gather_ex,
    "gala_gat_in_prep_f32": gat_in_prep,
    "gala_gat_in_fwd_f32": lambda: _in_fwd(False, False),
    "gala_gat_in_fwd_t_f32": lambda: _in_fwd(False, True),
    "gala_gat_in_fwd_rect_f32": lambda: _in_fwd(True, False),
    "gala_gat_in_fwd_t_rect_f32": lambda: _in_fwd(True, True),
    "gala_gat_in_q_rect_f32": gat_in_q_rect,
    "gala_gat_in_bwd_f32": lambda: _in_bwd("gala_gat_in_bwd_f32", False, False),
    "gala_gat_in_bwd_t_f32": lambda: _in_bwd("gala_gat_in_bwd_t_f32", False, True),
    "gala_gat_in_bwd_rect_f32": lambda: _in_bwd("gala_gat_in_bwd_rect_f32", True, False),
    "gala_gat_in_q_gather_f32": gat_in_q_gather,
    "gala_gat_in_q_scatter_f32": gat_in_q_scatter,
}

# further cases of an entry point that has one above: paths its first case does not reach
EXTRA_CASES = {
    "gala_dense_grad_f32-n0": dense_grad_empty,
}
ALL_CASES = {**CASES, **EXTRA_CASES}

# which wrapper-less or wrapper-bypassing cases call _abi.call themselves, and why (see each docstring)
DIRECT = ("gala_degree_f32", "gala_dense_grad_f32", "gala_gat_bwd_stats_exact_f32", "gala_gat_bwd_stats_exact_t_f32",
          "gala_csr_is_transpose_i32", "gala_gat_in_bwd_f32", "gala_gat_in_bwd_t_f32", "gala_gat_in_bwd_rect_f32")
