"""GPU: every device entry point of the C ABI on a side stream and under HIP-graph capture.

Each function of include/gala_hip.h takes a stream and promises that all its work -- memsets,
workspace passes, the hub rows' launches on the plan's side stream -- is ordered after what the
caller enqueued on that stream before the call and before what it enqueues after it, with no host
synchronisation and no allocation inside.  The other GPU tests call the library on the default
stream and synchronise, where a launch on stream 0, a missing fork or join, or a buffer that is
valid only the first time are all invisible.  The cases are tests/_stream_cases.py's, one per
entry point; the numbers are the other tests' business, only their order is checked here.

Delayed producer, poisoned consumer (test_side_stream_order): the reference is the op on the
default stream.  Then every float operand is NaN; on a side stream a delay, an event, NaN fills of
the outputs and workspaces, the copies of the real inputs, the op, the copies of its outputs and
NaN fills of the inputs are enqueued, and the event must still be pending when the last of them
has been enqueued: the inputs did not exist and the outputs were not yet poisoned when the op was
issued.  A launch on another stream reads NaN or is overwritten; side-stream work that is not
joined misses the copy of its output or reads the NaN fill that follows.

Capture and replay (test_capture_and_replay): the op captured by torch.cuda.graph after a warm-up,
replayed twice on new inputs, against the eager op bit for bit; the second replay is the one that
catches state valid only once.

The delay is torch.cuda._sleep calibrated once per process to DELAY_MS = 200 ms (a chain of matrix
products where the build has no _sleep) and then timed by events.  Measured on the MI355X: the
delay lasts 199.4 ms; enqueueing steps 4.1-4.6 takes 0.05-0.16 ms per ABI case (the longest,
0.16 ms, in the gala_gat_* cases) and at most 0.41 ms for a forward and backward of the operator
mirror (gat_input_layer_apply): the delay outlasts the longest enqueue window about 480 times.

Each of these, made in the library one at a time, turns tests of this file red: dense_grad's
memsets on stream 0 (both tests of gala_dense_grad_f32-n0), row_sum's HubFork::join dropped (both
tests of gala_row_sum_f32), the fork of spmm's hub launch dropped (both tests of gala_spmm_f32 and
gala_spmm_ex_f32).  gat_in_bwd's memset of M on stream 0 changes nothing a caller can see:
k_gat_in_reduce stores every element of M afterwards.
"""
import time

import pytest
import torch

import _stream_cases as S

pytestmark = pytest.mark.gpu
DELAY_MS = 200.0
NAN = float("nan")
_STATE = {}


def calibrate():
    """Once per process, outside every timed window: the delay's length, then the delay itself
    timed by events."""
    if "ready" in _STATE:
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(1_000_000)            # (loads the kernel)
        a.record()
        torch.cuda._sleep(10_000_000)
        b.record()
        b.synchronize()
        _STATE["cycles"] = int(10_000_000 * DELAY_MS / max(a.elapsed_time(b), 1e-3))
    else:
        m = torch.ones(4096, 4096, device="cuda") / 4096
        out = torch.mm(m, m)
        a.record()
        for _ in range(10):
            torch.mm(m, m, out=out)
        b.record()
        b.synchronize()
        _STATE["mm"] = (m, int(10 * DELAY_MS / max(a.elapsed_time(b), 1e-3)) + 1, out)
    _STATE["ready"] = True
    a.record()
    delay()
    b.record()
    b.synchronize()
    _STATE["measured_ms"] = a.elapsed_time(b)
    print(f"delay: {_STATE['measured_ms']:.1f} ms by events ({DELAY_MS:.0f} ms asked)")
    assert _STATE["measured_ms"] > 0.5 * DELAY_MS


@pytest.fixture(scope="module", autouse=True)
def _calibrated():
    calibrate()


def delay():
    """About DELAY_MS of device work on the current stream (calibrate() first)."""
    if "cycles" in _STATE:
        torch.cuda._sleep(_STATE["cycles"])
        return
    m, reps, out = _STATE["mm"]
    for _ in range(reps):
        torch.mm(m, m, out=out)


def poison(ts):
    for t in ts:
        t.fill_(NAN) if t.is_floating_point() else t.fill_(-1)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(got, want, name):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(bits(a), bits(b)), (
            f"{name}: output {k} differs in {int((bits(a) != bits(b)).sum())} of {a.numel()} elements, "
            f"{int(torch.isnan(a).sum()) if a.is_floating_point() else 0} NaN")


def perturbed(stage, seed):
    """New inputs of the same signs and magnitudes (factors in [0.5, 1.5))."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [s * (0.5 + torch.rand(s.shape, device="cuda", generator=gen)) for s in stage]


def load(inputs, values):
    for t, v in zip(inputs, values):
        t.copy_(v)


def written(b):
    """Every buffer the op writes: its outputs and the plans' workspaces."""
    return list(b.outputs) + b.workspaces()


def check_reference(b, want, name):
    """The reference run wrote its outputs: no NaN left of the poison (in part for tables / workspaces)."""
    for k, t in enumerate(want[:len(b.outputs)]):
        if t.is_floating_point() and t.numel():
            nan = torch.isnan(t)
            assert not bool(nan.all()), f"{name}: output {k} not written"
            assert k in b.partial or not bool(nan.any()), f"{name}: output {k} has {int(nan.sum())} NaN"


@pytest.mark.parametrize("name", sorted(S.ALL_CASES))
def test_side_stream_order(name):
    assert S.MODE == "equal"
    b = S.ALL_CASES[name]()
    stage = [t.clone() for t in b.inputs]
    warm = perturbed(stage, 1)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):      # warm-up on s, other inputs: workspaces, modules and s's memory pool
        load(b.inputs, warm)
        b.run()
        results = [torch.empty_like(t) for t in written(b)]
    s.synchronize()
    # 1. the reference on the default stream
    poison(written(b))
    load(b.inputs, stage)
    b.run()
    torch.cuda.synchronize()
    want = [t.clone() for t in written(b)]
    check_reference(b, want, name)
    # 2. nothing valid anywhere
    poison(b.inputs)
    poison(written(b))
    poison(results)
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(s):
        s.synchronize()             # (the allocator's blocks of the reference run are free again)
        t0 = time.perf_counter()
        delay()
        ev.record()
        poison(written(b))
        load(b.inputs, stage)
        b.run()
        outs = written(b)
        assert len(outs) == len(results)
        for r, t in zip(results, outs):
            r.copy_(t)
        poison(b.inputs)
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        pending = not ev.query()
    print(f"{name}: enqueued in {enqueue_ms:.2f} ms, delay {_STATE['measured_ms']:.0f} ms, still pending {pending}")
    assert pending, f"{name}: the delay had ended ({enqueue_ms:.1f} ms of enqueueing): the case proves nothing"
    s.synchronize()
    same(results, want, name)


@pytest.mark.parametrize("name", sorted(S.ALL_CASES))
def test_capture_and_replay(name):
    b = S.ALL_CASES[name]()
    stage = [t.clone() for t in b.inputs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up: workspaces grown outside the capture
        b.run()
    torch.cuda.current_stream().wait_stream(side)
    load(b.inputs, stage)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.run()
    captured = list(b.outputs)
    for seed in (2, 3):
        fresh = perturbed(stage, seed)
        poison(captured + b.workspaces())
        load(b.inputs, fresh)
        graph.replay()
        got = [t.clone() for t in captured + b.workspaces()]
        poison(captured + b.workspaces())
        load(b.inputs, fresh)
        b.run()
        same(got, written(b), f"{name} replay with seed {seed}")
        check_reference(b, got, name)


# ---- the operator mirror (host/gala_torch.cpp) on a side stream ---------------------------------

@pytest.fixture(scope="module")
def E():
    import gala
    return gala.torch_ext()


def _push(E, g, with_transpose):
    from gala import layout
    E.slots_clear()
    off, cols, vals = S.dev(g.rowptr), S.dev(g.col), torch.ones(g.nnz, device="cuda")
    E.slots_push(off, cols, vals, None, 1, False)
    if with_transpose:
        t, perm = layout.transpose(g)
        E.slots_push(S.dev(t.rowptr), S.dev(t.col), torch.ones(t.nnz, device="cuda"), None, 1, False)
        E.slots_set_transpose_perm(1, S.dev(perm))
    else:
        E.slots_push(off, cols, vals, None, 1, False)


def _gcn(E, g):
    _push(E, g, False)
    n = g.n_rows
    bufs = [S.rnd(201, n, 32), S.rnd(202, n, 1, lo=0.5, hi=1.5), S.rnd(203, n, 1, lo=0.5, hi=1.5), S.rnd(204, n, 32)]
    return bufs, [True, False, False], lambda X, pre, post: E.gcn_aggregate_apply(X, pre, post, 0)


def _gat_fixed(E, g):
    _push(E, g, True)
    n, H, F = g.n_rows, 4, 32
    bufs = [S.rnd(211, n, H), S.rnd(212, n, H), S.rnd(213, n, F), S.rnd(214, n, F)]
    return bufs, [True, True, True], lambda aL, aR, X: E.gat_aggregate_apply(aL, aR, X, 0, 0.2, 1)


def _gat_input(E, g):
    _push(E, g, False)
    fin, H, D = S.IN_SHAPE
    n, F = g.n_rows, H * D
    bufs = [S.rnd(221, n, fin), S.rnd(222, F, fin, lo=-0.3, hi=0.3), S.rnd(223, F), S.rnd(224, 1, F), S.rnd(225, H),
            S.rnd(226, 1, F), S.rnd(227, H), S.rnd(228, n, F)]
    assert E.gat_input_layer_eligible(bufs[0], bufs[1], 0, H, 0)
    return bufs, [False] + [True] * 6, lambda x, *params: E.gat_input_layer_apply(x, *params, 0, 0.2, 0, False)


EXT_CASES = {"gcn_aggregate_apply": _gcn, "gat_aggregate_apply-fixed": _gat_fixed, "gat_input_layer_apply": _gat_input}


@pytest.mark.parametrize("name", sorted(EXT_CASES))
def test_extension_on_a_side_stream(E, name):
    """One forward and backward of the mirror's autograd ops on the R-MAT graph, whose plan in the
    mirror (threshold 1024) has hub rows -- so its own aux stream forks and joins -- behind the
    delay on a side stream, the operands poisoned around it as in test_side_stream_order: the
    output and every gradient equal the same step on the default stream bit for bit."""
    import numpy as np
    from gala import layout
    g = S.host_graph("sym")
    assert np.diff(g.rowptr).max() > layout.split_threshold(g.n_rows, g.nnz)
    bufs, needs, fn = EXT_CASES[name](E, g)      # the last buffer is dY
    stage = [t.clone() for t in bufs]

    def step():
        leaves = [t.clone().requires_grad_(r) for t, r in zip(bufs[:-1], needs)]
        Y = fn(*leaves)
        Y.backward(bufs[-1])
        return [Y.detach()] + [t.grad for t, r in zip(leaves, needs) if r]

    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):          # warm-up on s: the mirror's workspaces, s's memory pool
        load(bufs, perturbed(stage, 1))
        results = [torch.empty_like(t) for t in step()]
    s.synchronize()
    load(bufs, stage)
    want = [t.clone() for t in step()]
    torch.cuda.synchronize()
    assert all(t is not None and bool(torch.isfinite(t).all()) for t in want)
    poison(bufs)
    poison(results)
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(s):
        t0 = time.perf_counter()
        delay()
        ev.record()
        load(bufs, stage)
        outs = step()
        for r, t in zip(results, outs):
            r.copy_(t)
        poison(bufs)
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        pending = not ev.query()
    print(f"{name}: enqueued in {enqueue_ms:.2f} ms, delay {_STATE['measured_ms']:.0f} ms, still pending {pending}")
    assert pending, f"{name}: the delay had ended ({enqueue_ms:.1f} ms of enqueueing): the case proves nothing"
    s.synchronize()
    same(results, want, name)
    E.slots_clear()
