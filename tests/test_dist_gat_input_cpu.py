"""CPU, world_size 2 and 3 (gloo): gala.dist.HaloGatInput on the host backend.

Every rank fetches the halo's raw input rows once, runs the input-space GAT layer over its table
(prep, the walk forward, the q exchange of its halo rows, the walk backward over the same local
pattern) and all-reduces its partials of M and G.  The gathered row outputs must be BIT-identical
to one rank on the whole graph (HaloGatInput at world 1, comm None); the all-reduced parameter
gradients meet the criteria of tests/test_gat_input_cpu.py and tests/test_gat_input_phases_cpu.py
against the oracle's pass-by-pass REF layer; halo_bytes() is 4 H per halo row.  Launched like
tests/test_dist_cpu.py's ranks (spawn, gloo on a free port, the results through a queue).
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle as orc  # noqa: F401  (the oracle's path, as the helpers below need it)
from gala import dist as gdist
from gala.backend import CpuBackend
from _gat_rect import PARTITIONS, check_grads_against_ref, compose_grads
from _graphs import phase_graph
from test_dist_cpu import _free_port
from test_gat_input_cpu import TOL, layer_inputs, ref_on_own_logits

SHAPE = (37, 4, 16)
ROW_KEYS = ("Y", "Ym", "q", "sma", "daL")
# world -> (bounds, halo layout): 2 over the p2p exchange; 3 (a middle rank with halo rows on both
# sides) over the dense table with one chunk
WORLDS = {2: (PARTITIONS[1][1], "p2p"), 3: (PARTITIONS[2][1], "dense")}


def run_rank(part, inp, comm):
    """One rank's forward_train + backward; numpy row outputs, partials and the halo accounting."""
    X, W, b, wL, bL, wR, bR, dY = (torch.from_numpy(a) for a in inp)
    heads = SHAPE[1]
    layer = gdist.HaloGatInput(part, X[part.r0:part.r0 + part.n].contiguous(), heads, CpuBackend(), comm)
    assert not layer.tmode          # the host has the walk only
    Y = layer.forward_train(None, W, b, wL, bL, wR, bR, relu=True)
    daL, M, (Gw, Gb) = layer.backward(dY[part.r0:part.r0 + part.n].contiguous())
    _, Ym, q, sma, _ = layer.saved
    Yi = layer.forward(None, W, b, wL, bL, wR, bR, relu=True)       # inference: no exchange
    assert torch.equal(Yi, Y)
    rows = {k: v.numpy() for k, v in dict(Y=Y, Ym=Ym, q=q, sma=sma, daL=daL).items()}
    return rows, M, Gw, Gb, layer


def _worker(rank, world, port, out):
    from gala.comm import Comm
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = phase_graph(True)
        bounds, mode = WORLDS[world]
        part = gdist.partition_graph(g, rank, world, bounds=np.asarray(bounds, np.int64), halo_mode=mode)
        inp = layer_inputs(g.n_rows, *SHAPE, seed=sum(SHAPE[:2]))
        rows, M, Gw, Gb, layer = run_rank(part, inp, Comm())
        for t in (M, Gw, Gb):       # the caller's all-reduce of the parameter gradients' partials
            dist.all_reduce(t)
        out.put((rank, rows, M.numpy(), Gw.numpy(), Gb.numpy(), layer.halo_bytes(), part.n_halo_rows,
                 layer.setup_bytes()))
        dist.barrier()              # every rank tears down together (gloo)
    finally:
        dist.destroy_process_group()
    out.close()
    out.join_thread()
    os._exit(0)   # skip library destructors: a gloo rank can abort in one at interpreter exit


@pytest.fixture(scope="module")
def one_rank():
    """World 1 (comm None: every exchange skipped) and the oracle's layer on its logits."""
    g = phase_graph(True)
    inp = layer_inputs(g.n_rows, *SHAPE, seed=sum(SHAPE[:2]))
    part = gdist.partition_graph(g, 0, 1, halo_mode="p2p")
    rows, M, Gw, Gb, layer = run_rank(part, inp, None)
    assert layer.halo_bytes() == 0 and layer.setup_bytes() == 0
    X, W, b, wL, bL, wR, bR, dY = inp
    got = dict(rows, xext=layer.xext.numpy(), **compose_grads(M.numpy(), Gw.numpy(), Gb.numpy(), W, b, wL, wR, SHAPE[1]))
    ref = ref_on_own_logits(g, got, *inp, SHAPE[1], relu=True)
    np.testing.assert_allclose(got["Y"], ref["Y"], **TOL)
    np.testing.assert_allclose(got["daL"], ref["daL"], **TOL)
    check_grads_against_ref(got, ref, X, SHAPE[1])
    return g, inp, got, ref


@pytest.mark.parametrize("world", sorted(WORLDS))
def test_halo_gat_input_matches_one_rank(one_rank, world):
    g, inp, one, ref = one_rank
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted((out.get(timeout=240) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for k in ROW_KEYS:
        assert np.array_equal(np.concatenate([r[1][k] for r in got]), one[k]), k
    X, W, b, wL, bL, wR, bR, dY = inp
    heads = SHAPE[1]
    bounds, mode = WORLDS[world]
    for rank, _, M, Gw, Gb, halo_bytes, n_halo, setup_bytes in got:
        assert np.array_equal(M, got[0][2]) and np.array_equal(Gw, got[0][3])      # all-reduced: the same everywhere
        assert n_halo > 0 and halo_bytes == 4 * heads * n_halo
        if mode == "p2p":
            assert setup_bytes == 4 * SHAPE[0] * n_halo
        grads = compose_grads(M, Gw, Gb, W, b, wL, wR, heads)
        check_grads_against_ref(grads, ref, X, heads)
