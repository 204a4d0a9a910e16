#!/usr/bin/env python3
"""Where the exact GAT backward's bytes and time go at 1 head, F = 47 (padded rows), against the
REF statistics backward, on the Products-shaped uniform graph.

Run three times under rocprofv3, each pass on its own (counters never together with tracing):

    rocprofv3 --pmc FETCH_SIZE  -d FETCH_DIR --output-format csv -- python3 tools/gat_exact_pmc.py
    rocprofv3 --pmc WRITE_SIZE  -d WRITE_DIR --output-format csv -- python3 tools/gat_exact_pmc.py
    rocprofv3 --kernel-trace    -d TRACE_DIR --output-format csv -- python3 tools/gat_exact_pmc.py
    python3 tools/gat_exact_pmc.py --sum FETCH_DIR WRITE_DIR TRACE_DIR OUT.json

The program launches, once each after one warm-up of each: the REF forward keeping p and the REF
backward from p (what the mirror runs at F <= 64), the exact forward and the exact backward
(pre-pass + gather).  --sum gives per kernel the fetched bytes (FETCH_SIZE x 2 on gfx950, as
tools/pmc_traffic.py), the written bytes and the duration of its last launch.
"""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"ref_fwd": "k_gat_fwd<", "ref_bwd": "k_gat_bwd_fused<", "exact_fwd": "k_gat_exact_fwd<",
           "exact_pre": "k_gat_exact_bwd_pre<", "exact_gather": "k_gat_exact_bwd<"}


def run():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "gala-gnn-acceleration-language_amd"))
    sys.path.insert(0, ROOT)
    import bench
    from gala import ops
    H, F = 1, 47
    hg = bench.products_graph("uniform", 1.0)
    dg = ops.DeviceGraph.from_host(hg)
    N = hg.n_rows
    gen = torch.Generator(device="cuda").manual_seed(4321)
    X = ops.pad_rows(torch.rand((N, F), device="cuda", generator=gen) * 2 - 1)
    dY = ops.pad_rows(torch.rand((N, F), device="cuda", generator=gen) * 2 - 1)
    aL = torch.rand((N, H), device="cuda", generator=gen) * 2 - 1
    aR = torch.rand((N, H), device="cuda", generator=gen) * 2 - 1
    for _ in range(2):
        f = ops.gat_fwd_stats(dg, aL, X, aR=aR, heads=H, want_p=True)
        ops.gat_bwd_stats(dg, aL, aR, dY, f[1], f[0], f[2], f[3], heads=H, p=f[4])
        torch.cuda.synchronize()
        del f
        Y, lse, Ym, sma, ar = ops.gat_fwd_stats_exact(dg, aL, X, aR=aR, heads=H)
        ops.gat_bwd_stats_exact(dg, aL, ar, X, dY, lse, Y, Ym, sma, heads=H, symmetric=True)
        torch.cuda.synchronize()
        del Y, lse, Ym, sma
    print(json.dumps({"rows": N, "edges": int(hg.nnz), "F": F, "heads": H}), flush=True)


def _last(d, pattern, pick):
    """{kernel class: value of its last dispatch} from the CSVs matching `pattern` under d."""
    out = {}
    for fn in glob.glob(os.path.join(d, "**", pattern), recursive=True):
        for r in csv.DictReader(open(fn)):
            v = pick(r)
            if v is None:
                continue
            for name, sub in KERNELS.items():
                if sub in r["Kernel_Name"]:
                    key = int(r.get("Dispatch_Id", 0))
                    if name not in out or key >= out[name][0]:
                        out[name] = (key, v)
    return {k: v[1] for k, v in out.items()}


def summarise(fdir, wdir, tdir, out):
    cnt = lambda name: (lambda r: float(r["Counter_Value"]) if r.get("Counter_Name") == name else None)
    fetch = _last(fdir, "*counter_collection.csv", cnt("FETCH_SIZE"))
    write = _last(wdir, "*counter_collection.csv", cnt("WRITE_SIZE"))
    dur = _last(tdir, "*kernel_trace.csv", lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    N, E, F = 2_449_029, 126_167_309, 48
    res = {"source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE / --kernel-trace, three passes; fetch x2 (gfx950)",
           "shape": {"rows": N, "edges": E, "heads": 1, "F": 47, "row_floats": F},
           "fetch_GB": {k: round(2 * v * 1024 / 1e9, 3) for k, v in fetch.items()},
           "write_GB": {k: round(v * 1024 / 1e9, 3) for k, v in write.items()},
           "ms": {k: round(v, 3) for k, v in dur.items()},
           "model_GB": {"one_row_per_edge": round(4 * E * F / 1e9, 3), "rows_once": round(4 * N * F / 1e9, 3),
                        "p_per_edge": round(4 * E / 1e9, 3), "side_line_per_edge_16B": round(16 * E / 1e9, 3)}}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--sum":
        summarise(*sys.argv[2:6])
    else:
        run()
