#!/usr/bin/env python
"""Cost of the generalised winding number walk (one GPU, one process, device events).

On the C3 mesh (geodesic icosphere, 1,003,520 faces) and the C2 mesh (13,776 faces) it answers `--rows` rows uniform
in the scene box widened by 10 % per side with msh_tree_winding_number_device at the default beta: ms per call
(median of `--steps` after `--warmup`), rows per second, the per-row counts of msh_tree_winding_stats (nodes
approximated, nodes opened, leaves evaluated, deepest stack), the table's bytes and build_ms.  Exact mode (beta = 0)
is timed on C2 only, on `--exact-rows` rows.  msh_tree_nearest_device on the same rows is the scale (calls
alternating).  Prints one JSON line; --out also writes it to a file (profiles/winding_<build id>.json).

`--beta-table` measures instead max |w_beta - w_brute| for beta in {2, 3, 4, 6, 8} on the three approximate-mode
fixtures of tests/test_gpu_winding.py (torus, open torus, ellipsoid; the test's rows and its numpy brute force) with
the per-row counts at each beta: the table MSH_WINDING_BETA_DEFAULT is chosen from.

    python scripts/bench_winding.py --out profiles/winding_$(python -c \\
        "from mesh_amd import _native as N; print(N.build_id())").json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def uniform_rows(torch, v, n, dev, seed):
    lo, hi = torch.from_numpy(v.min(0)).to(dev), torch.from_numpy(v.max(0)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.rand((n, 3), dtype=torch.float64, device=dev, generator=g)
    return (lo - 0.1 * (hi - lo) + u * (1.2 * (hi - lo))).contiguous()


def timed(torch, calls, steps, warmup):
    for _ in range(warmup):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(steps):
        for k, c in calls.items():  # alternating, so drift hits all alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def per_row(counts, S):
    return {"approximated": counts[0] / S, "opened": counts[1] / S, "leaves": counts[2] / S, "deepest_stack": counts[3]}


def measure(torch, tree, q, steps, warmup, beta=None, with_nearest=True):
    from mesh_amd.distributed import nearest_device, winding_number_device
    S, dev = q.shape[0], q.device
    w = torch.empty(S, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    calls = {"winding": lambda: winding_number_device(tree, q, w, beta, stream=stream)}
    if with_nearest:
        face = torch.empty(S, dtype=torch.int32, device=dev)
        part = torch.empty(S, dtype=torch.int32, device=dev)
        pt = torch.empty((S, 3), dtype=torch.float64, device=dev)
        calls["nearest"] = lambda: nearest_device(tree, q, face, part, pt, stream=stream)
    ms = timed(torch, calls, steps, warmup)
    med = float(np.median(ms["winding"]))
    out = {"rows": S, "beta": beta, "winding_ms": med, "winding_ms_all": ms["winding"],
           "rows_per_s": S / (med * 1e-3), "per_row": per_row(tree.winding_stats(q.data_ptr(), S, beta), S),
           "inside_rows": int((w > 0.5).sum().item())}
    if with_nearest:
        out["nearest_ms"] = float(np.median(ms["nearest"]))
        out["nearest_ms_all"] = ms["nearest"]
    return out


def beta_table(torch, dev):
    import tests.test_gpu_winding as T
    from oracle import oracle as O
    O.lib()
    meshes = dict(np.load(os.path.join(ROOT, "tests", "golden", "meshes.npz")))
    res = {}
    for name in ("torus", "open_torus", "ellipsoid"):
        v, f = T.mesh_of(meshes, name)
        q = T.make_rows(O, v, f)
        if name == "ellipsoid":
            q = np.ascontiguousarray(q[:500])
        ref = T.winding_brute(v, f, q)
        tree = T.tree_of(v, f)
        d_q = torch.from_numpy(q).to(dev)
        torch.cuda.synchronize()
        row = {"faces": int(f.shape[0]), "rows": int(q.shape[0]),
               "exact_err": float(np.abs(tree.winding_number(q, beta=0) - ref).max())}
        for beta in (2.0, 3.0, 4.0, 6.0, 8.0):
            err = float(np.abs(tree.winding_number(q, beta=beta) - ref).max())
            row["beta_%g" % beta] = {"max_err": err,
                                     "per_row": per_row(tree.cpp_handle.winding_stats(d_q.data_ptr(), q.shape[0], beta),
                                                        q.shape[0])}
        row["exact_per_row"] = per_row(tree.cpp_handle.winding_stats(d_q.data_ptr(), q.shape[0], 0.0), q.shape[0])
        row["max_depth"] = int(tree.cpp_handle.info().max_depth)
        res[name] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--exact-rows", type=int, default=100_000)
    ap.add_argument("--beta-table", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import workloads as W
    from mesh_amd import _native, spatialsearch

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    _native.set_device(0)
    res = {"build_id": _native.build_id(), "steps": args.steps, "warmup": args.warmup,
           "default_beta": _native.WINDING_BETA_DEFAULT}

    if args.beta_table:
        res["beta_table"] = beta_table(torch, dev)
    else:
        for key, (v, f) in (("c3", W.c3_mesh()), ("c2", W.c2_mesh())):
            v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.uint32)
            tree = spatialsearch.aabbtree_compute(v, f)
            tree.set_entry_cut(-1)  # the yardstick call's cut; the winding walk does not use it
            info = tree.winding_build()
            res[key + "_table"] = dict(info, faces=int(f.shape[0]), tree_build_ms=tree.info().build_ms,
                                       max_depth=int(tree.info().max_depth))
            q = uniform_rows(torch, v, args.rows, dev, 1)
            res[key] = measure(torch, tree, q, args.steps, args.warmup)
            if key == "c2":
                qe = q[:args.exact_rows].contiguous()
                res["c2_exact"] = measure(torch, tree, qe, args.steps, args.warmup, beta=0.0, with_nearest=False)
            del q
            tree.free()
            _native.device_pool_trim()
            torch.cuda.empty_cache()

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
