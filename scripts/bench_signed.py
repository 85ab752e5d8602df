#!/usr/bin/env python
"""Cost of the signed-distance path next to the plain closest-point path (one GPU, one process, device events).

For C3 (geodesic icosphere, 1,003,520 faces, bench.py's 100M-row stream, the fine entry cut) and C2 (13,776 faces,
10M near-surface rows) it warms both calls up, then times msh_tree_nearest_device and
msh_tree_signed_distance_device alternately, `--steps` pairs, and reports both medians, their difference (the sign
pass), the sign pass's bytes per row and the bandwidth that implies.  It also times msh_tree_sign_build on the C3
and C5 meshes beside the tree's own build_ms.  Prints one JSON line; --out also writes it to a file
(profiles/signed_distance_<build id>.json).

    python scripts/bench_signed.py --steps 5 --warmup 2 --out profiles/signed_distance_$(python -c \\
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


def pass_bytes_per_row(part):
    """HBM bytes one row of the sign pass asks for: q and point (24 + 24), face and part (4 + 4) streamed in, sdist
    (8) out, and its gathers by part code: fn[face] (24) always; an edge row opp (4) + fn[opp] (24); a vertex row
    f[face][k] (4) + vpn (24) (its fn[face] load is still issued).  Gathers hit in cache where neighbouring rows
    share a face, so this is the request volume, an upper bound on the traffic."""
    cnt = np.bincount(part, minlength=7).astype(np.float64)
    n = cnt.sum()
    edge, vert = cnt[1:4].sum() / n, cnt[4:7].sum() / n
    return {"streamed": 64.0, "gathered": 24.0 + 28.0 * edge + 28.0 * vert, "edge_rows": edge, "vertex_rows": vert}


def time_pair(torch, tree, q, steps, warmup):
    from mesh_amd.distributed import nearest_device, signed_distance_device
    S = q.shape[0]
    dev = q.device
    face = torch.empty(S, dtype=torch.int32, device=dev)
    part = torch.empty(S, dtype=torch.int32, device=dev)
    pt = torch.empty((S, 3), dtype=torch.float64, device=dev)
    sd = torch.empty(S, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    calls = {"nearest": lambda: nearest_device(tree, q, face, part, pt, stream=stream),
             "signed": lambda: signed_distance_device(tree, q, sd, face, part, pt, stream=stream)}
    for _ in range(warmup):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(steps):
        for k, c in calls.items():  # alternating, so drift hits both alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    near, sign = float(np.median(ms["nearest"])), float(np.median(ms["signed"]))
    b = pass_bytes_per_row(part.cpu().numpy().view(np.uint32))
    delta = sign - near
    out = {"rows": S, "nearest_ms": near, "signed_ms": sign, "sign_pass_ms": delta,
           "nearest_ms_all": ms["nearest"], "signed_ms_all": ms["signed"], "sign_pass_bytes_per_row": b,
           "inside_rows": int((sd < 0).sum().item())}
    if delta > 0:
        out["sign_pass_GBps"] = (b["streamed"] + b["gathered"]) * S / (delta * 1e-3) / 1e9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--c3-queries", type=int, default=100_000_000)
    ap.add_argument("--c2-queries", type=int, default=10_000_000)
    ap.add_argument("--skip-c5", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import workloads as W
    from mesh_amd import _native, spatialsearch

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    _native.set_device(0)
    res = {"build_id": _native.build_id(), "steps": args.steps, "warmup": args.warmup}

    # C3: bench.py's mesh, stream and fine cut
    v, f = W.c3_mesh()
    tree = spatialsearch.aabbtree_compute(v, f)
    info = tree.sign_build()
    res["c3_sign_build"] = {"faces": int(f.shape[0]), "vertices": int(v.shape[0]), "sign_build_ms": info["build_ms"],
                            "tree_build_ms": tree.info().build_ms, "bytes": info["bytes"],
                            "counters": [info[k] for k in ("boundary_edges", "nonmanifold_edges",
                                                           "inconsistent_edges", "degenerate_faces")]}
    res["c3_sign_build"]["sign_rebuild_ms"] = tree.sign_build()["build_ms"]  # warm allocations
    tree.set_entry_cut(-1)
    q = W.c3_stream(args.c3_queries, dev)
    res["c3"] = time_pair(torch, tree, q, args.steps, args.warmup)
    res["c3"]["entry_cut"] = tree.entry_cut_info()
    del q
    tree.free()
    _native.device_pool_trim()
    torch.cuda.empty_cache()

    # C2
    v, f = W.c2_mesh()
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.uint32)
    tree = spatialsearch.aabbtree_compute(v, f)
    info = tree.sign_build()
    res["c2_sign_build"] = {"faces": int(f.shape[0]), "sign_build_ms": info["build_ms"],
                            "tree_build_ms": tree.info().build_ms, "bytes": info["bytes"]}
    tree.set_entry_cut(-1)
    q = torch.from_numpy(W.c2_queries(args.c2_queries)).to(dev)
    res["c2"] = time_pair(torch, tree, q, args.steps, args.warmup)
    del q
    tree.free()
    _native.device_pool_trim()
    torch.cuda.empty_cache()

    if not args.skip_c5:
        v, f = W.c5_mesh()
        tree = spatialsearch.aabbtree_compute(np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.uint32))
        info = tree.sign_build()
        res["c5_sign_build"] = {"faces": int(f.shape[0]), "vertices": int(v.shape[0]),
                                "sign_build_ms": info["build_ms"], "sign_rebuild_ms": tree.sign_build()["build_ms"],
                                "tree_build_ms": tree.info().build_ms, "bytes": info["bytes"]}
        tree.free()

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
