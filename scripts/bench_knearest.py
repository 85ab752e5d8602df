#!/usr/bin/env python
"""Cost of the K-nearest / radius-capped walk (one GPU, one process, device events).

On the C3 mesh (geodesic icosphere, 1,003,520 faces) and on its vertex cloud (501,762 points) it answers `--rows` rows
uniform in the scene box widened by 10 % per side with msh_tree_knearest_device (face, dist, pt, part, count) and
msh_points_knearest_device for K in {1, 8, 16, 64} at r_max = inf, and for K = 16 under a cap chosen so that the mean
count is about K / 2 (the median distance to the 8th neighbour of a sample of the rows).  Per configuration: ms per
call (median of `--steps` after `--warmup`), rows per second, the "kbest" / "kbest_finish" split of msh_timing_get, the
per-row counts of msh_tree_knearest_stats (nodes visited, primitives evaluated, list insertions, deepest stack) and
the mean count.  The 1-NN entry point on the same rows is the scale, calls alternating with the K = 1 configuration:
msh_tree_nearest_device for the mesh (with its entry cut), and for the cloud msh_points_nearest, which has only a
host-buffer form, against the host-buffer msh_points_knearest at K = 1 (host clock around calls that end synchronised).
Prints one JSON line; --out also writes it to a file (profiles/knearest_<build id>.json).

    python scripts/bench_knearest.py --out profiles/knearest_$(python -c \\
        "from mesh_amd import _native as N; print(N.build_id())").json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

INF = float("inf")


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


def timed_host(calls, steps, warmup):
    for _ in range(warmup):
        for c in calls.values():
            c()
    ms = {k: [] for k in calls}
    for _ in range(steps):
        for k, c in calls.items():
            t0 = time.perf_counter()
            c()  # host-buffer calls return synchronised
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def knearest_call(torch, tree, q, K, r, tri):
    """the device call of one configuration and its output tensors"""
    from mesh_amd.distributed import points_knearest_device, tree_knearest_device
    S, dev = q.shape[0], q.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    ids = torch.empty((S, K), dtype=torch.int32, device=dev)
    dist = torch.empty((S, K), dtype=torch.float64, device=dev)
    count = torch.empty(S, dtype=torch.int32, device=dev)
    if tri:
        pt = torch.empty((S, K, 3), dtype=torch.float64, device=dev)
        part = torch.empty((S, K), dtype=torch.int32, device=dev)
        return (lambda: tree_knearest_device(tree, q, K, ids, dist, pt, part, count, r, stream=stream)), dist, count
    return (lambda: points_knearest_device(tree, q, K, ids, dist, count, r, stream=stream)), dist, count


def measure(torch, N, tree, q, K, r, tri, steps, warmup, scale=None):
    S = q.shape[0]
    call, dist, count = knearest_call(torch, tree, q, K, r, tri)
    calls = {"knearest": call}
    if scale is not None:
        calls["nearest"] = scale
    N.timing_reset()
    N.timing_enable(True)
    ms = timed(torch, calls, steps, warmup)
    N.timing_enable(False)
    walk, n_walk = N.timing_get("kbest")
    fin, n_fin = N.timing_get("kbest_finish")
    med = float(np.median(ms["knearest"]))
    st = tree.knearest_stats(q.data_ptr(), S, K, r)
    out = {"rows": S, "K": K, "r_max": None if r == INF else r, "ms": med, "ms_all": ms["knearest"],
           "rows_per_s": S / (med * 1e-3), "kbest_ms": walk / max(n_walk, 1), "kbest_finish_ms": fin / max(n_fin, 1),
           "per_row": {"nodes": st[0] / S, "primitives": st[1] / S, "insertions": st[2] / S, "deepest_stack": st[3]},
           "mean_count": float(count.double().mean().item())}
    if scale is not None:
        out["nearest_ms"] = float(np.median(ms["nearest"]))
        out["nearest_ms_all"] = ms["nearest"]
        out["ratio_to_nearest"] = med / out["nearest_ms"]
    del dist, count
    torch.cuda.empty_cache()
    print("[bench_knearest] %s K=%d r_max=%s: %.2f ms" % ("mesh" if tri else "cloud", K, out["r_max"], med),
          file=sys.stderr, flush=True)
    return out


def cap_for(torch, tree, q, K, tri):
    """r_max with a mean count of about K / 2: the median distance to the (K / 2)-th neighbour on a sample of the rows"""
    qs = q[:100000].contiguous()
    call, dist, _ = knearest_call(torch, tree, qs, K, INF, tri)
    call()
    torch.cuda.synchronize()
    return float(dist[:, K // 2 - 1].median().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 8, 16, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import workloads as W
    from mesh_amd import _native as N, spatialsearch
    from mesh_amd.distributed import nearest_device

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N.set_device(0)
    res = {"build_id": N.build_id(), "steps": args.steps, "warmup": args.warmup}
    v, f = W.c3_mesh()
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.uint32)
    q = uniform_rows(torch, v, args.rows, dev, 1)
    S = args.rows
    stream = torch.cuda.current_stream(dev).cuda_stream

    # ---- the mesh ----
    tree = spatialsearch.aabbtree_compute(v, f)
    tree.set_entry_cut(-1)  # the yardstick call's cut; the K-nearest walk does not use it
    face = torch.empty(S, dtype=torch.int32, device=dev)
    part = torch.empty(S, dtype=torch.int32, device=dev)
    pt = torch.empty((S, 3), dtype=torch.float64, device=dev)
    scale = lambda: nearest_device(tree, q, face, part, pt, stream=stream)
    res["c3_mesh"] = {"faces": int(f.shape[0]), "max_depth": int(tree.info().max_depth), "runs": []}
    for K in args.ks:
        res["c3_mesh"]["runs"].append(measure(torch, N, tree, q, K, INF, True, args.steps, args.warmup,
                                              scale if K == 1 else None))
    r = cap_for(torch, tree, q, 16, True)
    res["c3_mesh"]["runs"].append(measure(torch, N, tree, q, 16, r, True, args.steps, args.warmup))
    del face, part, pt
    tree.free()
    N.device_pool_trim()
    torch.cuda.empty_cache()

    # ---- its vertex cloud ----
    cloud = N.build_points(v)
    res["c3_cloud"] = {"points": int(v.shape[0]), "max_depth": int(cloud.info().max_depth), "runs": []}
    for K in args.ks:
        res["c3_cloud"]["runs"].append(measure(torch, N, cloud, q, K, INF, False, args.steps, args.warmup))
    r = cap_for(torch, cloud, q, 16, False)
    res["c3_cloud"]["runs"].append(measure(torch, N, cloud, q, 16, r, False, args.steps, args.warmup))
    # the 1-NN entry point of point trees takes host buffers only: host-buffer calls on both sides
    qh = q.cpu().numpy()
    idx1, dist1 = N.empty_results(((S,), np.uint32), ((S,), np.float64))
    idxk, distk, cntk = N.empty_results(((S, 1), np.uint32), ((S, 1), np.float64), ((S,), np.uint32))
    L = N.lib()
    host = timed_host({
        "points_nearest": lambda: N.check(L.msh_points_nearest(cloud.ptr, N.dptr(qh), S, N.uptr(idx1), N.dptr(dist1))),
        "points_knearest": lambda: N.check(L.msh_points_knearest(cloud.ptr, N.dptr(qh), S, 1, INF, N.uptr(idxk),
                                                                 N.dptr(distk), N.uptr(cntk))),
    }, args.steps, args.warmup)
    a, b = float(np.median(host["points_knearest"])), float(np.median(host["points_nearest"]))
    res["c3_cloud"]["host_k1"] = {"points_knearest_ms": a, "points_nearest_ms": b, "ratio_to_nearest": a / b,
                                  "points_knearest_ms_all": host["points_knearest"],
                                  "points_nearest_ms_all": host["points_nearest"],
                                  "equal": bool(np.array_equal(idxk[:, 0], idx1) and np.array_equal(distk[:, 0], dist1))}
    cloud.free()

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
