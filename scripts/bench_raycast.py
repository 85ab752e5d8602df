#!/usr/bin/env python
"""Cost of the ray-casting walks against the two ray kernels they generalise (one GPU, one process, device events).

On the C5 mesh (bumpy geodesic icosphere, 5,000,000 faces):
  (a) first hit  msh_tree_raycast_device (t, face, pt) on the +n halves of C5's nearest_alongnormal rays, o = p and
                 d = (p + n) - p, `--rows` of them.  Yardstick: msh_tree_nearest_alongnormal_device on the same (p, n),
                 which casts two rays per row and starts from the entry cut once the handle has built one.
  (b) occlusion  msh_tree_occluded_device on the vertex -> camera rays of the first `--cams` C5 cameras, formed on the
                 device as visibility forms them (dir = (cam - v) / |cam - v|, src = v + min_dist dir, d = (src + dir) -
                 src).  Yardstick: msh_visibility_device for the same cameras, which computes those rays in registers.
The calls of a pair alternate, so drift hits both alike; per call the median of `--steps` after `--warmup`, rays per
second, the kernels' own time (msh_timing_get) and nodes and leaves per ray from the stats entry points.  (b) also
counts the rows on which the two disagree (expected: 0).  Prints one JSON line; --out also writes it to a file
(profiles/raycast_<build id>.json).

    python scripts/bench_raycast.py --out profiles/raycast_$(python -c \\
        "from mesh_amd import _native as N; print(N.build_id())").json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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


def pair(torch, N, calls, timers, steps, warmup):
    """{name: {ms, ms_all, kernel_ms}} of alternating calls; timers: name -> msh_timing_get name"""
    N.timing_reset()
    N.timing_enable(True)
    ms = timed(torch, calls, steps, warmup)
    N.timing_enable(False)
    out = {}
    for k in calls:
        t, n = N.timing_get(timers[k])
        out[k] = {"ms": float(np.median(ms[k])), "ms_all": ms[k], "kernel_ms": t / max(n, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cams", type=int, default=4)
    ap.add_argument("--min-dist", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import workloads as W
    from mesh_amd import _native as N, spatialsearch
    from mesh_amd.distributed import alongnormal_device, visibility_device

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N.set_device(0)
    L = N.lib()
    vp = ctypes.c_void_p
    stream = torch.cuda.current_stream(dev).cuda_stream
    v, f = W.c5_mesh()
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.uint32)
    tree = spatialsearch.aabbtree_compute(v, f)
    res = {"build_id": N.build_id(), "steps": args.steps, "warmup": args.warmup, "faces": int(f.shape[0]),
           "max_depth": int(tree.info().max_depth)}
    nodes, leaves = ctypes.c_uint64(0), ctypes.c_uint64(0)

    # ---- (a) first hit on the +n halves of the alongnormal rays ----
    p, n, _, _ = W.c5_rays(v, f, args.rows, seed=5)
    S = p.shape[0]
    dp, dn = torch.from_numpy(p).to(dev), torch.from_numpy(n).to(dev)
    dd = ((dp + dn) - dp).contiguous()
    t = torch.empty(S, dtype=torch.float64, device=dev)
    face = torch.empty(S, dtype=torch.int32, device=dev)
    pt = torch.empty((S, 3), dtype=torch.float64, device=dev)
    dist = torch.empty(S, dtype=torch.float64, device=dev)
    aface = torch.empty(S, dtype=torch.int32, device=dev)
    apt = torch.empty((S, 3), dtype=torch.float64, device=dev)
    calls = {
        "raycast": lambda: N.check(L.msh_tree_raycast_device(tree.ptr, vp(dp.data_ptr()), vp(dd.data_ptr()), None, S,
                                                             vp(t.data_ptr()), vp(face.data_ptr()), vp(pt.data_ptr()),
                                                             None, vp(stream))),
        "alongnormal": lambda: alongnormal_device(tree, dp, dn, dist, aface, apt, stream=stream),
    }
    a = pair(torch, N, calls, {"raycast": "raycast", "alongnormal": "alongnormal"}, args.steps, args.warmup)
    n1, l1 = tree.raycast_stats(dp.data_ptr(), dd.data_ptr(), S)
    N.check(L.msh_tree_nearest_alongnormal_stats(tree.ptr, dp.data_ptr(), dn.data_ptr(), S, ctypes.byref(nodes),
                                                 ctypes.byref(leaves)))
    a["raycast"].update(rays=S, rays_per_s=S / (a["raycast"]["ms"] * 1e-3), nodes_per_ray=n1 / S, leaves_per_ray=l1 / S,
                        hits=int((face != -1).sum().item()))
    a["alongnormal"].update(rows=S, rays=2 * S, rows_per_s=S / (a["alongnormal"]["ms"] * 1e-3),
                            rays_per_s=2 * S / (a["alongnormal"]["ms"] * 1e-3), nodes_per_row=nodes.value / S,
                            leaves_per_row=leaves.value / S, entry_cut=tree.entry_cut_info()["state"])
    a["rows_per_s_ratio"] = a["alongnormal"]["ms"] / a["raycast"]["ms"]
    res["first_hit"] = a
    print("[bench_raycast] first hit %.2f ms, alongnormal %.2f ms" % (a["raycast"]["ms"], a["alongnormal"]["ms"]),
          file=sys.stderr, flush=True)
    del dp, dn, dd, t, face, pt, dist, aface, apt
    torch.cuda.empty_cache()

    # ---- (b) occlusion on the vertex -> camera rays of a few cameras ----
    cams = W.fibonacci_cameras(64, 3.0)[:args.cams]
    C, P = cams.shape[0], v.shape[0]
    dc, dv = torch.from_numpy(np.ascontiguousarray(cams)).to(dev), torch.from_numpy(v).to(dev)
    dirs = dc[:, None, :] - dv[None, :, :]  # (C, P, 3), camera-major like vis
    ln = torch.sqrt((dirs[..., 0] * dirs[..., 0] + dirs[..., 1] * dirs[..., 1]) + dirs[..., 2] * dirs[..., 2])
    dirs = dirs / ln[..., None]
    src = (dv[None, :, :] + args.min_dist * dirs).reshape(-1, 3).contiguous()
    dd = ((src + dirs.reshape(-1, 3)) - src).contiguous()
    del dirs, ln
    R = C * P
    hit = torch.empty(R, dtype=torch.uint8, device=dev)
    vis = torch.empty((C, P), dtype=torch.int32, device=dev)
    ndc = torch.empty((C, P), dtype=torch.float64, device=dev)
    calls = {
        "occluded": lambda: N.check(L.msh_tree_occluded_device(tree.ptr, vp(src.data_ptr()), vp(dd.data_ptr()), None, R,
                                                               vp(hit.data_ptr()), vp(stream))),
        "visibility": lambda: visibility_device(tree, dc, vis, ndc, min_dist=args.min_dist, stream=stream),
    }
    b = pair(torch, N, calls, {"occluded": "occluded", "visibility": "visibility"}, args.steps, args.warmup)
    n2, l2 = tree.raycast_stats(src.data_ptr(), dd.data_ptr(), R, any_hit=True)
    N.check(L.msh_visibility_stats(tree.ptr, dc.data_ptr(), C, args.min_dist, ctypes.byref(nodes), ctypes.byref(leaves)))
    b["occluded"].update(rays=R, rays_per_s=R / (b["occluded"]["ms"] * 1e-3), nodes_per_ray=n2 / R,
                         leaves_per_ray=l2 / R, occluded=int(hit.sum().item()))
    b["visibility"].update(rays=R, rays_per_s=R / (b["visibility"]["ms"] * 1e-3), nodes_per_ray=nodes.value / R,
                           leaves_per_ray=leaves.value / R)
    b["rays_per_s_ratio"] = b["visibility"]["ms"] / b["occluded"]["ms"]
    b["disagreements"] = int(((hit.reshape(C, P) != 0) != (vis == 0)).sum().item())
    b["cameras"] = C
    res["occlusion"] = b
    print("[bench_raycast] occluded %.2f ms, visibility %.2f ms" % (b["occluded"]["ms"], b["visibility"]["ms"]),
          file=sys.stderr, flush=True)

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
