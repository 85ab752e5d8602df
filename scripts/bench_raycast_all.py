#!/usr/bin/env python
"""First figures for the all-hits ray queries (one GPU, one process, device events around the _device calls).

On the C5 mesh (bumpy geodesic icosphere, 5,000,000 faces) and the +n halves of C5's nearest_alongnormal rays, o = p and
d = (p + n) - p, `--rows` of them -- case (a) of scripts/bench_raycast.py:
  count     msh_tree_raycast_count_device;
  all       msh_tree_raycast_all_device with pt and side (cap = K, so the whole list is written);
  all_bare  msh_tree_raycast_all_device with t and face alone.
Yardstick: msh_tree_raycast_device (t, face, pt) on the same rays.  The four calls alternate in one session, so drift
hits all alike; per call the median of `--steps` after `--warmup`, rays per second, and the kernels' own time per call
(msh_timing_get: raycast_count, raycast_scan, raycast_fill, raycast_order, raycast_emit).  The list calls include the
read-back of K, which waits for the count pass.  It also records the hits per ray and the longest row.  Prints one JSON
line; --out also writes it to a file (profiles/raycast_all_<build id>.json).

    python scripts/bench_raycast_all.py --out profiles/raycast_all_$(python -c \\
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

from scripts.bench_raycast import timed  # noqa: E402

STAGES = ("raycast_count", "raycast_scan", "raycast_fill", "raycast_order", "raycast_emit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import workloads as W
    from mesh_amd import _native as N, spatialsearch

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N.set_device(0)
    L = N.lib()
    vp = ctypes.c_void_p
    stream = torch.cuda.current_stream(dev).cuda_stream
    v, f = W.c5_mesh()
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.uint32)
    tree = spatialsearch.aabbtree_compute(v, f)
    p, n, _, _ = W.c5_rays(v, f, args.rows, seed=5)
    S = p.shape[0]
    dp, dn = torch.from_numpy(p).to(dev), torch.from_numpy(n).to(dev)
    dd = ((dp + dn) - dp).contiguous()
    del dn
    t1 = torch.empty(S, dtype=torch.float64, device=dev)
    face1 = torch.empty(S, dtype=torch.int32, device=dev)
    pt1 = torch.empty((S, 3), dtype=torch.float64, device=dev)
    counts = torch.empty(S, dtype=torch.int32, device=dev)
    K = N._sz(0)
    o_, d_ = vp(dp.data_ptr()), vp(dd.data_ptr())
    # the size of the list: one counting call (cap = 0, NULL list pointers)
    N.check(L.msh_tree_raycast_all_device(tree.ptr, o_, d_, None, S, vp(counts.data_ptr()), None, None, None, None, 0,
                                          ctypes.byref(K), vp(stream)))
    torch.cuda.synchronize()
    Kf = K.value
    longest = int(counts.max().item())
    hist = torch.bincount(counts.to(torch.int64).clamp(max=8), minlength=9).cpu().tolist()
    tt = torch.empty(max(Kf, 1), dtype=torch.float64, device=dev)
    face = torch.empty(max(Kf, 1), dtype=torch.int32, device=dev)
    pt = torch.empty((max(Kf, 1), 3), dtype=torch.float64, device=dev)
    side = torch.empty(max(Kf, 1), dtype=torch.int8, device=dev)

    def all_call(with_cols):
        N.check(L.msh_tree_raycast_all_device(tree.ptr, o_, d_, None, S, vp(counts.data_ptr()), vp(tt.data_ptr()),
                                              vp(face.data_ptr()), vp(pt.data_ptr()) if with_cols else None,
                                              vp(side.data_ptr()) if with_cols else None, Kf, ctypes.byref(K),
                                              vp(stream)))

    calls = {
        "raycast": lambda: N.check(L.msh_tree_raycast_device(tree.ptr, o_, d_, None, S, vp(t1.data_ptr()),
                                                             vp(face1.data_ptr()), vp(pt1.data_ptr()), None, vp(stream))),
        "count": lambda: N.check(L.msh_tree_raycast_count_device(tree.ptr, o_, d_, None, S, vp(counts.data_ptr()),
                                                                 vp(stream))),
        "all": lambda: all_call(True),
        "all_bare": lambda: all_call(False),
    }
    ms = timed(torch, calls, args.steps, args.warmup)
    res = {"build_id": N.build_id(), "steps": args.steps, "warmup": args.warmup, "faces": int(f.shape[0]),
           "max_depth": int(tree.info().max_depth), "rays": S, "hits": Kf, "hits_per_ray": Kf / S, "longest_row": longest,
           "rows_by_hits_0_to_8plus": hist}
    for k in calls:
        m = float(np.median(ms[k]))
        res[k] = {"ms": m, "ms_all": ms[k], "rays_per_s": S / (m * 1e-3)}
    for k in ("count", "all", "all_bare"):
        res[k]["ms_over_raycast"] = res[k]["ms"] / res["raycast"]["ms"]
    # the kernels' own time, one call of each kind under the timers
    for k in ("raycast", "count", "all", "all_bare"):
        N.timing_reset()
        N.timing_enable(True)
        calls[k]()
        torch.cuda.synchronize()
        N.timing_enable(False)
        names = ("raycast",) if k == "raycast" else STAGES
        res[k]["kernel_ms"] = {nm: N.timing_get(nm)[0] for nm in names if N.timing_get(nm)[1]}
    # the first entry of every non-empty row is the first hit
    st = torch.cumsum(counts.to(torch.int64), 0) - counts.to(torch.int64)
    ne = counts > 0
    all_call(True)
    calls["raycast"]()
    torch.cuda.synchronize()
    res["first_entry_mismatches"] = int(((tt[st[ne]] != t1[ne]) | (face[st[ne]] != face1[ne])).sum().item() +
                                        ((face1 != -1) != ne).sum().item())
    print("[bench_raycast_all] raycast %.2f ms, count %.2f ms, all %.2f ms, all_bare %.2f ms, %.3f hits per ray" % (
        res["raycast"]["ms"], res["count"]["ms"], res["all"]["ms"], res["all_bare"]["ms"], Kf / S), file=sys.stderr,
        flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
