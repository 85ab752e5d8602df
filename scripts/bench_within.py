#!/usr/bin/env python
"""Cost of the all-within-radius queries (one GPU, one process, device events).

On the C3 mesh (geodesic icosphere, 1,003,520 faces) and on its vertex cloud (501,762 points) it answers `--rows` rows
uniform in the scene box widened by 10 % per side -- the rows of scripts/bench_knearest.py -- at each radius of `--r`
(0.273: the capped configuration of that script, where the untruncated lists hold thousands of entries per row near the
surface; 0.0327: about 8 faces per row on average, every non-empty row longer than 32; 0.011: no row of the mesh
longer than 32) with
  the counts call   msh_*_within_count_device,
  the list call     msh_*_within_device (id, dist, and for the mesh pt and part; the capacity is the total of the
                    counts), left out at a radius whose total exceeds the 2^32 - 1 entries of one call,
  the yardstick     msh_*_knearest_device at K = 16 and the same radius,
alternating in one session.  Per call: ms (median of `--steps` after `--warmup`) and rows per second; the
per-kernel split of msh_timing_get ("within_count", "within_scan", "within_fill", "within_order", "within_emit"; the
yardstick's "kbest", "kbest_finish"); the per-row counts of msh_tree_within_stats (nodes visited, primitives evaluated,
entries, deepest stack); the total, the mean and the largest count; and on all rows the number of rows whose first entry
differs from the K = 1 answer at the same radius (expected 0).
Prints one JSON line; --out also writes it to a file (profiles/within_<build id>.json).

    python scripts/bench_within.py --out profiles/within_$(python -c \\
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_knearest import knearest_call, timed, uniform_rows  # noqa: E402

NAMES = ["within_count", "within_scan", "within_fill", "within_order", "within_emit", "kbest", "kbest_finish"]


def measure(torch, N, tree, q, r, tri, steps, warmup):
    L, vp = N.lib(), ctypes.c_void_p
    S, dev = q.shape[0], q.device
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    count_fn = L.msh_tree_within_count_device if tri else L.msh_points_within_count_device
    counts = torch.empty(S, dtype=torch.int32, device=dev)
    K = N._sz(0)

    def count_call():
        N.check(count_fn(tree.ptr, vp(q.data_ptr()), S, r, None, vp(counts.data_ptr()), stream))

    # the total decides whether the list call can run at this radius (its offsets are 32-bit) and sizes its outputs
    count_call()
    torch.cuda.synchronize()
    c = counts.long() & 0xFFFFFFFF
    total, longest = int(c.sum().item()), int(c.max().item())
    calls = {"count": count_call}
    listed = total <= 0xFFFFFFFF
    if listed:
        cap = total
        ids = torch.empty(cap, dtype=torch.int32, device=dev)
        dist = torch.empty(cap, dtype=torch.float64, device=dev)
        lcounts = torch.empty(S, dtype=torch.int32, device=dev)
        if tri:
            pt = torch.empty((cap, 3), dtype=torch.float64, device=dev)
            part = torch.empty(cap, dtype=torch.int32, device=dev)

            def list_call():
                N.check(L.msh_tree_within_device(tree.ptr, vp(q.data_ptr()), S, r, None, vp(lcounts.data_ptr()),
                                                 vp(ids.data_ptr()), vp(dist.data_ptr()), vp(pt.data_ptr()),
                                                 vp(part.data_ptr()), cap, ctypes.byref(K), stream))
        else:
            def list_call():
                N.check(L.msh_points_within_device(tree.ptr, vp(q.data_ptr()), S, r, None, vp(lcounts.data_ptr()),
                                                   vp(ids.data_ptr()), vp(dist.data_ptr()), cap, ctypes.byref(K),
                                                   stream))
        calls["list"] = list_call
    yard, _, _ = knearest_call(torch, tree, q, 16, r, tri)
    calls["knearest16"] = yard
    N.timing_reset()
    N.timing_enable(True)
    ms = timed(torch, calls, steps, warmup)
    N.timing_enable(False)
    split = {}
    for name in NAMES:
        t, n = N.timing_get(name)
        split[name + "_ms"] = t / n if n else None
    med = {k: float(np.median(x)) for k, x in ms.items()}
    st = tree.within_stats(q.data_ptr(), S, r)
    out = {"rows": S, "r": r, "entries": total, "mean_count": total / S, "max_count": longest, "list_call": listed,
           "ms": med, "ms_all": ms, "rows_per_s": {k: S / (m * 1e-3) for k, m in med.items()}, "split": split,
           "per_row": {"nodes": st[0] / S, "primitives": st[1] / S, "entries": st[2] / S, "deepest_stack": st[3]}}
    if listed:
        # the first entry of every non-empty row against the K = 1 answer at the same radius
        from mesh_amd.distributed import points_knearest_device, tree_knearest_device
        lc = lcounts.long() & 0xFFFFFFFF
        first = torch.cumsum(lc, 0) - lc
        have = lc > 0
        k_ids = torch.empty((S, 1), dtype=torch.int32, device=dev)
        k_dist = torch.empty((S, 1), dtype=torch.float64, device=dev)
        k_cnt = torch.empty(S, dtype=torch.int32, device=dev)
        if tri:
            tree_knearest_device(tree, q, 1, k_ids, k_dist, None, None, k_cnt, r)
        else:
            points_knearest_device(tree, q, 1, k_ids, k_dist, k_cnt, r)
        torch.cuda.synchronize()
        bad = (k_cnt.long() != torch.clamp(lc, max=1)) | (c != lc)
        at = first[have]
        bad[have] |= (ids[at] != k_ids[have, 0]) | (dist[at] != k_dist[have, 0])
        out["first_entry_mismatches"] = int(bad.sum().item())
        assert K.value == total
    print("[bench_within] %s r=%g: %s, mean count %.2f, longest row %d, first-entry mismatches %s" % (
        "mesh" if tri else "cloud", r, ", ".join("%s %.2f ms" % kv for kv in med.items()), out["mean_count"], longest,
        out.get("first_entry_mismatches")), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--r", type=float, nargs="+", default=[0.273, 0.0327, 0.011])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import workloads as W
    from mesh_amd import _native as N, spatialsearch

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N.set_device(0)
    res = {"build_id": N.build_id(), "steps": args.steps, "warmup": args.warmup}
    v, f = W.c3_mesh()
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.uint32)
    q = uniform_rows(torch, v, args.rows, dev, 1)
    tree = spatialsearch.aabbtree_compute(v, f)
    res["c3_mesh"] = {"faces": int(f.shape[0]), "max_depth": int(tree.info().max_depth),
                      "runs": [measure(torch, N, tree, q, r, True, args.steps, args.warmup) for r in args.r]}
    tree.free()
    N.device_pool_trim()
    torch.cuda.empty_cache()
    cloud = N.build_points(v)
    res["c3_cloud"] = {"points": int(v.shape[0]), "max_depth": int(cloud.info().max_depth),
                       "runs": [measure(torch, N, cloud, q, r, False, args.steps, args.warmup) for r in args.r]}
    cloud.free()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
