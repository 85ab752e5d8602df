#!/usr/bin/env python
"""Cost of the intersection pair lists next to the any-hit calls on the same inputs (one GPU, one process).

Three runs, each timed with msh_timing_get (device events around the launches) after one warm-up call, `--reps` calls
per round, the pair-list call and the any-hit call alternating over two rounds:
  a. C2's 13,776-face mesh in self mode (aabbtree_n_selfintersections_pairs against aabbtree_n_selfintersects);
  b. C2 against a copy scaled 0.97 and shifted 2 cm, query mode (aabbtree_intersections_pairs against
     aabbtree_intersections_indices);
  c. 300 copies of one triangle against themselves, 90,000 coplanar pairs: one msh_tree_intersection_pairs call with
     cap = K, and the Python shim, whose first guess at the capacity is too small here (two library calls).
Per run: K, the time under each timer (tritri_count, tritri_scan, tritri_fill, tritri_order, and the any-hit call's
tritri), and the ratio of the pair list's GPU time to the any-hit call's.  Prints one line per run; --out also writes
the record to a file (profiles/intersection_pairs_<build id>.json).

    python scripts/bench_pairs.py --out profiles/intersection_pairs_$(python -c \\
        "from mesh_amd import _native as N; print(N.build_id())").json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TIMERS = ["tritri_count", "tritri_scan", "tritri_fill", "tritri_order", "sort", "tritri"]


def timed(N, fn, reps):
    fn()  # warm-up
    N.timing_reset()
    N.timing_enable(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    wall = (time.perf_counter() - t0) / reps * 1e3
    N.timing_enable(False)
    t = {}
    for name in TIMERS:
        ms, n = N.timing_get(name)
        if n:
            t[name] = {"ms_per_call": ms / reps, "launches_per_call": n / reps}
    t["wall_ms_per_call"] = wall
    return out, t


def run(N, name, pairs_fn, anyhit_fn, reps):
    rounds = []
    for _ in range(2):
        pairs, tp = timed(N, pairs_fn, reps)
        _, ta = timed(N, anyhit_fn, reps)
        rounds.append({"pairs": tp, "anyhit": ta})
    # "sort" runs inside "tritri_order": not added again
    gpu_pairs = [sum(v["ms_per_call"] for k, v in r["pairs"].items() if k.startswith("tritri_")) for r in rounds]
    gpu_any = [r["anyhit"]["tritri"]["ms_per_call"] for r in rounds]
    res = {"K": int(len(pairs)), "rounds": rounds, "pairs_gpu_ms": gpu_pairs, "anyhit_gpu_ms": gpu_any,
           "ratio": [p / a for p, a in zip(gpu_pairs, gpu_any)]}
    print(name, json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import workloads as W
    from mesh_amd import _native as N, aabb_normals, spatialsearch
    if N.device_count() < 1:
        raise RuntimeError("bench_pairs: no HIP device visible")
    N.set_device(0)
    out = {"build_id": N.build_id(), "reps": args.reps, "runs": {}}
    v, f = W.c2_mesh()
    f = np.ascontiguousarray(f, dtype=np.uint32)
    h = aabb_normals.aabbtree_n_compute(v, f, 0.1)
    out["runs"]["a_c2_self"] = run(N, "a", lambda: aabb_normals.aabbtree_n_selfintersections_pairs(h),
                                   lambda: aabb_normals.aabbtree_n_selfintersects(h), args.reps)
    t = spatialsearch.aabbtree_compute(v, f)
    qv = v * 0.97 + np.array([0.02, 0.0, 0.0])
    out["runs"]["b_c2_vs_copy"] = run(N, "b", lambda: spatialsearch.aabbtree_intersections_pairs(t, qv, f),
                                      lambda: spatialsearch.aabbtree_intersections_indices(t, qv, f), args.reps)
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    cv = np.ascontiguousarray(np.tile(tri, (300, 1)))
    cf = np.arange(900, dtype=np.uint32).reshape(-1, 3)
    tc = spatialsearch.aabbtree_compute(cv, cf)
    c_pairs = np.empty((90000, 2), np.uint32)
    c_K = ctypes.c_size_t(0)

    def c_raw():
        N.check(N.lib().msh_tree_intersection_pairs(tc.ptr, N.dptr(cv), len(cv), N.uptr(cf), len(cf), N.uptr(c_pairs),
                                                    90000, None, ctypes.byref(c_K)))
        assert c_K.value == 90000
        return c_pairs

    anyhit_c = lambda: spatialsearch.aabbtree_intersections_indices(tc, cv, cf)
    out["runs"]["c_copies300"] = run(N, "c", c_raw, anyhit_c, args.reps)
    out["runs"]["c_copies300_shim_two_calls"] = run(N, "c2", lambda: spatialsearch.aabbtree_intersections_pairs(tc, cv, cf),
                                                    anyhit_c, args.reps)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
