"""Development tool: traversal cost model (see bvh_model.cpp).  python tools/bvh_model.py"""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SO = "/tmp/libbvhmodel.so"


def load():
    src = os.path.join(ROOT, "tools", "bvh_model.cpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-shared",
                               os.path.join(ROOT, "tools", "bvh_model.cpp"), "-o", SO])
    return ctypes.CDLL(SO)


def counts(v, f, q, kind=0):
    L = load()
    v = np.ascontiguousarray(v, np.float64)
    f = np.ascontiguousarray(f, np.uint32)
    q = np.ascontiguousarray(q, np.float64)
    S = q.shape[0]
    nn = np.zeros(S, np.uint32)
    nl = np.zeros(S, np.uint32)
    d = ctypes.c_int(0)
    P = ctypes.c_void_p
    L.model_counts(P(v.ctypes.data), P(f.ctypes.data), ctypes.c_int(f.shape[0]), P(q.ctypes.data), ctypes.c_long(S),
                   ctypes.c_int(kind), P(nn.ctypes.data), P(nl.ctypes.data), ctypes.byref(d))
    return nn, nl, d.value


def cut_rule(v, f, q, G, rule, K=7, widen=1.25, subdiv=0):
    """model_cut_rule: per query, nodes loaded and leaf tests of the walk from its cell's start list (k_cut_level's
    expansion; rule 0 the ball rule, 1 with the directional drop, proved on sub-cells down to depth subdiv), the list's
    size, whether it ended stuck, and the directional rule's evaluations while the list was formed."""
    L = load()
    v = np.ascontiguousarray(v, np.float64)
    f = np.ascontiguousarray(f, np.uint32)
    q = np.ascontiguousarray(q, np.float64)
    S = q.shape[0]
    mid, half = 0.5 * (v.max(0) + v.min(0)), 0.5 * (v.max(0) - v.min(0))
    half = widen * np.maximum(half, 0.05 * half.max())
    blo, bhi = np.ascontiguousarray(mid - half), np.ascontiguousarray(mid + half)
    out = [np.zeros(S, np.uint32) for _ in range(5)]
    P = ctypes.c_void_p
    L.model_cut_rule(P(v.ctypes.data), P(f.ctypes.data), ctypes.c_int(f.shape[0]), P(q.ctypes.data), ctypes.c_long(S),
                     P(blo.ctypes.data), P(bhi.ctypes.data), ctypes.c_int(G), ctypes.c_int(K), ctypes.c_int(rule),
                     ctypes.c_int(subdiv), *[P(o.ctypes.data) for o in out])
    return out


def cut_rule_bands(freq=224, n=20000, grids=(200, 400), depths=(0, 1, 2)):
    """python tools/bvh_model.py cut-rule [freq] [rows]: C3's predicted node visits per band of |r - 1| (the bands of
    scripts/cut_shell_probe.py), ball rule against directional rule at each sub-cell depth, one JSON line per grid and
    rule.  "evals": the directional rule's evaluations per cell list (the build's cost)."""
    import json
    import workloads as W
    v, f = W.geodesic_icosphere(freq)
    q = W.c3_stream(n, "cpu").numpy()
    d = np.abs(np.linalg.norm(q, axis=1) - 1.0)
    bands = (0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.4, 10.0)
    for G in grids:
        for rule, depth in [(0, 0)] + [(1, k) for k in depths]:
            nn, nl, size, stuck, ev = cut_rule(v, f, q, G, rule, subdiv=depth)
            rec = {"G": G, "rule": "directional" if rule else "ball", "subdiv": depth, "rows": n,
                   "nodes": float(nn.mean()), "leaves": float(nl.mean()), "entries": float(size.mean()),
                   "stuck": float(stuck.mean()), "evals": float(ev.mean()), "bands": []}
            for lo, hi in zip(bands[:-1], bands[1:]):
                m = (d >= lo) & (d < hi)
                rec["bands"].append({"band": [lo, hi], "frac": float(m.mean()), "nodes": float(nn[m].mean()),
                                     "leaves": float(nl[m].mean()), "entries": float(size[m].mean()),
                                     "stuck": float(stuck[m].mean())})
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    import workloads as W
    if len(sys.argv) > 1 and sys.argv[1] == "cut-rule":
        cut_rule_bands(*(int(x) for x in sys.argv[2:4]))
        sys.exit(0)
    freq = int(sys.argv[1]) if len(sys.argv) > 1 else 224
    v, f = W.geodesic_icosphere(freq)
    q = np.random.default_rng(3).uniform(-1.1, 1.1, (20000, 3))
    for kind in (0, 1):
        nn, nl, d = counts(v, f, q, kind)
        r = np.linalg.norm(q, axis=1)
        print("kind", kind, "depth", d, "nodes avg %.1f p50 %d p99 %d max %d" % (nn.mean(), np.median(nn), np.percentile(nn, 99), nn.max()),
              "leaves avg %.1f" % nl.mean())
        for lo, hi in [(0, 0.2), (0.2, 0.5), (0.5, 0.9), (0.9, 1.1), (1.1, 2)]:
            m = (r >= lo) & (r < hi)
            print("   r in [%.1f,%.1f): n=%d nodes %.0f leaves %.0f" % (lo, hi, m.sum(), nn[m].mean(), nl[m].mean()))
