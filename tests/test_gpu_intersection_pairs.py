"""Triangle-triangle intersection pair lists (msh_tree_intersection_pairs*, msh_tree_self_intersection_pairs* and the
Python layers over them).

The reference is a brute force restated here: for every row, numpy AABB-overlap candidates (closed boxes of the exact
fp64 corners, so no overlapping pair is dropped), then ``oracle.tri_tri_overlap(first, second)`` in the argument order
of the contract -- (query_i, mesh_j) in query mode, (tri_i, tri_j) with i < j in self mode, where pairs sharing an
exactly equal vertex coordinate are skipped.  Self-mode references assert on the way that the predicate is symmetric
on their candidates.  Comparisons are exact, on the whole (K, 2) array and on the counts.
"""
import ctypes

import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module", autouse=True)
def _device():
    from mesh_amd import _native
    _native.set_device(0)


# ---- the reference ----
def _tris(v, f):
    tri = np.ascontiguousarray(v[np.asarray(f).astype(np.int64)])
    return tri, tri.min(axis=1), tri.max(axis=1)


def brute_pairs(O, v, f, qv, qf):
    tri, lo, hi = _tris(v, f)
    qtri, qlo, qhi = _tris(qv, qf)
    out, counts = [], np.zeros(len(qf), np.uint32)
    # rows whose box misses the whole mesh's have no candidates
    near = np.nonzero(np.all(qlo <= hi.max(axis=0), axis=1) & np.all(lo.min(axis=0) <= qhi, axis=1))[0]
    for i in near:
        cand = np.nonzero(np.all(qlo[i] <= hi, axis=1) & np.all(lo <= qhi[i], axis=1))[0]
        for j in cand:
            if O.tri_tri_overlap(qtri[i], tri[j]):
                out.append((i, j))
                counts[i] += 1
    return np.array(out, np.uint32).reshape(-1, 2), counts


def brute_self_pairs(O, v, f):
    tri, lo, hi = _tris(v, f)
    T = len(f)
    ids = np.arange(T)
    out, counts = [], np.zeros(T, np.uint32)
    for i in range(T):
        cand = np.nonzero(np.all(lo[i] <= hi, axis=1) & np.all(lo <= hi[i], axis=1) & (ids > i))[0]
        for j in cand:
            if (tri[i][:, None, :] == tri[j][None, :, :]).all(-1).any():
                continue
            hit = O.tri_tri_overlap(tri[i], tri[j])
            assert hit == O.tri_tri_overlap(tri[j], tri[i]), ("oracle predicate not symmetric", i, j)
            if hit:
                out.append((i, j))
                counts[i] += 1
    return np.array(out, np.uint32).reshape(-1, 2), counts


# ---- inputs ----
def _soup_tris(pts):
    return np.ascontiguousarray(pts, dtype=np.float64), np.arange(len(pts), dtype=np.uint32).reshape(-1, 3)


LONG_TRI = np.array([[-5, -5, .013], [5, -5, .02], [0, 7, -.017]])
ONE_TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
# a triangle through ONE_TRI's interior, one far from it, one that touches it only at its vertex (1, 0, 0)
TINY_Q = np.array([[0.2, 0.2, -1.0], [0.2, 0.2, 1.0], [0.3, 0.6, 0.0],
                   [0.2, 0.2, 5.0], [0.2, 0.9, 5.0], [0.3, 0.6, 6.0],
                   [1.0, 0.0, 0.0], [2.0, 0.0, 1.0], [2.0, 1.0, 1.0]])


def _far_rows(n):
    """n tiny triangles far from everything"""
    base = np.array([[0.0, 0.0, 0.0], [1e-3, 0.0, 0.0], [0.0, 1e-3, 0.0]])
    return np.concatenate([np.zeros((0, 3))] + [base + np.array([100.0 + k, 100.0, 100.0]) for k in range(n)])


def _deep_mesh():
    # the clustered-and-spread mesh of test_gpu_knn_lean.test_deep_stack
    rng = np.random.default_rng(22)
    pts = np.vstack([rng.normal(size=(3000, 3)) * 1e-4, rng.normal(size=(3000, 3)) * 100])
    v = np.repeat(pts, 3, axis=0) + rng.normal(size=(18000, 3)) * 1e-6
    return v, np.arange(18000, dtype=np.uint32).reshape(-1, 3)


def _soup(extra):
    # the soups of test_gpu_parity.test_selfintersects_random
    v = np.random.default_rng(17).normal(size=(600, 3))
    f = np.arange(600, dtype=np.uint32).reshape(-1, 3)
    if extra:
        f = np.vstack([f, np.array([[0, 1, 5], [3, 4, 200]], np.uint32)])
    return v, f


def query_case(name, meshes, ref_tests):
    """(v, f, qv, qf) of a query-mode input"""
    if name == "icospheres":
        t = ref_tests["test_intersections"]
        v, f = meshes["icosphere_v"], meshes["icosphere_f"]
        return (v * t["radius"] + np.array(t["m_center"], float), f, v * t["radius"] + np.array(t["q_center"], float), f)
    if name.startswith("shift"):
        v, f = W.geodesic_icosphere(6)
        return v, f, v * 0.8 + np.array([float(name[5:]), 0.1, -0.05]), f
    if name.startswith("long"):
        v, f = W.geodesic_icosphere(64)
        rows, at = {"long1": (1, 0), "long130": (130, 64), "long600": (600, 599)}[name]
        far = _far_rows(rows - 1)
        qv, qf = _soup_tris(np.concatenate([far[:3 * at], LONG_TRI, far[3 * at:]]))
        return v, f, qv, qf
    if name.startswith("copies"):
        # every leaf overlaps every query (coplanar branch), nothing is pruned
        n = int(name[6:])
        v, f = _soup_tris(np.tile(ONE_TRI, (n, 1)))
        if n == 300:
            return v, f, v, f
        # a row of exactly n hits next to an empty one: n = 32 / 33 is where ordering changes hands
        qv, qf = _soup_tris(np.concatenate([_far_rows(1), TINY_Q[:3]]))
        return v, f, qv, qf
    if name == "deep":
        v, f = _deep_mesh()
        r = np.random.default_rng(5)
        qv, qf = _soup_tris(np.vstack([r.normal(size=(96, 3)) * 3e-4, r.normal(size=(96, 3)) * 150]))
        return v, f, qv, qf
    if name in ("tiny1", "tiny2"):
        if name == "tiny1":
            v, f = _soup_tris(ONE_TRI)
            qv, qf = _soup_tris(TINY_Q)
        else:  # a second triangle far above, and a fourth query through it
            up = np.array([0.0, 0.0, 50.0])
            v, f = _soup_tris(np.concatenate([ONE_TRI, ONE_TRI + up]))
            qv, qf = _soup_tris(np.concatenate([TINY_Q, TINY_Q[:3] + up]))
        return v, f, qv, qf
    raise KeyError(name)


def self_case(name, meshes):
    if name in ("self_intersecting_cyl", "test_doublebox", "cylinder"):
        return meshes[name + "_v"], meshes[name + "_f"]
    if name == "soup200":
        return _soup(False)
    if name == "soup202":
        return _soup(True)
    if name == "copies300":
        return _soup_tris(np.tile(ONE_TRI, (300, 1)))
    raise KeyError(name)


_REF = {}


def query_ref(name, oracle, meshes, ref_tests):
    """inputs and brute-force answer of a query-mode case, computed once"""
    if ("q", name) not in _REF:
        v, f, qv, qf = query_case(name, meshes, ref_tests)
        _REF[("q", name)] = (v, f, qv, qf) + brute_pairs(oracle, v, f, qv, qf)
    return _REF[("q", name)]


def self_ref(name, oracle, meshes):
    if ("s", name) not in _REF:
        v, f = self_case(name, meshes)
        _REF[("s", name)] = (v, f) + brute_self_pairs(oracle, v, f)
    return _REF[("s", name)]


def _check_pairs(got, counts, want, want_counts, what):
    assert got.dtype == np.uint32 and got.ndim == 2 and got.shape[1] == 2, what
    assert counts.dtype == np.uint32 and counts.shape == want_counts.shape, what
    print("%s: K = %d (brute force %d), rows with hits %d, longest row %d" %
          (what, len(got), len(want), np.count_nonzero(counts), counts.max() if counts.size else 0))
    assert np.array_equal(counts, want_counts), what
    assert np.array_equal(got, want), what


QUERY_CASES = ["icospheres", "shift0.3", "shift1.0", "shift3.0", "long1", "long130", "long600", "copies300", "copies32",
               "copies33", "deep", "tiny1", "tiny2"]
SELF_CASES = ["self_intersecting_cyl", "test_doublebox", "cylinder", "soup200", "soup202", "copies300"]


@pytest.mark.parametrize("name", QUERY_CASES)
def test_query_mode_equals_brute_force(name, oracle, meshes, ref_tests):
    from mesh_amd import spatialsearch
    v, f, qv, qf, want, want_counts = query_ref(name, oracle, meshes, ref_tests)
    t = spatialsearch.aabbtree_compute(v, f)
    got, counts = spatialsearch.aabbtree_intersections_pairs(t, qv, qf, return_counts=True)
    _check_pairs(got, counts, want, want_counts, name)
    # the any-hit call is the distinct first column
    assert np.array_equal(np.unique(got[:, 0]), spatialsearch.aabbtree_intersections_indices(t, qv, qf))
    # what each input is there for
    if name == "icospheres":
        assert np.unique(got[:, 0]).tolist() == ref_tests["test_intersections"]["expected"]
    if name == "shift3.0":
        assert got.shape == (0, 2)
    if name.startswith("long"):
        assert np.count_nonzero(counts) == 1 and counts.max() > 256 and np.all(np.diff(got[:, 1].astype(np.int64)) > 0)
    if name.startswith("copies"):
        n = int(name[6:])
        assert counts.max() == n and (n != 300 or (len(got) == 90000 and np.all(counts == 300)))
    if name == "deep":
        assert t.info().max_depth > 16
    if name.startswith("tiny"):
        assert want_counts[0] > 0 and want_counts[1] == 0 and want_counts[2] == 1


@pytest.mark.parametrize("name", SELF_CASES)
def test_self_mode_equals_brute_force(name, oracle, meshes, ref_tests):
    from mesh_amd import aabb_normals, spatialsearch
    v, f, want, want_counts = self_ref(name, oracle, meshes)
    t = spatialsearch.aabbtree_compute(v, f)
    got, counts = spatialsearch.aabbtree_selfintersections_pairs(t, return_counts=True)
    _check_pairs(got, counts, want, want_counts, name)
    assert np.all(got[:, 0] < got[:, 1])
    # a normals-metric handle of the same mesh gives the same bytes, and the any-hit count is the distinct faces
    h = aabb_normals.aabbtree_n_compute(v, f, 0.1)
    got_n, counts_n = aabb_normals.aabbtree_n_selfintersections_pairs(h, return_counts=True)
    assert got_n.tobytes() == got.tobytes() and counts_n.tobytes() == counts.tobytes()
    assert np.unique(got).size == aabb_normals.aabbtree_n_selfintersects(h)
    if name in ref_tests["test_selfintersects"]:
        assert np.unique(got).size == ref_tests["test_selfintersects"][name]
    if name in ("test_doublebox", "cylinder", "copies300"):
        assert got.shape == (0, 2) and not counts.any()
    if name.startswith("soup"):
        assert counts.max() > 64  # rows longer than a wave


def test_methods(oracle, meshes, ref_tests):
    from mesh_amd.mesh import Mesh
    v, f, want, _ = self_ref("self_intersecting_cyl", oracle, meshes)
    m = Mesh(v=v, f=f)
    for got in (m.self_intersection_pairs(), m.compute_aabb_tree().selfintersections_pairs(),
                m.compute_aabb_normals_tree().selfintersections_pairs()):
        assert got.dtype == np.uint32 and np.array_equal(got, want)
    v, f, qv, qf, want, _ = query_ref("icospheres", oracle, meshes, ref_tests)
    got = Mesh(v=v, f=f).compute_aabb_tree().intersections_pairs(qv, qf)
    assert got.dtype == np.uint32 and np.array_equal(got, want)


def test_no_query_faces(meshes):
    from mesh_amd import spatialsearch
    t = spatialsearch.aabbtree_compute(meshes["sphere_v"], meshes["sphere_f"])
    got, counts = spatialsearch.aabbtree_intersections_pairs(t, np.zeros((0, 3)), np.zeros((0, 3), np.uint32),
                                                             return_counts=True)
    assert got.shape == (0, 2) and got.dtype == np.uint32 and counts.shape == (0,)


def _raw_call(t, mode, qv, qf, cap, rows, with_pairs=True):
    """one raw C ABI call -> (status, K, pairs buffer of cap + 8 sentinel-filled rows or None, counts)"""
    from mesh_amd import _native as N
    L = N.lib()
    pairs = np.full((cap + 8, 2), SENTINEL, np.uint32) if with_pairs else None
    counts = np.full(rows, SENTINEL, np.uint32)
    K = ctypes.c_size_t(12345)
    if mode == "query":
        st = L.msh_tree_intersection_pairs(t.ptr, N.dptr(qv), qv.shape[0], N.uptr(qf), qf.shape[0], N.uptr(pairs), cap,
                                           N.uptr(counts), ctypes.byref(K))
    else:
        st = L.msh_tree_self_intersection_pairs(t.ptr, N.uptr(pairs), cap, N.uptr(counts), ctypes.byref(K))
    return st, K.value, pairs, counts


@pytest.mark.parametrize("mode,name", [("query", "shift0.3"), ("self", "soup200")])
def test_cap_protocol(mode, name, oracle, meshes, ref_tests):
    # short rows (ordered by their lanes) and long rows (ordered by the radix sort)
    from mesh_amd import _native as N, spatialsearch
    if mode == "query":
        v, f, qv, qf, want, want_counts = query_ref(name, oracle, meshes, ref_tests)
    else:
        v, f, want, want_counts = self_ref(name, oracle, meshes)
        qv = qf = None
    Kw = len(want)
    assert Kw > 8
    t = spatialsearch.aabbtree_compute(v, f)
    rows = len(want_counts)
    st, K, _, counts = _raw_call(t, mode, qv, qf, 0, rows, with_pairs=False)  # count only
    assert st == N.MSH_OK and K == Kw and np.array_equal(counts, want_counts)
    for cap in (Kw - 1, Kw, Kw + 7, 1):
        st, K, pairs, counts = _raw_call(t, mode, qv, qf, cap, rows)
        n = min(cap, Kw)
        assert st == N.MSH_OK and K == Kw, cap
        assert np.array_equal(pairs[:n], want[:n]), cap
        assert np.all(pairs[n:] == SENTINEL), cap
        assert np.array_equal(counts, want_counts), cap


@pytest.mark.parametrize("mode,name", [("query", "shift0.3"), ("self", "soup200")])
def test_shim_second_call(mode, name, oracle, meshes, ref_tests, monkeypatch):
    from mesh_amd import spatialsearch
    calls = []
    monkeypatch.setattr(spatialsearch, "_first_cap", lambda rows: calls.append(rows) or 1)
    if mode == "query":
        v, f, qv, qf, want, want_counts = query_ref(name, oracle, meshes, ref_tests)
        got, counts = spatialsearch.aabbtree_intersections_pairs(spatialsearch.aabbtree_compute(v, f), qv, qf, True)
    else:
        v, f, want, want_counts = self_ref(name, oracle, meshes)
        got, counts = spatialsearch.aabbtree_selfintersections_pairs(spatialsearch.aabbtree_compute(v, f), True)
    assert calls == [len(want_counts)]
    assert got.flags.owndata and np.array_equal(got, want) and np.array_equal(counts, want_counts)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_device_entry_points(oracle, meshes, ref_tests):
    import torch
    from mesh_amd import _native as N, spatialsearch
    L = N.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    mk = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device="cuda:0")
    for name in ("shift0.3", "copies33"):
        v, f, qv, qf, want, want_counts = query_ref(name, oracle, meshes, ref_tests)
        t = spatialsearch.aabbtree_compute(v, f)
        host, host_counts = spatialsearch.aabbtree_intersections_pairs(t, qv, qf, True)
        d_qv, d_qf = dev(qv), dev(qf.view(np.int32))
        d_pairs, d_counts = mk(len(want) + 4, 2), mk(len(qf))
        K = ctypes.c_size_t(0)
        st = L.msh_tree_intersection_pairs_device(t.ptr, d_qv.data_ptr(), len(qv), d_qf.data_ptr(), len(qf),
                                                  d_pairs.data_ptr(), len(want) + 4, d_counts.data_ptr(),
                                                  ctypes.byref(K), None)
        torch.cuda.synchronize()
        assert st == N.MSH_OK and K.value == len(want)
        assert _u32(d_pairs)[:K.value].tobytes() == host.tobytes() == want.tobytes()
        assert np.all(_u32(d_pairs)[K.value:] == 0xFFFFFFFF)
        assert _u32(d_counts).tobytes() == host_counts.tobytes()
        # a face index >= Pq: found on the device, nothing read out of bounds, and the handle goes on working
        bad = qf.copy()
        bad[len(bad) // 2, 1] = len(qv)
        d_bad = dev(bad.view(np.int32))
        st = L.msh_tree_intersection_pairs_device(t.ptr, d_qv.data_ptr(), len(qv), d_bad.data_ptr(), len(qf),
                                                  d_pairs.data_ptr(), len(want) + 4, None, ctypes.byref(K), None)
        torch.cuda.synchronize()
        assert st == N.MSH_EINVAL and b"out of range" in L.msh_last_error()
        again = spatialsearch.aabbtree_intersections_pairs(t, qv, qf)
        assert again.tobytes() == want.tobytes()
    for name in ("self_intersecting_cyl", "soup202"):
        v, f, want, want_counts = self_ref(name, oracle, meshes)
        t = spatialsearch.aabbtree_compute(v, f)
        d_pairs, d_counts = mk(len(want), 2), mk(len(f))
        K = ctypes.c_size_t(0)
        st = L.msh_tree_self_intersection_pairs_device(t.ptr, d_pairs.data_ptr(), len(want), d_counts.data_ptr(),
                                                       ctypes.byref(K), None)
        torch.cuda.synchronize()
        assert st == N.MSH_OK and K.value == len(want)
        assert _u32(d_pairs).tobytes() == want.tobytes() and _u32(d_counts).tobytes() == want_counts.tobytes()


def test_deterministic_across_calls_and_cut_states(oracle):
    # a mesh large enough for an entry cut (>= 4096 faces), and for more than one block of query rows
    from mesh_amd import _native as N, spatialsearch
    v, f = W.geodesic_icosphere(16)
    qv = v * 0.9 + np.array([0.25, 0.1, -0.05])
    want, want_counts = brute_pairs(oracle, v, f, qv, f)
    t = spatialsearch.aabbtree_compute(v, f)
    N.timing_reset()
    N.timing_enable(True)
    try:
        first, counts = spatialsearch.aabbtree_intersections_pairs(t, qv, f, True)
    finally:
        N.timing_enable(False)
    _check_pairs(first, counts, want, want_counts, "icosphere(16)")
    assert len(first) > 0
    for timer in ("tritri_count", "tritri_scan", "tritri_fill"):
        assert N.timing_get(timer)[1] >= 1, timer
    assert spatialsearch.aabbtree_intersections_pairs(t, qv, f).tobytes() == first.tobytes()
    t.set_entry_cut(0)
    assert spatialsearch.aabbtree_intersections_pairs(t, qv, f).tobytes() == first.tobytes()
    t.set_entry_cut(16)
    spatialsearch.aabbtree_nearest(t, qv[:64])
    assert t.entry_cut_info()["state"] == "built"
    again, counts2 = spatialsearch.aabbtree_intersections_pairs(t, qv, f, True)
    assert again.tobytes() == first.tobytes() and counts2.tobytes() == counts.tobytes()
    self_a = spatialsearch.aabbtree_selfintersections_pairs(t)
    assert self_a.tobytes() == spatialsearch.aabbtree_selfintersections_pairs(t).tobytes()


def test_rejected_handles(oracle, meshes):
    from mesh_amd import _native as N, aabb_normals, spatialsearch
    from mesh_amd.search import AabbTreeBatch
    L = N.lib()
    v, f = meshes["sphere_v"], meshes["sphere_f"]
    K = ctypes.c_size_t(0)
    points = N.build_points(v)
    batch = AabbTreeBatch(np.stack([v, v + 1.0]), f).cpp_handle
    for h in (points, batch):
        with pytest.raises(ValueError):
            spatialsearch.aabbtree_intersections_pairs(h, v, f)
        with pytest.raises(ValueError):
            spatialsearch.aabbtree_selfintersections_pairs(h)
        with pytest.raises(ValueError):
            aabb_normals.aabbtree_n_selfintersections_pairs(h)
        # and by the library itself
        assert L.msh_tree_intersection_pairs(h.ptr, N.dptr(v), len(v), N.uptr(f), len(f), None, 0, None,
                                             ctypes.byref(K)) == N.MSH_EINVAL
        assert L.msh_tree_self_intersection_pairs(h.ptr, None, 0, None, ctypes.byref(K)) == N.MSH_EINVAL
        assert L.msh_tree_self_intersection_pairs_device(h.ptr, None, 0, None, ctypes.byref(K), None) == N.MSH_EINVAL
    # query mode needs a plain triangle tree
    hn = aabb_normals.aabbtree_n_compute(v, f, 0.1)
    assert L.msh_tree_intersection_pairs(hn.ptr, N.dptr(v), len(v), N.uptr(f), len(f), None, 0, None,
                                         ctypes.byref(K)) == N.MSH_EINVAL
    # a query face index out of range is found on the host before any device work
    bad = f.copy()
    bad[3, 0] = len(v)
    with pytest.raises(spatialsearch.Mesh_IntersectionsError, match="references vertex"):
        spatialsearch.aabbtree_intersections_pairs(spatialsearch.aabbtree_compute(v, f), v, bad)
    # a tree with extra faces: no self mode; in query mode j ranges over the main faces, then the extra ones
    cv, cf = meshes["cylinder_v"], meshes["cylinder_f"]
    ev, ef = meshes["cylinder_trans_v"], meshes["cylinder_trans_f"]
    ex = N.build_tree(cv, cf, ev, ef)
    with pytest.raises(ValueError, match="extra faces"):
        spatialsearch.aabbtree_selfintersections_pairs(ex)
    qv, qf = meshes["self_intersecting_cyl_v"], meshes["self_intersecting_cyl_f"]
    got, counts = spatialsearch.aabbtree_intersections_pairs(ex, qv, qf, True)
    allv, allf = np.vstack([cv, ev]), np.vstack([cf, ef + np.uint32(len(cv))])
    want, want_counts = brute_pairs(oracle, allv, allf, qv, qf)
    _check_pairs(got, counts, want, want_counts, "extra faces")
    assert len(want) > 0 and want[:, 1].max() >= len(cf)
