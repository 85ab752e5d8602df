"""K-nearest and radius-capped queries on point trees and plain triangle trees (msh_points_knearest, msh_tree_knearest,
their *_device forms, msh_tree_knearest_stats and the Python layers over them).

Every comparison is bit-exact against brute force, with no row left out.
  points     numpy fp64 d2 = (dx*dx + dy*dy) + dz*dz per (row, point), np.lexsort by (d2, index), np.sqrt;
  triangles  oracle.brute_nearest(v, f[t:t+1], q) once per face t gives d2, point and part of every row against that
             face by the pinned construction; then lexsort by (d2, t).
The brute force of a case is computed once at the largest K; the answer for a smaller K is by definition its first K
columns (the first min(K, m) of the qualifying primitives in key order)."""
import ctypes
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NO_FACE = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def _device():
    from mesh_amd import _native
    _native.set_device(0)


def golden(meshes, name):
    return np.ascontiguousarray(meshes[name + "_v"], np.float64), np.ascontiguousarray(meshes[name + "_f"], np.uint32)


# ---- the references ----
def select(d2, K, r_max):
    """per row of the (S, n) matrix d2: the ids of the first min(K, m) entries with d2 <= r2 by (d2, id), and m"""
    S, n = d2.shape
    r2 = np.float64(r_max) * np.float64(r_max)
    ids = np.full((S, K), n, np.int64)
    m = np.zeros(S, np.int64)
    for i in range(S):
        ok = np.nonzero(d2[i] <= r2)[0]  # NaN (a non-finite row) never qualifies
        m[i] = ok.size
        if ok.size > K:  # everything up to the K-th smallest d2, ties included; the lexsort cuts through them
            ok = ok[d2[i, ok] <= np.partition(d2[i, ok], K - 1)[K - 1]]
        o = ok[np.lexsort((ok, d2[i, ok]))][:K]
        ids[i, :o.size] = o
    return ids, m


def point_d2(v, q):
    with np.errstate(invalid="ignore"):
        dx, dy, dz = (q[:, None, k] - v[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
    d2[~np.isfinite(q).all(1)] = np.nan  # a row with a non-finite coordinate has no neighbours
    return d2


def brute_points(v, q, K, r_max=INF):
    """(idx (S,K) u32, dist (S,K), count (S,), m (S,)) with the specified padding"""
    d2 = point_d2(v, q)
    ids, m = select(d2, K, r_max)
    have = ids < v.shape[0]
    idx = np.where(have, ids, NO_FACE).astype(np.uint32)
    dist = np.where(have, np.sqrt(np.take_along_axis(d2, np.minimum(ids, v.shape[0] - 1), 1)), np.inf)
    return idx, dist, np.minimum(m, K).astype(np.uint32), m


def face_table(oracle, v, f, q):
    """d2 (S,T), part (S,T), pt (S,T,3) of every row against every face, one oracle call per face"""
    cols = [oracle.brute_nearest(v, f[t:t + 1], q, threads=1) for t in range(f.shape[0])]
    return (np.stack([c[3] for c in cols], 1), np.stack([c[1] for c in cols], 1), np.stack([c[2] for c in cols], 1))


def brute_faces(table, K, r_max=INF):
    d2, part, pt = table
    T = d2.shape[1]
    ids, m = select(d2, K, r_max)
    have = ids < T
    g = np.minimum(ids, T - 1)
    face = np.where(have, ids, NO_FACE).astype(np.uint32)
    dist = np.where(have, np.sqrt(np.take_along_axis(d2, g, 1)), np.inf)
    prt = np.where(have, np.take_along_axis(part, g, 1), 0).astype(np.uint32)
    p = np.where(have[..., None], np.take_along_axis(pt, g[..., None], 1), np.nan)
    return face, prt, p, dist, m


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def check_points(h, v, q, Ks, r_max=INF):
    from mesh_amd import spatialsearch
    full = brute_points(v, q, max(Ks), r_max)
    for K in Ks:
        idx, dist, count = spatialsearch.points_nearest_k(h, q, K, r_max)
        assert same(idx, np.ascontiguousarray(full[0][:, :K])), K
        assert same(dist, np.ascontiguousarray(full[1][:, :K])), K
        assert same(count, np.minimum(full[3], K).astype(np.uint32)), K
        # the padding, stated on its own
        pad = np.arange(K)[None, :] >= count[:, None]
        assert (idx[pad] == NO_FACE).all() and np.isposinf(dist[pad]).all() and np.isfinite(dist[~pad]).all()
    return full


# ---- 1. point trees against brute force ----
CLOUD_SIZES = [1, 2, 7, 8, 9, 65, 1000]
# P < K, the boundaries of the list variants (registers 1, LDS 8 and 16, memory beyond), the maximum
POINT_KS = [1, 2, 8, 9, 16, 17, 64]


def cloud(P):
    rng = np.random.default_rng(100 + P)
    v = rng.uniform(0.0, 1.0, (P, 3))
    q = rng.uniform(-0.2, 1.2, (257, 3))  # 257 rows: a ragged last wave and a ragged block
    return v, q


@pytest.mark.parametrize("P", CLOUD_SIZES)
def test_points_against_brute_force(P):
    from mesh_amd import _native as N, spatialsearch
    v, q = cloud(P)
    h = N.build_points(v)
    check_points(h, v, q, POINT_KS)
    # column 0 of the K answers is msh_points_nearest bit for bit
    idx1 = np.empty(q.shape[0], np.uint32)
    dist1 = np.empty(q.shape[0])
    N.check(N.lib().msh_points_nearest(h.ptr, N.dptr(q), q.shape[0], N.uptr(idx1), N.dptr(dist1)))
    for K in (1, 9):
        idx, dist, _ = spatialsearch.points_nearest_k(h, q, K)
        assert same(np.ascontiguousarray(idx[:, 0]), idx1) and same(np.ascontiguousarray(dist[:, 0]), dist1)


# ---- 2. ties ----
def lattice(n=6):
    g = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


@pytest.mark.parametrize("copies", [1, 3])
def test_ties_are_decided_by_id(copies):
    from mesh_amd import _native as N
    lat = lattice()
    v = np.ascontiguousarray(np.concatenate([lat] * copies))  # equal coordinates, different ids
    centres = lattice(5) + 0.5  # 8-way ties (24-way with three copies)
    q = np.ascontiguousarray(np.concatenate([centres, lat]))  # lattice rows: d2 = 0, then 6-way ties
    h = N.build_points(v)
    full = check_points(h, v, q, [3, 8, 9, 17])
    # K cuts through tie groups: a centre's ranks 0..7 all lie at d2 = 3/4, and the ids ascend within the group
    nc = centres.shape[0]
    assert (full[1][:nc, :8] == np.sqrt(0.75)).all()
    assert (np.diff(full[0][:nc, :8].astype(np.int64), axis=1) > 0).all()
    assert (full[1][nc:, 0] == 0.0).all()


# ---- 3. the radius cap ----
def test_radius_cap():
    from mesh_amd import _native as N, spatialsearch
    v, q = cloud(1000)
    q = np.random.default_rng(3).uniform(-0.3, 1.3, (257, 3))
    h = N.build_points(v)
    K, r = 8, 0.13
    full = check_points(h, v, q, [K, 1, 64], r)
    assert (full[3] == 0).any() and (full[3] > K).any()  # rows with nothing in range, rows with more than K
    # r_max = 0: exact hits only
    rows = np.ascontiguousarray(v[::7])
    idx, dist, count = spatialsearch.points_nearest_k(h, rows, 4, 0.0)
    assert (count >= 1).all() and (dist[:, 0] == 0.0).all() and (idx[:, 0] == np.arange(0, 1000, 7)).all()
    check_points(h, v, rows, [4], 0.0)
    idx, dist, count = spatialsearch.points_nearest_k(h, rows + 1e-9, 4, 0.0)
    assert (count == 0).all() and (idx == NO_FACE).all() and np.isposinf(dist).all()


def test_kth_neighbour_exactly_on_the_cap():
    from mesh_amd import _native as N, spatialsearch
    v = lattice()
    h = N.build_points(v)
    q = np.array([[2.0, 2.0, 2.0]])
    # r2 = 1 exactly: the point itself and its 6 axis neighbours at d2 == r2
    idx, dist, count = spatialsearch.points_nearest_k(h, q, 7, 1.0)
    assert count[0] == 7 and dist[0, 0] == 0.0 and (dist[0, 1:] == 1.0).all()
    idx, dist, count = spatialsearch.points_nearest_k(h, q, 8, 1.0)
    assert count[0] == 7 and idx[0, 7] == NO_FACE and np.isposinf(dist[0, 7])
    # r2 = 4: 1 + 6 + 12 + 8 + 6 lattice points at d2 = 0, 1, 2, 3, 4
    for K in (33, 64):
        idx, dist, count = spatialsearch.points_nearest_k(h, q, K, 2.0)
        assert count[0] == 33 and dist[0, 32] == 2.0
    check_points(h, v, np.ascontiguousarray(np.concatenate([q, lattice(5) + 0.5])), [7, 33, 64], 2.0)


def test_non_finite_rows():
    from mesh_amd import _native as N, spatialsearch
    v, q = cloud(1000)
    q = q.copy()
    q[3, 1] = np.nan
    q[64, 0] = np.inf
    q[256, 2] = -np.inf
    h = N.build_points(v)
    for K in (1, 8, 16):
        for r in (INF, 0.2):
            idx, dist, count = spatialsearch.points_nearest_k(h, q, K, r)
            for i in (3, 64, 256):
                assert count[i] == 0 and (idx[i] == NO_FACE).all() and np.isposinf(dist[i]).all()
    check_points(h, v, q, [8, 16])


# ---- 4. triangle trees ----
TRI_MESHES = ["sphere", "test_doublebox", "icosphere"]
_tables = {}


def tri_case(meshes, oracle, name):
    """mesh, rows and the (row, face) table, computed once per mesh"""
    if name not in _tables:
        v, f = golden(meshes, name)
        rng = np.random.default_rng(5)
        lo, hi = v.min(0), v.max(0)
        j = rng.choice(v.shape[0], min(40, v.shape[0]), replace=False)
        uni = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (200 - 2 * j.size, 3))
        far = lo - 10.0 * (hi - lo) * np.array([[1.0, 0.5, 0.25], [0.25, 1.0, 2.0]])  # far outside: nothing under a cap
        q = np.ascontiguousarray(np.concatenate([uni, 1.5 * v[j], 0.5 * v[j], far]))
        _tables[name] = (v, f, q, face_table(oracle, v, f, q))
    return _tables[name]


@pytest.mark.parametrize("name", TRI_MESHES)
def test_triangles_against_brute_force(meshes, oracle, name):
    from mesh_amd import spatialsearch
    v, f, q, table = tri_case(meshes, oracle, name)
    # rows along a vertex direction see every face around the vertex at the same exact d2
    s = np.sort(table[0], 1)
    assert ((s[:, :5] == s[:, :1]).all(1)).any(), "no row with a 5-way exact d2 tie"
    t = spatialsearch.aabbtree_compute(v, f)
    full = brute_faces(table, 24)
    got = {}
    for K in (1, 6, 16, 24):  # 24: the list in memory (and more than test_doublebox's 20 faces)
        face, part, pt, dist = got[K] = spatialsearch.aabbtree_nearest_k(t, q, K)
        assert same(face, np.ascontiguousarray(full[0][:, :K])), K
        assert same(dist, np.ascontiguousarray(full[3][:, :K])), K
        assert same(pt, np.ascontiguousarray(full[2][:, :K])), K
        assert same(part, np.ascontiguousarray(full[1][:, :K])), K
    # column 0 is aabbtree_nearest bit for bit
    face1, part1, pt1 = spatialsearch.aabbtree_nearest(t, q)
    for K in (1, 6):
        face, part, pt, dist = got[K]
        assert np.array_equal(face[:, 0], face1[0]) and np.array_equal(part[:, 0], part1[0])
        assert np.array_equal(pt[:, 0], pt1)
    # K = 6 is a prefix of K = 16
    for a, b in zip(got[6], got[16]):
        assert np.array_equal(a, b[:, :6], equal_nan=True)
    # with a cap: against brute force again, and the rows far outside get nothing
    r = 0.08 * float(np.linalg.norm(v.max(0) - v.min(0)))
    capped = brute_faces(table, 6, r)
    face, part, pt, dist = spatialsearch.aabbtree_nearest_k(t, q, 6, r)
    assert same(face, capped[0]) and same(part, capped[1]) and same(pt, capped[2]) and same(dist, capped[3])
    assert (capped[4] > 0).any()
    assert (face[-2:] == NO_FACE).all() and np.isposinf(dist[-2:]).all() and np.isnan(pt[-2:]).all()
    assert (part[-2:] == 0).all()


# ---- 5. one primitive ----
def test_one_primitive(oracle):
    from mesh_amd import _native as N, spatialsearch
    q = np.random.default_rng(8).uniform(-1.0, 2.0, (257, 3))
    v = np.array([[0.25, 0.5, 0.75]])
    check_points(N.build_points(v), v, q, [4])
    tv = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.2], [0.2, 1.0, 0.5]])
    tf = np.array([[0, 1, 2]], np.uint32)
    t = spatialsearch.aabbtree_compute(tv, tf)
    full = brute_faces(face_table(oracle, tv, tf, q), 4)
    face, part, pt, dist = spatialsearch.aabbtree_nearest_k(t, q, 4)
    assert same(face, full[0]) and same(part, full[1]) and same(pt, full[2]) and same(dist, full[3])
    assert (face[:, 0] == 0).all() and (face[:, 1:] == NO_FACE).all()


# ---- 6. prefix and independence ----
def _dev_points(h, q, K, r=INF, count=True):
    import torch
    from mesh_amd import distributed
    S = q.shape[0]
    d_q = torch.from_numpy(q).to("cuda:0")
    d_idx = torch.full((S, K), 7, dtype=torch.int32, device="cuda:0")
    d_dist = torch.full((S, K), -7.0, dtype=torch.float64, device="cuda:0")
    d_cnt = torch.full((S,), 77, dtype=torch.int32, device="cuda:0") if count else None
    distributed.points_knearest_device(h, d_q, K, d_idx, d_dist, d_cnt, r)
    torch.cuda.synchronize()
    return (d_idx.cpu().numpy().view(np.uint32), d_dist.cpu().numpy(),
            d_cnt.cpu().numpy().view(np.uint32) if count else None)


def _dev_faces(t, q, K, r=INF, pt=True, part=True, count=True):
    import torch
    from mesh_amd import distributed
    S = q.shape[0]
    d_q = torch.from_numpy(q).to("cuda:0")
    d_face = torch.full((S, K), 7, dtype=torch.int32, device="cuda:0")
    d_dist = torch.full((S, K), -7.0, dtype=torch.float64, device="cuda:0")
    d_pt = torch.full((S, K, 3), -7.0, dtype=torch.float64, device="cuda:0") if pt else None
    d_part = torch.full((S, K), 7, dtype=torch.int32, device="cuda:0") if part else None
    d_cnt = torch.full((S,), 77, dtype=torch.int32, device="cuda:0") if count else None
    distributed.tree_knearest_device(t, d_q, K, d_face, d_dist, d_pt, d_part, d_cnt, r)
    torch.cuda.synchronize()
    u = lambda x: None if x is None else x.cpu().numpy().view(np.uint32)
    return u(d_face), d_dist.cpu().numpy(), None if d_pt is None else d_pt.cpu().numpy(), u(d_part), u(d_cnt)


def test_points_independence():
    """5,000 rows (above the 4,096 below which the rows are not reordered): a shuffle permutes the answers and changes
    no byte, a small unsorted call on some of the rows gives those rows' bytes, the device entry point equals the host
    one, and count = NULL leaves idx and dist unchanged."""
    from mesh_amd import _native as N, spatialsearch
    v, _ = cloud(1000)
    rng = np.random.default_rng(21)
    q = rng.uniform(-0.2, 1.2, (5000, 3))
    h = N.build_points(v)
    for K, r in ((9, INF), (8, 0.15)):
        idx, dist, count = spatialsearch.points_nearest_k(h, q, K, r)
        p = rng.permutation(q.shape[0])
        idx_p, dist_p, count_p = spatialsearch.points_nearest_k(h, np.ascontiguousarray(q[p]), K, r)
        assert np.array_equal(idx_p, idx[p]) and np.array_equal(dist_p, dist[p]) and np.array_equal(count_p, count[p])
        some = np.ascontiguousarray(q[1000:1257])
        idx_s, dist_s, count_s = spatialsearch.points_nearest_k(h, some, K, r)
        assert np.array_equal(idx_s, idx[1000:1257]) and np.array_equal(dist_s, dist[1000:1257])
        assert np.array_equal(count_s, count[1000:1257])
        check_points(h, v, some, [K], r)
        d = _dev_points(h, q, K, r)
        assert same(d[0], idx) and same(d[1], dist) and same(d[2], count)
        d = _dev_points(h, q, K, r, count=False)
        assert same(d[0], idx) and same(d[1], dist)
        # a larger K answers the smaller one in its first columns
        idx2, dist2, _ = spatialsearch.points_nearest_k(h, q, 2 * K, r)
        assert np.array_equal(idx2[:, :K], idx) and np.array_equal(dist2[:, :K], dist)


def test_triangles_independence(meshes):
    from mesh_amd import spatialsearch
    v, f = golden(meshes, "sphere")
    rng = np.random.default_rng(22)
    lo, hi = v.min(0), v.max(0)
    q = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (5000, 3))
    t = spatialsearch.aabbtree_compute(v, f)
    K = 6
    face, part, pt, dist = spatialsearch.aabbtree_nearest_k(t, q, K)
    p = rng.permutation(q.shape[0])
    got = spatialsearch.aabbtree_nearest_k(t, np.ascontiguousarray(q[p]), K)
    for a, b in zip(got, (face, part, pt, dist)):
        assert np.array_equal(a, b[p])
    got = spatialsearch.aabbtree_nearest_k(t, np.ascontiguousarray(q[2000:2257]), K)
    for a, b in zip(got, (face, part, pt, dist)):
        assert np.array_equal(a, b[2000:2257])
    d_face, d_dist, d_pt, d_part, d_cnt = _dev_faces(t, q, K)
    assert same(d_face, face) and same(d_dist, dist) and same(d_pt, pt) and same(d_part, part)
    assert (d_cnt == K).all()
    # pt = part = NULL and count = NULL leave the other outputs unchanged
    n_face, n_dist, _, _, n_cnt = _dev_faces(t, q, K, pt=False, part=False)
    assert same(n_face, face) and same(n_dist, dist) and same(n_cnt, d_cnt)
    n_face, n_dist, n_pt, n_part, _ = _dev_faces(t, q, K, count=False)
    assert same(n_face, face) and same(n_dist, dist) and same(n_pt, pt) and same(n_part, part)
    n_face, n_dist, n_pt, _, _ = _dev_faces(t, q, K, part=False)
    assert same(n_face, face) and same(n_pt, pt)
    # column 0 of the 5,000 sorted rows is aabbtree_nearest's
    face1, part1, pt1 = spatialsearch.aabbtree_nearest(t, q)
    assert np.array_equal(face[:, 0], face1[0]) and np.array_equal(part[:, 0], part1[0]) and np.array_equal(pt[:, 0], pt1)


# ---- 7. a walk deeper than the LDS stack ----
def lds_stack():
    m = re.search(r"^#define MSH_KSTACK\s+(\d+)", open(os.path.join(ROOT, "mesh_amd", "csrc", "common.h")).read(),
                  flags=re.M)
    return int(m.group(1))


def test_deep_walk():
    """2^18 random points: the tree is deeper than the LDS stack (max_depth > kStack), but the far rows' walk is not --
    measured: deepest stack 16 entries at kStack = 16 (40,278 nodes, 23,239 points, 23,098 insertions for the 256
    rows), so this cloud fills the LDS stack and never spills.  test_graded_cloud_spills covers the spill."""
    import torch
    from mesh_amd import _native as N
    k_stack = lds_stack()
    rng = np.random.default_rng(31)
    v = rng.uniform(0.0, 1.0, (1 << 18, 3))
    q = rng.uniform(3.0, 4.0, (256, 3))  # far outside the cloud
    h = N.build_points(v)
    assert h.info().max_depth > k_stack
    K = 64
    from mesh_amd import spatialsearch
    idx, dist, count = spatialsearch.points_nearest_k(h, q, K)
    ref_idx = np.empty((256, K), np.uint32)
    ref_dist = np.empty((256, K))
    for i0 in range(0, 256, 32):  # the (row, point) matrix in slices of 32 rows
        b = brute_points(v, q[i0:i0 + 32], K)
        ref_idx[i0:i0 + 32], ref_dist[i0:i0 + 32] = b[0], b[1]
    assert same(idx, ref_idx) and same(dist, ref_dist) and (count == K).all()
    d_q = torch.from_numpy(q).to("cuda:0")
    torch.cuda.synchronize()
    nodes, prims, ins, deepest = h.knearest_stats(d_q.data_ptr(), 256, K)
    print("deep walk: nodes %d primitives %d insertions %d deepest stack %d (LDS %d)" % (nodes, prims, ins, deepest,
                                                                                        k_stack))
    assert 0 < deepest <= h.info().max_depth and prims >= ins >= 256 * K


def graded_cloud():
    """A point tree that is a chain: cluster i (three points) lies in the cell of the build's 1024^3 Morton grid whose
    code has bit 29 - i alone set, so the LBVH splits one cluster off per level, and a row beyond the origin corner
    walks down the chain pushing a cluster (an internal node) at every level."""
    pts = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]  # the scene box is the unit cube
    for i in range(28):
        bit = 29 - i
        axis = 2 - bit % 3  # Morton bit 3 m + 2 is x's bit m, 3 m + 1 y's, 3 m z's
        c = np.zeros(3)
        c[axis] = (1 << (bit // 3)) / 1024.0
        for j in range(3):
            pts.append(c + (j + 1) * 1e-5)
    return np.ascontiguousarray(np.array(pts))


def test_graded_cloud_spills():
    import torch
    from mesh_amd import _native as N
    k_stack = lds_stack()
    v = graded_cloud()
    h = N.build_points(v)
    rng = np.random.default_rng(33)
    q = np.ascontiguousarray(-0.5 + 0.01 * rng.uniform(-1.0, 1.0, (257, 3)))
    check_points(h, v, q, [64, 9, 1])
    check_points(h, v, q, [64], 0.9)
    d_q = torch.from_numpy(q).to("cuda:0")
    torch.cuda.synchronize()
    nodes, prims, ins, deepest = h.knearest_stats(d_q.data_ptr(), q.shape[0], 64)
    print("graded cloud: max_depth %d nodes %d primitives %d insertions %d deepest stack %d (LDS %d)" % (
        h.info().max_depth, nodes, prims, ins, deepest, k_stack))
    assert deepest > k_stack  # the walk went through the global spill area


# ---- 8. chunks and replicas ----
def test_chunks_and_replicas(monkeypatch):
    """100,000 rows at K = 16 are 22 MB of rows (24 + 16 * 12 + 4 B each): above the 16 MB small-call limit, so the
    chunk pipeline runs; MESH_AMD_HOST_CHUNK = 32768 makes four chunks, the last ragged."""
    from mesh_amd import _native as N, spatialsearch
    v, _ = cloud(1000)
    S, K = 100000, 16
    assert S * (24 + K * 12 + 4) > 16 << 20
    q = np.random.default_rng(41).uniform(-0.2, 1.2, (S, 3))
    h = N.build_points(v)
    dev = _dev_points(h, q, K)
    monkeypatch.setenv("MESH_AMD_HOST_CHUNK", "32768")
    monkeypatch.setattr(N, "PINNED_MIN_BYTES", 1 << 20)
    pooled = spatialsearch.points_nearest_k(h, q, K)
    assert pooled[0].base is not None  # carved from the pinned pool: downloaded in place
    for a, b in zip(pooled, dev):
        assert same(a, b)
    assert N.lib().msh_host_pool_trim() == 0
    monkeypatch.setenv("MESH_AMD_PINNED_POOL_MB", "0")
    staged = spatialsearch.points_nearest_k(h, q, K)
    assert staged[0].base is None  # pool disabled: plain np.empty arrays, staged downloads
    for a, b in zip(staged, dev):
        assert same(a, b)
    monkeypatch.delenv("MESH_AMD_PINNED_POOL_MB")
    # capped, with counts that vary
    dev_c = _dev_points(h, q, K, 0.2)
    for a, b in zip(spatialsearch.points_nearest_k(h, q, K, 0.2), dev_c):
        assert same(a, b)
    assert dev_c[2].min() == 0 and dev_c[2].max() == K
    # a handle replicated on the same device twice
    try:
        N.set_devices([0, 0])
        h2 = N.build_points(v)
        assert N.tree_devices(h2) == [0, 0]
        for a, b in zip(spatialsearch.points_nearest_k(h2, q, K), dev):
            assert same(a, b)
        monkeypatch.delenv("MESH_AMD_HOST_CHUNK")
        big = np.ascontiguousarray(np.concatenate([q, q]))  # 44 MB of rows: above the 32 MB split threshold
        got = spatialsearch.points_nearest_k(h2, big, K)
        for a, b in zip(got, dev):
            assert same(np.ascontiguousarray(a[:S]), b) and same(np.ascontiguousarray(a[S:]), b)
    finally:
        N.set_device(0)


# ---- 9. stats ----
def test_stats(meshes):
    import torch
    from mesh_amd import _native as N, spatialsearch
    v, q = cloud(1000)
    h = N.build_points(v)
    d_q = torch.from_numpy(q).to("cuda:0")
    torch.cuda.synchronize()
    for K, r in ((8, INF), (9, INF), (16, 0.2), (1, INF)):
        count = spatialsearch.points_nearest_k(h, q, K, r)[2]
        st = h.knearest_stats(d_q.data_ptr(), q.shape[0], K, r)
        assert st[0] > 0 and st[1] >= count.sum() and st[2] >= count.sum() and st[1] >= st[2]
        assert st == h.knearest_stats(d_q.data_ptr(), q.shape[0], K, r)
    # triangle trees are accepted too; S = 0 gives zeros
    tv, tf = golden(meshes, "icosphere")
    t = spatialsearch.aabbtree_compute(tv, tf)
    st = t.knearest_stats(d_q.data_ptr(), q.shape[0], 6)
    assert st[0] > 0 and st[1] >= 6 * q.shape[0] and st[2] >= 6 * q.shape[0]
    counts = (ctypes.c_uint64 * 4)(1, 1, 1, 1)
    assert N.lib().msh_tree_knearest_stats(t.ptr, None, 0, 6, INF, counts) == N.MSH_OK and list(counts) == [0, 0, 0, 0]


def test_empty_and_wrong_kinds(meshes):
    from mesh_amd import _native as N, aabb_normals, spatialsearch
    L = N.lib()
    v, _ = cloud(9)
    h = N.build_points(v)
    tv, tf = golden(meshes, "icosphere")
    t = spatialsearch.aabbtree_compute(tv, tf)
    nt = aabb_normals.aabbtree_n_compute(tv, tf, 0.1)
    idx, dist, count = spatialsearch.points_nearest_k(h, np.empty((0, 3)), 5)
    assert idx.shape == (0, 5) and dist.shape == (0, 5) and count.shape == (0,)
    assert L.msh_points_knearest_device(h.ptr, None, 0, 5, INF, None, None, None, None) == N.MSH_OK
    assert L.msh_tree_knearest_device(t.ptr, None, 0, 5, INF, None, None, None, None, None, None) == N.MSH_OK
    q, out_i, out_d = np.zeros((1, 3)), np.zeros(5, np.uint32), np.zeros(5)
    for name, call in (
            ("msh_points_knearest", lambda: L.msh_points_knearest(t.ptr, N.dptr(q), 1, 5, INF, N.uptr(out_i),
                                                                  N.dptr(out_d), None)),
            ("msh_tree_knearest", lambda: L.msh_tree_knearest(h.ptr, N.dptr(q), 1, 5, INF, N.uptr(out_i),
                                                              N.dptr(out_d), None, None, None)),
            ("msh_tree_knearest", lambda: L.msh_tree_knearest(nt.ptr, N.dptr(q), 1, 5, INF, N.uptr(out_i),
                                                              N.dptr(out_d), None, None, None)),
            ("msh_tree_knearest_stats", lambda: L.msh_tree_knearest_stats(nt.ptr, None, 1, 5, INF,
                                                                          (ctypes.c_uint64 * 4)()))):
        assert call() == N.MSH_EINVAL, name
        assert name.encode() in L.msh_last_error(), (name, L.msh_last_error())


# ---- 10. scipy's conventions ----
def test_scipy_conventions():
    spatial = pytest.importorskip("scipy.spatial")
    from mesh_amd import search
    from types import SimpleNamespace
    v, q = cloud(1000)
    n = v.shape[0]
    ours = search.ClosestPointTree(SimpleNamespace(v=v))
    theirs = spatial.cKDTree(v)
    for k in (1, 5):
        for r in (INF, 0.08):
            d, i = ours.query(q, k, distance_upper_bound=r)
            sd, si = theirs.query(q, k, distance_upper_bound=r)
            assert d.shape == sd.shape and i.shape == si.shape and d.dtype == sd.dtype and i.dtype == si.dtype
            # the same rows miss the same number of neighbours, marked the same way
            assert np.array_equal(i == n, si == n) and np.array_equal(np.isposinf(d), np.isposinf(sd))
            assert np.array_equal(np.isposinf(d), i == n)
            # the values: against brute force (scipy's order among ties is unspecified)
            b = brute_points(v, q, k, r)
            bi = np.where(b[0] == NO_FACE, n, b[0]).astype(np.intp)
            assert np.array_equal(i.reshape(-1, k), bi) and np.array_equal(d.reshape(-1, k), b[1])
            if r != INF:
                assert (i == n).any() and (i != n).any()
    d, i = ours.query(q[0], 5)
    sd, si = theirs.query(q[0], 5)
    assert d.shape == sd.shape == (5,) and i.shape == si.shape and i.dtype == si.dtype
    d, i = ours.query(q[0])
    sd, si = theirs.query(q[0])
    assert np.shape(d) == np.shape(sd) == () and np.shape(i) == np.shape(si) == () and i == si


def test_mesh_methods(meshes):
    from mesh_amd.mesh import Mesh
    v, f = golden(meshes, "icosphere")
    q = np.random.default_rng(51).uniform(-1.2, 1.2, (50, 3))
    mesh = Mesh(v=v, f=f)
    d, i = mesh.closest_vertices_k(q, 3)
    b = brute_points(v, q, 3)
    assert np.array_equal(i, b[0].astype(np.intp)) and np.array_equal(d, b[1])
    faces, pts, dist = mesh.closest_faces_and_points_k(q, 4, 0.5)
    assert faces.shape == (50, 4) and pts.shape == (50, 4, 3) and dist.shape == (50, 4)
    tree = mesh.compute_aabb_tree()
    faces2, parts2, pts2, dist2 = tree.nearest_k(q, 4, 0.5, nearest_part=True)
    assert np.array_equal(faces, faces2) and np.array_equal(pts, pts2, equal_nan=True) and np.array_equal(dist, dist2)
    assert parts2.shape == (50, 4) and (dist[faces != NO_FACE] <= 0.5).all()
