"""All primitives within a radius on point trees and plain triangle trees (msh_points_within, msh_tree_within, their
counts calls, *_device forms, msh_tree_within_stats and the Python layers over them).

Every comparison is bit-exact against brute force, with no row left out.
  points     numpy fp64 d2 = (dx*dx + dy*dy) + dz*dz per (row, point), d2 <= r*r, np.lexsort((id, d2)), np.sqrt;
  triangles  oracle.brute_nearest(v, f[t:t+1], q) once per face t gives d2, point and part of every row against that
             face by the pinned construction; then d2 <= r*r and the lexsort by (d2, t).
A row with a non-finite coordinate, or with a negative or NaN radius of its own, has no neighbours."""
import ctypes
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
K_LANE_SORT = 32  # internal.h kLaneSort: rows up to this length are ordered by their own lane


@pytest.fixture(scope="module", autouse=True)
def _device():
    from mesh_amd import _native
    _native.set_device(0)


def golden(meshes, name):
    return np.ascontiguousarray(meshes[name + "_v"], np.float64), np.ascontiguousarray(meshes[name + "_f"], np.uint32)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def starts_of(counts):
    return np.concatenate([[0], np.cumsum(counts.astype(np.int64))])


# ---- the references ----
def radii(r, S):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(r, np.float64), (S,)))


def select(d2, r):
    """per row of the (S, n) matrix d2 and its radius: the ids with d2 <= r*r ordered by (d2, id) -> (counts, ids)"""
    S = d2.shape[0]
    rr = radii(r, S)
    with np.errstate(invalid="ignore"):
        r2 = rr * rr
        valid = rr >= 0.0  # a negative or NaN radius: no neighbours
    counts = np.zeros(S, np.uint32)
    ids = []
    for i in range(S):
        if not valid[i]:
            continue
        ok = np.nonzero(d2[i] <= r2[i])[0]  # NaN (a non-finite row) never qualifies
        ids.append(ok[np.lexsort((ok, d2[i, ok]))])
        counts[i] = ok.size
    ids = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    return counts, ids.astype(np.int64)


def point_d2(v, q):
    with np.errstate(invalid="ignore"):
        dx, dy, dz = (q[:, None, k] - v[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
    d2[~np.isfinite(q).all(1)] = np.nan
    return d2


def brute_points(v, q, r):
    """(counts (S,) u32, idx (K,) u32, dist (K,))"""
    d2 = point_d2(v, q)
    counts, ids = select(d2, r)
    rows = np.repeat(np.arange(q.shape[0]), counts)
    return counts, ids.astype(np.uint32), np.sqrt(d2[rows, ids])


def face_table(oracle, v, f, q):
    """d2 (S,T), part (S,T), pt (S,T,3) of every row against every face, one oracle call per face"""
    fin = np.isfinite(q).all(1)
    qq = np.where(fin[:, None], q, 0.0)
    cols = [oracle.brute_nearest(v, f[t:t + 1], qq, threads=1) for t in range(f.shape[0])]
    d2 = np.stack([c[3] for c in cols], 1)
    d2[~fin] = np.nan
    return d2, np.stack([c[1] for c in cols], 1), np.stack([c[2] for c in cols], 1)


def brute_faces(table, r):
    """(counts, face (K,) u32, dist (K,), pt (K,3), part (K,) u32)"""
    d2, part, pt = table
    counts, ids = select(d2, r)
    rows = np.repeat(np.arange(d2.shape[0]), counts)
    return (counts, ids.astype(np.uint32), np.sqrt(d2[rows, ids]), np.ascontiguousarray(pt[rows, ids]),
            part[rows, ids].astype(np.uint32))


def check_points(h, v, q, r):
    from mesh_amd import spatialsearch
    ref = brute_points(v, q, r)
    got = spatialsearch.points_within(h, q, r)
    for a, b, what in zip(got, ref, ("counts", "idx", "dist")):
        assert same(a, b), what
    assert same(spatialsearch.points_within_count(h, q, r), ref[0])
    return ref


def check_faces(t, table, q, r):
    from mesh_amd import spatialsearch
    ref = brute_faces(table, r)
    got = spatialsearch.aabbtree_within(t, q, r, points=True, parts=True)
    for a, b, what in zip(got, ref, ("counts", "face", "dist", "pt", "part")):
        assert same(a, b), what
    # the optional columns leave the others unchanged
    for a, b in zip(spatialsearch.aabbtree_within(t, q, r), ref[:3]):
        assert same(a, b)
    got = spatialsearch.aabbtree_within(t, q, r, parts=True)
    assert same(got[3], ref[4]) and same(got[1], ref[1])
    assert same(spatialsearch.aabbtree_within_count(t, q, r), ref[0])
    return ref


def order_samples(run):
    """run() under the kernel timers -> (its result, the number of within_order samples it left)"""
    from mesh_amd import _native as N
    N.timing_reset()
    N.timing_enable(True)
    try:
        out = run()
    finally:
        N.timing_enable(False)
    assert N.timing_get("within_count")[1] >= 1
    return out, N.timing_get("within_order")[1]


# ---- 1. clouds ----
CLOUD_SIZES = [1, 2, 7, 8, 9, 65, 1000]


def cloud(P):
    rng = np.random.default_rng(100 + P)
    v = rng.uniform(0.0, 1.0, (P, 3))
    q = rng.uniform(-0.2, 1.2, (257, 3))  # 257 rows: a ragged last wave and a ragged block
    return v, q


def mean4_radius(P):
    # a ball of radius r holds P * 4/3 pi r^3 of the unit cube's P points: about 4 of them (the rows reach 0.2 outside
    # the cube, so fewer on average; small clouds get the whole cube)
    return min(float((3.0 / np.pi / P) ** (1.0 / 3.0)), 2.0)


@pytest.mark.parametrize("P", CLOUD_SIZES)
def test_points_against_brute_force(P):
    from mesh_amd import _native as N, spatialsearch
    v, q = cloud(P)
    S = q.shape[0]
    h = N.build_points(v)
    r4 = mean4_radius(P)
    c0 = check_points(h, v, q, 0.0)[0]
    assert (c0 == 0).all()
    check_points(h, v, q, r4)
    full = check_points(h, v, q, INF)
    assert (full[0] == P).all()  # every row lists all P points in order
    mixed = np.tile([0.0, r4, INF, 2.0 * r4], S)[:S]
    ref = check_points(h, v, q, mixed)
    assert (ref[0][2::4] == P).all() and (ref[0][0::4] == 0).all()
    # entry 0 at r = +inf is msh_points_nearest bit for bit
    idx1 = np.empty(S, np.uint32)
    dist1 = np.empty(S)
    N.check(N.lib().msh_points_nearest(h.ptr, N.dptr(q), S, N.uptr(idx1), N.dptr(dist1)))
    first = starts_of(full[0])[:-1]
    assert same(np.ascontiguousarray(full[1][first]), idx1) and same(np.ascontiguousarray(full[2][first]), dist1)
    # r = 0 on the points themselves: exact hits only
    rows = np.ascontiguousarray(v[::7])
    counts, idx, dist = spatialsearch.points_within(h, rows, 0.0)
    assert (counts == 1).all() and np.array_equal(idx, np.arange(0, P, 7)) and (dist == 0.0).all()


# ---- 2. boundaries and ties ----
def lattice(n=6):
    g = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


@pytest.mark.parametrize("copies", [1, 3])
def test_lattice_boundaries_and_ties(copies):
    from mesh_amd import _native as N
    lat = lattice()
    n = lat.shape[0]
    v = np.ascontiguousarray(np.concatenate([lat] * copies))  # equal coordinates, different ids
    q = np.ascontiguousarray(np.concatenate([lat, lattice(5) + 0.5]))
    h = N.build_points(v)
    centre = int(np.nonzero((lat == 2.0).all(1))[0][0])
    # neighbours exactly at d2 = r2 are in; sqrt(2) and sqrt(3): r*r rounds to one side of 2 and 3 in the test and in
    # the library alike
    for r in (1.0, 2.0, 3.0, np.sqrt(2.0), np.sqrt(3.0)):
        counts, idx, dist = check_points(h, v, q, r)
        st = starts_of(counts)
        row = slice(st[centre], st[centre + 1])
        d2 = ((lat - lat[centre]) ** 2).sum(1)
        assert counts[centre] == copies * int((d2 <= np.float64(r) * np.float64(r)).sum())
        if r in (1.0, 2.0, 3.0):
            assert dist[row][-1] == r  # the last entry lies exactly on the sphere
        # duplicates: j before j + n before j + 2n at equal d2
        ids = idx[row].astype(np.int64)
        grp = np.flatnonzero(np.diff(dist[row]) == 0.0)
        assert (np.diff(ids)[grp] > 0).all()
        if copies == 3:
            assert np.array_equal(ids[0:3], [centre, centre + n, centre + 2 * n])


# ---- 3. both ordering paths ----
def test_lane_and_radix_paths():
    from mesh_amd import _native as N, spatialsearch
    v = np.zeros((40, 3))
    v[:, 0] = np.arange(1, 41)
    h = N.build_points(v)
    q = np.zeros((8, 3))
    q[5, 1] = np.nan

    def run(r):
        r = np.asarray(r, np.float64)
        (counts, idx, dist), n = order_samples(lambda: spatialsearch.points_within(h, q, r))
        ref = brute_points(v, q, r)
        assert same(counts, ref[0]) and same(idx, ref[1]) and same(dist, ref[2])
        assert n == (1 if counts.max() > K_LANE_SORT else 0)  # the radix path ran exactly when a row exceeds kLaneSort
        return counts

    assert run([31, 0.5, 32, -1.0, 32, 40, 31, np.nan]).tolist() == [31, 0, 32, 0, 32, 0, 31, 0]
    assert run([31, 0.5, 33, -1.0, 32, 40, 40, np.nan]).tolist() == [31, 0, 33, 0, 32, 0, 40, 0]
    assert run([33, 33, 33, 33, 33, 33, 33, 33]).tolist() == [33] * 5 + [0] + [33] * 2
    assert run([32, 32, 32, 32, 32, 32, 32, 32]).max() == 32


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
        far = lo - 10.0 * (hi - lo) * np.array([[1.0, 0.5, 0.25], [0.25, 1.0, 2.0]])
        q = np.ascontiguousarray(np.concatenate([uni, 1.5 * v[j], 0.5 * v[j], far]))
        _tables[name] = (v, f, q, face_table(oracle, v, f, q))
    return _tables[name]


@pytest.mark.parametrize("name", TRI_MESHES)
def test_triangles_against_brute_force(meshes, oracle, name):
    from mesh_amd import spatialsearch
    v, f, q, table = tri_case(meshes, oracle, name)
    S, T = q.shape[0], f.shape[0]
    s = np.sort(table[0], 1)
    assert ((s[:, :5] == s[:, :1]).all(1)).any(), "no row with a 5-way exact d2 tie"
    t = spatialsearch.aabbtree_compute(v, f)
    diag = float(np.linalg.norm(v.max(0) - v.min(0)))
    ref = check_faces(t, table, q, 0.08 * diag)
    assert (ref[0] == 0).any() and (ref[0] > 1).any() and (ref[0][-2:] == 0).all()
    check_faces(t, table, q, 0.0)
    full = check_faces(t, table, q, INF)
    assert (full[0] == T).all()
    mixed = np.tile([0.08 * diag, INF, 0.0, 0.3 * diag, -1.0, np.nan], S)[:S]
    check_faces(t, table, q, mixed)
    # entry 0 at r = +inf is aabbtree_nearest bit for bit
    face1, part1, pt1 = spatialsearch.aabbtree_nearest(t, q)
    first = starts_of(full[0])[:-1]
    assert np.array_equal(full[1][first], face1[0]) and np.array_equal(full[4][first], part1[0])
    assert np.array_equal(full[3][first], pt1)


def soup(n):
    """n parallel triangles in the planes z = 1 + 0.125 k"""
    v = np.zeros((3 * n, 3))
    for k in range(n):
        v[3 * k:3 * k + 3] = [[0.0, 0.0, 1 + 0.125 * k], [1.0, 0.0, 1 + 0.125 * k], [0.0, 1.0, 1 + 0.125 * k]]
    return v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def test_soup_rows_of_0_1_32_33_100(oracle):
    from mesh_amd import spatialsearch
    v, f = soup(100)
    t = spatialsearch.aabbtree_compute(v, f)
    rng = np.random.default_rng(9)
    q = np.zeros((10, 3))
    q[:, :2] = rng.uniform(0.05, 0.45, (10, 2))  # below the triangles' interior: face k lies at distance 1 + k / 8
    table = face_table(oracle, v, f, q)
    r = np.array([0.5, 1.0, 4.875, 5.0, INF, 4.875, 1.0, 0.5, 4.875, 1.0])
    (ref, n) = order_samples(lambda: check_faces(t, table, q, r))
    assert ref[0].tolist() == [0, 1, 32, 33, 100, 32, 1, 0, 32, 1] and n >= 1
    short = [0, 1, 2, 5]
    (ref, n) = order_samples(lambda: check_faces(t, tuple(x[short] for x in table), q[short], r[short]))
    assert ref[0].tolist() == [0, 1, 32, 32] and n == 0


def test_extra_faces(meshes, oracle):
    from mesh_amd import _native as N
    v, f = golden(meshes, "icosphere")
    T = len(f)
    lo, hi = v.min(0), v.max(0)
    z = hi[2] + 0.5
    ev = np.array([[lo[0] - 1, lo[1] - 1, z], [hi[0] + 1, lo[1] - 1, z], [hi[0] + 1, hi[1] + 1, z], [lo[0] - 1, hi[1] + 1, z]])
    ef = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
    t = N.build_tree(v, f, ev, ef)
    av = np.ascontiguousarray(np.vstack([v, ev]))
    af = np.ascontiguousarray(np.vstack([f, ef + len(v)]).astype(np.uint32))
    rng = np.random.default_rng(3)
    q = np.column_stack([rng.uniform(lo[0], hi[0], 64), rng.uniform(lo[1], hi[1], 64), np.full(64, z + 0.25)])
    table = face_table(oracle, av, af, q)
    ref = check_faces(t, table, q, 0.3)
    assert (ref[0] >= 1).all() and (ref[1] >= T).all() and (ref[1] < T + 2).all()
    ref = check_faces(t, table, q, INF)
    assert (ref[0] == T + 2).all()


def lds_stack():
    m = re.search(r"^#define MSH_KSTACK\s+(\d+)", open(os.path.join(ROOT, "mesh_amd", "csrc", "common.h")).read(),
                  flags=re.M)
    return int(m.group(1))


def test_deep_tree_spills(oracle):
    """the deep mesh of test_gpu_parity.test_deep_tree_spill_path (clustered + spread triangles): with r = +inf the walk
    prunes nothing and goes through the global spill area"""
    import torch
    from mesh_amd import spatialsearch
    rng = np.random.default_rng(22)
    pts = np.vstack([rng.normal(size=(3000, 3)) * 1e-4, rng.normal(size=(3000, 3)) * 100])
    v = np.repeat(pts, 3, axis=0) + rng.normal(size=(18000, 3)) * 1e-6
    f = np.arange(18000, dtype=np.uint32).reshape(-1, 3)
    t = spatialsearch.aabbtree_compute(v, f)
    assert t.info().max_depth > lds_stack()
    q = np.ascontiguousarray(np.vstack([rng.normal(size=(24, 3)) * 50, rng.normal(size=(8, 3)) * 1e-4]))
    table = face_table(oracle, v, f, q)
    r = np.tile([INF, 60.0, 1e-4, 150.0], 8)
    ref = check_faces(t, table, q, r)
    assert (ref[0][0::4] == 6000).all() and ref[0].min() < 100
    d_q = torch.from_numpy(q).to("cuda:0")
    d_r = torch.from_numpy(r).to("cuda:0")
    torch.cuda.synchronize()
    nodes, prims, entries, deepest = t.within_stats(d_q.data_ptr(), q.shape[0], 0.0, d_r.data_ptr())
    print("deep tree: max_depth %d nodes %d primitives %d entries %d deepest stack %d (LDS %d)" % (
        t.info().max_depth, nodes, prims, entries, deepest, lds_stack()))
    assert entries == int(ref[0].sum()) and prims >= entries and deepest > lds_stack()


def test_graded_cloud_spills():
    """test_gpu_knearest's chain-shaped point tree: one cluster splits off per level"""
    import torch
    from mesh_amd import _native as N
    pts = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
    for i in range(28):
        bit = 29 - i
        c = np.zeros(3)
        c[2 - bit % 3] = (1 << (bit // 3)) / 1024.0
        for j in range(3):
            pts.append(c + (j + 1) * 1e-5)
    v = np.ascontiguousarray(np.array(pts))
    h = N.build_points(v)
    q = np.ascontiguousarray(-0.5 + 0.01 * np.random.default_rng(33).uniform(-1.0, 1.0, (257, 3)))
    check_points(h, v, q, INF)
    check_points(h, v, q, 0.9)
    d_q = torch.from_numpy(q).to("cuda:0")
    torch.cuda.synchronize()
    st = h.within_stats(d_q.data_ptr(), q.shape[0], INF)
    assert st[2] == 257 * v.shape[0] and st[3] > lds_stack()


# ---- 5. relations to the K-nearest queries ----
def prefix_rows(counts, K):
    """for every row the positions of its first min(K, count) entries, and that number"""
    st = starts_of(counts)
    m = np.minimum(counts.astype(np.int64), K)
    pos = np.concatenate([np.arange(st[i], st[i] + m[i]) for i in range(len(counts))]) if len(counts) else np.zeros(0, int)
    col = np.concatenate([np.arange(m[i]) for i in range(len(counts))]) if len(counts) else np.zeros(0, int)
    return pos.astype(np.int64), np.repeat(np.arange(len(counts)), m), col.astype(np.int64), m


@pytest.mark.parametrize("K", [1, 8, 16, 64])
def test_prefix_is_the_k_nearest_answer(meshes, K):
    from mesh_amd import _native as N, spatialsearch
    v, q = cloud(1000)
    h = N.build_points(v)
    tv, tf = golden(meshes, "sphere")
    t = spatialsearch.aabbtree_compute(tv, tf)
    lo, hi = tv.min(0), tv.max(0)
    tq = np.random.default_rng(6).uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (257, 3))
    diag = float(np.linalg.norm(hi - lo))
    S = q.shape[0]
    pick = np.arange(S) % 3
    for rs, trs in ((0.25, 0.2 * diag), (np.array([0.1, 0.25, INF])[pick], np.array([0.05, 0.3, INF])[pick] * diag)):
        counts, idx, dist = spatialsearch.points_within(h, q, rs)
        tc, face, tdist, pt, part = spatialsearch.aabbtree_within(t, tq, trs, points=True, parts=True)
        assert counts.max() > K or K == 64
        for r in np.unique(radii(rs, S)):
            rows = np.flatnonzero(radii(rs, S) == r)
            kidx, kdist, kcount = spatialsearch.points_nearest_k(h, np.ascontiguousarray(q[rows]), K, float(r))
            pos, row, col, m = prefix_rows(counts, K)
            keep = np.isin(row, rows)
            at = np.searchsorted(rows, row[keep])
            assert np.array_equal(kcount, m[rows])
            assert same(idx[pos[keep]], kidx[at, col[keep]]) and same(dist[pos[keep]], kdist[at, col[keep]])
        for r in np.unique(radii(trs, S)):
            rows = np.flatnonzero(radii(trs, S) == r)
            kface, kpart, kpt, kdist = spatialsearch.aabbtree_nearest_k(t, np.ascontiguousarray(tq[rows]), K, float(r))
            pos, row, col, m = prefix_rows(tc, K)
            keep = np.isin(row, rows)
            at = np.searchsorted(rows, row[keep])
            assert np.array_equal((kface != 0xFFFFFFFF).sum(1), m[rows])
            assert same(face[pos[keep]], kface[at, col[keep]]) and same(tdist[pos[keep]], kdist[at, col[keep]])
            assert same(pt[pos[keep]], kpt[at, col[keep]]) and same(part[pos[keep]], kpart[at, col[keep]])


# ---- 6. invalid rows ----
def test_invalid_rows():
    from mesh_amd import _native as N, spatialsearch
    v, q = cloud(1000)
    h = N.build_points(v)
    S = q.shape[0]
    r = np.full(S, 0.2)
    good = spatialsearch.points_within(h, q, r)
    q, r = q.copy(), r.copy()
    q[3, 1] = np.nan
    q[64, 0] = np.inf
    q[256, 2] = -np.inf
    r[10] = -0.5
    r[65] = np.nan
    r[128] = -INF
    bad = np.array([3, 10, 64, 65, 128, 256])
    counts, idx, dist = check_points(h, v, q, r)
    assert (counts[bad] == 0).all() and (good[0][bad] > 0).any()
    others = np.setdiff1d(np.arange(S), bad)
    assert np.array_equal(counts[others], good[0][others])
    keep = np.isin(np.repeat(np.arange(S), good[0]), others)  # the rows around them are untouched
    assert same(idx, good[1][keep]) and same(dist, good[2][keep])
    with pytest.raises(ValueError):
        spatialsearch.points_within(h, q, -1.0)
    with pytest.raises(ValueError):
        spatialsearch.points_within_count(h, q, float("nan"))


# ---- 7. shapes and handles ----
@pytest.mark.parametrize("S", [0, 1, 63, 64, 65])
def test_row_counts(meshes, oracle, S):
    from mesh_amd import _native as N, spatialsearch
    v, q = cloud(65)
    q = np.ascontiguousarray(q[:S])
    h = N.build_points(v)
    ref = check_points(h, v, q, 0.4)
    assert ref[0].shape == (S,) and (S == 0 or ref[0].sum() > 0)
    tv, tf = golden(meshes, "test_doublebox")
    t = spatialsearch.aabbtree_compute(tv, tf)
    tq = np.ascontiguousarray(tri_case(meshes, oracle, "test_doublebox")[2][:S])
    table = tuple(x[:S] for x in tri_case(meshes, oracle, "test_doublebox")[3])
    if S:
        check_faces(t, table, tq, 0.5)
    else:
        got = spatialsearch.aabbtree_within(t, tq, 0.5, points=True, parts=True)
        assert [x.shape for x in got] == [(0,), (0,), (0,), (0, 3), (0,)]
        assert spatialsearch.aabbtree_within_count(t, tq, 0.5).shape == (0,)


def test_one_primitive(oracle):
    from mesh_amd import _native as N, spatialsearch
    q = np.random.default_rng(8).uniform(-1.0, 2.0, (257, 3))
    v = np.array([[0.25, 0.5, 0.75]])
    h = N.build_points(v)
    assert 0 < check_points(h, v, q, 1.0)[0].sum() < 257
    check_points(h, v, q, INF)
    tv = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.2], [0.2, 1.0, 0.5]])
    tf = np.array([[0, 1, 2]], np.uint32)
    t = spatialsearch.aabbtree_compute(tv, tf)
    table = face_table(oracle, tv, tf, q)
    assert 0 < check_faces(t, table, q, 0.7)[0].sum() < 257
    check_faces(t, table, q, INF)


# ---- 8. the cap protocol through the C ABI ----
def abi_points(h, q, r_max, r_rows, cap, want=True, pad=3):
    from mesh_amd import _native as N
    S = len(q)
    counts = np.full(S, 0xDEADBEEF, np.uint32)
    idx = np.full(cap + pad, 0xABABABAB, np.uint32)
    dist = np.full(cap + pad, -7.0)
    K = N._sz(0)
    N.check(N.lib().msh_points_within(h.ptr, N.dptr(q), S, r_max, N.dptr(r_rows), N.uptr(counts),
                                      N.uptr(idx) if want else None, N.dptr(dist) if want else None, cap,
                                      ctypes.byref(K)))
    return K.value, counts, idx, dist


def abi_faces(t, q, r_max, r_rows, cap, want=True, want_pt=True, want_part=True, want_counts=True, pad=3):
    from mesh_amd import _native as N
    S = len(q)
    counts = np.full(S, 0xDEADBEEF, np.uint32)
    face = np.full(cap + pad, 0xABABABAB, np.uint32)
    dist = np.full(cap + pad, -7.0)
    pt = np.full((cap + pad, 3), -7.0)
    part = np.full(cap + pad, 0xCDCDCDCD, np.uint32)
    K = N._sz(0)
    N.check(N.lib().msh_tree_within(t.ptr, N.dptr(q), S, r_max, N.dptr(r_rows), N.uptr(counts) if want_counts else None,
                                    N.uptr(face) if want else None, N.dptr(dist) if want else None,
                                    N.dptr(pt) if want_pt else None, N.uptr(part) if want_part else None, cap,
                                    ctypes.byref(K)))
    return K.value, counts, face, dist, pt, part


@pytest.mark.parametrize("long_rows", [False, True])
def test_cap_protocol(long_rows):
    from mesh_amd import _native as N, spatialsearch
    v, f = soup(100)
    t = spatialsearch.aabbtree_compute(v, f)
    q = np.zeros((14, 3))
    q[:, :2] = np.random.default_rng(10).uniform(0.05, 0.45, (14, 2))
    r = np.tile([4.875, 1.0, 2.0, 0.5], 4)[:14].copy()  # 32, 1, 9, 0 faces
    if long_rows:
        r[0] = r[13] = INF  # the first and the last row are long ones
    full = spatialsearch.aabbtree_within(t, q, r, points=True, parts=True)
    Kf = int(full[0].sum())
    assert (full[0].max() > K_LANE_SORT) == long_rows and Kf > 150
    K, counts, *_ = abi_faces(t, q, 0.0, r, 0, want=False, want_pt=False, want_part=False)
    assert K == Kf and np.array_equal(counts, full[0])
    for cap in (Kf - 1, 1, 150, Kf, Kf + 2):
        K, counts, face, dist, pt, part = abi_faces(t, q, 0.0, r, cap)
        n = min(cap, Kf)
        assert K == Kf and np.array_equal(counts, full[0]), cap
        assert face[:n].tobytes() == full[1][:n].tobytes() and dist[:n].tobytes() == full[2][:n].tobytes(), cap
        assert pt[:n].tobytes() == full[3][:n].tobytes() and part[:n].tobytes() == full[4][:n].tobytes(), cap
        assert (face[n:] == 0xABABABAB).all() and (dist[n:] == -7.0).all() and (pt[n:] == -7.0).all(), cap
        assert (part[n:] == 0xCDCDCDCD).all(), cap
    # pt, part and counts NULL each leave the other columns unchanged
    K, counts, face, dist, pt, part = abi_faces(t, q, 0.0, r, Kf, want_pt=False)
    assert K == Kf and same(face[:Kf], full[1]) and same(dist[:Kf], full[2]) and same(part[:Kf], full[4])
    assert (pt == -7.0).all()
    K, counts, face, dist, pt, part = abi_faces(t, q, 0.0, r, Kf, want_part=False, want_counts=False)
    assert K == Kf and same(face[:Kf], full[1]) and same(pt[:Kf], full[3]) and (part == 0xCDCDCDCD).all()
    assert (counts == 0xDEADBEEF).all()
    # the point tree's list call
    pv = np.zeros((40, 3))
    pv[:, 0] = np.arange(1, 41)
    h = N.build_points(pv)
    pq = np.zeros((6, 3))
    pr = np.array([31.0, 2.0, 40.0 if long_rows else 32.0, 0.5, 7.0, 31.0])
    pf = spatialsearch.points_within(h, pq, pr)
    Kp = int(pf[0].sum())
    K, counts, *_ = abi_points(h, pq, 0.0, pr, 0, want=False)
    assert K == Kp and np.array_equal(counts, pf[0])
    for cap in (Kp - 1, 1, Kp, Kp + 2):
        K, counts, idx, dist = abi_points(h, pq, 0.0, pr, cap)
        n = min(cap, Kp)
        assert K == Kp and np.array_equal(counts, pf[0])
        assert idx[:n].tobytes() == pf[1][:n].tobytes() and dist[:n].tobytes() == pf[2][:n].tobytes()
        assert (idx[n:] == 0xABABABAB).all() and (dist[n:] == -7.0).all()
    # the scalar radius through the ABI equals the array of equal radii
    K, counts, idx, dist = abi_points(h, pq, 7.0, None, 64)
    assert K == 42 and (counts == 7).all() and np.array_equal(idx[:K], np.tile(np.arange(7, dtype=np.uint32), 6))


# ---- 9. repeatability and independence ----
def test_repeatability_and_independence(meshes):
    from mesh_amd import _native as N, spatialsearch
    v, _ = cloud(1000)
    rng = np.random.default_rng(21)
    S = 5000  # above the 4,096 rows below which the rows are not reordered
    q = rng.uniform(-0.2, 1.2, (S, 3))
    r = rng.uniform(0.02, 0.16, S)
    r[::17] = 0.45  # rows longer than kLaneSort
    h = N.build_points(v)
    a = spatialsearch.points_within(h, q, r)
    b = spatialsearch.points_within(h, q, r)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert a[0].max() > K_LANE_SORT and (a[0] == 0).any()
    p = rng.permutation(S)
    c = spatialsearch.points_within(h, np.ascontiguousarray(q[p]), np.ascontiguousarray(r[p]))
    st = starts_of(a[0])
    src = np.concatenate([np.arange(st[i], st[i + 1]) for i in p])
    assert np.array_equal(c[0], a[0][p]) and c[1].tobytes() == a[1][src].tobytes()
    assert c[2].tobytes() == a[2][src].tobytes()
    some = slice(1000, 1257)
    for x, y in zip(spatialsearch.points_within(h, np.ascontiguousarray(q[some]), np.ascontiguousarray(r[some])),
                    brute_points(v, q[some], r[some])):
        assert same(x, y)
    ref = brute_points(v, q[some], r[some])
    assert same(a[0][some], ref[0]) and same(a[1][st[1000]:st[1257]], ref[1]) and same(a[2][st[1000]:st[1257]], ref[2])
    # short rows only: the lanes' ordering in slot order
    rs = np.minimum(r, 0.1)
    a = spatialsearch.points_within(h, q, rs)
    assert a[0].max() <= K_LANE_SORT
    c = spatialsearch.points_within(h, np.ascontiguousarray(q[p]), np.ascontiguousarray(rs[p]))
    st = starts_of(a[0])
    src = np.concatenate([np.arange(st[i], st[i + 1]) for i in p])
    assert np.array_equal(c[0], a[0][p]) and c[1].tobytes() == a[1][src].tobytes()
    ref = brute_points(v, q[some], rs[some])
    assert same(a[1][st[1000]:st[1257]], ref[1]) and same(a[2][st[1000]:st[1257]], ref[2])
    # triangles
    tv, tf = golden(meshes, "sphere")
    t = spatialsearch.aabbtree_compute(tv, tf)
    lo, hi = tv.min(0), tv.max(0)
    tq = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (S, 3))
    tr = rng.uniform(0.02, 0.25, S) * float(np.linalg.norm(hi - lo))
    a = spatialsearch.aabbtree_within(t, tq, tr, points=True, parts=True)
    b = spatialsearch.aabbtree_within(t, tq, tr, points=True, parts=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    c = spatialsearch.aabbtree_within(t, np.ascontiguousarray(tq[p]), np.ascontiguousarray(tr[p]), points=True, parts=True)
    st = starts_of(a[0])
    src = np.concatenate([np.arange(st[i], st[i + 1]) for i in p])
    assert np.array_equal(c[0], a[0][p])
    for x, y in zip(c[1:], a[1:]):
        assert x.tobytes() == y[src].tobytes()


# ---- 10. device entry points, the pipeline, replicas ----
def dev_points(h, q, r_max, r_rows, cap):
    import torch
    from mesh_amd import _native as N
    vp, dev, S = ctypes.c_void_p, torch.device("cuda:0"), len(q)
    dq = torch.from_numpy(q).to(dev)
    dr = torch.from_numpy(r_rows).to(dev) if r_rows is not None else None
    dc = torch.full((S,), 77, dtype=torch.int32, device=dev)
    dc2 = torch.full((S,), 77, dtype=torch.int32, device=dev)
    di = torch.full((cap,), 7, dtype=torch.int32, device=dev)
    dd = torch.full((cap,), -7.0, dtype=torch.float64, device=dev)
    K = N._sz(0)
    rp = vp(dr.data_ptr()) if dr is not None else None
    N.check(N.lib().msh_points_within_device(h.ptr, vp(dq.data_ptr()), S, r_max, rp, vp(dc.data_ptr()),
                                             vp(di.data_ptr()) if cap else None, vp(dd.data_ptr()) if cap else None, cap,
                                             ctypes.byref(K), None))
    N.check(N.lib().msh_points_within_count_device(h.ptr, vp(dq.data_ptr()), S, r_max, rp, vp(dc2.data_ptr()), None))
    torch.cuda.synchronize()
    n = min(cap, K.value)
    return (K.value, dc.cpu().numpy().view(np.uint32), di.cpu().numpy().view(np.uint32)[:n], dd.cpu().numpy()[:n],
            dc2.cpu().numpy().view(np.uint32))


def dev_faces(t, q, r_max, r_rows, cap):
    import torch
    from mesh_amd import _native as N
    vp, dev, S = ctypes.c_void_p, torch.device("cuda:0"), len(q)
    dq = torch.from_numpy(q).to(dev)
    dr = torch.from_numpy(r_rows).to(dev) if r_rows is not None else None
    dc = torch.full((S,), 77, dtype=torch.int32, device=dev)
    dc2 = torch.full((S,), 77, dtype=torch.int32, device=dev)
    df = torch.full((cap,), 7, dtype=torch.int32, device=dev)
    dd = torch.full((cap,), -7.0, dtype=torch.float64, device=dev)
    dp = torch.full((cap, 3), -7.0, dtype=torch.float64, device=dev)
    dpart = torch.full((cap,), 7, dtype=torch.int32, device=dev)
    K = N._sz(0)
    rp = vp(dr.data_ptr()) if dr is not None else None
    N.check(N.lib().msh_tree_within_device(t.ptr, vp(dq.data_ptr()), S, r_max, rp, vp(dc.data_ptr()),
                                           vp(df.data_ptr()), vp(dd.data_ptr()), vp(dp.data_ptr()),
                                           vp(dpart.data_ptr()), cap, ctypes.byref(K), None))
    N.check(N.lib().msh_tree_within_count_device(t.ptr, vp(dq.data_ptr()), S, r_max, rp, vp(dc2.data_ptr()), None))
    torch.cuda.synchronize()
    n = min(cap, K.value)
    u = lambda x: x.cpu().numpy().view(np.uint32)
    return K.value, u(dc), u(df)[:n], dd.cpu().numpy()[:n], dp.cpu().numpy()[:n], u(dpart)[:n], u(dc2)


def test_device_entry_points(meshes):
    from mesh_amd import _native as N, spatialsearch
    v, _ = cloud(1000)
    rng = np.random.default_rng(23)
    S = 5000
    q = rng.uniform(-0.2, 1.2, (S, 3))
    r = rng.uniform(0.02, 0.2, S)
    r[7] = -1.0
    h = N.build_points(v)
    for r_max, r_rows in ((0.12, None), (0.0, r)):
        host = spatialsearch.points_within(h, q, r_max if r_rows is None else r_rows)
        Kf = int(host[0].sum())
        K, counts, idx, dist, counts2 = dev_points(h, q, r_max, r_rows, Kf + 5)
        assert K == Kf and same(counts, host[0]) and same(idx, host[1]) and same(dist, host[2]) and same(counts2, host[0])
        K, counts, idx, dist, _ = dev_points(h, q, r_max, r_rows, 1000)
        assert K == Kf and same(counts, host[0]) and same(idx, host[1][:1000]) and same(dist, host[2][:1000])
        K, counts, _, _, _ = dev_points(h, q, r_max, r_rows, 0)
        assert K == Kf and same(counts, host[0])
    tv, tf = golden(meshes, "icosphere")
    t = spatialsearch.aabbtree_compute(tv, tf)
    tq = rng.uniform(-1.2, 1.2, (S, 3))
    tr = rng.uniform(0.05, 0.6, S)
    for r_max, r_rows in ((0.3, None), (0.0, tr)):
        host = spatialsearch.aabbtree_within(t, tq, r_max if r_rows is None else r_rows, points=True, parts=True)
        Kf = int(host[0].sum())
        got = dev_faces(t, tq, r_max, r_rows, Kf)
        assert got[0] == Kf and same(got[6], host[0])
        for a, b in zip(got[1:6], host):
            assert same(a, b)
    # the stats call: entries is the sum of the counts, and the call repeats
    import torch
    d_q = torch.from_numpy(tq).to("cuda:0")
    d_r = torch.from_numpy(tr).to("cuda:0")
    torch.cuda.synchronize()
    st = t.within_stats(d_q.data_ptr(), S, 0.0, d_r.data_ptr())
    assert st[0] > 0 and st[1] >= st[2] == Kf and st[3] >= 1
    assert st == t.within_stats(d_q.data_ptr(), S, 0.0, d_r.data_ptr())
    assert t.within_stats(d_q.data_ptr(), S, 0.3)[2] == int(spatialsearch.aabbtree_within_count(t, tq, 0.3).sum())


@pytest.mark.parametrize("S,chunk", [(350001, 100001), (500001, 150001)])
def test_counts_through_the_pipeline(monkeypatch, S, chunk):
    """The counts call on host arrays against the _device entry point, results carved from the pinned pool and with the
    pool disabled (staged).  A row with a radius of its own is 36 B (24 + 8 + 4): 350,001 rows are 12.6 MB, under the
    16 MB below which a host call makes one round trip, so that case runs as one launch whatever MESH_AMD_HOST_CHUNK
    says; 500,001 rows are 18 MB and go through the slab pipeline in four chunks of an odd number of rows, the last
    ragged."""
    from mesh_amd import _native as N, spatialsearch
    v, _ = cloud(1000)
    launches = 1 if S * 36 <= 16 << 20 else 4
    assert S % 2 == 1 and chunk % 2 == 1 and S % chunk not in (0, chunk - 1) and -(-S // chunk) == 4
    rng = np.random.default_rng(41)
    q = rng.uniform(-0.2, 1.2, (S, 3))
    r = rng.uniform(0.0, 0.15, S)
    r[5::1001] = -1.0  # empty rows in every chunk
    h = N.build_points(v)
    dev_r = dev_points(h, q, 0.0, r, 0)[4]
    dev_s = dev_points(h, q, 0.1, None, 0)[4]
    assert dev_r.max() > 8 and (dev_r[5::1001] == 0).all()
    some = slice(chunk - 64, chunk + 64)  # across a chunk boundary
    assert same(np.ascontiguousarray(dev_r[some]), brute_points(v, q[some], r[some])[0])
    monkeypatch.setenv("MESH_AMD_HOST_CHUNK", str(chunk))
    monkeypatch.setattr(N, "PINNED_MIN_BYTES", 1 << 16)
    for pool in (True, False):
        if not pool:
            assert N.lib().msh_host_pool_trim() == 0
            monkeypatch.setenv("MESH_AMD_PINNED_POOL_MB", "0")
        N.timing_reset()
        N.timing_enable(True)
        cn = spatialsearch.points_within_count(h, q, r)
        N.timing_enable(False)
        assert N.timing_get("within_count")[1] == launches  # one launch per chunk
        assert (cn.base is not None) == pool
        assert np.array_equal(cn, dev_r), "per-row radii (pool %s)" % pool
        assert np.array_equal(spatialsearch.points_within_count(h, q, 0.1), dev_s), "scalar radius (pool %s)" % pool
    monkeypatch.delenv("MESH_AMD_PINNED_POOL_MB")
    # a handle replicated on the same device twice
    try:
        N.set_devices([0, 0])
        h2 = N.build_points(v)
        assert N.tree_devices(h2) == [0, 0]
        assert np.array_equal(spatialsearch.points_within_count(h2, q, r), dev_r)
        monkeypatch.delenv("MESH_AMD_HOST_CHUNK")
        reps = 3 if S > 400000 else 4  # 54 and 50.4 MB of rows: above the 32 MB below which a call is not split
        big_q = np.ascontiguousarray(np.concatenate([q] * reps))
        big_r = np.ascontiguousarray(np.concatenate([r] * reps))
        got = spatialsearch.points_within_count(h2, big_q, big_r)
        assert np.array_equal(got.reshape(reps, S), np.tile(dev_r, (reps, 1)))
        # the list call stays on the handle's own device
        a = spatialsearch.points_within(h2, np.ascontiguousarray(q[:5000]), np.ascontiguousarray(r[:5000]))
        b = spatialsearch.points_within(h, np.ascontiguousarray(q[:5000]), np.ascontiguousarray(r[:5000]))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    finally:
        N.set_device(0)


# ---- 11. refusals ----
def test_wrong_kinds(meshes):
    from mesh_amd import _native as N, aabb_normals, spatialsearch
    L = N.lib()
    v, _ = cloud(9)
    h = N.build_points(v)
    tv, tf = golden(meshes, "icosphere")
    t = spatialsearch.aabbtree_compute(tv, tf)
    nt = aabb_normals.aabbtree_n_compute(tv, tf, 0.1)
    bt = N.build_batch(np.ascontiguousarray(np.stack([tv, tv + 1.0])), tf)
    q, c, i, d = np.zeros((1, 3)), np.zeros(1, np.uint32), np.zeros(4, np.uint32), np.zeros(4)
    K = N._sz(0)
    for name, call in (
            ("msh_points_within", lambda: L.msh_points_within(t.ptr, N.dptr(q), 1, 1.0, None, N.uptr(c), N.uptr(i),
                                                              N.dptr(d), 4, ctypes.byref(K))),
            ("msh_points_within_count", lambda: L.msh_points_within_count(t.ptr, N.dptr(q), 1, 1.0, None, N.uptr(c))),
            ("msh_tree_within", lambda: L.msh_tree_within(h.ptr, N.dptr(q), 1, 1.0, None, N.uptr(c), N.uptr(i),
                                                          N.dptr(d), None, None, 4, ctypes.byref(K))),
            ("msh_tree_within", lambda: L.msh_tree_within(nt.ptr, N.dptr(q), 1, 1.0, None, N.uptr(c), N.uptr(i),
                                                          N.dptr(d), None, None, 4, ctypes.byref(K))),
            ("msh_tree_within", lambda: L.msh_tree_within(bt.ptr, N.dptr(q), 1, 1.0, None, N.uptr(c), N.uptr(i),
                                                          N.dptr(d), None, None, 4, ctypes.byref(K))),
            ("msh_tree_within_count", lambda: L.msh_tree_within_count(h.ptr, N.dptr(q), 1, 1.0, None, N.uptr(c))),
            ("msh_tree_within_count", lambda: L.msh_tree_within_count(nt.ptr, N.dptr(q), 1, 1.0, None, N.uptr(c))),
            ("msh_tree_within_count_device", lambda: L.msh_tree_within_count_device(h.ptr, None, 1, 1.0, None, None,
                                                                                    None)),
            ("msh_points_within_device", lambda: L.msh_points_within_device(t.ptr, None, 1, 1.0, None, None, None, None,
                                                                            0, ctypes.byref(K), None)),
            ("msh_tree_within_stats", lambda: L.msh_tree_within_stats(nt.ptr, None, 1, 1.0, None,
                                                                      (ctypes.c_uint64 * 4)()))):
        assert call() == N.MSH_EINVAL, name
        assert name.encode() in L.msh_last_error(), (name, L.msh_last_error())
    # the list pointers are needed only with a capacity; K always
    assert L.msh_tree_within(t.ptr, N.dptr(q), 1, 1.0, None, None, None, None, None, None, 4,
                             ctypes.byref(K)) == N.MSH_EINVAL
    assert L.msh_tree_within(t.ptr, N.dptr(q), 1, 1.0, None, None, None, None, None, None, 0, None) == N.MSH_EINVAL
    assert L.msh_tree_within(t.ptr, N.dptr(q), 1, 5.0, None, None, None, None, None, None, 0,
                             ctypes.byref(K)) == N.MSH_OK and K.value == len(tf)
    # S = 0 is MSH_OK with K = 0
    K.value = 9
    assert L.msh_points_within(h.ptr, None, 0, 1.0, None, None, None, None, 0, ctypes.byref(K)) == N.MSH_OK
    assert K.value == 0
    assert L.msh_tree_within_count_device(t.ptr, None, 0, 1.0, None, None, None) == N.MSH_OK
    with pytest.raises(TypeError):
        spatialsearch.points_within(t, q, 1.0)
    with pytest.raises(TypeError):
        spatialsearch.aabbtree_within_count(h, q, 1.0)


# ---- 12. scipy's conventions ----
def test_query_ball_point_against_scipy():
    spatial = pytest.importorskip("scipy.spatial")
    from mesh_amd import search
    from types import SimpleNamespace
    v, q = cloud(1000)
    S = q.shape[0]
    r = np.random.default_rng(77).uniform(0.05, 0.3, S)
    # scipy's boundary arithmetic is its own: no (row, point) pair of these inputs lies near its sphere
    d2 = point_d2(v, q)
    for rr in (r, np.full(S, 0.17)):
        r2 = (rr * rr)[:, None]
        assert (np.abs(d2 - r2) > 1e-9 * r2).all()
    ours = search.ClosestPointTree(SimpleNamespace(v=v))
    theirs = spatial.cKDTree(v)
    for rr in (r, 0.17):
        a = ours.query_ball_point(q, rr)
        b = theirs.query_ball_point(q, rr, return_sorted=True)
        assert a.shape == b.shape == (S,) and a.dtype == b.dtype == object
        assert all(isinstance(x, list) for x in a)
        assert all(x == y for x, y in zip(a, b))  # None on multi-point input: sorted by index
        assert any(len(x) > 3 for x in a) and any(len(x) == 0 for x in a)
        n = ours.query_ball_point(q, rr, return_length=True)
        sn = theirs.query_ball_point(q, rr, return_length=True)
        assert n.shape == sn.shape and n.dtype == sn.dtype and np.array_equal(n, sn)
        c = ours.query_ball_point(q, rr, return_sorted=False)  # nearest first
        ref = brute_points(v, q, rr)
        st = starts_of(ref[0])
        assert all(c[i] == ref[1][st[i]:st[i + 1]].tolist() for i in range(S))
        assert all(sorted(c[i]) == a[i] for i in range(S))
        assert all(x == y for x, y in zip(ours.query_ball_point(q, rr, return_sorted=True), a))
    one = ours.query_ball_point(q[5], 0.25)
    sone = theirs.query_ball_point(q[5], 0.25)
    assert isinstance(one, list) and sorted(one) == sorted(sone) and len(one) > 1
    ref = brute_points(v, q[5:6], 0.25)
    assert one == ref[1].tolist()  # None on a single point: not sorted by index (nearest first)
    assert ours.query_ball_point(q[5], 0.25, return_sorted=True) == sorted(sone)
    assert ours.query_ball_point(q[5], 0.25, return_length=True) == theirs.query_ball_point(q[5], 0.25, return_length=True)
    g = ours.query_ball_point(q[:6].reshape(2, 3, 3), 0.25)
    sg = theirs.query_ball_point(q[:6].reshape(2, 3, 3), 0.25, return_sorted=True)
    assert g.shape == sg.shape == (2, 3) and all(g[i, j] == sg[i, j] for i in range(2) for j in range(3))
    for kw in ({"p": 1}, {"eps": 0.1}):
        with pytest.raises(ValueError):
            ours.query_ball_point(q, 0.1, **kw)
    assert ours.query_ball_point(q[5], 0.25, workers=4) == one


def test_search_and_mesh_methods(meshes):
    from mesh_amd import search, spatialsearch
    from mesh_amd.mesh import Mesh
    v, f = golden(meshes, "icosphere")
    q = np.random.default_rng(51).uniform(-1.2, 1.2, (50, 3))
    r = np.linspace(0.1, 0.6, 50)
    mesh = Mesh(v=v, f=f)
    counts, idx, dist = mesh.vertices_within(q, r)
    ref = brute_points(v, q, r)
    assert same(counts, ref[0]) and idx.dtype == np.intp and np.array_equal(idx, ref[1]) and same(dist, ref[2])
    tree = mesh.compute_aabb_tree()
    a = tree.within(q, r, points=True, parts=True)
    b = spatialsearch.aabbtree_within(tree.cpp_handle, q, r, points=True, parts=True)
    assert all(same(x, y) for x, y in zip(a, b)) and a[0].sum() > 50
    assert same(tree.count_within(q, r), a[0]) and same(tree.count_within(q, 0.3), tree.within(q, 0.3)[0])
    c = mesh.faces_within(q, r, points=True)
    assert len(c) == 4 and all(same(x, y) for x, y in zip(c, a[:4]))
    assert len(mesh.faces_within(q, 0.3)) == 3
