"""All-hits ray casting on the GPU (msh_tree_raycast_count, msh_tree_raycast_all and the Python layers over them), every
comparison bit for bit.

The reference is the numpy restatement of tests/test_gpu_raycast.py (pinned to the oracle's C++ there): hit_table gives
(t, kind) per ray and face, which is the hit set itself, and ref_cast on the table with the earlier winners masked gives
entry k of every row -- its t, face and point.  The side is restated here from ray_tri's den = n . d."""
import ctypes

import numpy as np
import pytest

import test_gpu_raycast as R

pytestmark = pytest.mark.gpu

INF = np.inf
NO_FACE = R.NO_FACE
case1 = R.case1  # the 257 generic rays per mesh, with their trees and hit tables (module scope, never changed)


# ---- the reference ----
def ref_all(tri, o, d, rng=None, table=None):
    """(counts (S,), t (K,), face (K,), pt (K,3), side (K,), kind (K,)) sorted by (row, t by value, face id)"""
    tt, kind = table if table is not None else R.hit_table(tri, o, d, rng)
    tt, kind = tt.copy(), kind.copy()
    S = len(o)
    counts = (kind != 0).sum(axis=1).astype(np.uint32)
    rows, ts, faces, pts, kinds = [], [], [], [], []
    ar = np.arange(S)
    for _ in range(int(counts.max()) if S else 0):
        t, face, pt, _, hit = R.ref_cast(tri, o, d, table=(tt, kind))
        j = np.where(hit, face, 0).astype(np.int64)
        rows.append(ar[hit]); ts.append(t[hit]); faces.append(face[hit]); pts.append(pt[hit]); kinds.append(kind[ar, j][hit])
        tt[ar[hit], j[hit]] = INF
        kind[ar[hit], j[hit]] = 0
    if not rows:
        return counts, np.zeros(0), np.zeros(0, np.uint32), np.zeros((0, 3)), np.zeros(0, np.int8), np.zeros(0, np.int8)
    rows, ts, faces, pts, kinds = (np.concatenate(x) for x in (rows, ts, faces, pts, kinds))
    order = np.argsort(rows, kind="stable")  # rounds are in rank order already
    rows, ts, faces, pts, kinds = rows[order], ts[order], faces[order], pts[order], kinds[order]
    a, b, c = tri[faces, 0], tri[faces, 1], tri[faces, 2]
    with np.errstate(all="ignore"):
        den = R.vdot(R.vcross(b - a, c - a), d[rows])
    side = np.where(kinds == 2, 0, np.where(den < 0, 1, np.where(den > 0, -1, 0))).astype(np.int8)
    assert np.array_equal(np.bincount(rows, minlength=S), counts)
    return counts, ts, faces.astype(np.uint32), pts, side, kinds


def gpu_all(tree, o, d, rng=None):
    from mesh_amd import spatialsearch
    out = spatialsearch.aabbtree_raycast_all(tree, o, d, rng, points=True, sides=True)
    counts, t, face, pt, side = out
    K = int(counts.sum())
    assert counts.dtype == np.uint32 and counts.shape == (len(o),)
    assert t.dtype == np.float64 and t.shape == (K,) and face.dtype == np.uint32 and face.shape == (K,)
    assert pt.dtype == np.float64 and pt.shape == (K, 3) and side.dtype == np.int8 and side.shape == (K,)
    return out


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


def assert_same(got, ref, what=""):
    for name, g, r in zip(("counts", "t", "face", "pt", "side"), got, ref):
        assert g.shape == r.shape, "%s %s: shape %r, reference %r" % (what, name, g.shape, r.shape)
        bad = np.nonzero(~((g == r) | ((g != g) & (r != r))).reshape(len(g), -1).all(axis=1))[0]
        assert bad.size == 0, "%s %s: %d entries differ, first %d: got %r, reference %r" % (
            what, name, bad.size, bad[0], g[bad[0]], r[bad[0]])


def starts_of(counts):
    return np.concatenate([[0], np.cumsum(counts.astype(np.int64))])


def soup(N, dup=False):
    """N parallel copies of the triangle (0,0,0), (1,0,0), (0,1,0) at z = 0.125 k; dup: every triangle twice, as faces j
    and j + N"""
    z = 0.125 * np.arange(N)
    v = np.stack([np.stack([np.zeros(N), np.zeros(N), z], 1), np.stack([np.ones(N), np.zeros(N), z], 1),
                  np.stack([np.zeros(N), np.ones(N), z], 1)], 1).reshape(-1, 3)
    f = np.arange(3 * N, dtype=np.uint32).reshape(-1, 3)
    if dup:
        f = np.vstack([f, f])
    return np.ascontiguousarray(v), np.ascontiguousarray(f)


def order_samples(run):
    """run() under the kernel timers -> (its result, the number of raycast_order samples it left)"""
    from mesh_amd import _native as N
    N.timing_reset()
    N.timing_enable(True)
    try:
        out = run()
    finally:
        N.timing_enable(False)
    assert N.timing_get("raycast_count")[1] >= 1
    return out, N.timing_get("raycast_order")[1]


# ---- 1. generic rays ----
@pytest.mark.parametrize("name", R.MESHES)
def test_generic_rays(case1, name):
    tree, tri, o, d, table, _, _ = case1[name]
    ref = ref_all(tri, o, d, table=table)
    counts = ref[0]
    print("%s: rows by hits %r" % (name, np.bincount(counts).tolist()))
    assert (counts == 0).any() and (counts > 0).any() and counts.max() <= 4
    assert (ref[5] == 1).all()  # no coplanar hit
    assert ((counts >= 2).any()) == (name != "sphere1")
    got = gpu_all(tree, o, d)
    assert_same(got, ref[:5], name)
    assert set(np.unique(got[4])) <= {-1, 1}


# ---- 2. relations to the existing calls ----
@pytest.mark.parametrize("name", R.MESHES)
def test_relations(case1, name):
    from mesh_amd import spatialsearch
    tree, tri, o, d, table, _, _ = case1[name]
    counts, t, face, pt, side = gpu_all(tree, o, d)
    st = starts_of(counts)
    ft, ff, fp = spatialsearch.aabbtree_raycast(tree, o, d)
    ne = counts > 0
    first = st[:-1][ne]
    assert same(t[first], ft[ne]) and same(face[first], ff[ne]) and same(pt[first], fp[ne])
    assert np.isinf(ft[~ne]).all() and (ff[~ne] == NO_FACE).all()
    assert np.array_equal(ne, spatialsearch.aabbtree_occluded(tree, o, d))
    c2 = spatialsearch.aabbtree_raycast_count(tree, o, d)
    assert c2.dtype == np.uint32 and np.array_equal(c2, counts)
    # peeling: past entry k (one ulp above its t) the first hit is entry k + 1, or a miss after the last
    rows = np.repeat(np.arange(len(o)), counts)
    tied = np.zeros(len(o), bool)
    eq = (rows[1:] == rows[:-1]) & (t[1:] == t[:-1])
    tied[rows[1:][eq]] = True
    keep = ~tied[rows]
    assert keep.sum() >= (1 if name == "sphere1" else 100)
    k = np.nonzero(keep)[0]
    last = (k + 1 == st[1:][rows[k]])
    pr = np.stack([np.nextafter(t[k], INF), np.full(len(k), INF)], 1)
    nt, nf, npt = spatialsearch.aabbtree_raycast(tree, o[rows[k]], d[rows[k]], pr)
    nxt = np.minimum(k + 1, len(t) - 1)
    assert same(nt, np.where(last, INF, t[nxt])) and same(nf, np.where(last, NO_FACE, face[nxt]).astype(np.uint32))
    assert same(npt, np.where(last[:, None], np.nan, pt[nxt]))


# ---- 3. the oracle ----
@pytest.mark.parametrize("name", ["sphere", "cylinder"])
def test_pinned_to_the_oracle(meshes, oracle, name):
    """nearest_alongnormal takes the minimum of |pt - p| over all intersections of the two rays (p, (p + n) - p) and
    (p, (p - n) - p): the same minimum over the two hit lists, computed as the oracle computes it, is its distance, and
    the rows whose lists are both empty are its no-hit rows"""
    from mesh_amd import spatialsearch
    v, f = meshes[name + "_v"], meshes[name + "_f"]
    tree = spatialsearch.aabbtree_compute(v, f)
    rng = np.random.default_rng(1)
    lo, hi = v.min(0), v.max(0)
    p = rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (2000, 3))
    n = rng.normal(size=(2000, 3))
    bd, bf, bpt = oracle.brute_alongnormal(v, f, p, n)
    best = np.full(2000, INF)
    total = np.zeros(2000, np.int64)
    for dk in ((p + n) - p, (p - n) - p):
        counts, t, face, pt = spatialsearch.aabbtree_raycast_all(tree, p, dk, points=True)
        rows = np.repeat(np.arange(2000), counts)
        e = pt - p[rows]
        dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        np.minimum.at(best, rows, dist)
        total += counts
    hs = bd < 1e100
    print("%s: %d hitting rows, %d hits in all" % (name, hs.sum(), total.sum()))
    assert hs.sum() > 500 and (~hs).sum() > 500
    assert np.array_equal(total == 0, ~hs)
    assert np.array_equal(np.where(total == 0, 1e100, best), bd)


# ---- 4. row counts ----
@pytest.mark.parametrize("S", [1, 63, 64, 65])
def test_ragged_sizes(case1, S):
    tree, tri, o, d, table, _, _ = case1["sphere"]
    ref = ref_all(tri, o[:S], d[:S], table=(table[0][:S], table[1][:S]))
    assert_same(gpu_all(tree, o[:S].copy(), d[:S].copy()), ref[:5], "S=%d" % S)


def test_no_rows(case1):
    from mesh_amd import _native as N, spatialsearch
    tree = case1["sphere"][0]
    e = np.zeros((0, 3))
    counts, t, face, pt, side = gpu_all(tree, e, e)
    assert counts.shape == (0,) and t.shape == (0,) and pt.shape == (0, 3) and side.shape == (0,)
    out = spatialsearch.aabbtree_raycast_all(tree, e, e)
    assert len(out) == 3
    c = spatialsearch.aabbtree_raycast_count(tree, e, e)
    assert c.shape == (0,) and c.dtype == np.uint32
    K = N._sz(5)
    assert N.lib().msh_tree_raycast_all(tree.ptr, None, None, None, 0, None, None, None, None, None, 0,
                                        ctypes.byref(K)) == N.MSH_OK and K.value == 0


# ---- 5. long rows ----
def long_rows(N):
    """rays against soup(N): rows of N hits (unit and half-length directions), misses and rows a range leaves one hit"""
    o = np.array([[0.25, 0.25, -1.0], [5.0, 5.0, -1.0], [0.25, 0.25, -1.0], [0.125, 0.5, -1.0], [0.25, 0.25, -1.0],
                  [0.25, 0.25, 40.0], [0.5, 0.25, -1.0]])
    d = np.array([[0, 0, 1.0], [0, 0, 1.0], [0, 0, 0.5], [0, 0, 1.0], [0, 0, 1.0], [0, 0, 1.0], [0, 0, 1.0]])
    rr = np.array([[0, INF], [0, INF], [0, INF], [1.125, 1.125], [0, 1.0], [0, INF], [0, INF]])
    rep = 3
    return np.tile(o, (rep, 1)), np.tile(d, (rep, 1)), np.tile(rr, (rep, 1))


def test_long_rows():
    from mesh_amd import spatialsearch
    Nf = 100
    v, f = soup(Nf)
    tree = spatialsearch.aabbtree_compute(v, f)
    tri = R.tris_of(v, f)
    o, d, rr = long_rows(Nf)
    ref = ref_all(tri, o, d, rr)
    assert ref[0][:7].tolist() == [100, 0, 100, 1, 1, 0, 100]
    got, n_order = order_samples(lambda: gpu_all(tree, o, d, rr))
    assert n_order >= 1  # a row above 32 hits: the radix path
    assert_same(got, ref[:5], "soup of 100")
    counts, t, face, pt, side = got
    st = starts_of(counts)
    k = np.arange(100)
    assert np.array_equal(t[st[0]:st[1]], 1.0 + 0.125 * k) and np.array_equal(face[st[0]:st[1]], k)
    assert np.array_equal(t[st[2]:st[3]], 2.0 * (1.0 + 0.125 * k)) and np.array_equal(face[st[2]:st[3]], k)
    assert t[st[3]] == 1.125 and face[st[3]] == 1 and t[st[4]] == 1.0 and face[st[4]] == 0
    assert np.array_equal(pt[st[0]:st[1]], np.stack([np.full(100, 0.25), np.full(100, 0.25), 0.125 * k], 1))
    assert (side == -1).all()  # the normal of every triangle is +z, and so is every direction: the backs


@pytest.mark.parametrize("hits", [32, 33])
def test_lane_and_radix_boundary(hits):
    """33 triangles, ranges that admit exactly 32 and exactly 33 of them: the longest row decides between the lanes'
    own ordering (<= 32, no raycast_order sample) and the radix sorts (a sample)"""
    from mesh_amd import spatialsearch
    v, f = soup(33)
    tree = spatialsearch.aabbtree_compute(v, f)
    tri = R.tris_of(v, f)
    o = np.array([[0.25, 0.25, -1.0], [5.0, 5.0, -1.0], [0.25, 0.25, 40.0], [0.125, 0.25, -1.0]])
    d = np.array([[0, 0, 1.0], [0, 0, 1.0], [0, 0, -2.0], [0, 0, 0.5]])
    t_end = 1.0 + 0.125 * (hits - 1)
    rr = np.array([[0, t_end], [0, INF], [0, 0.5 * (40.0 - 0.125 * (33 - hits))], [0, 2 * t_end]])
    ref = ref_all(tri, o, d, rr)
    assert ref[0].tolist() == [hits, 0, hits, hits]
    got, n_order = order_samples(lambda: gpu_all(tree, o, d, rr))
    assert (n_order >= 1) == (hits == 33)
    assert_same(got, ref[:5], "%d hits" % hits)
    st = starts_of(got[0])
    assert np.array_equal(got[2][st[2]:st[3]], 32 - np.arange(hits))  # from above: descending z, ascending t
    assert np.array_equal(got[1][st[3]:st[4]], 2.0 * (1.0 + 0.125 * np.arange(hits)))
    assert (got[4][st[2]:st[3]] == 1).all() and (got[4][st[0]:st[1]] == -1).all()


# ---- 6. ties ----
@pytest.mark.parametrize("Nf", [10, 20])
def test_duplicated_faces(Nf):
    """faces j and j + N are the same triangle: equal t, ascending face id (N = 10: 20 hits, the lanes' ordering; N = 20:
    40 hits, the radix sorts)"""
    from mesh_amd import spatialsearch
    v, f = soup(Nf, dup=True)
    tree = spatialsearch.aabbtree_compute(v, f)
    tri = R.tris_of(v, f)
    o = np.array([[0.25, 0.25, -1.0], [0.5, 0.125, -3.0], [7.0, 7.0, 0.0]])
    d = np.array([[0, 0, 1.0], [0, 0, 2.0], [0, 0, 1.0]])
    got, n_order = order_samples(lambda: gpu_all(tree, o, d))
    assert (n_order >= 1) == (2 * Nf > 32)
    assert_same(got, ref_all(tri, o, d)[:5], "duplicated soup")
    counts, t, face, _, _ = got
    assert counts.tolist() == [2 * Nf, 2 * Nf, 0]
    k = np.arange(Nf)
    assert np.array_equal(t[:2 * Nf], np.repeat(1.0 + 0.125 * k, 2))
    assert np.array_equal(face[:2 * Nf], np.stack([k, k + Nf], 1).reshape(-1))
    assert np.array_equal(t[2 * Nf:], np.repeat(0.5 * (3.0 + 0.125 * k), 2))
    assert np.array_equal(face[2 * Nf:], np.stack([k, k + Nf], 1).reshape(-1))


def test_cube_vertex_and_edge():
    """0/1 coordinates: every determinant is exact.  The diagonal meets the six faces around vertex (0,0,0) at t = 1 and
    the six around (1,1,1) at t = 2; the ray through the midpoints of the edges y = z = 0 and y = z = 1 meets the two
    faces of each"""
    from mesh_amd import spatialsearch
    v, f = R.unit_cube()
    tree = spatialsearch.aabbtree_compute(v, f)
    tri = R.tris_of(v, f)
    o = np.array([[-1.0, -1.0, -1.0], [0.5, -1.0, -1.0]])
    d = np.array([[1.0, 1.0, 1.0], [0.0, 1.0, 1.0]])
    got = gpu_all(tree, o, d)
    assert_same(got, ref_all(tri, o, d)[:5], "cube")
    counts, t, face, pt, side = got
    assert counts.tolist() == [12, 4]
    assert t.tolist() == [1.0] * 6 + [2.0] * 6 + [1.0, 1.0, 2.0, 2.0]
    assert face.tolist() == [0, 1, 4, 5, 8, 9, 2, 3, 6, 7, 10, 11, 1, 4, 3, 6]
    assert np.array_equal(pt[:6], np.zeros((6, 3))) and np.array_equal(pt[6:12], np.ones((6, 3)))
    assert np.array_equal(pt[12:14], [[0.5, 0, 0]] * 2) and np.array_equal(pt[14:], [[0.5, 1, 1]] * 2)


# ---- 7. coplanar ----
def test_coplanar_hit():
    from mesh_amd import spatialsearch
    v, f = soup(8)
    tree = spatialsearch.aabbtree_compute(v, f)
    tri = R.tris_of(v, f)
    o = np.array([[2.0, 0.25, 0.375], [0.25, 0.25, -1.0], [2.0, 0.25, 0.375]])
    d = np.array([[-1.0, 0, 0], [0, 0, 1.0], [-1.0, 0, 0]])
    rr = np.array([[0, INF], [0, INF], [1.5, INF]])  # the third row starts inside the overlap [1.25, 2]
    ref = ref_all(tri, o, d, rr)
    assert ref[0].tolist() == [1, 8, 1] and ref[5][0] == 2 and ref[5][9] == 2
    got = gpu_all(tree, o, d, rr)
    assert_same(got, ref[:5], "coplanar")
    counts, t, face, pt, side = got
    assert t[0] == 1.25 and face[0] == 3 and side[0] == 0 and np.array_equal(pt[0], o[0] + t[0] * d[0])
    assert t[9] == 1.5 and face[9] == 3 and side[9] == 0 and np.array_equal(pt[9], o[2] + t[9] * d[2])
    assert (side[1:9] == -1).all()


# ---- 8. sides and parity ----
def test_sides_and_parity(meshes):
    from mesh_amd import spatialsearch
    v, f = meshes["sphere_v"], meshes["sphere_f"]
    tree = spatialsearch.aabbtree_compute(v, f)
    tri = R.tris_of(v, f)
    c = 0.5 * (v.min(0) + v.max(0))
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = np.abs(((tri[:, 0] - c) * n).sum(1) / np.linalg.norm(n, axis=1)).min()  # the nearest face plane
    r_out = np.linalg.norm(v - c, axis=1).max()
    rng = np.random.default_rng(8)
    S = 512
    u = rng.normal(size=(S, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    inside = np.arange(S) % 2 == 0
    o = c + u * np.where(inside, 0.95 * r_in * rng.uniform(0, 1, S), 1.05 * r_out * rng.uniform(1, 3, S))[:, None]
    d = rng.normal(size=(S, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[1::4] = c - o[1::4] + rng.normal(size=(S // 4, 3)) * 0.3 * r_in  # half of the outside rays aimed at the mesh
    d /= np.linalg.norm(d, axis=1)[:, None]
    d *= 10.0 ** rng.uniform(-3, 3, (S, 1))
    counts, t, face, side = spatialsearch.aabbtree_raycast_all(tree, o, d, sides=True)
    rows = np.repeat(np.arange(S), counts)
    out = np.zeros(S, bool)
    out[rows[side == 0]] = True
    eq = (rows[1:] == rows[:-1]) & (t[1:] == t[:-1])
    out[rows[1:][eq]] = True
    print("parity: %d rows left out, hits per row up to %d, %d outside rows hit" % (
        out.sum(), counts.max(), (counts[~inside] > 0).sum()))
    assert out.sum() <= S // 100
    assert (counts[~inside] > 0).sum() > 50
    keep = ~out
    assert np.array_equal((counts % 2 == 1)[keep], inside[keep])
    sums = np.zeros(S, np.int64)
    np.add.at(sums, rows, side.astype(np.int64))
    s_in = np.unique(sums[keep & inside])
    assert len(s_in) == 1 and abs(int(s_in[0])) == 1
    assert (sums[keep & ~inside] == 0).all()


# ---- 9. ranges ----
def test_ranges(case1):
    tree, tri, o, d, table, _, _ = case1["sphere"]
    S = len(o)
    base = ref_all(tri, o, d, table=table)
    counts, t = base[0], base[1]
    st = starts_of(counts)
    two = counts >= 2
    assert two.sum() > 50
    t2 = np.where(two, t[np.minimum(st[:-1] + 1, len(t) - 1)], 0.0)
    zero, inf = np.zeros(S), np.full(S, INF)
    blocks = {
        "the second hit alone": np.stack([t2, np.where(two, t2, INF)], 1),
        "ends one ulp below the second": np.stack([zero, np.where(two, np.nextafter(t2, -INF), INF)], 1),
        "ends at the second": np.stack([zero, np.where(two, t2, INF)], 1),
        "starts one ulp above the second": np.stack([np.where(two, np.nextafter(t2, INF), 0.0), inf], 1),
        "negative start": np.stack([np.full(S, -5.0), inf], 1),
    }
    names = list(blocks)
    oo, dd = np.tile(o, (len(names), 1)), np.tile(d, (len(names), 1))
    rr = np.vstack([blocks[k] for k in names])
    got = gpu_all(tree, oo, dd, rr)
    assert_same(got, ref_all(tri, oo, dd, rr)[:5], "ranges")
    gc = got[0].reshape(len(names), S)
    gst = starts_of(got[0])
    n_at = np.array([(t[st[i]:st[i + 1]] == t2[i]).sum() for i in range(S)])
    n_below = np.array([(t[st[i]:st[i + 1]] < t2[i]).sum() for i in range(S)])
    assert np.array_equal(gc[0][two], n_at[two])
    first = gst[:-1][:S][two]
    assert np.array_equal(got[1][first], t2[two])
    assert np.array_equal(gc[1][two], n_below[two]) and np.array_equal(gc[2][two], (n_below + n_at)[two])
    assert np.array_equal(gc[3][two], (counts - n_below - n_at)[two])
    assert np.array_equal(gc[4], counts)
    neg = tuple(x[gst[4 * S]:] if i else x[4 * S:] for i, x in enumerate(got))
    assert_same(neg, base[:5], "t0 < 0 behaves as 0")


def test_rows_that_cannot_be_cast(case1):
    tree, tri, o, d, table, _, _ = case1["icosphere"]
    o, d = o[:64].copy(), d[:64].copy()
    rng = np.tile([0.0, INF], (64, 1))
    good = gpu_all(tree, o, d, rng)
    gst = starts_of(good[0])
    bad = {3: ("o", np.nan), 10: ("o", INF), 17: ("d", np.nan), 24: ("d", -INF), 31: ("d", 0.0), 38: ("r", np.nan),
           45: ("r", None), 52: ("r1", np.nan)}
    for i, (what, val) in bad.items():
        if what == "o":
            o[i, i % 3] = val
        elif what == "d" and val == 0.0:
            d[i] = 0.0
        elif what == "d":
            d[i, i % 3] = val
        elif what == "r" and val is None:
            rng[i] = [2.0, 1.0]  # t0 > t1
        elif what == "r":
            rng[i, 0] = val
        else:
            rng[i, 1] = val
    got = gpu_all(tree, o, d, rng)
    rows = np.array(sorted(bad))
    assert (got[0][rows] == 0).all()
    others = np.setdiff1d(np.arange(64), rows)
    assert np.array_equal(got[0][others], good[0][others]) and good[0][others].sum() > 0
    keep = np.isin(np.repeat(np.arange(64), good[0]), others)
    for g, h in zip(got[1:], good[1:]):
        assert same(g, h[keep])
    assert_same(got, ref_all(tri, o, d, rng)[:5], "uncastable")
    assert gst[-1] > got[0].sum()  # the bad rows had hits before


# ---- 10. the cap protocol through the C ABI ----
def abi_all(tree, o, d, rr, cap, want_t=True, want_pt=True, want_side=True, pad=3):
    """msh_tree_raycast_all with arrays of cap + pad entries filled with sentinels -> (K, counts, t, face, pt, side)"""
    from mesh_amd import _native as N
    S = len(o)
    counts = np.full(S, 0xDEADBEEF, np.uint32)
    t = np.full(cap + pad, -7.0)
    face = np.full(cap + pad, 0xABABABAB, np.uint32)
    pt = np.full((cap + pad, 3), -7.0)
    side = np.full(cap + pad, 77, np.int8)
    K = N._sz(0)
    i8p = ctypes.POINTER(ctypes.c_int8)
    N.check(N.lib().msh_tree_raycast_all(tree.ptr, N.dptr(o), N.dptr(d), N.dptr(rr), S, N.uptr(counts),
                                         N.dptr(t) if want_t else None, N.uptr(face) if want_t else None,
                                         N.dptr(pt) if want_pt else None,
                                         side.ctypes.data_as(i8p) if want_side else None, cap, ctypes.byref(K)))
    return K.value, counts, t, face, pt, side


def test_cap_protocol():
    from mesh_amd import spatialsearch
    v, f = soup(100)
    tree = spatialsearch.aabbtree_compute(v, f)
    o, d, rr = long_rows(100)
    o, d, rr = o[:14], d[:14], rr[:14]  # the first and the last row are long ones
    o[13], d[13], rr[13] = o[0], d[0], rr[0]
    full = gpu_all(tree, o, d, rr)
    Kf = int(full[0].sum())
    assert full[0][0] == 100 and full[0][-1] == 100 and Kf > 500
    K, counts, *_ = abi_all(tree, o, d, rr, 0, want_t=False, want_pt=False, want_side=False)
    assert K == Kf and np.array_equal(counts, full[0])
    for cap in (Kf - 1, 1, 150, Kf, Kf + 2):
        K, counts, t, face, pt, side = abi_all(tree, o, d, rr, cap)
        n = min(cap, Kf)
        assert K == Kf and np.array_equal(counts, full[0]), cap
        assert t[:n].tobytes() == full[1][:n].tobytes() and face[:n].tobytes() == full[2][:n].tobytes(), cap
        assert pt[:n].tobytes() == full[3][:n].tobytes() and side[:n].tobytes() == full[4][:n].tobytes(), cap
        assert (t[n:] == -7.0).all() and (face[n:] == 0xABABABAB).all() and (pt[n:] == -7.0).all() and (side[n:] == 77).all()
    # pt NULL and side NULL each leave the other columns unchanged
    K, counts, t, face, pt, side = abi_all(tree, o, d, rr, Kf, want_pt=False)
    assert K == Kf and same(t[:Kf], full[1]) and same(face[:Kf], full[2]) and same(side[:Kf], full[4]) and (pt == -7.0).all()
    K, counts, t, face, pt, side = abi_all(tree, o, d, rr, Kf, want_side=False)
    assert K == Kf and same(t[:Kf], full[1]) and same(face[:Kf], full[2]) and same(pt[:Kf], full[3]) and (side == 77).all()
    # the lanes' ordering under a cap: short rows only
    o2, d2, rr2 = o[[3, 4, 3, 4, 3]], d[[3, 4, 3, 4, 3]], np.tile([0.0, 1.25], (5, 1))
    full2 = gpu_all(tree, o2, d2, rr2)
    assert full2[0].tolist() == [3] * 5
    for cap in (1, 4, 14):
        K, counts, t, face, pt, side = abi_all(tree, o2, d2, rr2, cap)
        assert K == 15 and np.array_equal(counts, full2[0])
        assert same(t[:cap], full2[1][:cap]) and same(face[:cap], full2[2][:cap]) and same(pt[:cap], full2[3][:cap])
        assert same(side[:cap], full2[4][:cap]) and (t[cap:] == -7.0).all() and (side[cap:] == 77).all()


# ---- 11. determinism and independence ----
def test_determinism_and_independence(meshes):
    from mesh_amd import spatialsearch
    v, f = meshes["icosphere_v"], meshes["icosphere_f"]
    tree = spatialsearch.aabbtree_compute(v, f)
    tri = R.tris_of(v, f)
    S = 5000  # above the threshold of the query sort: rays run in the slot order of their origins
    o, d = R.generic_rays(tri, S, seed=11)
    rr = np.tile([0.0, INF], (S, 1))
    rr[::3] = [0.5, 20.0]
    a = gpu_all(tree, o, d, rr)
    b = gpu_all(tree, o, d, rr)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert_same(a, ref_all(tri, o, d, rr)[:5], "sorted path")
    assert (a[0] >= 2).sum() > 500 and (a[0] == 0).sum() > 500
    perm = np.random.default_rng(5).permutation(S)
    p = gpu_all(tree, o[perm], d[perm], rr[perm])
    assert np.array_equal(p[0], a[0][perm])
    st = starts_of(a[0])
    src = np.concatenate([np.arange(st[r], st[r + 1]) for r in perm])
    for x, y in zip(p[1:], a[1:]):
        assert x.tobytes() == y[src].tobytes()


# ---- 12. deep tree ----
def test_deep_tree():
    """the mesh and the rays of test_gpu_raycast.test_deep_tree: a walk that never prunes, on a tree deeper than the LDS
    stack"""
    from mesh_amd import spatialsearch
    rng = np.random.default_rng(22)
    pts = np.vstack([rng.normal(size=(3000, 3)) * 1e-4, rng.normal(size=(3000, 3)) * 100])
    v = np.repeat(pts, 3, axis=0) + rng.normal(size=(18000, 3)) * 1e-6
    f = np.arange(18000, dtype=np.uint32).reshape(-1, 3)
    tree = spatialsearch.aabbtree_compute(v, f)
    assert tree.info().max_depth > 16
    tri = R.tris_of(v, f)
    rng = np.random.default_rng(61)
    fi = rng.choice(6000, 384, replace=False)
    n = rng.normal(size=(512, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    cen = tri[fi].mean(axis=1)
    o = np.vstack([cen + rng.uniform(-2e-4, 2e-4, (384, 1)) * n[:384], rng.normal(size=(128, 3)) * 50])
    d = n * 10.0 ** rng.uniform(-2, 2, (512, 1))
    d[:384:2] *= -1.0
    d[384:448] = tri[rng.integers(0, 3000, 64)].mean(axis=1) - o[384:448]
    ref = ref_all(tri, o, d)
    print("deep tree: rows by hits %r" % np.bincount(ref[0]).tolist())
    assert (ref[0] > 0).sum() >= 100 and (ref[0] == 0).sum() >= 100
    assert_same(gpu_all(tree, o, d), ref[:5], "deep tree")


# ---- 13. extra faces ----
def test_extra_faces(meshes):
    from mesh_amd import _native as N
    v, f = meshes["icosphere_v"], meshes["icosphere_f"]
    T = len(f)
    lo, hi = v.min(0), v.max(0)
    z = hi[2] + 0.5
    ev = np.array([[lo[0] - 1, lo[1] - 1, z], [hi[0] + 1, lo[1] - 1, z], [hi[0] + 1, hi[1] + 1, z], [lo[0] - 1, hi[1] + 1, z]])
    ef = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
    tree = N.build_tree(np.ascontiguousarray(v), np.ascontiguousarray(f), ev, ef)
    tri = np.vstack([R.tris_of(v, f), R.tris_of(ev, ef)])
    rng = np.random.default_rng(3)
    o = np.column_stack([rng.uniform(lo[0], hi[0], 128), rng.uniform(lo[1], hi[1], 128), np.full(128, z + 1.0)])
    o[64:, 2] = lo[2] - 1.0  # from below: the mesh first, the extra faces last
    d = np.zeros((128, 3))
    d[:64, 2], d[64:, 2] = -0.5, 3.0
    got = gpu_all(tree, o, d)
    assert_same(got, ref_all(tri, o, d)[:5], "extra faces")
    counts, t, face, _, _ = got
    st = starts_of(counts)
    assert (face[st[:64]] >= T).all() and (face[st[:64]] < T + 2).all()
    assert (face[st[65:129] - 1] >= T).all() and (counts >= 3).any()


# ---- 14. device entry points and the pipeline ----
def device_all(tree, o, d, rr, cap, with_pt=True, with_side=True):
    import torch
    from mesh_amd import _native as N
    L, vp, dev, S = N.lib(), ctypes.c_void_p, torch.device("cuda:0"), len(o)
    do, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    dr = torch.from_numpy(rr).to(dev) if rr is not None else None
    dc = torch.empty(S, dtype=torch.int32, device=dev)
    dt = torch.empty(cap, dtype=torch.float64, device=dev)
    df = torch.empty(cap, dtype=torch.int32, device=dev)
    dp = torch.empty((cap, 3), dtype=torch.float64, device=dev)
    ds = torch.empty(cap, dtype=torch.int8, device=dev)
    K = N._sz(0)
    N.check(L.msh_tree_raycast_all_device(tree.ptr, vp(do.data_ptr()), vp(dd.data_ptr()),
                                          vp(dr.data_ptr()) if dr is not None else None, S, vp(dc.data_ptr()),
                                          vp(dt.data_ptr()) if cap else None, vp(df.data_ptr()) if cap else None,
                                          vp(dp.data_ptr()) if cap and with_pt else None,
                                          vp(ds.data_ptr()) if cap and with_side else None, cap, ctypes.byref(K), None))
    torch.cuda.synchronize()
    n = min(cap, K.value)
    return (K.value, dc.cpu().numpy().view(np.uint32), dt.cpu().numpy()[:n], df.cpu().numpy().view(np.uint32)[:n],
            dp.cpu().numpy()[:n], ds.cpu().numpy()[:n])


def device_count(tree, o, d, rr):
    import torch
    from mesh_amd import _native as N
    vp, dev, S = ctypes.c_void_p, torch.device("cuda:0"), len(o)
    do, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    dr = torch.from_numpy(rr).to(dev) if rr is not None else None
    dc = torch.empty(S, dtype=torch.int32, device=dev)
    N.check(N.lib().msh_tree_raycast_count_device(tree.ptr, vp(do.data_ptr()), vp(dd.data_ptr()),
                                                  vp(dr.data_ptr()) if dr is not None else None, S, vp(dc.data_ptr()),
                                                  None))
    torch.cuda.synchronize()
    return dc.cpu().numpy().view(np.uint32)


def test_device_entry_points(meshes):
    from mesh_amd import spatialsearch
    v, f = meshes["icosphere_v"], meshes["icosphere_f"]
    tree = spatialsearch.aabbtree_compute(v, f)
    S = 5000
    o, d = R.generic_rays(R.tris_of(v, f), S, seed=11)
    rr = np.tile([0.0, INF], (S, 1))
    rr[::3] = [0.5, 20.0]
    host = gpu_all(tree, o, d, rr)
    Kf = int(host[0].sum())
    K0, c0, *_ = device_all(tree, o, d, rr, 0)
    assert K0 == Kf and np.array_equal(c0, host[0])
    K, counts, t, face, pt, side = device_all(tree, o, d, rr, Kf)
    assert K == Kf
    for g, h in zip((counts, t, face, pt, side), host):
        assert g.tobytes() == h.tobytes()
    K, counts, t, face, pt, side = device_all(tree, o, d, rr, Kf // 2, with_pt=False)
    assert K == Kf and t.tobytes() == host[1][:Kf // 2].tobytes() and side.tobytes() == host[4][:Kf // 2].tobytes()
    assert np.array_equal(device_count(tree, o, d, rr), host[0])
    hn = gpu_all(tree, o, d)  # a NULL range on the device is [0, inf]
    assert np.array_equal(device_count(tree, o, d, None), hn[0]) and not np.array_equal(hn[0], host[0])
    Kn, cn, tn, *_ = device_all(tree, o, d, None, int(hn[0].sum()))
    assert np.array_equal(cn, hn[0]) and tn.tobytes() == hn[1].tobytes()
    from mesh_amd.mesh import Mesh
    from mesh_amd.search import AabbTree
    m = Mesh(v=v, f=f).ray_cast_all(o[:65], d[:65], rr[:65], points=True, sides=True)
    n65 = int(host[0][:65].sum())
    assert np.array_equal(m[0], host[0][:65]) and all(same(a, b[:n65]) for a, b in zip(m[1:], host[1:]))
    at = AabbTree.__new__(AabbTree)
    at.cpp_handle = tree
    assert np.array_equal(at.ray_count(o, d, rr), host[0])
    a3 = at.ray_cast_all(o, d, rr)
    assert len(a3) == 3 and same(a3[1], host[1]) and same(a3[2], host[2])


def test_count_chunk_pipeline(meshes, monkeypatch):
    """msh_tree_raycast_count through the slab pipeline, as test_gpu_raycast.test_chunk_pipeline sends the first-hit
    call: 350,001 rays are 18 MB of rows (24 + 24 + 4 B each with a NULL range), above the 16 MB small-call limit;
    MESH_AMD_HOST_CHUNK = 100,001 makes four chunks of an odd number of rows, the last ragged.  The counts must equal
    the _device entry point's, with results carved from the pinned pool and with the pool disabled (staged)."""
    from mesh_amd import _native as N, spatialsearch
    v, f = meshes["icosphere_v"], meshes["icosphere_f"]
    tree = spatialsearch.aabbtree_compute(v, f)
    S, chunk = 350001, 100001
    assert S * (24 + 24 + 4) > 16 << 20 and S % 2 == 1 and chunk % 2 == 1 and S % chunk not in (0, chunk - 1)
    o, d = R.generic_rays(R.tris_of(v, f), S, seed=13)
    rr = np.tile([0.0, INF], (S, 1))
    rr[::3] = [0.5, 20.0]
    rr[5::1001] = [2.0, 1.0]  # rows that cannot be cast, in every chunk
    dev_r, dev_n = device_count(tree, o, d, rr), device_count(tree, o, d, None)
    assert 0 < dev_r.sum() < dev_n.sum() and (dev_r[5::1001] == 0).all() and dev_n.max() >= 2
    L = N.lib()
    monkeypatch.setenv("MESH_AMD_HOST_CHUNK", str(chunk))
    monkeypatch.setattr(N, "PINNED_MIN_BYTES", 1 << 16)
    for pool in (True, False):
        if not pool:
            assert L.msh_host_pool_trim() == 0
            monkeypatch.setenv("MESH_AMD_PINNED_POOL_MB", "0")
        N.timing_reset()
        N.timing_enable(True)
        cn = spatialsearch.aabbtree_raycast_count(tree, o, d)
        N.timing_enable(False)
        assert N.timing_get("raycast_count")[1] == 4  # one launch per chunk
        assert (cn.base is not None) == pool
        assert np.array_equal(cn, dev_n), "NULL range (pool %s)" % pool
        assert np.array_equal(spatialsearch.aabbtree_raycast_count(tree, o, d, rr), dev_r), "range (pool %s)" % pool
    monkeypatch.delenv("MESH_AMD_PINNED_POOL_MB")


# ---- 15. refusals ----
def test_other_tree_kinds_are_refused(meshes):
    from mesh_amd import _native as N
    v, f = np.ascontiguousarray(meshes["icosphere_v"]), np.ascontiguousarray(meshes["icosphere_f"])
    L = N.lib()
    o, d = np.zeros((1, 3)), np.ones((1, 3))
    counts, t, face = np.zeros(1, np.uint32), np.zeros(1), np.zeros(1, np.uint32)
    K = N._sz(0)
    for h in (N.build_ntree(v, f, 0.1), N.build_points(v), N.build_batch(np.ascontiguousarray(np.stack([v, v + 1.0])), f)):
        calls = {
            "msh_tree_raycast_count": lambda: L.msh_tree_raycast_count(h.ptr, N.dptr(o), N.dptr(d), None, 1,
                                                                       N.uptr(counts)),
            "msh_tree_raycast_count_device": lambda: L.msh_tree_raycast_count_device(h.ptr, None, None, None, 1, None,
                                                                                     None),
            "msh_tree_raycast_all": lambda: L.msh_tree_raycast_all(h.ptr, N.dptr(o), N.dptr(d), None, 1, N.uptr(counts),
                                                                   N.dptr(t), N.uptr(face), None, None, 1,
                                                                   ctypes.byref(K)),
            "msh_tree_raycast_all_device": lambda: L.msh_tree_raycast_all_device(h.ptr, None, None, None, 1, None, None,
                                                                                 None, None, None, 0, ctypes.byref(K),
                                                                                 None),
        }
        for name, call in calls.items():
            assert call() == N.MSH_EINVAL, (name, h.kind)
            assert name.encode() + b":" in L.msh_last_error(), (name, L.msh_last_error())
