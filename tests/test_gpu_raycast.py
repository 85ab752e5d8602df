"""Ray casting on the GPU (msh_tree_raycast, msh_tree_occluded and the Python layers over them), every comparison bit
for bit.

The reference lives here: a numpy fp64 restatement of ray_tri, cgal_plane_line, heidrich_bary and the first-hit
selection with the operation order of mesh_amd/csrc/common.h (vdot is (ax bx + ay by) + az bz; vcross and plane_of as
written there), every ray against every face, and a scalar restatement of coplanar_ray_tri for the few coplanar rows.
test_pinned_to_the_oracle ties it to the oracle's C++ (brute_alongnormal, brute_visibility) through the relations the
header states, so the kernel is not only compared with this file's own numpy."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INF = np.inf
NO_FACE = 0xFFFFFFFF


# ---- the restatement ----
def vdot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def vcross(v, w):
    return np.stack([v[..., 1] * w[..., 2] - v[..., 2] * w[..., 1], v[..., 2] * w[..., 0] - v[..., 0] * w[..., 2],
                     v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0]], axis=-1)


def coplanar_ray_tri(p, d, a, b, c, t0, t1):
    """rays.h coplanar_ray_tri on one ray and one triangle: the entry parameter, or None"""
    n = vcross(b - a, c - a)
    if n[0] == 0.0 and n[1] == 0.0 and n[2] == 0.0:
        return None
    tlo, thi = t0, t1
    for s, t in ((a, b), (b, c), (c, a)):
        et = t - s
        f0 = vdot(n, vcross(et, p - s))
        f1 = vdot(n, vcross(et, d))
        if f1 == 0.0:
            if f0 < 0.0:
                return None
        else:
            tt = -f0 / f1
            if f1 > 0.0:
                tlo = max(tlo, tt)
            else:
                thi = min(thi, tt)
    if tlo > thi:
        return None
    return tlo


def castable(o, d, rng):
    ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1)
    with np.errstate(invalid="ignore"):
        return ok & (rng[:, 0] <= rng[:, 1])


def hit_table(tri, o, d, rng):
    """(t (S,F), kind (S,F)): per ray and face the hit parameter (inf: no hit in the row's range) and ray_tri's kind"""
    S = o.shape[0]
    if rng is None:
        rng = np.tile([0.0, INF], (S, 1))
    ok = castable(o, d, rng)
    t0 = np.maximum(rng[:, 0], 0.0)[:, None]
    t1 = rng[:, 1][:, None]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    p, dd = o[:, None, :], d[:, None, :]
    with np.errstate(all="ignore"):
        u, v, w = a - p, b - p, c - p
        s0, s1, s2 = vdot(vcross(u, v), dd), vdot(vcross(v, w), dd), vdot(vcross(w, u), dd)
        side = ((s0 >= 0) & (s1 >= 0) & (s2 >= 0)) | ((s0 <= 0) & (s1 <= 0) & (s2 <= 0))
        n = vcross(b - a, c - a)
        num, den = vdot(n, u), vdot(n, dd)
        cop = (den == 0) | ((s0 == 0) & (s1 == 0) & (s2 == 0))
        t = num / den
        proper = side & ~cop & (t >= t0) & (t <= t1) & ok[:, None]
    tt = np.where(proper, t, INF)
    kind = proper.astype(np.int8)
    for i, j in zip(*np.nonzero(side & cop & (num == 0) & ok[:, None])):
        e = coplanar_ray_tri(o[i], d[i], tri[j, 0], tri[j, 1], tri[j, 2], t0[i, 0], t1[i, 0])
        if e is not None and e == e:
            tt[i, j] = e
            kind[i, j] = 2
    return tt, kind


def heidrich_bary(p, a, b, c):
    u, v = b - a, c - a
    n = vcross(u, v)
    s = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
    s = np.where(s == 0.0, 2.220446049250313e-16, s)
    inv = 1.0 / s
    w = p - a
    b2 = vdot(vcross(u, w), n) * inv
    b1 = vdot(vcross(w, v), n) * inv
    return np.stack([1.0 - b1 - b2, b1, b2], axis=-1)


def ref_cast(tri, o, d, rng=None, table=None):
    """(t, face, pt, w, hit) of the first hits: lexicographic minimum of (t, face id), alongnormal's point, the weights"""
    tt, kind = table if table is not None else hit_table(tri, o, d, rng)
    S = o.shape[0]
    j = np.argmin(tt, axis=1)  # the first of equal minima: the smaller face id
    t = tt[np.arange(S), j]
    hit = kind.any(axis=1)
    face = np.where(hit, j, NO_FACE).astype(np.uint32)
    t = np.where(hit, t, INF)
    a, b, c = tri[j, 0], tri[j, 1], tri[j, 2]
    with np.errstate(all="ignore"):
        # plane_of(a, b, c) and cgal_plane_line
        rp, rq = a - c, b - c
        A = rp[:, 1] * rq[:, 2] - rq[:, 1] * rp[:, 2]
        B = rp[:, 2] * rq[:, 0] - rq[:, 2] * rp[:, 0]
        C = rp[:, 0] * rq[:, 1] - rq[:, 0] * rp[:, 1]
        D = -A * c[:, 0] - B * c[:, 1] - C * c[:, 2]
        num = A * o[:, 0] + B * o[:, 1] + C * o[:, 2] + D
        den = A * d[:, 0] + B * d[:, 1] + C * d[:, 2]
        line = (den[:, None] * o - num[:, None] * d) / den[:, None]
        along = o + t[:, None] * d
        pt = np.where(((kind[np.arange(S), j] == 2) | (den == 0))[:, None], along, line)
        w = heidrich_bary(pt, a, b, c)
    pt[~hit] = np.nan
    w[~hit] = np.nan
    return t, face, pt, w, hit


# ---- the code under test ----
def gpu_cast(tree, o, d, rng=None):
    from mesh_amd import spatialsearch
    t, face, pt, w = spatialsearch.aabbtree_raycast(tree, o, d, rng, barycentric=True)
    hit = spatialsearch.aabbtree_occluded(tree, o, d, rng)
    assert t.shape == (len(o),) and face.dtype == np.uint32 and pt.shape == (len(o), 3) and hit.dtype == bool
    return t, face, pt, w, hit


def assert_same(got, ref, what=""):
    for name, g, r in zip(("t", "face", "pt", "w", "hit"), got, ref):
        bad = np.nonzero(~((g == r) | ((g != g) & (r != r))).reshape(len(g), -1).all(axis=1))[0]
        assert bad.size == 0, "%s %s: %d rows differ, first %d: got %r, reference %r" % (
            what, name, bad.size, bad[0], g[bad[0]], r[bad[0]])


def tris_of(v, f):
    return np.ascontiguousarray(v[f.astype(np.int64)])


def generic_rays(tri, S, seed):
    """S rays around the triangles: origins in their box widened by 0.3 of its extent per side; every other ray is aimed
    at a point of a face (so hits occur), the rest at random; directions unnormalised, lengths over 10^+-3"""
    rng = np.random.default_rng(seed)
    pts = tri.reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    o = rng.uniform(lo - 0.3 * ext, hi + 0.3 * ext, (S, 3))
    fi = rng.integers(0, len(tri), S)
    bc = rng.dirichlet([1, 1, 1], S)
    target = (tri[fi] * bc[:, :, None]).sum(axis=1)
    d = np.where((np.arange(S) % 2 == 0)[:, None], target - o, rng.normal(size=(S, 3)))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return o, d * 10.0 ** rng.uniform(-3, 3, (S, 1))


MESHES = ["sphere", "icosphere", "cylinder", "test_box", "sphere1", "sphere2"]


def mesh_of(meshes, name):
    if name in ("sphere1", "sphere2"):  # the first 1 and 2 faces of the sphere: a tree of one leaf has no internal node
        return meshes["sphere_v"], np.ascontiguousarray(meshes["sphere_f"][:int(name[-1])])
    return meshes[name + "_v"], meshes[name + "_f"]


@pytest.fixture(scope="module")
def case1(meshes):
    """per mesh: (tree, triangles, origins, directions, hit table) of the 257 generic rays; computed once, never changed"""
    from mesh_amd import spatialsearch
    out = {}
    for name in MESHES:
        v, f = mesh_of(meshes, name)
        tri = tris_of(v, f)
        o, d = generic_rays(tri, 257, seed=7 + len(tri))
        out[name] = (spatialsearch.aabbtree_compute(v, f), tri, o, d, hit_table(tri, o, d, None), v, f)
    return out


@pytest.mark.parametrize("name", MESHES)
def test_generic_rays(case1, oracle, name):
    tree, tri, o, d, table, v, f = case1[name]
    ref = ref_cast(tri, o, d, table=table)
    n_hit = int(ref[4].sum())
    print("%s: %d faces, %d of 257 rays hit" % (name, len(tri), n_hit))
    assert 0 < n_hit < 257  # both hits and misses
    lens = np.linalg.norm(d, axis=1)
    assert lens.min() < 1e-2 and lens.max() > 1e2
    got = gpu_cast(tree, o, d)
    assert_same(got, ref, name)
    hs = ref[4]
    assert np.isinf(got[0][~hs]).all() and (got[1][~hs] == NO_FACE).all() and np.isnan(got[2][~hs]).all()
    # the weights are the ones the reference's mesh code computes for those points on those faces
    _, wb = oracle.barycentric_coordinates_for_points(v, f, got[2][hs], got[1][hs])
    assert np.array_equal(np.asarray(wb).reshape(-1, 3), got[3][hs])


@pytest.mark.parametrize("S", [1, 63, 64, 65])
def test_ragged_sizes(case1, S):
    tree, tri, o, d, table, _, _ = case1["sphere"]
    ref = ref_cast(tri, o[:S], d[:S], table=(table[0][:S], table[1][:S]))
    assert_same(gpu_cast(tree, o[:S].copy(), d[:S].copy()), ref, "S=%d" % S)


def test_pinned_to_the_oracle(meshes, oracle):
    from mesh_amd import spatialsearch
    # occlusion == brute_visibility's decision, row for row: (src, (src + dir) - src) formed as visibility.cpp does
    v, f = meshes["sphere_v"], meshes["sphere_f"]
    tree = spatialsearch.aabbtree_compute(v, f)
    centre, ext = 0.5 * (v.min(0) + v.max(0)), (v.max(0) - v.min(0)).max()
    cams = centre + 3.0 * ext * np.array([[1.0, 0.2, 0.1], [-0.3, -1.0, 0.4], [0.1, 0.3, -1.0]])
    min_dist = 1e-3
    bv, _ = oracle.brute_visibility(v, f, cams, min_dist=min_dist)
    for ic, cam in enumerate(cams):
        dirs = cam[None, :] - v
        ln = np.sqrt(vdot(dirs, dirs))
        dirs = dirs / ln[:, None]
        src = v + min_dist * dirs
        occ = spatialsearch.aabbtree_occluded(tree, src, (src + dirs) - src)
        print("camera %d: %d of %d vertices occluded" % (ic, occ.sum(), len(v)))
        assert 0 < occ.sum() < len(v)
        assert np.array_equal(occ, bv[ic] == 0)
    # nearest_alongnormal(p, n) is the nearer, by (|pt - p|, face), of the first hits of (p, (p + n) - p) and
    # (p, (p - n) - p)
    for name in ("sphere", "cylinder"):
        v, f = meshes[name + "_v"], meshes[name + "_f"]
        tri = tris_of(v, f)
        tree = spatialsearch.aabbtree_compute(v, f)
        rng = np.random.default_rng(1)
        lo, hi = v.min(0), v.max(0)
        p = rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (2000, 3))
        n = rng.normal(size=(2000, 3))
        bd, bf, bpt = oracle.brute_alongnormal(v, f, p, n)
        dirs = [(p + n) - p, (p - n) - p]
        res = [spatialsearch.aabbtree_raycast(tree, p, dk) for dk in dirs]
        dist = []
        for t, face, pt in res:
            e = pt - p
            with np.errstate(invalid="ignore"):
                dist.append(np.where(face != NO_FACE, np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]),
                                     INF))
        second = (dist[1] < dist[0]) | ((dist[1] == dist[0]) & (res[1][1] < res[0][1]))
        gd = np.where(second, dist[1], dist[0])
        gf = np.where(second, res[1][1], res[0][1])
        gp = np.where(second[:, None], res[1][2], res[0][2])
        gd = np.where(gf == NO_FACE, 1e100, gd)
        # rows may be left out only where the numpy brute force shows the two smallest t of a direction nearly tied
        near = np.zeros(2000, bool)
        for dk in dirs:
            two = np.sort(hit_table(tri, p, dk, None)[0], axis=1)[:, :2]
            with np.errstate(invalid="ignore"):
                near |= np.isfinite(two[:, 1]) & (two[:, 1] - two[:, 0] <= 1e-9 * np.maximum(1.0, np.abs(two[:, 0])))
        keep = ~near
        hs = bd < 1e100
        print("%s: %d hitting rows, %d rows left out" % (name, hs.sum(), near.sum()))
        assert near.sum() <= 20 and hs.sum() > 500 and (~hs).sum() > 500
        assert np.array_equal(gd[keep], bd[keep]) and np.array_equal(gf[keep], bf[keep])
        assert np.array_equal(gp[keep & hs], bpt[keep & hs])


def test_ranges(case1):
    tree, tri, o, d, table, _, _ = case1["sphere"]
    S = len(o)
    srt = np.sort(table[0], axis=1)
    t1st = srt[:, 0]
    # the next distinct hit parameter after the first (inf: none)
    t2nd = np.array([row[row > row[0]][0] if (row > row[0]).any() else INF for row in srt])
    two = np.isfinite(t2nd)
    assert two.sum() > 50 and (np.isfinite(t1st) & ~two).sum() > 20
    zero, inf = np.zeros(S), np.full(S, INF)
    fin = np.isfinite(t1st)
    blocks = {
        "ends at the first hit": np.stack([zero, t1st], 1),
        "ends one ulp below it": np.stack([zero, np.where(fin, np.nextafter(t1st, -INF), INF)], 1),
        "starts at the first hit": np.stack([np.where(fin, t1st, 0.0), inf], 1),
        "starts one ulp above it": np.stack([np.where(fin, np.nextafter(t1st, INF), 0.0), inf], 1),
        "the second hit alone": np.stack([np.where(two, t2nd, 0.0), np.where(two, t2nd, INF)], 1),
        "negative start": np.stack([np.full(S, -5.0), inf], 1),
    }
    names = list(blocks)
    oo, dd = np.tile(o, (len(names), 1)), np.tile(d, (len(names), 1))
    rr = np.vstack([blocks[k] for k in names])
    got = gpu_cast(tree, oo, dd, rr)
    ref = ref_cast(tri, oo, dd, rr)
    assert_same(got, ref, "ranges")
    part = {k: tuple(x[i * S:(i + 1) * S] for x in got) for i, k in enumerate(names)}
    base = ref_cast(tri, o, d, table=table)
    assert_same(part["ends at the first hit"], base, "ends at the first hit")
    assert not part["ends one ulp below it"][4][fin].any() and np.isinf(part["ends one ulp below it"][0]).all()
    assert_same(part["starts at the first hit"], base, "starts at the first hit")
    assert np.array_equal(part["starts one ulp above it"][0][two], t2nd[two])
    assert not part["starts one ulp above it"][4][fin & ~two].any()
    assert np.array_equal(part["the second hit alone"][0][two], t2nd[two])
    assert_same(part["negative start"], base, "t0 < 0 behaves as 0")
    # segments a -> b with [0, 1]: from each origin to a point before, on and behind its first hit
    lam = np.where(np.arange(S) % 3 == 0, 0.5, np.where(np.arange(S) % 3 == 1, 1.0, 2.0))
    b = o + np.where(fin, t1st * lam, 1.0)[:, None] * d
    seg = b - o
    got = gpu_cast(tree, o, seg, (0.0, 1.0))
    ref = ref_cast(tri, o, seg, np.tile([0.0, 1.0], (S, 1)))
    assert_same(got, ref, "segments")
    assert got[4].any() and not got[4].all()
    from mesh_amd.search import AabbTree
    at = AabbTree.__new__(AabbTree)
    at.cpp_handle = tree
    assert np.array_equal(at.line_of_sight(o, b), ~ref[4])
    assert_same(tuple(at.ray_cast(o, seg, (0.0, 1.0), barycentric=True)) + (at.occluded(o, seg, (0.0, 1.0)),), ref, "AabbTree")


def unit_cube():
    v = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])  # index 4x + 2y + z
    f = np.array([[0, 2, 6], [0, 6, 4],    # z = 0 (diagonal x = y)
                  [1, 5, 7], [1, 7, 3],    # z = 1
                  [0, 4, 5], [0, 5, 1],    # y = 0
                  [2, 3, 7], [2, 7, 6],    # y = 1
                  [0, 1, 3], [0, 3, 2],    # x = 0
                  [4, 6, 7], [4, 7, 5]], dtype=np.uint32)  # x = 1
    return v, f


def test_exact_arithmetic():
    """a cube with 0/1 coordinates: every determinant is exact, so ties and boundary cases are exactly what they seem"""
    from mesh_amd import spatialsearch
    v, f = unit_cube()
    tree = spatialsearch.aabbtree_compute(v, f)
    tri = tris_of(v, f)
    e = 2.0 ** -30
    rays = [
        ((0.5, 0.5, -1), (0, 0, 1)),      # 0 the midpoint of a face diagonal: a tie on t, the smaller face id wins
        ((-1, -1, -1), (1, 1, 1)),        # 1 through a vertex
        ((0.5, -1, -1), (0, 1, 1)),       # 2 through a cube edge
        ((0.25, 0.5, 0), (0, 0, 1)),      # 3 an origin on the surface
        ((-1, 0.25, 0), (1, 0, 0)),       # 4 in the plane z = 0, entering the face at x = 0
        ((-1, 0, 0), (1, 0, 0)),          # 5 along an edge
        ((-1, 0.5, -e), (1, 0, 0)),       # 6 parallel, just off the face z = 0
        ((-1, 0.5, 1 + e), (2, 0, 0)),    # 7 parallel, just off the face z = 1
        ((0.25, 0.5, 0.5), (0, 0, -4)),   # 8 from inside, a long direction
        ((0.5, 0.5, -1), (0, 0, -1)),     # 9 pointing away
    ]
    o = np.array([r[0] for r in rays], dtype=np.float64)
    d = np.array([r[1] for r in rays], dtype=np.float64)
    ref = ref_cast(tri, o, d)
    got = gpu_cast(tree, o, d)
    assert_same(got, ref, "cube")
    t, face, pt, w, hit = got
    assert t[0] == 1.0 and face[0] == 0 and np.array_equal(pt[0], [0.5, 0.5, 0.0])
    assert np.array_equal(w[0], [0.5, 0.0, 0.5])
    assert t[1] == 1.0 and face[1] == 0 and np.array_equal(pt[1], [0.0, 0.0, 0.0])
    assert t[2] == 1.0 and face[2] == 1 and np.array_equal(pt[2], [0.5, 0.0, 0.0])
    assert t[3] == 0.0 and face[3] == 0 and np.array_equal(pt[3], [0.25, 0.5, 0.0])
    assert t[4] == 1.0 and face[4] == 0 and np.array_equal(pt[4], [0.0, 0.25, 0.0])
    assert t[5] == 1.0 and face[5] == 0 and np.array_equal(pt[5], [0.0, 0.0, 0.0])
    assert list(hit) == [True] * 6 + [False, False, True, False]
    assert np.isinf(t[6]) and face[6] == NO_FACE and np.isnan(pt[6]).all() and np.isnan(w[6]).all()
    assert t[8] == 0.125 and np.array_equal(pt[8], [0.25, 0.5, 0.0])
    kinds = hit_table(tri, o, d, None)[1]
    assert (kinds[4] == 2).any() and (kinds[5] == 2).any()  # the coplanar branch is reached
    # ranges on exact ties: [1, 1] keeps the hit, a range that ends just before it or starts just after it does not
    rr = np.array([[1.0, 1.0], [0.0, np.nextafter(1.0, 0.0)], [np.nextafter(1.0, 2.0), 1.5], [1.0, 1.0], [0.5, 1.0]])
    assert_same(gpu_cast(tree, o[:5], d[:5], rr), ref_cast(tri, o[:5], d[:5], rr), "cube ranges")


def test_rows_that_cannot_be_cast(case1):
    tree, tri, o, d, table, _, _ = case1["icosphere"]
    o, d = o[:64].copy(), d[:64].copy()
    rng = np.tile([0.0, INF], (64, 1))
    good = gpu_cast(tree, o, d, rng)
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
    got = gpu_cast(tree, o, d, rng)
    assert_same(got, ref_cast(tri, o, d, rng), "uncastable")
    rows = np.array(sorted(bad))
    assert np.isinf(got[0][rows]).all() and (got[1][rows] == NO_FACE).all() and not got[4][rows].any()
    assert np.isnan(got[2][rows]).all() and np.isnan(got[3][rows]).all()
    others = np.setdiff1d(np.arange(64), rows)
    assert_same(tuple(x[others] for x in got), tuple(x[others] for x in good), "neighbours")
    assert good[4][others].any()


def test_deep_tree():
    from mesh_amd import spatialsearch
    rng = np.random.default_rng(22)
    pts = np.vstack([rng.normal(size=(3000, 3)) * 1e-4, rng.normal(size=(3000, 3)) * 100])
    v = np.repeat(pts, 3, axis=0) + rng.normal(size=(18000, 3)) * 1e-6
    f = np.arange(18000, dtype=np.uint32).reshape(-1, 3)
    tree = spatialsearch.aabbtree_compute(v, f)
    assert tree.info().max_depth > 16
    tri = tris_of(v, f)
    rng = np.random.default_rng(61)
    fi = rng.choice(6000, 384, replace=False)
    n = rng.normal(size=(512, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    cen = tri[fi].mean(axis=1)
    o = np.vstack([cen + rng.uniform(-2e-4, 2e-4, (384, 1)) * n[:384], rng.normal(size=(128, 3)) * 50])
    d = n * 10.0 ** rng.uniform(-2, 2, (512, 1))
    d[:384:2] *= -1.0  # half of the near rays point back through their face
    aim = tri[rng.integers(0, 3000, 64)].mean(axis=1) - o[384:448]  # far sources aimed into the cluster
    d[384:448] = aim
    ref = ref_cast(tri, o, d)
    print("deep tree: %d hits, %d misses" % (ref[4].sum(), (~ref[4]).sum()))
    assert ref[4].sum() >= 100 and (~ref[4]).sum() >= 100
    assert_same(gpu_cast(tree, o, d), ref, "deep tree")


def test_extra_faces(meshes):
    from mesh_amd import _native as N, spatialsearch
    v, f = meshes["icosphere_v"], meshes["icosphere_f"]
    T = len(f)
    lo, hi = v.min(0), v.max(0)
    z = hi[2] + 0.5
    ev = np.array([[lo[0] - 1, lo[1] - 1, z], [hi[0] + 1, lo[1] - 1, z], [hi[0] + 1, hi[1] + 1, z], [lo[0] - 1, hi[1] + 1, z]])
    ef = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
    tree = N.build_tree(np.ascontiguousarray(v), np.ascontiguousarray(f), ev, ef)
    tri = np.vstack([tris_of(v, f), tris_of(ev, ef)])
    rng = np.random.default_rng(3)
    o = np.column_stack([rng.uniform(lo[0], hi[0], 128), rng.uniform(lo[1], hi[1], 128), np.full(128, z + 1.0)])
    o[64:, 2] = lo[2] - 1.0  # from below: the mesh first
    d = np.zeros((128, 3))
    d[:64, 2], d[64:, 2] = -0.5, 3.0
    got = gpu_cast(tree, o, d)
    assert_same(got, ref_cast(tri, o, d), "extra faces")
    assert ((got[1][:64] >= T) & (got[1][:64] < T + 2)).all() and (got[1][64:] < T).any()
    rr = np.tile([3.0, INF], (128, 1))  # past the extra faces from above: the mesh behind them
    got = gpu_cast(tree, o, d, rr)
    assert_same(got, ref_cast(tri, o, d, rr), "extra faces, ranged")
    assert (got[1][:64] < T).any()


def test_independence(meshes):
    import torch
    from mesh_amd import _native as N, spatialsearch
    v, f = meshes["icosphere_v"], meshes["icosphere_f"]
    tree = spatialsearch.aabbtree_compute(v, f)
    tri = tris_of(v, f)
    S = 5000  # above the threshold of the query sort: rays run in the slot order of their origins
    o, d = generic_rays(tri, S, seed=11)
    rr = np.tile([0.0, INF], (S, 1))
    rr[::3] = [0.5, 20.0]
    ref = ref_cast(tri, o, d, rr)
    assert 0 < ref[4].sum() < S
    got = gpu_cast(tree, o, d, rr)
    assert_same(got, ref, "sorted path")
    # a row permutation gives the permuted answers
    perm = np.random.default_rng(5).permutation(S)
    gp = gpu_cast(tree, o[perm], d[perm], rr[perm])
    assert_same(gp, tuple(x[perm] for x in got), "permutation")
    # pt and w NULL leave t and face unchanged
    L = N.lib()
    t2, f2 = np.empty(S), np.empty(S, np.uint32)
    N.check(L.msh_tree_raycast(tree.ptr, N.dptr(o), N.dptr(d), N.dptr(rr), S, N.dptr(t2), N.uptr(f2), None, None))
    assert np.array_equal(t2, got[0]) and np.array_equal(f2, got[1])
    # the device entry points on torch tensors give the same bytes; a NULL range on the device is [0, inf]
    gd = device_cast(tree, o, d, rr, False) + (device_cast(tree, o, d, rr, True),)
    assert_same(gd, got, "device entry points")
    assert np.array_equal(device_cast(tree, o, d, None, True), ref_cast(tri, o, d)[4])
    # the stats call walks the same rays and returns non-zero counts (it takes no output array)
    do, dd, dr = (torch.from_numpy(x).to("cuda:0") for x in (o, d, rr))
    n1, l1 = tree.raycast_stats(do.data_ptr(), dd.data_ptr(), S, dr.data_ptr())
    n2, l2 = tree.raycast_stats(do.data_ptr(), dd.data_ptr(), S, dr.data_ptr(), any_hit=True)
    print("stats: first hit %d nodes %d leaves, occlusion %d nodes %d leaves" % (n1, l1, n2, l2))
    assert n1 > 0 and l1 > 0 and n2 > 0 and l2 > 0 and l2 <= S * len(tri)
    # S == 0 and the Mesh layer
    assert L.msh_tree_raycast(tree.ptr, None, None, None, 0, None, None, None, None) == N.MSH_OK
    e = spatialsearch.aabbtree_raycast(tree, np.zeros((0, 3)), np.zeros((0, 3)))
    assert e[0].shape == (0,) and e[2].shape == (0, 3)
    from mesh_amd.mesh import Mesh
    m = Mesh(v=v, f=f)
    mt, mf, mp = m.ray_cast(o[:65], d[:65], rr[:65])
    assert np.array_equal(mt, got[0][:65]) and np.array_equal(mf, got[1][:65])
    b = o[:65] + d[:65]
    assert np.array_equal(m.line_of_sight(o[:65], b), ~ref_cast(tri, o[:65], b - o[:65], np.tile([0.0, 1.0], (65, 1)))[4])


def device_cast(tree, o, d, rr, any_hit):
    """the _device entry points on torch tensors: (t, face, pt, w) of the first hits, or hit with any_hit"""
    import torch
    from mesh_amd import _native as N
    L, vp, dev, S = N.lib(), ctypes.c_void_p, torch.device("cuda:0"), len(o)
    do, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    dr = torch.from_numpy(rr).to(dev) if rr is not None else None
    pr = vp(dr.data_ptr()) if dr is not None else None
    if any_hit:
        dhit = torch.empty(S, dtype=torch.uint8, device=dev)
        N.check(L.msh_tree_occluded_device(tree.ptr, vp(do.data_ptr()), vp(dd.data_ptr()), pr, S, vp(dhit.data_ptr()),
                                           None))
        torch.cuda.synchronize()
        return dhit.cpu().numpy().astype(bool)
    dt = torch.empty(S, dtype=torch.float64, device=dev)
    dface = torch.empty(S, dtype=torch.int32, device=dev)
    dpt = torch.empty((S, 3), dtype=torch.float64, device=dev)
    dw = torch.empty((S, 3), dtype=torch.float64, device=dev)
    N.check(L.msh_tree_raycast_device(tree.ptr, vp(do.data_ptr()), vp(dd.data_ptr()), pr, S, vp(dt.data_ptr()),
                                      vp(dface.data_ptr()), vp(dpt.data_ptr()), vp(dw.data_ptr()), None))
    torch.cuda.synchronize()
    return dt.cpu().numpy(), dface.cpu().numpy().view(np.uint32), dpt.cpu().numpy(), dw.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


def test_chunk_pipeline(meshes, monkeypatch):
    """The host entry points through the slab pipeline: 350,001 rays are 17 MB of rows even for the narrowest call
    (occlusion with a NULL range: 24 + 24 + 1 B each), above the 16 MB small-call limit, so every call below runs in
    chunks; MESH_AMD_HOST_CHUNK = 100,001 makes four chunks of an odd number of rows, the last ragged (49,998).  Each
    column set -- range given and NULL, pt and w present and absent -- must equal the _device entry points' bytes, with
    results carved from the pinned pool (downloaded in place) and with the pool disabled (staged downloads)."""
    from mesh_amd import _native as N, spatialsearch
    v, f = meshes["icosphere_v"], meshes["icosphere_f"]
    tree = spatialsearch.aabbtree_compute(v, f)
    S, chunk = 350001, 100001
    assert S * (24 + 24 + 1) > 16 << 20 and S % 2 == 1 and chunk % 2 == 1 and S % chunk not in (0, chunk - 1)
    o, d = generic_rays(tris_of(v, f), S, seed=13)
    rr = np.tile([0.0, INF], (S, 1))
    rr[::3] = [0.5, 20.0]
    rr[5::1001] = [2.0, 1.0]  # rows that cannot be cast, in every chunk
    dev_r = device_cast(tree, o, d, rr, False)
    dev_n = device_cast(tree, o, d, None, False)
    hit_r, hit_n = device_cast(tree, o, d, rr, True), device_cast(tree, o, d, None, True)
    assert 0 < hit_r.sum() < hit_n.sum() < S and not same(dev_r[0], dev_n[0])
    L = N.lib()
    monkeypatch.setenv("MESH_AMD_HOST_CHUNK", str(chunk))
    monkeypatch.setattr(N, "PINNED_MIN_BYTES", 1 << 16)
    for pool in (True, False):
        if not pool:
            assert L.msh_host_pool_trim() == 0
            monkeypatch.setenv("MESH_AMD_PINNED_POOL_MB", "0")
        N.timing_reset()
        N.timing_enable(True)
        got = spatialsearch.aabbtree_raycast(tree, o, d, rr, barycentric=True)  # every column: 124 B per row
        h = spatialsearch.aabbtree_occluded(tree, o, d)  # the narrowest rows
        N.timing_enable(False)
        # one launch per chunk: the calls went through the pipeline, not the one-shot path of small calls
        assert N.timing_get("raycast")[1] == 4 and N.timing_get("occluded")[1] == 4
        assert same(h, hit_n), "occlusion, NULL range (pool %s)" % pool
        assert (got[0].base is not None) == pool
        assert all(same(a, b) for a, b in zip(got, dev_r)), "first hit, range, pt, w (pool %s)" % pool
        got = spatialsearch.aabbtree_raycast(tree, o, d)  # NULL range, no w
        assert all(same(a, b) for a, b in zip(got, dev_n[:3])), "first hit, NULL range, pt (pool %s)" % pool
        h = spatialsearch.aabbtree_occluded(tree, o, d, rr)
        assert same(h, hit_r), "occlusion, range (pool %s)" % pool
        # pt and w absent: t (8 B) and face (4 B) alone after the inputs
        t2, f2 = N.empty_results(((S,), np.float64), ((S,), np.uint32))
        N.check(L.msh_tree_raycast(tree.ptr, N.dptr(o), N.dptr(d), N.dptr(rr), S, N.dptr(t2), N.uptr(f2), None, None))
        assert same(t2, dev_r[0]) and same(f2, dev_r[1]), "first hit, pt and w absent (pool %s)" % pool
        # w without pt
        t3, f3, w3 = N.empty_results(((S,), np.float64), ((S,), np.uint32), ((S, 3), np.float64))
        N.check(L.msh_tree_raycast(tree.ptr, N.dptr(o), N.dptr(d), None, S, N.dptr(t3), N.uptr(f3), None, N.dptr(w3)))
        assert same(t3, dev_n[0]) and same(f3, dev_n[1]) and same(w3, dev_n[3]), "w without pt (pool %s)" % pool
    monkeypatch.delenv("MESH_AMD_PINNED_POOL_MB")


def test_other_tree_kinds_are_refused(meshes):
    """normals-metric, point and batched trees are MSH_EINVAL for all five entry points, with a message naming them"""
    from mesh_amd import _native as N
    v, f = np.ascontiguousarray(meshes["icosphere_v"]), np.ascontiguousarray(meshes["icosphere_f"])
    L = N.lib()
    o, d = np.zeros((1, 3)), np.ones((1, 3))
    t, face = np.zeros(1), np.zeros(1, np.uint32)
    hit = np.zeros(1, np.uint8)
    hp = hit.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    nodes, leaves = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for h in (N.build_ntree(v, f, 0.1), N.build_points(v), N.build_batch(np.ascontiguousarray(np.stack([v, v + 1.0])), f)):
        calls = {
            "msh_tree_raycast": lambda: L.msh_tree_raycast(h.ptr, N.dptr(o), N.dptr(d), None, 1, N.dptr(t), N.uptr(face),
                                                           None, None),
            "msh_tree_raycast_device": lambda: L.msh_tree_raycast_device(h.ptr, None, None, None, 1, None, None, None,
                                                                         None, None),
            "msh_tree_occluded": lambda: L.msh_tree_occluded(h.ptr, N.dptr(o), N.dptr(d), None, 1, hp),
            "msh_tree_occluded_device": lambda: L.msh_tree_occluded_device(h.ptr, None, None, None, 1, None, None),
            "msh_tree_raycast_stats": lambda: L.msh_tree_raycast_stats(h.ptr, None, None, None, 1, 0, ctypes.byref(nodes),
                                                                       ctypes.byref(leaves)),
        }
        for name, call in calls.items():
            assert call() == N.MSH_EINVAL, (name, h.kind)
            assert name.encode() in L.msh_last_error(), (name, L.msh_last_error())
