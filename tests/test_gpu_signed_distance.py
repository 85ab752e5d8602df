"""Signed distance and inside/outside queries on triangle trees (msh_tree_sign_build, msh_tree_signed_distance*,
msh_tree_sign_from_faces_device and the Python layers over them).

The reference for the sign is the generalised winding number, computed here in numpy fp64 (Van Oosterom and
Strackee's solid angle per face, summed, chunked over the queries): a row is inside when w > 0.5.  Every test first
asserts |w - round(w)| < 1e-9 on its rows, so the reference checks itself.  Rows nearer than 1e-9 x the bounding-box
diagonal to the surface (by the oracle's exhaustive squared distance) are left out of the sign comparison, at most
0.1 % of a test's rows.  The pseudonormals the table is checked against entry by entry are restated in numpy from
Baerentzen and Aanaes 2005: face normal, sum of the two unit face normals at an edge, angle-weighted sum at a vertex.
"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_FACE = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def _device():
    from mesh_amd import _native
    _native.set_device(0)


# ---- meshes ----
def torus(nu=24, nv=12, R=1.0, r=0.35):
    """closed, outward-oriented nu x nv torus (concave): 2 nu nv faces"""
    u = np.arange(nu) * (2 * np.pi / nu)
    w = np.arange(nv) * (2 * np.pi / nv)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(ww)) * np.cos(uu), (R + r * np.cos(ww)) * np.sin(uu), r * np.sin(ww)], -1).reshape(-1, 3)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [(a, b, c), (a, c, d)]
    return np.ascontiguousarray(v), np.array(f, np.uint32)


def ellipsoid(seg=84, rings=82, radii=(0.3, 0.85, 0.15)):
    """closed, outward-oriented UV ellipsoid: seg x rings + 2 vertices (poles of valence seg), 2 seg rings faces"""
    th = (np.arange(rings) + 1) * (np.pi / (rings + 1))
    ph = np.arange(seg) * (2 * np.pi / seg)
    tt, pp = np.meshgrid(th, ph, indexing="ij")
    body = np.stack([np.sin(tt) * np.cos(pp), np.sin(tt) * np.sin(pp), np.cos(tt)], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 0.0, 1.0]], body, [[0.0, 0.0, -1.0]]]) * np.asarray(radii)
    top, bot = 0, 1 + rings * seg
    f = []
    for j in range(seg):
        jn = (j + 1) % seg
        f.append((top, 1 + j, 1 + jn))
        f.append((bot, 1 + (rings - 1) * seg + jn, 1 + (rings - 1) * seg + j))
        for i in range(rings - 1):
            a, b = 1 + i * seg + j, 1 + i * seg + jn
            c, d = 1 + (i + 1) * seg + jn, 1 + (i + 1) * seg + j
            f += [(a, d, c), (a, c, b)]
    return np.ascontiguousarray(v), np.array(f, np.uint32)


def closed_mesh(meshes, name):
    if name == "torus":
        return torus()
    return np.ascontiguousarray(meshes[name + "_v"], np.float64), np.ascontiguousarray(meshes[name + "_f"], np.uint32)


CLOSED = ["sphere", "test_box", "test_doublebox", "icosphere", "torus"]


def diag_of(v):
    return float(np.linalg.norm(v.max(0) - v.min(0)))


# ---- references ----
def winding_number(v, f, q, chunk=128):
    """generalised winding number of the (S,3) rows q about the mesh, numpy fp64"""
    tri = v[f.astype(np.int64)]  # (T, corner, xyz)
    out = np.empty(q.shape[0])
    for s in range(0, q.shape[0], chunk):
        x = q[s:s + chunk]
        # corner k relative to the query, by component: (chunk, T) arrays
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = (
            [tri[None, :, k, d] - x[:, None, d] for d in range(3)] for k in range(3))
        la = np.sqrt(ax * ax + ay * ay + az * az)
        lb = np.sqrt(bx * bx + by * by + bz * bz)
        lc = np.sqrt(cx * cx + cy * cy + cz * cz)
        num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
        den = (la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la +
               (cx * ax + cy * ay + cz * az) * lb)
        out[s:s + chunk] = np.arctan2(num, den).sum(1) / (2.0 * np.pi)
    return out


def pseudonormals(v, f):
    """(unit face normals (T,3), {(lo, hi): [faces]}, angle-weighted vertex pseudonormals (P,3))"""
    fi = f.astype(np.int64)
    a, b, c = v[fi[:, 0]], v[fi[:, 1]], v[fi[:, 2]]
    n = np.cross(b - a, c - a)
    fn = n / np.linalg.norm(n, axis=1)[:, None]
    vpn = np.zeros_like(v)
    edges = {}
    for k in range(3):
        p0, p1, p2 = v[fi[:, k]], v[fi[:, (k + 1) % 3]], v[fi[:, (k + 2) % 3]]
        ang = np.arctan2(np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1), ((p1 - p0) * (p2 - p0)).sum(1))
        np.add.at(vpn, fi[:, k], ang[:, None] * fn)
        for t in range(fi.shape[0]):
            u, w = int(fi[t, k]), int(fi[t, (k + 1) % 3])
            edges.setdefault((min(u, w), max(u, w)), []).append(t)
    return fn, edges, vpn


def feature(v, f, pn, t, part):
    """the point (centroid, edge midpoint or vertex) and the pseudonormal of feature `part` of face t"""
    fn, edges, vpn = pn
    i = [int(x) for x in f[t]]
    if part == 0:
        return v[i].mean(0), fn[t]
    if part <= 3:
        u, w = i[part - 1], i[part % 3]
        return 0.5 * (v[u] + v[w]), fn[edges[(min(u, w), max(u, w))]].sum(0)
    return v[i[part - 4]], vpn[i[part - 4]]


def make_queries(v, f, seed=7):
    """4,000 rows uniform in the bounding box widened 10 % per side, 1,000 at random vertices and 1,000 at random
    points of random edges, both plus N(0, 1e-3 diag)"""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    d = diag_of(v)
    q0 = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (4000, 3))
    q1 = v[rng.integers(0, v.shape[0], 1000)] + rng.normal(scale=1e-3 * d, size=(1000, 3))
    t, k, s = rng.integers(0, f.shape[0], 1000), rng.integers(0, 3, 1000), rng.uniform(size=(1000, 1))
    e0, e1 = v[f[t, k].astype(np.int64)], v[f[t, (k + 1) % 3].astype(np.int64)]
    q2 = e0 + s * (e1 - e0) + rng.normal(scale=1e-3 * d, size=(1000, 3))
    return np.ascontiguousarray(np.concatenate([q0, q1, q2]))


def inside_reference(oracle, v, f, q):
    """(inside (S,) bool by the winding number, keep (S,) bool: rows far enough from the surface to compare)"""
    w = winding_number(v, f, q)
    err = float(np.abs(w - np.round(w)).max())
    print("winding number: max |w - round(w)| = %.3g over %d rows" % (err, q.shape[0]))
    assert err < 1e-9
    d2 = oracle.brute_nearest(v, f, q)[3]
    keep = np.sqrt(d2) >= 1e-9 * diag_of(v)
    print("rows left out (nearer than 1e-9 diag): %d" % int((~keep).sum()))
    assert (~keep).sum() <= 1e-3 * q.shape[0]
    return w > 0.5, keep


_CASES = {}


@pytest.fixture(scope="module")
def case(oracle, meshes):
    """per closed mesh: (v, f, q, inside, keep), computed once and shared"""
    def get(name):
        if name not in _CASES:
            v, f = closed_mesh(meshes, name)
            q = make_queries(v, f)
            inside, keep = inside_reference(oracle, v, f, q)
            for a in (v, f, q, inside, keep):
                a.setflags(write=False)
            _CASES[name] = (v, f, q, inside, keep)
        return _CASES[name]
    return get


def tree_of(v, f):
    from mesh_amd import spatialsearch
    return spatialsearch.aabbtree_compute(np.array(v), np.array(f))


# ---- 1. sign against the winding number ----
@pytest.mark.parametrize("name", CLOSED)
def test_sign_matches_winding_number(case, name):
    from mesh_amd import spatialsearch
    v, f, q, inside, keep = case(name)
    t = tree_of(v, f)
    sd, face, part, pt = spatialsearch.aabbtree_signed_distance(t, q)
    assert sd.shape == (6000,) and sd.dtype == np.float64 and face.shape == part.shape == (6000,)
    assert face.dtype == part.dtype == np.uint32 and pt.shape == (6000, 3)
    bad = np.flatnonzero(((sd < 0) != inside) & keep)
    print("%s: %d sign mismatches of %d rows; parts seen %s" % (name, bad.size, int(keep.sum()),
                                                                np.bincount(part, minlength=7).tolist()))
    assert bad.size == 0, (bad[:10], sd[bad[:10]], part[bad[:10]])
    assert (part == 0).any() and ((part >= 1) & (part <= 3)).any() and (part >= 4).any()
    # a partial last block (6,001 - 64 rows) and a single row: the same rows' answers
    for S in (6001 - 64, 1):
        sd2, face2, part2, pt2 = spatialsearch.aabbtree_signed_distance(t, np.array(q[:S]))
        assert np.array_equal(sd2, sd[:S]) and np.array_equal(face2, face[:S])
        assert np.array_equal(part2, part[:S]) and np.array_equal(pt2, pt[:S])
        assert not (((sd2 < 0) != inside[:S]) & keep[:S]).any()


# ---- 2. the same answer as nearest ----
@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_same_answer_as_nearest(case, name):
    from mesh_amd import spatialsearch
    v, f, q, _, _ = case(name)
    t = tree_of(v, f)
    sd, face, part, pt = spatialsearch.aabbtree_signed_distance(t, q)
    f0, p0, pt0 = spatialsearch.aabbtree_nearest(t, q)
    assert np.array_equal(face, f0[0]) and np.array_equal(part, p0[0]) and np.array_equal(pt, pt0)
    d = q - pt
    ref = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    ulps = np.abs(np.abs(sd) - ref) / np.spacing(ref)
    print("%s: |sdist| against numpy: max %.3g ulp, %d rows differ" % (name, ulps.max(), int((ulps > 0).sum())))
    assert ulps.max() <= 1.0


# ---- 3. every table entry ----
@pytest.mark.parametrize("name", ["test_box", "torus"])
def test_every_table_entry(meshes, name):
    import torch
    from mesh_amd import distributed
    v, f = closed_mesh(meshes, name)
    pn = pseudonormals(v, f)
    T, d = f.shape[0], diag_of(v)
    face = np.repeat(np.arange(T, dtype=np.uint32), 7)
    part = np.tile(np.arange(7, dtype=np.uint32), T)
    p = np.empty((7 * T, 3))
    nrm = np.empty((7 * T, 3))
    for i in range(7 * T):
        p[i], nrm[i] = feature(v, f, pn, int(face[i]), int(part[i]))
    assert np.linalg.norm(nrm, axis=1).min() > 0
    step = 0.1 * d * nrm / np.linalg.norm(nrm, axis=1)[:, None]
    t = tree_of(v, f)
    t.sign_build()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d_face, d_part, d_p = dev(face.view(np.int32)), dev(part.view(np.int32)), dev(p)
    for sgn in (1.0, -1.0):
        q = p + sgn * step
        out = torch.full((7 * T,), float("nan"), dtype=torch.float64, device="cuda:0")
        distributed.sign_from_faces_device(t, dev(q), d_face, d_part, d_p, out)
        torch.cuda.synchronize()
        sd = out.cpu().numpy()
        wrong = np.flatnonzero(np.sign(sd) != sgn)
        assert wrong.size == 0, (sgn, face[wrong[:10]], part[wrong[:10]], sd[wrong[:10]])
        assert np.abs(np.abs(sd) - 0.1 * d).max() < 1e-12 * d


# ---- 4. topology counters ----
def zero_area_box(meshes):
    """test_box with edge (0, 1) of face 0 split at its midpoint m and the sliver (0, 1, m) added: still closed and
    consistently oriented, with one face of exactly zero area"""
    v, f = closed_mesh(meshes, "test_box")
    a, b, c = (int(x) for x in f[0])
    m = v.shape[0]
    v = np.concatenate([v, [0.5 * (v[a] + v[b])]])
    f = np.concatenate([[(a, m, c), (m, b, c)], f[1:], [(a, b, m)]]).astype(np.uint32)
    return v, f


def defective(meshes, kind):
    v, f = closed_mesh(meshes, "test_box")
    if kind == "open":
        return closed_mesh(meshes, "cylinder"), {"boundary_edges": 18}
    if kind == "reversed":
        f = f.copy()
        f[5] = f[5][::-1]
        return (v, f), {"inconsistent_edges": 3}
    if kind == "duplicate":
        return (v, np.concatenate([f, f[:1]])), {"nonmanifold_edges": 3}
    return zero_area_box(meshes), {"degenerate_faces": 1}


COUNTERS = ("boundary_edges", "nonmanifold_edges", "inconsistent_edges", "degenerate_faces")


@pytest.mark.parametrize("name", CLOSED)
def test_closed_meshes_have_zero_counters(meshes, name):
    from mesh_amd import search
    v, f = closed_mesh(meshes, name)
    tree = search.AabbTree(types.SimpleNamespace(v=v, f=f))
    assert tree.orientation_info() == dict((k, 0) for k in COUNTERS)
    info = tree.cpp_handle.sign_info()
    assert info["state"] == "built" and info["bytes"] == 48 * f.shape[0] + 24 * v.shape[0]


@pytest.mark.parametrize("kind", ["open", "reversed", "duplicate", "zero_area"])
def test_defective_meshes_are_counted(meshes, kind):
    from mesh_amd import search
    (v, f), want = defective(meshes, kind)
    tree = search.AabbTree(types.SimpleNamespace(v=v, f=f))
    info = tree.orientation_info()
    print(kind, info)
    for k, n in want.items():
        assert info[k] == n
    if kind != "duplicate":  # the duplicated face's edges are non-manifold; nothing else is wrong with the others
        assert all(info[k] == 0 for k in COUNTERS if k not in want)
    q = make_queries(v, f)[:500]
    with pytest.raises(ValueError, match="mesh is not a closed, consistently oriented manifold: .*%s" %
                       list(want)[0].replace("_", " ")):
        tree.signed_distance(q)
    with pytest.raises(ValueError, match="not a closed"):
        tree.contains(q)
    sd, face, pt = tree.signed_distance(q, check=False)
    assert np.isfinite(sd).all() and np.isfinite(pt).all() and (face < f.shape[0]).all()
    assert tree.contains(q, check=False).dtype == np.bool_


# ---- 5. a tree large enough for an entry cut and a multi-block sort ----
def test_large_tree_entry_cut(oracle):
    from mesh_amd import spatialsearch
    v, f = ellipsoid()
    assert v.shape == (6890, 3) and f.shape == (13776, 3)
    q = np.ascontiguousarray(make_queries(v, f)[::3])  # uniform, vertex and edge rows
    assert q.shape[0] == 2000
    inside, keep = inside_reference(oracle, v, f, q)
    t = tree_of(v, f)
    info = t.sign_build()
    assert all(info[k] == 0 for k in COUNTERS)
    t.set_entry_cut(24)
    sd_cut, face, part, _ = spatialsearch.aabbtree_signed_distance(t, q)
    assert t.entry_cut_info()["state"] == "built" and t.entry_cut_info()["G"] == 24
    t.set_entry_cut(0)
    sd_root = spatialsearch.aabbtree_signed_distance(t, q)[0]
    assert np.array_equal(sd_cut, sd_root)
    bad = np.flatnonzero(((sd_cut < 0) != inside) & keep)
    assert bad.size == 0, (bad[:10], sd_cut[bad[:10]], part[bad[:10]])
    assert inside.any() and (~inside).any()
    assert (part == 0).any() and ((part >= 1) & (part <= 3)).any() and (part >= 4).any()


# ---- 6. replicas ----
def test_replicas_bit_equal(meshes):
    from mesh_amd import _native, spatialsearch
    v, f = closed_mesh(meshes, "sphere")
    rng = np.random.default_rng(11)
    lo, hi = v.min(0), v.max(0)
    q = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (600000, 3))  # 64 B per row: above the 32 MB fan-out threshold
    one = spatialsearch.aabbtree_signed_distance(tree_of(v, f), q)
    try:
        _native.set_devices([0, 0])
        t2 = tree_of(v, f)
        assert _native.tree_devices(t2) == [0, 0]
        two = spatialsearch.aabbtree_signed_distance(t2, q)
    finally:
        _native.set_device(0)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    assert (one[0] < 0).any() and (one[0] > 0).any()


# ---- 7. the device path ----
def test_device_path_equals_host(case):
    import torch
    from mesh_amd import distributed, spatialsearch
    v, f, q, _, _ = case("torus")
    q = np.array(q)
    q[17] = np.nan
    t = tree_of(v, f)
    host = spatialsearch.aabbtree_signed_distance(t, q)
    assert np.isnan(host[0][17]) and host[1][17] == NO_FACE and np.isfinite(np.delete(host[0], 17)).all()
    S = q.shape[0]
    d_q = torch.from_numpy(q).to("cuda:0")
    mk = lambda *shape, dt: torch.empty(shape, dtype=dt, device="cuda:0")
    sd, face, part, pt = mk(S, dt=torch.float64), mk(S, dt=torch.int32), mk(S, dt=torch.int32), mk(S, 3, dt=torch.float64)
    distributed.signed_distance_device(t, d_q, sd, face, part, pt)
    sd_np, face_np, pt_np = mk(S, dt=torch.float64), mk(S, dt=torch.int32), mk(S, 3, dt=torch.float64)
    distributed.signed_distance_device(t, d_q, sd_np, face_np, None, pt_np)  # part codes from workspace scratch
    torch.cuda.synchronize()
    got = (sd.cpu().numpy(), distributed.as_numpy_u32(face), distributed.as_numpy_u32(part), pt.cpu().numpy())
    for a, b in zip(host, got):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(sd_np.cpu().numpy(), host[0], equal_nan=True)
    assert np.array_equal(distributed.as_numpy_u32(face_np), host[1])
    assert np.array_equal(pt_np.cpu().numpy(), host[3], equal_nan=True)


def test_chunked_host_call_equals_device(meshes, monkeypatch):
    """A host call above the 16 MB small-call limit runs the chunk pipeline: 300,000 rows on the golden sphere are
    19.2 MB at 64 B per row, and MESH_AMD_HOST_CHUNK = 131072 makes three chunks, the last ragged.  Its four arrays
    equal msh_tree_signed_distance_device on the same rows, with results carved from the pinned pool (downloaded in
    place), with the pool off (staged), with the caller's arrays registered in place, and with part == NULL (the
    part slab is then the sign pass's scratch and is not downloaded)."""
    import torch
    from mesh_amd import _native as N, distributed, spatialsearch
    v, f = closed_mesh(meshes, "sphere")
    S = 300000
    lo, hi = v.min(0), v.max(0)
    q = np.random.default_rng(31).uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (S, 3))
    assert 64 * S > 16 << 20
    monkeypatch.setenv("MESH_AMD_HOST_CHUNK", "131072")
    monkeypatch.setattr(N, "PINNED_MIN_BYTES", 1 << 20)
    t = tree_of(v, f)
    t.sign_build()
    d_q = torch.from_numpy(q).to("cuda:0")
    mk = lambda *shape, dt: torch.empty(shape, dtype=dt, device="cuda:0")
    sd, face, part, pt = mk(S, dt=torch.float64), mk(S, dt=torch.int32), mk(S, dt=torch.int32), mk(S, 3, dt=torch.float64)
    distributed.signed_distance_device(t, d_q, sd, face, part, pt)
    torch.cuda.synchronize()
    dev = (sd.cpu().numpy(), distributed.as_numpy_u32(face), distributed.as_numpy_u32(part), pt.cpu().numpy())
    assert (dev[0] < 0).any() and (dev[0] > 0).any()

    def check(got):
        for a, b in zip(got, dev):
            assert a.shape == b.shape and np.array_equal(a, b)

    assert N.lib().msh_host_pool_trim() == 0  # a disabled pool still hands out a released block that fits
    monkeypatch.setenv("MESH_AMD_PINNED_POOL_MB", "0")
    staged = spatialsearch.aabbtree_signed_distance(t, q)
    assert staged[0].base is None  # pool disabled: plain np.empty arrays
    check(staged)
    monkeypatch.setenv("MESH_AMD_HOST_REGISTER", "1")
    check(spatialsearch.aabbtree_signed_distance(t, q))
    monkeypatch.delenv("MESH_AMD_HOST_REGISTER")
    monkeypatch.setenv("MESH_AMD_PINNED_POOL_MB", "1024")
    pooled = spatialsearch.aabbtree_signed_distance(t, q)
    owner = pooled[0]
    while isinstance(owner, np.ndarray):
        owner = owner.base
    assert isinstance(owner, N._PinnedBlock)
    check(pooled)
    del pooled, owner
    # the C entry point without part codes (the Python layer always asks for them)
    sdist, hface, hpt = np.full(S, 7.0), np.full(S, 7, np.uint32), np.full((S, 3), 7.0)
    N.check(N.lib().msh_tree_signed_distance(t.ptr, N.dptr(q), S, N.dptr(sdist), N.uptr(hface), None, N.dptr(hpt)))
    check((sdist, hface, dev[2], hpt))
    assert N.lib().msh_host_pool_trim() == 0


# ---- 8. refusals ----
def test_refusals(meshes):
    import torch
    from mesh_amd import _native, aabb_normals, spatialsearch
    L = _native.lib()
    v, f = closed_mesh(meshes, "sphere")
    q = make_queries(v, f)[:100]
    sd, face, part, pt = np.empty(100), np.empty(100, np.uint32), np.empty(100, np.uint32), np.empty((100, 3))

    def c_query(h):
        return L.msh_tree_signed_distance(h.ptr, _native.dptr(q), 100, _native.dptr(sd), _native.uptr(face),
                                          _native.uptr(part), _native.dptr(pt))

    ntree = aabb_normals.aabbtree_n_compute(v, f, 0.1)
    ptree = _native.build_points(v)
    btree = _native.build_batch(np.ascontiguousarray(np.stack([v, v + 1.0])), f)
    xtree = _native.build_tree(v, f, v + 5.0, f)
    for h in (ntree, ptree, btree, xtree):
        assert L.msh_tree_sign_build(h.ptr, _native.uptr(f), f.shape[0]) == _native.MSH_EINVAL, h
        assert L.msh_last_error()
        assert c_query(h) == _native.MSH_EINVAL, h
    for h in (ntree, ptree, btree):
        with pytest.raises(TypeError):
            spatialsearch.aabbtree_signed_distance(h, q)
    with pytest.raises(ValueError, match="extra faces"):
        spatialsearch.aabbtree_signed_distance(xtree, q)

    t = tree_of(v, f)
    with pytest.raises(ValueError, match="faces do not match the tree"):
        t.sign_build(np.ascontiguousarray(f[::-1]))
    with pytest.raises(ValueError, match="out of range"):
        t.sign_build(np.where(f == 3, 100000, f).astype(np.uint32))
    with pytest.raises(ValueError, match="faces given"):
        t.sign_build(f[:-1])
    assert t.sign_info()["state"] == "none"
    assert c_query(t) == _native.MSH_EINVAL and b"msh_tree_sign_build" in L.msh_last_error()

    # a blob-unpacked handle keeps no faces and has no table until sign_build(f)
    blob = torch.empty(_native.blob_size(t), dtype=torch.uint8, device="cuda:0")
    _native.blob_pack(t, blob.data_ptr())
    torch.cuda.synchronize()
    t.sign_build()
    u = _native.blob_unpack(blob.data_ptr(), blob.numel(), 0)
    assert u.faces is None and u.sign_info()["state"] == "none"
    assert c_query(u) == _native.MSH_EINVAL and b"msh_tree_sign_build" in L.msh_last_error()
    with pytest.raises(ValueError, match=r"sign_build\(f\)"):
        spatialsearch.aabbtree_signed_distance(u, q)
    u.sign_build(f)
    a, b = spatialsearch.aabbtree_signed_distance(u, q), spatialsearch.aabbtree_signed_distance(t, q)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # building twice replaces the table
    assert t.sign_build()["state"] == "built"
    assert all(np.array_equal(x, y) for x, y in zip(spatialsearch.aabbtree_signed_distance(t, q), b))
    # S = 0 is accepted
    e = spatialsearch.aabbtree_signed_distance(t, np.empty((0, 3)))
    assert [x.shape for x in e] == [(0,), (0,), (0,), (0, 3)]
    assert L.msh_tree_signed_distance_device(t.ptr, None, 0, None, None, None, None, None) == _native.MSH_OK
    assert L.msh_tree_sign_from_faces_device(t.ptr, None, 0, None, None, None, None, None) == _native.MSH_OK


def test_mesh_facade(meshes):
    from mesh_amd.mesh import Mesh
    v, f = closed_mesh(meshes, "test_box")
    m = Mesh(v=v, f=f)
    q = np.array([[0.0, 0.0, 0.0], [0.4, 0.4, 0.4], [2.0, 0.0, 0.0], [0.6, 0.6, 0.6]])
    sd = m.signed_distances(q)
    assert np.allclose(sd, [-0.5, -0.1, 1.5, np.sqrt(0.03)], rtol=0, atol=1e-14)
    assert m.contains(q).tolist() == [True, True, False, False]
