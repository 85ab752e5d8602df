"""The entry cut's directional drop (cutbuild.hip k_cut_level / cut_dir_drop) changes no answer.

Walks that start from a cut built with the directional rule give the arrays of walks from the root, bit for bit, on
the closest-point path (lean and generic kernels, 32-B and 64-B records, grids whose cell half-diagonal r runs from
comparable to the queries' distance d to far below it, the two-stage fine grid) and on the alongnormal path, whose
rays start at the root in a cell the rule shortened (the record's flag).

Trees under 4096 faces take no entry cut at all (entrycut.cpp kCutMinLeaves), so the small meshes of the list below (the
640-face icosphere, the 16 x 16 flat grid, the two-triangle mesh, the small mesh with a zero-area face) only pin that
nothing changes for them; a 48 x 48 flat grid and the 5120-face icosphere with a zero-area face added put the same
geometry (foot points on boundary edges, a degenerate face) through a built cut.
"""
import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    from mesh_amd import _native
    _native.set_device(0)


def _bumpy(freq):
    v, f = W.geodesic_icosphere(freq)
    th = np.arccos(np.clip(v[:, 2], -1, 1))
    ph = np.arctan2(v[:, 1], v[:, 0])
    return v * (1 + 0.1 * np.sin(5 * th) * np.sin(4 * ph))[:, None], f


def _flat_grid(n):
    x = np.linspace(-1.0, 1.0, n + 1)
    X, Y = np.meshgrid(x, x, indexing="ij")
    v = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], 1)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + n + 1, i + n + 2], 1), np.stack([i, i + n + 2, i + 1], 1)])
    return v, f


def _with_zero_area(v, f):
    # one more face with two equal corners: zero area, its points already on the mesh
    return v, np.concatenate([f, [[f[0, 0], f[0, 1], f[0, 1]]]])


def _mesh(name):
    if name == "ico8":
        return W.geodesic_icosphere(8)
    if name == "ico16":
        return W.geodesic_icosphere(16)
    if name == "bumpy16":
        return _bumpy(16)
    if name == "flat16":
        return _flat_grid(16)
    if name == "flat48":
        return _flat_grid(48)
    if name == "two":
        return (np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0.2], [0, 1, 0]]), np.array([[0, 1, 2], [0, 2, 3]]))
    if name == "zero_small":
        return _with_zero_area(*W.geodesic_icosphere(8))
    if name == "zero16":
        return _with_zero_area(*W.geodesic_icosphere(16))
    raise KeyError(name)


def _grid_box(v):
    # entrycut.cpp build_entry_cut: the scene box widened by 1/4 (an axis at least 5 % of the largest)
    lo, hi = v.min(0), v.max(0)
    half = 0.5 * (hi - lo)
    e = 1.25 * np.maximum(half, 0.05 * half.max())
    return 0.5 * (lo + hi) - e, 2 * e


def _surface(v, f, n, seed):
    p, fi = W.surface_samples(v, f, n, seed=seed, sigma=0.0)
    tri = v[np.asarray(f)[fi].astype(np.int64)]
    nn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    ln = np.linalg.norm(nn, axis=1)
    nn[ln == 0] = [0.0, 0.0, 1.0]
    nn /= np.maximum(ln, 1e-300)[:, None]
    nn[ln == 0] = [0.0, 0.0, 1.0]
    return p, nn


def _queries(v, f, G, seed):
    """Five groups of rows for a G^3 grid: uniform rows reaching past the grid, rows within 0.05 of the mesh's
    centre (exact ties on a sphere; the centre itself), rows on cell corners and cell faces, rows within 1e-3 of the
    surface, rows 0.5-0.9 off the surface."""
    rng = np.random.default_rng(seed)
    glo, ext = _grid_box(v)
    mid = glo + 0.5 * ext
    uni = mid + rng.uniform(-0.75, 0.75, (3000, 3)) * ext  # the grid spans +-0.5 ext
    ctr = mid + rng.uniform(-1, 1, (1500, 3)) * 0.05 / np.sqrt(3.0)
    ctr[0] = mid
    w = ext / G
    corners = glo + rng.integers(0, G + 1, (1500, 3)) * w
    faces = glo + rng.uniform(0, 1, (1500, 3)) * ext
    ax = rng.integers(0, 3, 1500)
    faces[np.arange(1500), ax] = (glo + rng.integers(0, G + 1, (1500, 3)) * w)[np.arange(1500), ax]
    p, nn = _surface(v, f, 6000, seed + 1)
    near = p[:3000] + nn[:3000] * rng.uniform(-1e-3, 1e-3, (3000, 1))
    far = p[3000:] + nn[3000:] * (rng.uniform(0.5, 0.9, (3000, 1)) * rng.choice([-1.0, 1.0], (3000, 1)))
    q = np.concatenate([uni, ctr, corners, faces, near, far])
    assert q.shape[0] >= 4096
    return np.ascontiguousarray(q)


def _nearest(t, q):
    from mesh_amd import spatialsearch
    face, part, pt = spatialsearch.aabbtree_nearest(t, q)
    return face[0], part[0], pt


def _same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), "rows %s" % np.nonzero(np.asarray(x != y).reshape(len(x), -1).any(1))[0][:10]


MESHES = ["ico8", "ico16", "bumpy16", "flat16", "flat48", "two", "zero_small", "zero16"]


@pytest.mark.parametrize("name", MESHES)
def test_directional_cut_bit_exact(oracle, monkeypatch, name):
    from mesh_amd import spatialsearch
    v, f = _mesh(name)
    v = np.ascontiguousarray(v, np.float64)
    f = np.ascontiguousarray(f, np.uint32)
    t = spatialsearch.aabbtree_compute(v, f)
    cut = f.shape[0] >= 4096
    flagged = 0
    for g in (16, 32, 64, -1):
        # the grid the fine automatic request builds (entrycut.cpp cut_grid): twice the coarse one's cells per axis
        G = g if g > 0 else 2 * max(16, int(round(np.cbrt(min(8 * f.shape[0], 1 << 23)))))
        q = _queries(v, f, G, seed=100 + abs(g))
        t.set_entry_cut(0)
        ref = _nearest(t, q)
        t.set_entry_cut(g)
        _same(ref, _nearest(t, q))
        info = t.entry_cut_info()
        assert info["state"] == ("built" if cut else "off"), info
        if cut:
            assert info["G"] == G and info["bytes"] == G ** 3 * 32, info
            flagged += info["flagged"]
        monkeypatch.setenv("MESH_AMD_KNN_LEAN", "0")  # the generic kernel reads the same records
        _same(ref, _nearest(t, q))
        monkeypatch.delenv("MESH_AMD_KNN_LEAN")
        rows = np.random.default_rng(7).choice(q.shape[0], 2000, replace=False)
        bf = oracle.brute_nearest(v, f, q[rows])[0]
        assert np.array_equal(ref[0][rows], bf)
    if cut:
        assert flagged > 0  # the far rows' cells took the directional rule: the masked-flag path ran


@pytest.mark.parametrize("name", ["ico16", "bumpy16", "flat48"])
def test_directional_cut_alongnormal_bit_exact(name):
    # rays from 0.3-0.9 off the surface (cells the directional rule shortened: the record's flag sends them to the
    # root) and from the surface itself (unflagged cells: the start list), against walks without the cut
    from mesh_amd import spatialsearch
    v, f = _mesh(name)
    v = np.ascontiguousarray(v, np.float64)
    f = np.ascontiguousarray(f, np.uint32)
    rng = np.random.default_rng(5)
    p, nn = _surface(v, f, 8192, seed=9)
    off = rng.uniform(0.3, 0.9, (4096, 1)) * rng.choice([-1.0, 1.0], (4096, 1))
    p[:4096] += nn[:4096] * off
    rd = rng.normal(size=(2048, 3))
    nn[:2048] = rd / np.linalg.norm(rd, axis=1)[:, None]  # half of the far rays in random directions
    t = spatialsearch.aabbtree_compute(v, f)
    t.set_entry_cut(0)
    ref = spatialsearch.aabbtree_nearest_alongnormal(t, p, nn)
    flagged = []
    for g in (16, 32, 64, -1):
        t.set_entry_cut(g)
        got = spatialsearch.aabbtree_nearest_alongnormal(t, p, nn)
        info = t.entry_cut_info()
        assert info["state"] == "built", info
        flagged.append(info["flagged"])
        assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])
        assert np.array_equal(ref[2].view(np.int64), got[2].view(np.int64))  # NaN points of misses too
    print("flagged cells per grid", flagged)
    assert flagged[2] > 0 and flagged[3] > 0  # r far below the far rays' 0.3-0.9: the rule applies there


def test_directional_cut_flag_sends_rays_to_root():
    # far rays fall in flagged cells: their walks with the cut visit what walks without it visit (they start at the
    # root), while surface rays, in unflagged cells, visit fewer nodes from the start list
    from mesh_amd import _native, spatialsearch
    v, f = _mesh("ico16")
    v = np.ascontiguousarray(v, np.float64)
    f = np.ascontiguousarray(f, np.uint32)
    p, nn = _surface(v, f, 8192, seed=11)
    far = np.ascontiguousarray(p[:4096] * 1.6)
    t = spatialsearch.aabbtree_compute(v, f)

    def visits(rows, nrm):
        import ctypes
        import torch
        dp = torch.from_numpy(rows).cuda()
        dn = torch.from_numpy(np.ascontiguousarray(nrm)).cuda()
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _native.check(_native.lib().msh_tree_nearest_alongnormal_stats(t.ptr, dp.data_ptr(), dn.data_ptr(), rows.shape[0],
                                                               ctypes.byref(a), ctypes.byref(b)))
        return a.value

    t.set_entry_cut(0)
    spatialsearch.aabbtree_nearest(t, far)
    root_far = visits(far, nn[:4096])
    t.set_entry_cut(64)
    spatialsearch.aabbtree_nearest(t, far)  # builds the grid
    assert t.entry_cut_info()["flagged"] > 0
    cut_far = visits(far, nn[:4096])
    print("alongnormal node visits of the far rays: from the root", root_far, "with the cut", cut_far)
    assert cut_far == root_far


def test_directional_cut_wide_records(oracle):
    # trees over 2^20 leaves keep 64-B records, whose flag is a zero radius word: C5's 5M-face mesh (the way
    # test_entry_cut_wide_records gets them), closest points and alongnormal rays against walks from the root.  The
    # brute-force sample is 64 rows here (5M faces each).
    from mesh_amd import spatialsearch
    v, f = W.c5_mesh()
    v = np.ascontiguousarray(v, np.float64)
    f = np.ascontiguousarray(f, np.uint32)
    t = spatialsearch.aabbtree_compute(v, f)
    rng = np.random.default_rng(3)
    p, nn = _surface(v, f, 8192, seed=13)
    p[:4096] += nn[:4096] * (rng.uniform(0.3, 0.9, (4096, 1)) * rng.choice([-1.0, 1.0], (4096, 1)))
    flagged = 0
    for g in (32, 96):
        q = _queries(v, f, g, seed=200 + g)
        t.set_entry_cut(0)
        ref = _nearest(t, q)
        rays = spatialsearch.aabbtree_nearest_alongnormal(t, p, nn)
        t.set_entry_cut(g)
        _same(ref, _nearest(t, q))
        info = t.entry_cut_info()
        assert info["state"] == "built" and info["bytes"] == g ** 3 * 64, info
        flagged += info["flagged"]
        got = spatialsearch.aabbtree_nearest_alongnormal(t, p, nn)
        assert np.array_equal(rays[0], got[0]) and np.array_equal(rays[1], got[1])
        assert np.array_equal(rays[2].view(np.int64), got[2].view(np.int64))
    assert flagged > 0
    rows = rng.choice(q.shape[0], 64, replace=False)
    assert np.array_equal(ref[0][rows], oracle.brute_nearest(v, f, q[rows])[0])
