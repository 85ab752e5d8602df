"""K-nearest and radius-capped queries: the checks that need no GPU -- every new C entry point refuses a NULL handle, a
K outside 1..MSH_KNEAREST_MAX and a negative or NaN r_max with MSH_EINVAL and a message naming it (K and r_max are
checked before the handle, so no device is needed to see the refusal), the Python layers validate their arguments
before any device work, and ClosestPointTree.query follows scipy's shape rules (on a stubbed native call).  (The
header / ctypes table agreement of the new exports is covered by tests/test_abi.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _calls(L, N, handle, K, r):
    q = np.zeros(3)
    idx, dist, cnt = np.zeros(64, np.uint32), np.zeros(64), np.zeros(1, np.uint32)
    pt, part = np.zeros(192), np.zeros(64, np.uint32)
    counts = (ctypes.c_uint64 * 4)()
    return {
        "msh_points_knearest": lambda: L.msh_points_knearest(handle, N.dptr(q), 1, K, r, N.uptr(idx), N.dptr(dist),
                                                             N.uptr(cnt)),
        "msh_points_knearest_device": lambda: L.msh_points_knearest_device(handle, None, 1, K, r, None, None, None,
                                                                           None),
        "msh_tree_knearest": lambda: L.msh_tree_knearest(handle, N.dptr(q), 1, K, r, N.uptr(idx), N.dptr(dist),
                                                         N.dptr(pt), N.uptr(part), N.uptr(cnt)),
        "msh_tree_knearest_device": lambda: L.msh_tree_knearest_device(handle, None, 1, K, r, None, None, None, None,
                                                                       None, None),
        "msh_tree_knearest_stats": lambda: L.msh_tree_knearest_stats(handle, None, 1, K, r, counts),
    }


def test_null_handles_rejected():
    from mesh_amd import _native as N
    L = N.lib()
    for name, call in _calls(L, N, None, 4, INF).items():
        assert call() == N.MSH_EINVAL, name
        msg = L.msh_last_error()
        assert msg and b"null" in msg and name.encode() in msg, (name, msg)


@pytest.mark.parametrize("K", [0, 65])
def test_bad_k_rejected(K):
    from mesh_amd import _native as N
    L = N.lib()
    for name, call in _calls(L, N, None, K, INF).items():
        assert call() == N.MSH_EINVAL, (name, K)
        msg = L.msh_last_error()
        assert b"K must be" in msg and name.encode() in msg, (name, K, msg)


@pytest.mark.parametrize("r", [-1.0, float("nan")])
def test_bad_r_max_rejected(r):
    from mesh_amd import _native as N
    L = N.lib()
    for name, call in _calls(L, N, None, 4, r).items():
        assert call() == N.MSH_EINVAL, (name, r)
        msg = L.msh_last_error()
        assert b"r_max" in msg and name.encode() in msg, (name, r, msg)


def test_knearest_max_matches_header():
    from mesh_amd import _native as N
    txt = open(os.path.join(ROOT, "include", "meshsearch.h")).read()
    m = re.search(r"^#define MSH_KNEAREST_MAX\s+(\d+)", txt, flags=re.M)
    assert m and int(m.group(1)) == N.KNEAREST_MAX == 64


def test_python_validation_before_device_work():
    from mesh_amd import _native as N, search, spatialsearch
    fake = N.Handle(1, "triangles")  # never dereferenced: validation must raise first
    fake_n = N.Handle(1, "normals")
    fake_p = N.Handle(1, "points")
    q = np.zeros((4, 3))
    try:
        with pytest.raises(ValueError, match="Input must be Nx3"):
            spatialsearch.aabbtree_nearest_k(fake, np.zeros((4, 2)), 3)
        with pytest.raises(ValueError, match="Input must be Nx3"):
            spatialsearch.aabbtree_nearest_k(fake, np.zeros(3), 3)
        with pytest.raises(TypeError, match=r"aabbtree_nearest_k\(\) argument 2 must be numpy.ndarray"):
            spatialsearch.aabbtree_nearest_k(fake, [[0.0, 0.0, 0.0]], 3)
        with pytest.raises(TypeError, match="not a triangle tree"):
            spatialsearch.aabbtree_nearest_k(fake_n, q, 3)
        with pytest.raises(TypeError, match="point tree"):
            spatialsearch.aabbtree_nearest_k(fake_p, q, 3)
        with pytest.raises(TypeError, match="expected a tree handle"):
            spatialsearch.aabbtree_nearest_k(None, q, 3)
        with pytest.raises(TypeError, match="not a point tree"):
            spatialsearch.points_nearest_k(fake, q, 3)
        with pytest.raises(TypeError, match="not a point tree"):
            spatialsearch.points_nearest_k(fake_n, q, 3)
        with pytest.raises(ValueError, match="Input must be Nx3"):
            spatialsearch.points_nearest_k(fake_p, np.zeros((4, 2)), 3)
        for k in (0, 65, -1, 2.5, True):
            with pytest.raises(ValueError, match="k must be"):
                spatialsearch.aabbtree_nearest_k(fake, q, k)
            with pytest.raises(ValueError, match="k must be"):
                spatialsearch.points_nearest_k(fake_p, q, k)
        for r in (-1.0, float("nan")):
            with pytest.raises(ValueError, match="distance cap"):
                spatialsearch.aabbtree_nearest_k(fake, q, 3, r)
            with pytest.raises(ValueError, match="distance cap"):
                spatialsearch.points_nearest_k(fake_p, q, 3, r)
        # the classes over them: the same refusals, still with no device work
        tree = search.AabbTree.__new__(search.AabbTree)
        tree.cpp_handle = fake
        with pytest.raises(ValueError, match="k must be"):
            tree.nearest_k(q, 0)
        with pytest.raises(ValueError, match="distance cap"):
            tree.nearest_k(q, 3, max_distance=-2.0)
        cpt = search.ClosestPointTree.__new__(search.ClosestPointTree)
        cpt.v, cpt._h = np.zeros((5, 3)), fake_p
        with pytest.raises(ValueError, match="k must be"):
            cpt.query(q, k=65)
        with pytest.raises(ValueError, match="distance cap"):
            cpt.query(q, k=2, distance_upper_bound=float("nan"))
    finally:
        fake.ptr = fake_n.ptr = fake_p.ptr = None


def test_query_shape_rules(monkeypatch):
    """ClosestPointTree.query over a stubbed points_nearest_k: (S,) for k = 1, (S, k) otherwise, () / (k,) for a single
    (3,) point, S = 0, intp indices, and the missing neighbour as (n, inf)."""
    from mesh_amd import _native as N, search, spatialsearch
    n = 5
    seen = []

    def stub(tree, q, k, max_distance=np.inf):
        assert q.ndim == 2 and q.shape[1] == 3 and q.dtype == np.float64
        seen.append((q.shape[0], k, max_distance))
        S = q.shape[0]
        idx = np.tile(np.arange(k, dtype=np.uint32), (S, 1))
        dist = np.tile(np.arange(k, dtype=np.float64), (S, 1))
        idx[:, k - 1:] = N.NO_FACE  # the last rank is missing
        dist[:, k - 1:] = np.inf
        return idx, dist, np.full(S, k - 1, np.uint32)

    monkeypatch.setattr(spatialsearch, "points_nearest_k", stub)
    cpt = search.ClosestPointTree.__new__(search.ClosestPointTree)
    cpt.v, cpt._h = np.zeros((n, 3)), None
    d, i = cpt.query(np.zeros((7, 3)))
    assert d.shape == (7,) and i.shape == (7,) and i.dtype == np.intp and d.dtype == np.float64
    assert (i == n).all() and np.isinf(d).all()
    d, i = cpt.query(np.zeros((7, 3)), k=4, distance_upper_bound=2.5)
    assert d.shape == (7, 4) and i.shape == (7, 4) and i.dtype == np.intp
    assert (i[:, :3] == [0, 1, 2]).all() and (i[:, 3] == n).all() and np.isinf(d[:, 3]).all()
    d, i = cpt.query(np.zeros(3))
    assert np.shape(d) == () and np.shape(i) == () and i == n
    d, i = cpt.query(np.zeros(3), k=3)
    assert d.shape == (3,) and i.shape == (3,) and i.dtype == np.intp
    d, i = cpt.query(np.zeros((0, 3)), k=1)
    assert d.shape == (0,) and i.shape == (0,)
    d, i = cpt.query(np.zeros((0, 3)), k=2)
    assert d.shape == (0, 2) and i.shape == (0, 2) and i.dtype == np.intp
    assert seen == [(7, 1, np.inf), (7, 4, 2.5), (1, 1, np.inf), (1, 3, np.inf), (0, 1, np.inf), (0, 2, np.inf)]
