"""All-within-radius queries: the checks that need no GPU -- every new C entry point refuses a NULL handle and a negative
or NaN scalar radius with MSH_EINVAL and a message naming it (the scalar is checked before the handle, so no device is
needed to see the refusal), the ctypes prototypes agree with the header, the Python layers validate their arguments
before any device work, and ClosestPointTree.query_ball_point follows scipy's shape rules (on stubbed native calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAMES = ["msh_points_within_count", "msh_points_within_count_device", "msh_tree_within_count",
         "msh_tree_within_count_device", "msh_points_within", "msh_points_within_device", "msh_tree_within",
         "msh_tree_within_device", "msh_tree_within_stats"]


def _calls(L, N, handle, r, r_rows=None):
    q = np.zeros(3)
    idx, dist, cnt = np.zeros(4, np.uint32), np.zeros(4), np.zeros(1, np.uint32)
    pt, part = np.zeros(12), np.zeros(4, np.uint32)
    K = N._sz(0)
    st = (ctypes.c_uint64 * 4)()
    rr = N.dptr(r_rows)
    return {
        "msh_points_within_count": lambda: L.msh_points_within_count(handle, N.dptr(q), 1, r, rr, N.uptr(cnt)),
        "msh_points_within_count_device": lambda: L.msh_points_within_count_device(handle, None, 1, r, None, None, None),
        "msh_tree_within_count": lambda: L.msh_tree_within_count(handle, N.dptr(q), 1, r, rr, N.uptr(cnt)),
        "msh_tree_within_count_device": lambda: L.msh_tree_within_count_device(handle, None, 1, r, None, None, None),
        "msh_points_within": lambda: L.msh_points_within(handle, N.dptr(q), 1, r, rr, N.uptr(cnt), N.uptr(idx),
                                                         N.dptr(dist), 4, ctypes.byref(K)),
        "msh_points_within_device": lambda: L.msh_points_within_device(handle, None, 1, r, None, None, None, None, 0,
                                                                       ctypes.byref(K), None),
        "msh_tree_within": lambda: L.msh_tree_within(handle, N.dptr(q), 1, r, rr, N.uptr(cnt), N.uptr(idx), N.dptr(dist),
                                                     N.dptr(pt), N.uptr(part), 4, ctypes.byref(K)),
        "msh_tree_within_device": lambda: L.msh_tree_within_device(handle, None, 1, r, None, None, None, None, None,
                                                                   None, 0, ctypes.byref(K), None),
        "msh_tree_within_stats": lambda: L.msh_tree_within_stats(handle, None, 1, r, None, st),
    }


def test_null_handles_rejected():
    from mesh_amd import _native as N
    L = N.lib()
    calls = _calls(L, N, None, 1.0)
    assert sorted(calls) == sorted(NAMES)
    for name, call in calls.items():
        assert call() == N.MSH_EINVAL, name
        msg = L.msh_last_error()
        assert msg and b"null" in msg and name.encode() in msg, (name, msg)
    # with per-row radii the scalar is ignored, so a bad one reaches the handle check
    for name, call in _calls(L, N, None, -1.0, np.ones(1)).items():
        if name.endswith("_device") or name.endswith("_stats"):
            continue
        assert call() == N.MSH_EINVAL, name
        assert b"null" in L.msh_last_error(), (name, L.msh_last_error())


@pytest.mark.parametrize("r", [-1.0, float("nan"), -INF])
def test_bad_scalar_radius_rejected(r):
    from mesh_amd import _native as N
    L = N.lib()
    for name, call in _calls(L, N, None, r).items():
        assert call() == N.MSH_EINVAL, (name, r)
        msg = L.msh_last_error()
        assert b"r_max" in msg and name.encode() in msg, (name, r, msg)


def test_prototypes_match_header():
    """every within entry point of the header is exported, has a ctypes prototype, and the two agree on the number of
    arguments and on which are passed by value (size_t, double)"""
    from mesh_amd import _native as N
    txt = open(os.path.join(ROOT, "include", "meshsearch.h")).read()
    decls = dict(re.findall(r"^int (msh_\w*within\w*)\(([^;]*)\);", txt, flags=re.M | re.S))
    assert sorted(decls) == sorted(NAMES)
    sigs = {name: (res, args) for name, res, args in N.SIGNATURES}
    L = N.lib()
    for name, params in decls.items():
        assert hasattr(L, name), name
        res, args = sigs[name]
        params = [p.strip() for p in params.replace("\n", " ").split(",")]
        assert res is ctypes.c_int and len(args) == len(params), (name, params)
        for p, a in zip(params, args):
            if p.startswith("size_t "):
                assert a is ctypes.c_size_t, (name, p)
            elif p.startswith("double "):
                assert a is ctypes.c_double, (name, p)
            else:
                assert "*" in p or "[" in p, (name, p)
                assert a not in (ctypes.c_size_t, ctypes.c_double), (name, p)


def test_check_within():
    from mesh_amd import _native as N
    assert N.check_within(0.5, 7, "f") == (0.5, None)
    assert N.check_within(INF, 0, "f") == (INF, None)
    assert N.check_within(np.float32(2.0), 3, "f") == (2.0, None)
    assert N.check_within(0, 3, "f") == (0.0, None)
    r_max, rows = N.check_within([1, -2, float("nan")], 3, "f")  # per-row values are not judged: those rows are empty
    assert r_max == 0.0 and rows.dtype == np.float64 and rows.flags.c_contiguous and rows.shape == (3,)
    assert rows[0] == 1.0 and rows[1] == -2.0 and np.isnan(rows[2])
    rows = N.check_within(np.arange(8.0)[::2], 4, "f")[1]
    assert rows.flags.c_contiguous and rows.tolist() == [0.0, 2.0, 4.0, 6.0]
    assert N.check_within(np.zeros(0), 0, "f")[1].shape == (0,)
    for bad in (-1.0, float("nan"), -INF):
        with pytest.raises(ValueError, match="f: the radius must be >= 0"):
            N.check_within(bad, 3, "f")
    for bad in (np.zeros(2), np.zeros((3, 1)), np.zeros((1, 3)), [1.0]):
        with pytest.raises(ValueError, match="f: r must be a scalar or of shape"):
            N.check_within(bad, 3, "f")


def test_python_validation_before_device_work():
    from mesh_amd import _native as N, search, spatialsearch
    fake = N.Handle(1, "triangles")  # never dereferenced: validation must raise first
    fake_n = N.Handle(1, "normals")
    fake_p = N.Handle(1, "points")
    q = np.zeros((4, 3))
    tri_fns = (spatialsearch.aabbtree_within, spatialsearch.aabbtree_within_count)
    pt_fns = (spatialsearch.points_within, spatialsearch.points_within_count)
    try:
        for fn, good, others in ((tri_fns, fake, (fake_n, fake_p)), (pt_fns, fake_p, (fake, fake_n))):
            for f in fn:
                with pytest.raises(ValueError, match="Input must be Nx3"):
                    f(good, np.zeros((4, 2)), 1.0)
                with pytest.raises(ValueError, match="Input must be Nx3"):
                    f(good, np.zeros(3), 1.0)
                with pytest.raises(TypeError, match=r"%s\(\) argument 2 must be numpy.ndarray" % f.__name__):
                    f(good, [[0.0, 0.0, 0.0]], 1.0)
                with pytest.raises(TypeError, match="expected a tree handle"):
                    f(None, q, 1.0)
                for h in others:
                    with pytest.raises(TypeError, match="is not a (point|triangle) tree"):
                        f(h, q, 1.0)
                for r in (-1.0, float("nan")):
                    with pytest.raises(ValueError, match="radius must be >= 0"):
                        f(good, q, r)
                for r in (np.zeros(3), np.zeros((4, 1)), np.zeros((2, 2))):
                    with pytest.raises(ValueError, match="r must be a scalar or of shape"):
                        f(good, q, r)
        # the classes over them: the same refusals, still with no device work
        tree = search.AabbTree.__new__(search.AabbTree)
        tree.cpp_handle = fake
        with pytest.raises(ValueError, match="radius must be >= 0"):
            tree.within(q, -2.0)
        with pytest.raises(ValueError, match="r must be a scalar or of shape"):
            tree.count_within(q, np.zeros(5))
        cpt = search.ClosestPointTree.__new__(search.ClosestPointTree)
        cpt.v, cpt._h = np.zeros((5, 3)), fake_p
        with pytest.raises(ValueError, match="radius must be >= 0"):
            cpt.within(q, float("nan"))
        with pytest.raises(ValueError, match="radius must be >= 0"):
            cpt.query_ball_point(q, -1.0)
        with pytest.raises(ValueError, match="only p = 2"):
            cpt.query_ball_point(q, 1.0, p=1)
        with pytest.raises(ValueError, match="only p = 2"):
            cpt.query_ball_point(q, 1.0, p=np.inf)
        with pytest.raises(ValueError, match="only eps = 0"):
            cpt.query_ball_point(q, 1.0, eps=0.5)
        with pytest.raises(ValueError, match=r"x must have shape \(\.\.\., 3\)"):
            cpt.query_ball_point(np.zeros((4, 2)), 1.0)
        with pytest.raises(ValueError, match="does not broadcast"):
            cpt.query_ball_point(q, np.zeros(3))
    finally:
        fake.ptr = fake_n.ptr = fake_p.ptr = None


def test_query_ball_point_shape_rules(monkeypatch):
    """ClosestPointTree.query_ball_point over stubbed points_within / points_within_count: a list (or an int) for a
    single (3,) point, an object array of lists (or an intp array) of the leading shape otherwise, r broadcast against
    the rows, and the three values of return_sorted."""
    from mesh_amd import search, spatialsearch
    seen = []

    def rows_of(q, r):
        assert q.ndim == 2 and q.shape[1] == 3 and q.dtype == np.float64 and q.flags.c_contiguous
        r = np.asarray(r)
        assert r.ndim == 0 or (r.shape == (q.shape[0],) and r.dtype == np.float64 and r.flags.c_contiguous)
        return q.shape[0], np.broadcast_to(r, (q.shape[0],))

    def within(tree, q, r):
        # row i lists the indices 2 i + 3, 2 i + 1, ..., nearest first: floor(r_i) of them
        S, rr = rows_of(q, r)
        seen.append(("within", S, np.asarray(r).ndim))
        counts = rr.astype(np.uint32)
        idx = np.concatenate([2 * i + 3 - 2 * np.arange(c) for i, c in enumerate(counts)] + [np.zeros(0, np.int64)])
        dist = np.concatenate([np.arange(c, dtype=np.float64) for c in counts] + [np.zeros(0)])
        return counts, idx.astype(np.uint32), dist

    def within_count(tree, q, r):
        S, rr = rows_of(q, r)
        seen.append(("count", S, np.asarray(r).ndim))
        return rr.astype(np.uint32)

    monkeypatch.setattr(spatialsearch, "points_within", within)
    monkeypatch.setattr(spatialsearch, "points_within_count", within_count)
    cpt = search.ClosestPointTree.__new__(search.ClosestPointTree)
    cpt.v, cpt._h = np.zeros((50, 3)), None
    one = cpt.query_ball_point(np.zeros(3), 2.0)
    assert one == [3, 1] and all(type(x) is int for x in one)  # None on a single point: as found, nearest first
    assert cpt.query_ball_point(np.zeros(3), 2.0, return_sorted=True) == [1, 3]
    assert cpt.query_ball_point(np.zeros(3), 2.0, return_sorted=False) == [3, 1]
    n = cpt.query_ball_point(np.zeros(3), 2.0, return_length=True)
    assert n == 2 and type(n) is int
    assert cpt.query_ball_point([0.0, 0.0, 0.0], 0.5) == []
    many = cpt.query_ball_point(np.zeros((3, 3)), [2.0, 0.0, 3.0])
    assert many.shape == (3,) and many.dtype == object and all(type(x) is list for x in many)
    assert list(many) == [[1, 3], [], [3, 5, 7]]  # None on multi-point input: ascending by index
    assert list(cpt.query_ball_point(np.zeros((3, 3)), 2.0, return_sorted=True)) == [[1, 3], [3, 5], [5, 7]]
    assert list(cpt.query_ball_point(np.zeros((3, 3)), 2.0, return_sorted=False)) == [[3, 1], [5, 3], [7, 5]]
    n = cpt.query_ball_point(np.zeros((3, 3)), [2.0, 0.0, 3.0], return_length=True)
    assert n.shape == (3,) and n.dtype == np.intp and n.tolist() == [2, 0, 3]
    grid = cpt.query_ball_point(np.zeros((2, 2, 3)), [[1.0], [2.0]])  # r (2,1) against the (2,2) samples
    assert grid.shape == (2, 2) and grid.dtype == object
    assert grid[0, 0] == [3] and grid[0, 1] == [5] and grid[1, 0] == [5, 7] and grid[1, 1] == [7, 9]
    n = cpt.query_ball_point(np.zeros((2, 2, 3)), 1.0, return_length=True)
    assert n.shape == (2, 2) and n.dtype == np.intp and (n == 1).all()
    empty = cpt.query_ball_point(np.zeros((0, 3)), 1.0)
    assert empty.shape == (0,) and empty.dtype == object
    assert cpt.query_ball_point(np.zeros((0, 3)), 1.0, return_length=True).shape == (0,)
    assert cpt.query_ball_point(np.zeros(3), 2.0, workers=-1) == [3, 1]
    assert seen[:5] == [("within", 1, 0), ("within", 1, 0), ("within", 1, 0), ("count", 1, 0), ("within", 1, 0)]
    assert ("within", 3, 1) in seen and ("within", 4, 1) in seen and ("count", 4, 0) in seen
    # ClosestPointTree.within: the CSR as it comes, indices as intp
    counts, idx, dist = cpt.within(np.zeros((2, 3)), 2.0)
    assert counts.tolist() == [2, 2] and idx.dtype == np.intp and idx.tolist() == [3, 1, 5, 3] and dist.dtype == np.float64
