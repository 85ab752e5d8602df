"""A walk does not queue the leaf its query has already evaluated (knn.h WalkerT::step_list / step_collect).

A leaf that was evaluated for the query before the walk reaches it -- the cell's hint leaf in the lean kernel, the
query's best leaf in the generic ones -- is dropped there, so its second exact construction never runs.  That
construction could only offer a (d2, face) already offered, so every answer must stay what brute force gives, bit for
bit on face, part and point.  The cases
are the ones where a wrong rule would show: the skipped leaf is the winner; the skipped leaf ties with others of a
lower or a higher face index; the cut's entries are ~leaf refs (the step's `node < 0` branch); rows past their step
budget, deferred to pass 2 or refused by a full list and resumed.

Every case has 4096 + 37 rows (64 full tiles and a partial one of a sorted launch) on a geodesic sphere of 8,820 faces
(>= 4096 leaves: nothing takes the small-tree path), runs with the fine automatic grid and with an explicit 8^3 one,
and is asked again of the generic list kernel (MESH_AMD_KNN_LEAN=0), of the list without the node prefetch
(MESH_AMD_LEAF_LIST=2) and of the per-lane queues (MESH_AMD_LEAF_LIST=0); only the plain closest-point call runs under
those hooks.
"""
import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

NO_FACE = 0xFFFFFFFF
SORT_MIN = 4096  # api.cpp kSortMin: launches below it are unsorted
S = SORT_MIN + 37
GRIDS = {"auto_grid": -1, "grid8": 8}


@pytest.fixture(scope="module", autouse=True)
def _device():
    from mesh_amd import _native
    _native.set_device(0)


def _nearest_tree(t, q):
    from mesh_amd import spatialsearch
    face, part, pt = spatialsearch.aabbtree_nearest(t, np.ascontiguousarray(q, np.float64))
    return face[0], part[0], pt


def _timed(t, q, name):
    """the arrays, and how many launches ran under the timer `name`"""
    from mesh_amd import _native
    _native.timing_reset()
    _native.timing_enable(True)
    try:
        out = _nearest_tree(t, q)
    finally:
        _native.timing_enable(False)
    return out, _native.timing_get(name)[1]


def _expect(oracle, v, f, q):
    """brute force on the finite rows, NO_FACE / 0 / NaN on the others: an answer for every row"""
    fin = np.isfinite(q).all(axis=1)
    face = np.full(q.shape[0], NO_FACE, np.uint32)
    part = np.zeros(q.shape[0], np.uint32)
    pt = np.full((q.shape[0], 3), np.nan)
    bf, bp, bpt, _ = oracle.brute_nearest(v, f, np.ascontiguousarray(q[fin]))
    face[fin], part[fin], pt[fin] = bf, bp, bpt
    return face, part, pt


def _assert_equal(got, want, what):
    face, part, pt = got
    wf, wp, wpt = want
    assert np.array_equal(face, wf), "%s: faces differ at rows %s" % (what, np.nonzero(face != wf)[0][:10])
    assert np.array_equal(part, wp), "%s: parts differ at rows %s" % (what, np.nonzero(part != wp)[0][:10])
    assert np.array_equal(pt, wpt, equal_nan=True), "%s: points differ" % what
    assert np.array_equal(np.isnan(pt), np.isnan(wpt))


def _auto_G(f):
    # entrycut.cpp cut_grid: the fine automatic grid, twice the coarse one's resolution (8 cells per face, at least 16^3)
    return 2 * max(16, int(round(np.cbrt(8 * f.shape[0]))))


def _grid_planes(v, G):
    # entrycut.cpp build_entry_cut: the scene box (fp32 bounds of the vertices) widened by 1/4, G cells per axis
    lo32, hi32 = v.astype(np.float32).min(0).astype(np.float64), v.astype(np.float32).max(0).astype(np.float64)
    half = 0.5 * (hi32 - lo32)
    m = 0.5 * (hi32 + lo32)
    e = 1.25 * np.maximum(half, 0.05 * half.max())
    return m - e, 2.0 * e / G


@pytest.fixture(scope="module")
def ico():
    v, f = W.geodesic_icosphere(21)
    assert f.shape[0] == 8820
    return np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.uint32)


def _unit_normals(v, f):
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n /= np.linalg.norm(n, axis=1)[:, None]
    c = v[f].mean(axis=1)
    return np.where((n * c).sum(1)[:, None] < 0, -n, n), c  # outward: the sphere is centred at the origin


def _edges(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64), axis=1)
    return np.unique(e, axis=0)


@pytest.fixture(scope="module")
def cases(ico, oracle):
    """name -> (rows, brute-force answer), each computed once"""
    v, f = ico
    rng = np.random.default_rng(1001)
    n, c = _unit_normals(v, f)
    out = {}
    # 1: the hint leaf is the answer -- 1e-3 off the centroids of a sample of the faces, on either side
    pick = rng.choice(f.shape[0], S, replace=False)
    out["hint_wins"] = c[pick] + 1e-3 * rng.choice([-1.0, 1.0], S)[:, None] * n[pick]
    # 2: ties -- on vertices (5 or 6 faces at d2 = 0) and on the outward normal through edge midpoints (2 faces)
    nv = 2100
    vi = rng.choice(v.shape[0], nv, replace=False)
    e = _edges(f)
    e = e[rng.choice(e.shape[0], S - nv, replace=False)]
    mid = 0.5 * (v[e[:, 0]] + v[e[:, 1]])
    up = mid / np.linalg.norm(mid, axis=1)[:, None]
    out["ties"] = np.concatenate([v[vi], mid + rng.choice([0.0, 1e-3, 0.05], S - nv)[:, None] * up])
    # 3: within 1e-4 of the surface -- the fine grid's cells there hold ~leaf entries
    fi = rng.integers(0, f.shape[0], S)
    b = rng.dirichlet([1.0, 1.0, 1.0], S)
    on = (b[:, :, None] * v[f[fi]]).sum(axis=1)
    out["near_surface"] = on + rng.uniform(-1e-4, 1e-4, S)[:, None] * n[fi]
    # 4: past the step budget (max(64, T / 16) = 551 node steps; from the centre nearly every one of the 17,639 nodes
    # is within the bound) -- the centre, 2000 rows around it, non-finite rows, uniform rows for the rest
    d = rng.normal(size=(2000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    bad = rng.uniform(-1.0, 1.0, (36, 3))
    bad[np.arange(36), rng.integers(0, 3, 36)] = np.array([np.nan, np.inf, -np.inf])[np.arange(36) % 3]
    bad[:3] = np.array([[np.nan] * 3, [np.inf] * 3, [-np.inf] * 3])
    q = np.concatenate([np.zeros((1, 3)), d * rng.uniform(0.0, 0.02, (2000, 1)), bad,
                        rng.uniform(-1.2, 1.2, (S - 2037, 3))])
    out["deferral"] = q[rng.permutation(S)]
    res = {}
    for name, q in out.items():
        q = np.ascontiguousarray(q)
        assert q.shape == (S, 3)
        res[name] = (q, _expect(oracle, v, f, q))
    res["hint_pick"] = pick
    res["ties_nv"] = nv
    res["ties_vi"] = vi
    return res


def test_case_premises(ico, oracle, cases):
    # CPU, from the oracle alone: the cases are what they say
    v, f = ico
    q, want = cases["hint_wins"]
    assert np.array_equal(want[0], cases["hint_pick"].astype(np.uint32))  # case 1: each row answers its own face
    # case 2: the faces around a vertex row's vertex that hold the smallest d2 tie (the construction gives exactly 0 for
    # most, not all, of them), and the lowest of them is the answer; in both grids some tied rows sit in a cell whose
    # hint (the face nearest to the cell's centre) is a tied face with a higher index, and some in a cell whose hint is
    # the answer itself
    q, want = cases["ties"]
    nv, vi = cases["ties_nv"], cases["ties_vi"]
    around = [[] for _ in range(v.shape[0])]
    for k, tri in enumerate(f):
        for j in tri:
            around[j].append(k)
    tied = []
    for r in range(nv):
        d2 = [oracle.point_triangle(q[r], *v[f[k]])[2] for k in around[vi[r]]]
        tied.append({k for k, d in zip(around[vi[r]], d2) if d == min(d2)})
        assert int(want[0][r]) == min(tied[r]) and np.array_equal(want[2][r], q[r])
    assert sum(len(s) >= 5 for s in tied) > nv // 2
    for G in (_auto_G(f), 8):
        lo, w = _grid_planes(v, G)
        cell = np.clip(np.floor((q - lo) / w).astype(np.int64), 0, G - 1)
        ucell, inv = np.unique(cell, axis=0, return_inverse=True)
        hint = oracle.brute_nearest(v, f, np.ascontiguousarray(lo + (ucell + 0.5) * w))[0][inv.reshape(-1)]
        assert (hint != want[0]).any() and (hint == want[0]).any()
        higher = sum(int(hint[r]) in tied[r] and hint[r] > want[0][r] for r in range(nv))
        lowest = sum(len(tied[r]) > 1 and hint[r] == want[0][r] for r in range(nv))
        assert higher > 0, "G = %d: no hint is a tied face of a higher index" % G
        assert lowest > 0, "G = %d: no hint is the lowest tied face" % G


@pytest.fixture(scope="module", params=list(GRIDS), ids=list(GRIDS))
def cut_tree(ico, request):
    """the sphere's tree with its entry cut built: the fine automatic grid, or 8^3 cells"""
    from mesh_amd import spatialsearch
    v, f = ico
    G = GRIDS[request.param]
    t = spatialsearch.aabbtree_compute(v, f)
    t.set_entry_cut(G)
    _nearest_tree(t, np.zeros((1, 3)))  # a requested grid is built by the next call, whatever its size
    info = t.entry_cut_info()
    assert info["state"] == "built" and info["G"] == (_auto_G(f) if G < 0 else G)
    return t


HOOKS = [{}, {"MESH_AMD_KNN_LEAN": "0"}, {"MESH_AMD_LEAF_LIST": "2"}, {"MESH_AMD_LEAF_LIST": "0"}]


def _check_all_kernels(t, q, want, what, monkeypatch, extra=None):
    for hook in HOOKS:
        with monkeypatch.context() as m:
            for k, val in dict(hook, **(extra or {})).items():
                m.setenv(k, val)
            got, n_lean = _timed(t, q, "knn_lean")
        assert n_lean == (0 if hook else 1), "%s, %s: %d lean launches" % (what, hook, n_lean)
        _assert_equal(got, want, "%s, %s" % (what, hook or "lean kernel"))


@pytest.mark.parametrize("case", ["hint_wins", "ties", "near_surface"])
def test_bit_exact(cut_tree, cases, monkeypatch, case):
    q, want = cases[case]
    _check_all_kernels(cut_tree, q, want, case, monkeypatch)


@pytest.mark.parametrize("cap", [None, "8"])
def test_deferral_bit_exact(cut_tree, cases, monkeypatch, cap):
    # the whole list: pass 2 finishes the rows past their budget from their records (best leaf included); a list of
    # MESH_AMD_MAX_DEFERRED=8 records: all but 8 of them are refused and take their walk up again in pass 1
    q, want = cases["deferral"]
    extra = {"MESH_AMD_MAX_DEFERRED": cap} if cap else None
    _check_all_kernels(cut_tree, q, want, "deferral, list of %s" % (cap or "default"), monkeypatch, extra)
