"""The lean pass-1 kernel of cut-started closest-point launches (nearest.hip k_knn_lean) against brute force.

launch_knn takes the lean kernel for a sorted launch (>= 4096 rows: direct stores) of a tree with a narrow entry cut;
MESH_AMD_KNN_LEAN=0 forces the generic kernel.  Every case runs on a mesh small enough for the exhaustive oracle to
answer every row, with the fine automatic grid and with an explicit small one, and every row is compared: face, part
code and point are bit-exact, non-finite rows answer NO_FACE / part 0 / NaN.  Launches of fewer than 4096 rows are
unsorted and go to the generic kernel whatever the hook says, so the small row counts come twice: as they are, and
on top of 4096 rows (64 full tiles), where the lean kernel meets the same partial tile.
"""
import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

NO_FACE = 0xFFFFFFFF
SORT_MIN = 4096  # api.cpp kSortMin: launches below it are unsorted


@pytest.fixture(scope="module", autouse=True)
def _device():
    from mesh_amd import _native
    _native.set_device(0)


def _tree(v, f, G):
    from mesh_amd import spatialsearch
    t = spatialsearch.aabbtree_compute(np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.uint32))
    t.set_entry_cut(G)
    return t


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


def _grid_planes(v, G):
    # entrycut.cpp build_entry_cut: the scene box (fp32 bounds of the vertices) widened by 1/4, G cells per axis
    lo32, hi32 = v.astype(np.float32).min(0).astype(np.float64), v.astype(np.float32).max(0).astype(np.float64)
    half = 0.5 * (hi32 - lo32)
    m = 0.5 * (hi32 + lo32)
    e = 1.25 * np.maximum(half, 0.05 * half.max())
    return m - e, 2.0 * e / G


@pytest.fixture(scope="module")
def ico():
    v, f = W.geodesic_icosphere(15)
    assert f.shape[0] == 4500
    return np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.uint32)


def _auto_G(f):
    # entrycut.cpp cut_grid: the fine automatic grid, twice the coarse one's resolution (8 cells per face, at least 16^3)
    return 2 * max(16, int(round(np.cbrt(8 * f.shape[0]))))


@pytest.fixture(scope="module")
def mixed(ico, oracle):
    """one query set mixing the starts the lean kernel knows, with its brute-force answer (computed once)"""
    v, f = ico
    rng = np.random.default_rng(701)
    parts = [rng.uniform(-1.2, 1.2, (3000, 3))]                       # inside the grid
    out = rng.uniform(-1.0, 1.0, (300, 3))
    out[np.arange(300), rng.integers(0, 3, 300)] = rng.choice([-3.0, 3.0], 300)
    parts.append(out)                                                  # outside it: no cell, root start
    for G in (_auto_G(f), 8):                                          # on cell faces of both grids
        lo, w = _grid_planes(v, G)
        on = rng.uniform(-1.2, 1.2, (1000, 3))
        ax = rng.integers(0, 3, 1000)
        on[np.arange(1000), ax] = lo[ax] + rng.integers(0, G + 1, 1000) * w[ax]
        parts.append(on)
    parts.append(v)                                                    # ties: the smallest face wins
    parts.append(np.concatenate([0.5 * (v[f[:, a]] + v[f[:, b]]) for a, b in ((0, 1), (1, 2), (2, 0))]))
    d = rng.normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    parts.append(np.zeros((1, 3)))                                     # past the step budget: deferred to pass 2
    parts.append(d * rng.uniform(0.0, 0.02, (500, 1)))
    bad = rng.uniform(-1.0, 1.0, (30, 3))
    bad[np.arange(30), rng.integers(0, 3, 30)] = np.array([np.nan, np.inf, -np.inf])[np.arange(30) % 3]
    bad[:3] = np.array([[np.nan] * 3, [np.inf] * 3, [-np.inf] * 3])
    parts.append(bad)
    q = np.concatenate(parts)
    q = np.ascontiguousarray(q[rng.permutation(q.shape[0])])
    assert q.shape[0] >= SORT_MIN
    return q, _expect(oracle, v, f, q)


@pytest.fixture(scope="module")
def rows(ico, oracle):
    """20,000 + 4096 uniform rows with their brute-force answer: the row-count cases are prefixes of it"""
    v, f = ico
    q = np.random.default_rng(702).uniform(-1.3, 1.3, (SORT_MIN + 20_000, 3))
    return q, _expect(oracle, v, f, q)


@pytest.fixture(scope="module", params=[-1, 8], ids=["auto_grid", "grid8"])
def cut_tree(ico, request):
    """the icosphere's tree with its entry cut built: the fine automatic grid, or 8^3 cells"""
    v, f = ico
    G = request.param
    t = _tree(v, f, G)
    _nearest_tree(t, np.zeros((1, 3)))  # a requested grid is built by the next call, whatever its size
    info = t.entry_cut_info()
    assert info["state"] == "built" and info["G"] == (_auto_G(f) if G < 0 else G) and info["bytes"] == info["G"] ** 3 * 32
    return t


@pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 20_000, SORT_MIN + 1, SORT_MIN + 63, SORT_MIN + 65, SORT_MIN + 257])
def test_row_counts(cut_tree, rows, S):
    # a partial tile, fewer tiles than a block has waves, ring wrap; from 4096 rows on through the lean kernel
    from mesh_amd import _native
    q, want = rows
    got, n_lean = _timed(cut_tree, q[:S], "knn_lean")
    assert n_lean == (1 if S >= SORT_MIN else 0)
    assert _native.timing_get("knn_pass1")[1] == 1
    _assert_equal(got, tuple(w[:S] for w in want), "S = %d" % S)


def _node_steps(t, q):
    """node visits of the instrumented traversal of q (pass 1 + pass 2; msh_tree_nearest_stats)"""
    import ctypes
    import torch
    from mesh_amd import _native
    dq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    nodes, leaves = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _native.check(_native.lib().msh_tree_nearest_stats(t.ptr, dq.data_ptr(), q.shape[0], ctypes.byref(nodes),
                                                       ctypes.byref(leaves)))
    torch.cuda.synchronize()
    return nodes.value


def test_centre_rows_pass_their_budget(cut_tree, ico):
    # what makes the mixed set reach the deferral and resume records: from either cut, the walk of a row at the centre
    # visits more nodes than pass 1's budget of max(64, T / 16) = 281 steps, so pass 1 hands it to pass 2 (the
    # instrumented traversal starts from the same cut records and visits in the same order)
    v, f = ico
    budget = max(64, f.shape[0] // 16)
    assert budget == 281
    assert _node_steps(cut_tree, np.zeros((64, 3))) > 64 * budget


def test_mixed_queries_bit_exact(cut_tree, mixed):
    q, want = mixed
    got, n_lean = _timed(cut_tree, q, "knn_lean")
    assert n_lean == 1
    _assert_equal(got, want, "mixed queries")


def test_lean_equals_generic(cut_tree, mixed, monkeypatch):
    t = cut_tree
    q, want = mixed
    lean, n_lean = _timed(t, q, "knn_lean")
    assert n_lean == 1
    monkeypatch.setenv("MESH_AMD_KNN_LEAN", "0")
    generic, n_lean0 = _timed(t, q, "knn_lean")
    from mesh_amd import _native
    assert n_lean0 == 0 and _native.timing_get("knn_all")[1] == 1
    monkeypatch.delenv("MESH_AMD_KNN_LEAN")
    for a, b in zip(lean, generic):
        assert np.array_equal(a, b, equal_nan=True)
    _assert_equal(generic, want, "generic kernel")


@pytest.mark.parametrize("lean", ["1", "0"])
@pytest.mark.parametrize("cap", ["1", "16"])
def test_deferred_list_full(cut_tree, mixed, monkeypatch, cap, lean):
    # MESH_AMD_MAX_DEFERRED shortens the deferred list to 1 or 16 records, far fewer than the 501 rows at and around
    # the centre that pass their step budget: a lane whose claim is refused takes its walk up again and finishes in
    # pass 1 (the lean kernel's retry after the tile's loop; the generic kernel's in-loop form with the hook at 0),
    # no record is written past the list, and every row is still answered exactly
    q, want = mixed
    monkeypatch.setenv("MESH_AMD_MAX_DEFERRED", cap)
    monkeypatch.setenv("MESH_AMD_KNN_LEAN", lean)
    got, n_lean = _timed(cut_tree, q, "knn_lean")
    assert n_lean == int(lean)
    _assert_equal(got, want, "deferred list of %s, lean %s" % (cap, lean))


def test_deep_stack(oracle):
    # the clustered-and-spread mesh of test_deep_tree_spill_path: an LBVH deeper than the 16-entry LDS stack, walked
    # from a forced cut, so lanes go through the step's hoisted spill branch
    rng = np.random.default_rng(22)
    pts = np.vstack([rng.normal(size=(3000, 3)) * 1e-4, rng.normal(size=(3000, 3)) * 100])
    v = np.repeat(pts, 3, axis=0) + rng.normal(size=(18000, 3)) * 1e-6
    f = np.arange(18000, dtype=np.uint32).reshape(-1, 3)
    q = rng.normal(size=(5000, 3)) * 50
    t = _tree(v, f, 16)
    _nearest_tree(t, q)  # builds the cut
    assert t.entry_cut_info()["state"] == "built"
    # deeper than the LDS stack (whether a lane's stack reaches 16 entries is not visible from outside the kernel; the
    # depth is the condition the mesh is built for)
    assert t.info().max_depth > 16
    got, n_lean = _timed(t, q, "knn_lean")
    assert n_lean == 1
    _assert_equal(got, _expect(oracle, v, f, q), "deep stack")


@pytest.mark.parametrize("S", [64, SORT_MIN + 64])
def test_every_leaf_a_tie(oracle, S):
    # 6,000 copies of one triangle: every leaf ties with every other, nothing is pruned, and lanes hold dozens of
    # pending leaves, up to the two ring places the lean kernel keeps free; the smallest face index wins
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    v = np.ascontiguousarray(np.tile(tri, (6000, 1)))
    f = np.arange(18000, dtype=np.uint32).reshape(-1, 3)
    rng = np.random.default_rng(703)
    q = np.column_stack([rng.uniform(-0.5, 1.5, S), rng.uniform(-0.5, 1.5, S), rng.uniform(0.1, 1.0, S)])
    t = _tree(v, f, 8)
    _nearest_tree(t, q)  # builds the cut
    assert t.entry_cut_info()["state"] == "built"
    got, n_lean = _timed(t, q, "knn_lean")
    assert n_lean == (1 if S >= SORT_MIN else 0)
    want = _expect(oracle, v, f, q)
    assert (want[0] == 0).all()
    _assert_equal(got, want, "tied leaves, S = %d" % S)
