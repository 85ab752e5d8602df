"""The directional drop proved on sub-cells (cutbuild.hip cut_dir_drop, depth MESH_AMD_CUT_SUBDIV = 0 / 1 / 2) changes no
answer.

As tests/test_gpu_cut_directional.py: walks without a cut (set_entry_cut(0)) are the reference, and walks from a cut
built at each depth -- freshly built each time, on grids 16, 32, 64 and the fine automatic one -- give face, part and
point array_equal to them, from the lean pass-1 kernel and from the generic one; a 2,000-row sample of the reference is
checked against the oracle's exhaustive search.  Every mesh has at least 4096 faces (smaller trees take no cut).  The
rows are that file's five groups plus rows where a sub-cell rule could go wrong at a seam: on the planes that bound
the octants and their octants (coordinates glo + m w / 8: cell faces, mid-planes, the pieces' own centre planes), one
ulp to either side of them, and on the pieces' corners.  The nested shells put the centre's closest point pc and a
row's answer on different sheets, where |q - pc| is a poor bound of d(q).

The alongnormal walks give the answers of walks without the cut at every depth, and a deeper rule flags no fewer cells
than depth 0 on the same grid (it only adds drops).

The depth a build takes is pinned too: the hook changes the cut (strictly more flagged cells per depth on the fine
grids), the volume policy's own upgrade stays at depth 0 and a requested fine grid takes depth 2.

No instrumented (*_stats) entry point is called here.
"""
import functools

import numpy as np
import pytest

import test_gpu_cut_directional as D
import workloads as W

pytestmark = pytest.mark.gpu

GRIDS = (16, 32, 64, -1)
DEPTHS = (0, 1, 2)
MESHES = ["ico16", "bumpy16", "flat48", "zero16", "shells16"]
HOOK = "MESH_AMD_CUT_SUBDIV"


@pytest.fixture(scope="module", autouse=True)
def _device():
    from mesh_amd import _native
    _native.set_device(0)


def _mesh(name):
    if name == "shells16":  # the icosphere at radius 1 and at 0.6, one mesh
        v, f = W.geodesic_icosphere(16)
        f = np.asarray(f)
        return np.concatenate([v, 0.6 * v]), np.concatenate([f, f + v.shape[0]])
    return D._mesh(name)


def _grid(g, T):
    # the grid the fine automatic request builds (entrycut.cpp cut_grid): twice the coarse one's cells per axis
    return g if g > 0 else 2 * max(16, int(round(np.cbrt(min(8 * T, 1 << 23)))))


def _seam_rows(v, G, seed):
    """Rows on the planes x_k = glo_k + m w_k / 8 (m integer: every boundary and centre plane of the cells, their
    octants and the octants' octants), the same rows one ulp below and above the plane, and rows on the pieces' corners
    (all three coordinates on multiples of w / 4)."""
    rng = np.random.default_rng(seed)
    glo, ext = D._grid_box(v)
    w = ext / G
    n = 1500
    on = glo + rng.uniform(0, 1, (n, 3)) * ext
    ax = rng.integers(0, 3, n)
    plane = (glo + rng.integers(0, 8 * G + 1, (n, 3)) * (w / 8))[np.arange(n), ax]
    on[np.arange(n), ax] = plane
    below, above = on.copy(), on.copy()
    below[np.arange(n), ax] = np.nextafter(plane, -np.inf)
    above[np.arange(n), ax] = np.nextafter(plane, np.inf)
    corners = glo + rng.integers(0, 4 * G + 1, (n, 3)) * (w / 4)
    return np.concatenate([on, below, above, corners])


@functools.lru_cache(maxsize=None)
def _case(name):
    """The mesh's tree, and per grid its rows and their answers from walks without a cut (computed once, shared by the
    depths)."""
    from mesh_amd import spatialsearch
    v, f = _mesh(name)
    v = np.ascontiguousarray(v, np.float64)
    f = np.ascontiguousarray(f, np.uint32)
    assert f.shape[0] >= 4096
    t = spatialsearch.aabbtree_compute(v, f)
    t.set_entry_cut(0)
    rows = {}
    for g in GRIDS:
        G = _grid(g, f.shape[0])
        q = np.ascontiguousarray(np.concatenate([D._queries(v, f, G, seed=300 + abs(g)), _seam_rows(v, G, 400 + abs(g))]))
        assert q.shape[0] >= 4096
        ref = D._nearest(t, q)
        for a in (q,) + tuple(ref):
            a.setflags(write=False)
        rows[g] = (G, q, ref)
    return v, f, t, rows


@pytest.mark.parametrize("name", MESHES)
def test_subcell_reference_is_the_oracles(oracle, name):
    v, f, _, rows = _case(name)
    for g in GRIDS:
        _, q, ref = rows[g]
        pick = np.random.default_rng(7).choice(q.shape[0], 2000, replace=False)
        assert np.array_equal(ref[0][pick], oracle.brute_nearest(v, f, q[pick])[0])


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", MESHES)
def test_subcell_cut_bit_exact(monkeypatch, name, depth):
    v, f, t, rows = _case(name)
    monkeypatch.setenv(HOOK, str(depth))  # read when the cut is built
    flagged = 0
    try:
        for g in GRIDS:
            G, q, ref = rows[g]
            t.set_entry_cut(0)  # drops the installed cut: the next one is built afresh at this depth
            t.set_entry_cut(g)
            D._same(ref, D._nearest(t, q))
            info = t.entry_cut_info()
            assert info["state"] == "built" and info["G"] == G and info["bytes"] == G ** 3 * 32, info
            flagged += info["flagged"]
            monkeypatch.setenv("MESH_AMD_KNN_LEAN", "0")  # the generic kernel reads the same records
            D._same(ref, D._nearest(t, q))
            monkeypatch.delenv("MESH_AMD_KNN_LEAN")
    finally:
        t.set_entry_cut(0)
    assert flagged > 0  # the far rows' cells took the directional rule


@pytest.mark.parametrize("name", ["ico16", "bumpy16", "flat48", "shells16"])
def test_subcell_cut_alongnormal_bit_exact(monkeypatch, name):
    # rays from 0.3-0.9 off the surface (half of them in random directions) and from the surface itself, against
    # walks without the cut, at every depth
    from mesh_amd import spatialsearch
    v, f, t, _ = _case(name)
    rng = np.random.default_rng(5)
    p, nn = D._surface(v, f, 8192, seed=9)
    off = rng.uniform(0.3, 0.9, (4096, 1)) * rng.choice([-1.0, 1.0], (4096, 1))
    p[:4096] += nn[:4096] * off
    rd = rng.normal(size=(2048, 3))
    nn[:2048] = rd / np.linalg.norm(rd, axis=1)[:, None]
    t.set_entry_cut(0)
    ref = spatialsearch.aabbtree_nearest_alongnormal(t, p, nn)
    flagged = {}
    try:
        for depth in DEPTHS:
            monkeypatch.setenv(HOOK, str(depth))
            for g in GRIDS:
                t.set_entry_cut(0)
                t.set_entry_cut(g)
                got = spatialsearch.aabbtree_nearest_alongnormal(t, p, nn)
                info = t.entry_cut_info()
                assert info["state"] == "built", info
                flagged[depth, g] = info["flagged"]
                assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])
                assert np.array_equal(ref[2].view(np.int64), got[2].view(np.int64))  # NaN points of misses too
    finally:
        t.set_entry_cut(0)
    print("flagged cells per (depth, grid)", flagged)
    for g in GRIDS:
        assert flagged[1, g] >= flagged[0, g] and flagged[2, g] >= flagged[0, g], (g, flagged)
    assert flagged[0, 64] > 0 and flagged[0, -1] > 0
    # the hook is read: each depth proves drops in cells the depth before it could not shorten (cells 0.3-0.9 off the
    # surface, r far below that), so the three builds differ
    for g in (64, -1):
        assert flagged[0, g] < flagged[1, g] < flagged[2, g], (g, flagged)


def test_subcell_depth_of_automatic_and_requested_grids(monkeypatch):
    """The fine grid the volume policy builds on its own keeps the drop on whole cells (its rows threshold is sized
    for that build); a fine grid the caller asks for takes the sub-cell depth.  Seen without instrumented kernels in
    the number of flagged records: the automatic upgrade's equals that of a requested grid built with the hook at 0,
    and the requested grid's default exceeds it and equals the hook at 2."""
    from mesh_amd import spatialsearch
    monkeypatch.delenv(HOOK, raising=False)
    v, f = _mesh("ico16")
    v = np.ascontiguousarray(v, np.float64)
    f = np.ascontiguousarray(f, np.uint32)
    G = _grid(-1, f.shape[0])
    glo, ext = D._grid_box(v)
    # entrycut.cpp: the fine grid once the handle has answered 16 rows per fine cell (64 cells per leaf)
    rows = 16 * 64 * f.shape[0] + 4096
    q = np.ascontiguousarray(glo + np.random.default_rng(21).uniform(0, 1, (rows, 3)) * ext)
    t = spatialsearch.aabbtree_compute(v, f)
    auto_ans = D._nearest(t, q)  # this call reaches the volume: the automatic fine grid, then the walks from it
    auto = t.entry_cut_info()
    assert auto["state"] == "built" and auto["G"] == G, auto
    got = {}
    for hook in ("0", None, "2"):
        if hook is None:
            monkeypatch.delenv(HOOK, raising=False)
        else:
            monkeypatch.setenv(HOOK, hook)
        t.set_entry_cut(0)
        t.set_entry_cut(-1)
        D._same([a[:8192] for a in auto_ans], D._nearest(t, q[:8192]))
        info = t.entry_cut_info()
        assert info["state"] == "built" and info["G"] == G, info
        got[hook] = info["flagged"]
    print("flagged: automatic", auto["flagged"], "requested", got)
    assert auto["flagged"] == got["0"]
    assert got[None] == got["2"] > got["0"] > 0
