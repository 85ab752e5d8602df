"""Drop-in for the ``psbody.mesh.spatialsearch`` extension (mesh/src/spatialsearchmodule.cpp).

Same function names, argument order, return shapes/dtypes and ValueError messages as the reference;
the work runs in libmeshsearch's gfx950 kernels (LBVH build, Morton-sorted traversal, fp64 CGAL
constructions).  Deliberate differences:
  * ``aabbtree_nearest`` coerces the query to (N,3) float64 C order instead of reading raw memory
    (reference: spatialsearchmodule.cpp:175-180 checks only dims[1]).
  * ``aabbtree_nearest_alongnormal`` fills face=0xFFFFFFFF / point=NaN on rows with no hit (reference:
    uninitialised memory, :309-311); dist stays 1e100 as in the reference.
  * ``aabbtree_intersections_indices`` is registered and returns ascending indices (reference: not in
    the method table, :35-40, and racy push_back, :393-402).
Beyond the reference: ``aabbtree_intersections_pairs`` / ``aabbtree_selfintersections_pairs`` return which face
hits which face, as a sorted (K, 2) pair list; ``aabbtree_signed_distance`` and ``aabbtree_winding_number`` answer
inside / outside, the first on closed manifold meshes, the second on any triangle set; ``aabbtree_nearest_k`` and
``points_nearest_k`` return the K nearest faces or points of every row, optionally within a radius;
``aabbtree_raycast`` and ``aabbtree_occluded`` answer first-hit and occlusion queries for arbitrary rays,
``aabbtree_raycast_count`` and ``aabbtree_raycast_all`` return how many faces each ray meets and all of them in order;
``aabbtree_within`` / ``points_within`` and their ``_count`` forms return every face or point within a radius of every
row, untruncated, as CSR lists or per-row counts.
"""
import numpy as np

from . import _native as N


class Mesh_IntersectionsError(Exception):
    """Module error object (spatialsearchmodule.cpp:33,60-62)."""


def _check_mesh_arrays(v, f):
    # spatialsearchmodule.cpp:79-97 ("O!O!" + dtype/ndim/Nx3 checks)
    if not isinstance(v, np.ndarray) or not isinstance(f, np.ndarray):
        raise TypeError("aabbtree_compute() arguments must be numpy.ndarray")
    if v.dtype != np.float64 or v.ndim != 2:
        raise ValueError("Vertices must be of type double, and 2 dimensional")
    if f.dtype != np.uint32 or f.ndim != 2:
        raise ValueError("Faces must be of type uint32, and 2 dimensional")
    if v.shape[1] != 3 or f.shape[1] != 3:
        raise ValueError("Input must be Nx3")
    return np.ascontiguousarray(v), np.ascontiguousarray(f)


def aabbtree_compute(v, f):
    """Build the search tree over triangles ``v[f]`` -> opaque handle (capsule in the reference)."""
    v, f = _check_mesh_arrays(v, f)
    return N.build_tree(v, f)


def _tree(tree, fn):
    if not isinstance(tree, N.Handle) or tree.ptr is None:
        raise TypeError("%s: expected a tree handle from aabbtree_compute" % fn)
    if tree.kind == "points":
        raise TypeError("%s: handle is a point tree" % fn)
    return tree


def aabbtree_nearest(tree, q):
    """(face (1,S) uint32, part (1,S) uint32, point (S,3) float64): spatialsearchmodule.cpp:165-220."""
    tree = _tree(tree, "aabbtree_nearest")
    if not isinstance(q, np.ndarray):
        raise TypeError("aabbtree_nearest() argument 2 must be numpy.ndarray")
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("Input must be Nx3")
    q = np.ascontiguousarray(q, dtype=np.float64)
    S = q.shape[0]
    face, part, pt = N.empty_results(((1, S), np.uint32), ((1, S), np.uint32), ((S, 3), np.float64))
    N.check(N.lib().msh_tree_nearest(tree.ptr, N.dptr(q), S, N.uptr(face), N.uptr(part), N.dptr(pt)))
    return face, part, pt


def aabbtree_signed_distance(tree, q):
    """(sdist (S,) float64, face (S,) uint32, part (S,) uint32, point (S,3) float64): ``aabbtree_nearest``'s answer
    and the signed distance to it -- negative inside an outward-oriented closed mesh, positive outside, NaN on
    non-finite rows (no reference counterpart).

    The sign is that of ``(q - point) . N`` with N the angle-weighted pseudonormal of the feature the closest point
    lies on (chosen by ``part``; Baerentzen and Aanaes 2005): exact on a closed, consistently oriented manifold mesh,
    undefined near the edges and faces ``tree.sign_info()`` counts otherwise.  The table behind it is built on
    first use from ``tree.faces``; a handle that keeps no faces (one unpacked from a blob) needs
    ``tree.sign_build(f)`` first."""
    tree = _tree(tree, "aabbtree_signed_distance")
    if not isinstance(q, np.ndarray):
        raise TypeError("aabbtree_signed_distance() argument 2 must be numpy.ndarray")
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("Input must be Nx3")
    if tree.kind != "triangles":
        raise TypeError("aabbtree_signed_distance: handle is not a triangle tree")
    q = np.ascontiguousarray(q, dtype=np.float64)
    if tree.sign_info()["state"] != "built":
        if tree.faces is None:
            raise ValueError("aabbtree_signed_distance: the tree has no sign table and keeps no face array: "
                             "call tree.sign_build(f) with the faces it was built with")
        tree.sign_build()
    S = q.shape[0]
    sdist, face, part, pt = N.empty_results(((S,), np.float64), ((S,), np.uint32), ((S,), np.uint32),
                                            ((S, 3), np.float64))
    N.check(N.lib().msh_tree_signed_distance(tree.ptr, N.dptr(q), S, N.dptr(sdist), N.uptr(face), N.uptr(part),
                                             N.dptr(pt)))
    return sdist, face, part, pt


def aabbtree_winding_number(tree, q, beta=None):
    """w (S,) float64: the generalised winding number of every row of ``q`` about the tree's triangles -- 1 inside an
    outward-oriented closed mesh, 0 outside, fractional near openings; a row is inside iff ``w > 0.5``; NaN on
    non-finite rows (no reference counterpart).

    It needs no closed or manifold mesh (scans with holes, open templates, soups).  ``beta`` is the accuracy of the
    far-field approximation (Barill et al. 2018): a subtree farther than ``beta`` times its radius contributes its
    dipole; larger is more accurate and slower, 0 is exact (every triangle evaluated), ``None`` the library default
    (error <= 1e-2).  A row exactly on the surface gets a finite, otherwise unspecified value.  The table behind it
    is built on first use from the tree itself."""
    tree = _tree(tree, "aabbtree_winding_number")
    if not isinstance(q, np.ndarray):
        raise TypeError("aabbtree_winding_number() argument 2 must be numpy.ndarray")
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("Input must be Nx3")
    if tree.kind != "triangles":
        raise TypeError("aabbtree_winding_number: handle is not a triangle tree")
    beta = N.WINDING_BETA_DEFAULT if beta is None else float(beta)
    q = np.ascontiguousarray(q, dtype=np.float64)
    S = q.shape[0]
    w, = N.empty_results(((S,), np.float64))
    N.check(N.lib().msh_tree_winding_number(tree.ptr, N.dptr(q), S, beta, N.dptr(w)))
    return w


def aabbtree_nearest_k(tree, q, k, max_distance=np.inf):
    """(face (S,k) uint32, part (S,k) uint32, point (S,k,3) float64, dist (S,k) float64): for every row of ``q`` the
    at most ``k`` faces within ``max_distance`` of it, nearest first (no reference counterpart).

    The order is ascending by (squared distance, face id) with the exact squared distance ``aabbtree_nearest``
    computes, so ties are decided by the face id, column 0 of an uncapped answer is ``aabbtree_nearest``'s, and a
    smaller ``k`` gives a prefix of a larger one.  A row with fewer than ``k`` faces in range (or a non-finite row) is
    padded with face 0xFFFFFFFF, part 0, a NaN point and distance inf.  ``1 <= k <= 64``; ``max_distance = 0`` keeps
    exact hits only.  The extra faces of a tree built with them are included."""
    tree = _tree(tree, "aabbtree_nearest_k")
    if not isinstance(q, np.ndarray):
        raise TypeError("aabbtree_nearest_k() argument 2 must be numpy.ndarray")
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("Input must be Nx3")
    if tree.kind != "triangles":
        raise TypeError("aabbtree_nearest_k: handle is not a triangle tree")
    k, r = N.check_knearest(k, max_distance, "aabbtree_nearest_k")
    q = np.ascontiguousarray(q, dtype=np.float64)
    S = q.shape[0]
    face, part, pt, dist = N.empty_results(((S, k), np.uint32), ((S, k), np.uint32), ((S, k, 3), np.float64),
                                           ((S, k), np.float64))
    N.check(N.lib().msh_tree_knearest(tree.ptr, N.dptr(q), S, k, r, N.uptr(face), N.dptr(dist), N.dptr(pt),
                                      N.uptr(part), None))
    return face, part, pt, dist


def points_nearest_k(tree, q, k, max_distance=np.inf):
    """(idx (S,k) uint32, dist (S,k) float64, count (S,) uint32): for every row of ``q`` the at most ``k`` points of a
    point tree (``_native.build_points``) within ``max_distance`` of it, ascending by (squared distance, point index);
    ranks past ``count`` hold 0xFFFFFFFF and inf.  ``search.ClosestPointTree.query`` is its scipy-shaped form."""
    if not isinstance(tree, N.Handle) or tree.ptr is None:
        raise TypeError("points_nearest_k: expected a point tree handle")
    if not isinstance(q, np.ndarray):
        raise TypeError("points_nearest_k() argument 2 must be numpy.ndarray")
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("Input must be Nx3")
    if tree.kind != "points":
        raise TypeError("points_nearest_k: handle is not a point tree")
    k, r = N.check_knearest(k, max_distance, "points_nearest_k")
    q = np.ascontiguousarray(q, dtype=np.float64)
    S = q.shape[0]
    idx, dist, count = N.empty_results(((S, k), np.uint32), ((S, k), np.float64), ((S,), np.uint32))
    N.check(N.lib().msh_points_knearest(tree.ptr, N.dptr(q), S, k, r, N.uptr(idx), N.dptr(dist), N.uptr(count)))
    return idx, dist, count


def _within_args(tree, q, r, fn, kind):
    """The validated arguments of a radius query: (q (S,3) float64 C order, r_max, r_rows or None)."""
    if not isinstance(tree, N.Handle) or tree.ptr is None:
        raise TypeError("%s: expected a tree handle" % fn)
    if not isinstance(q, np.ndarray):
        raise TypeError("%s() argument 2 must be numpy.ndarray" % fn)
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("Input must be Nx3")
    if tree.kind != kind:
        raise TypeError("%s: handle is not a %s tree" % (fn, "point" if kind == "points" else "triangle"))
    r_max, r_rows = N.check_within(r, q.shape[0], fn)
    return np.ascontiguousarray(q, dtype=np.float64), r_max, r_rows


def _within_call(S, specs, call):
    """The list form of a radius query: one call with a first guess at the capacity, a second with cap = K only when
    K > cap (as ``_pairs_call``) -> (counts (S,) uint32, the owned (K, ...) arrays of ``specs``; None where a spec is
    None).  ``call(counts, out, cap, K)`` returns the status."""
    counts = np.empty(S, dtype=np.uint32)
    K = N._sz(0)

    def run(cap):
        out = [None if sp is None else np.empty((cap,) + sp[0], dtype=sp[1]) for sp in specs]
        N.check(call(counts, out, cap, K))
        return out

    cap = _first_cap(S)
    out = run(cap)
    if K.value > cap:
        out = run(K.value)
    return (counts,) + tuple(x[:K.value].copy() for x in out if x is not None)


def points_within_count(tree, q, r):
    """counts (S,) uint32: how many points of a point tree lie within ``r`` of every row of ``q`` (``d2 <= r * r`` with
    the exact squared distance of ``points_nearest_k``).  ``r`` is a scalar (negative or NaN: ValueError) or an (S,)
    array (a negative or NaN entry, like a non-finite row, counts 0)."""
    q, r_max, r_rows = _within_args(tree, q, r, "points_within_count", "points")
    S = q.shape[0]
    counts, = N.empty_results(((S,), np.uint32))
    N.check(N.lib().msh_points_within_count(tree.ptr, N.dptr(q), S, r_max, N.dptr(r_rows), N.uptr(counts)))
    return counts


def points_within(tree, q, r):
    """(counts (S,) uint32, idx (K,) uint32, dist (K,) float64): every point of a point tree within ``r`` of every row
    of ``q``, as CSR -- the exclusive scan of ``counts`` indexes the lists -- sorted by (row, squared distance, point
    index).  No row is truncated: the first ``k`` entries of a row are ``points_nearest_k(tree, q, k, r)``'s, bit for
    bit.  ``r`` as for ``points_within_count``; ``r = inf`` lists every point.
    ``search.ClosestPointTree.query_ball_point`` is its scipy-shaped form."""
    q, r_max, r_rows = _within_args(tree, q, r, "points_within", "points")
    S = q.shape[0]
    fn = N.lib().msh_points_within
    return _within_call(S, [((), np.uint32), ((), np.float64)],
                        lambda counts, out, cap, K: fn(tree.ptr, N.dptr(q), S, r_max, N.dptr(r_rows), N.uptr(counts),
                                                       N.uptr(out[0]), N.dptr(out[1]), cap, N.ctypes.byref(K)))


def aabbtree_within_count(tree, q, r):
    """counts (S,) uint32: how many faces lie within ``r`` of every row of ``q`` (``d2 <= r * r`` with the exact squared
    distance ``aabbtree_nearest`` computes; the extra faces of a tree built with them are included).  ``r`` is a scalar
    (negative or NaN: ValueError) or an (S,) array (a negative or NaN entry, like a non-finite row, counts 0)."""
    q, r_max, r_rows = _within_args(tree, q, r, "aabbtree_within_count", "triangles")
    S = q.shape[0]
    counts, = N.empty_results(((S,), np.uint32))
    N.check(N.lib().msh_tree_within_count(tree.ptr, N.dptr(q), S, r_max, N.dptr(r_rows), N.uptr(counts)))
    return counts


def aabbtree_within(tree, q, r, points=False, parts=False):
    """(counts (S,) uint32, face (K,) uint32, dist (K,) float64[, point (K,3) float64][, part (K,) uint32]): every face
    within ``r`` of every row of ``q``, as CSR -- the exclusive scan of ``counts`` indexes the lists -- sorted by (row,
    squared distance, face id) (no reference counterpart).  No row is truncated: the first ``k`` entries of a row are
    ``aabbtree_nearest_k(tree, q, k, r)``'s face, dist, point and part, bit for bit, and with ``r = inf`` entry 0 is
    ``aabbtree_nearest``'s.  ``r`` as for ``aabbtree_within_count``."""
    q, r_max, r_rows = _within_args(tree, q, r, "aabbtree_within", "triangles")
    S = q.shape[0]
    fn = N.lib().msh_tree_within
    specs = [((), np.uint32), ((), np.float64), ((3,), np.float64) if points else None,
             ((), np.uint32) if parts else None]
    return _within_call(S, specs,
                        lambda counts, out, cap, K: fn(tree.ptr, N.dptr(q), S, r_max, N.dptr(r_rows), N.uptr(counts),
                                                       N.uptr(out[0]), N.dptr(out[1]), N.dptr(out[2]), N.uptr(out[3]),
                                                       cap, N.ctypes.byref(K)))


def aabbtree_nearest_barycentric(tree, q):
    """(face (S,) uint32, point (S,3) float64, weights (S,3) float64) of the closest point.

    One launch replaces ``aabbtree_nearest`` followed by ``Mesh.barycentric_coordinates_for_points``
    (mesh.py:218-222; Heidrich's projection, geometry/barycentric_coordinates_of_projection.py:9-49), the
    pair landmarks.py:58-63 calls: the weights are computed in the traversal kernel from the winning
    triangle and refer to its vertices ``f[face]``.
    """
    tree = _tree(tree, "aabbtree_nearest_barycentric")
    if not isinstance(q, np.ndarray):
        raise TypeError("aabbtree_nearest_barycentric() argument 2 must be numpy.ndarray")
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("Input must be Nx3")
    if tree.kind != "triangles":
        raise TypeError("aabbtree_nearest_barycentric: handle is not a triangle tree")
    q = np.ascontiguousarray(q, dtype=np.float64)
    S = q.shape[0]
    face, pt, w = N.empty_results(((S,), np.uint32), ((S, 3), np.float64), ((S, 3), np.float64))
    N.check(N.lib().msh_tree_nearest_bary(tree.ptr, N.dptr(q), S, N.uptr(face), N.dptr(pt), N.dptr(w)))
    return face, pt, w


def aabbtree_nearest_alongnormal(tree, p, n):
    """(dist (S,) float64, face (S,) uint32, point (S,3) float64): spatialsearchmodule.cpp:222-323."""
    tree = _tree(tree, "aabbtree_nearest_alongnormal")
    if not isinstance(p, np.ndarray) or not isinstance(n, np.ndarray):
        raise TypeError("aabbtree_nearest_alongnormal() arguments must be numpy.ndarray")
    if p.ndim != 2 or n.ndim != 2 or p.shape[1] != 3 or n.shape[1] != 3 or p.shape[0] != n.shape[0]:
        raise ValueError("Points and normals must be Nx3")
    p = np.ascontiguousarray(p, dtype=np.float64)
    n = np.ascontiguousarray(n, dtype=np.float64)
    S = p.shape[0]
    dist, face, pt = N.empty_results(((S,), np.float64), ((S,), np.uint32), ((S, 3), np.float64))
    N.check(N.lib().msh_tree_nearest_alongnormal(tree.ptr, N.dptr(p), N.dptr(n), S, N.dptr(dist), N.uptr(face),
                                                  N.dptr(pt)))
    return dist, face, pt


def _ray_args(tree, o, d, t_range, fn):
    """The validated arguments of a ray query: (tree, origins (S,3), directions (S,3), range (S,2) or None)."""
    tree = _tree(tree, fn)
    if not isinstance(o, np.ndarray) or not isinstance(d, np.ndarray):
        raise TypeError("%s() arguments must be numpy.ndarray" % fn)
    if o.ndim != 2 or d.ndim != 2 or o.shape[1] != 3 or d.shape[1] != 3 or o.shape[0] != d.shape[0]:
        raise ValueError("Origins and directions must be Nx3")
    if tree.kind != "triangles":
        raise TypeError("%s: handle is not a triangle tree" % fn)
    S = o.shape[0]
    rng = None
    if t_range is not None:
        r = np.asarray(t_range, dtype=np.float64)
        if r.shape == (2,):
            # a pair of scalars for every row: a range no ray can have is the caller's mistake
            if not r[0] <= r[1]:
                raise ValueError("%s: t_range must be (t0, t1) with t0 <= t1 (not NaN), got %r" % (fn, t_range))
            rng = np.empty((S, 2), dtype=np.float64)
            rng[:] = r
        elif r.shape == (S, 2):
            rng = np.ascontiguousarray(r)  # per-row ranges: a NaN or t0 > t1 makes that row a miss
        else:
            raise ValueError("%s: t_range must be None, a pair (t0, t1) or an Nx2 array" % fn)
    return tree, np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64), rng


def aabbtree_raycast(tree, origins, directions, t_range=None, barycentric=False):
    """(t (S,) float64, face (S,) uint32, point (S,3) float64), and with ``barycentric`` the weights (S,3) float64 of
    the point in ``f[face]``: the first hit of every ray ``origins[i] + t directions[i]`` with ``t`` in the closed
    range ``t_range`` (no reference counterpart).

    A direction may have any non-zero length and is used as given.  ``t_range`` is None for ``[0, inf]``, a pair
    ``(t0, t1)`` for every row, or an (S,2) array; ``t0 < 0`` is taken as 0.  The hit is the lexicographic minimum of
    (t, face id) over the faces the ray meets (closed ray, closed triangles; a ray lying in a face's plane enters it at
    the lower end of their overlap), with the predicate and the point construction of
    ``aabbtree_nearest_alongnormal``.  A miss gives ``t = inf``, face 0xFFFFFFFF and NaN point and weights; so does a
    row that cannot be cast (non-finite values, a zero direction, a NaN range or ``t0 > t1`` in an array row).  The
    extra faces of a tree built with them are included, with ids after the main faces."""
    tree, o, d, rng = _ray_args(tree, origins, directions, t_range, "aabbtree_raycast")
    S = o.shape[0]
    specs = [((S,), np.float64), ((S,), np.uint32), ((S, 3), np.float64)]
    if barycentric:
        specs.append(((S, 3), np.float64))
    out = N.empty_results(*specs)
    N.check(N.lib().msh_tree_raycast(tree.ptr, N.dptr(o), N.dptr(d), N.dptr(rng), S, N.dptr(out[0]), N.uptr(out[1]),
                                     N.dptr(out[2]), N.dptr(out[3]) if barycentric else None))
    return tuple(out)


def aabbtree_occluded(tree, origins, directions, t_range=None):
    """bool (S,): whether the ray ``origins[i] + t directions[i]``, ``t`` in ``t_range``, meets any face (the hit set
    of ``aabbtree_raycast``; the search stops at the first hit it finds).  With ``directions = b - a`` and
    ``t_range = (0, 1)`` it tells whether the segment a -> b is blocked."""
    tree, o, d, rng = _ray_args(tree, origins, directions, t_range, "aabbtree_occluded")
    S = o.shape[0]
    hit, = N.empty_results(((S,), np.uint8))
    N.check(N.lib().msh_tree_occluded(tree.ptr, N.dptr(o), N.dptr(d), N.dptr(rng), S,
                                      hit.ctypes.data_as(N.ctypes.POINTER(N.ctypes.c_uint8))))
    return hit.astype(bool)


def aabbtree_raycast_count(tree, origins, directions, t_range=None):
    """counts (S,) uint32: how many faces each ray ``origins[i] + t directions[i]``, ``t`` in ``t_range``, meets -- the
    size of the hit set of ``aabbtree_raycast`` (no reference counterpart).  ``counts > 0`` is ``aabbtree_occluded``."""
    tree, o, d, rng = _ray_args(tree, origins, directions, t_range, "aabbtree_raycast_count")
    S = o.shape[0]
    counts, = N.empty_results(((S,), np.uint32))
    N.check(N.lib().msh_tree_raycast_count(tree.ptr, N.dptr(o), N.dptr(d), N.dptr(rng), S, N.uptr(counts)))
    return counts


def aabbtree_raycast_all(tree, origins, directions, t_range=None, points=False, sides=False):
    """(counts (S,) uint32, t (K,) float64, face (K,) uint32[, point (K,3) float64][, side (K,) int8]): every hit of
    every ray, as CSR -- the exclusive scan of ``counts`` indexes the lists (no reference counterpart).

    Rays, ranges and the hit set are ``aabbtree_raycast``'s.  The list is sorted by (row, t, face id): ``t`` is
    compared by value and equal ``t`` (shared edges and vertices, duplicated faces) goes to the smaller face id, so
    the first entry of every non-empty row is ``aabbtree_raycast``'s answer bit for bit.  ``point`` is that function's
    construction; ``side`` is +1 where the ray meets the front of the face (against the normal of ``f[face]``), -1
    where it meets the back, 0 for a ray lying in the face's plane.  A row that cannot be cast has no hits."""
    tree, o, d, rng = _ray_args(tree, origins, directions, t_range, "aabbtree_raycast_all")
    S = o.shape[0]
    fn = N.lib().msh_tree_raycast_all
    i8p = N.ctypes.POINTER(N.ctypes.c_int8)
    counts = np.empty(S, dtype=np.uint32)
    K = N._sz(0)

    def call(cap):
        out = [np.empty(cap, dtype=np.float64), np.empty(cap, dtype=np.uint32),
               np.empty((cap, 3), dtype=np.float64) if points else None, np.empty(cap, dtype=np.int8) if sides else None]
        N.check(fn(tree.ptr, N.dptr(o), N.dptr(d), N.dptr(rng), S, N.uptr(counts), N.dptr(out[0]), N.uptr(out[1]),
                   N.dptr(out[2]), out[3].ctypes.data_as(i8p) if sides else None, cap, N.ctypes.byref(K)))
        return out

    # one call with a first guess at the capacity, a second with cap = K only when K > cap (as _pairs_call)
    cap = _first_cap(S)
    out = call(cap)
    if K.value > cap:
        out = call(K.value)
    return (counts,) + tuple(x[:K.value].copy() for x in out if x is not None)


def aabbtree_intersections_indices(tree, qv, qf):
    """Ascending indices of query faces intersecting the mesh: spatialsearchmodule.cpp:326-417."""
    tree = _tree(tree, "aabbtree_intersections_indices")
    if not isinstance(qv, np.ndarray) or not isinstance(qf, np.ndarray):
        raise TypeError("aabbtree_intersections_indices() arguments must be numpy.ndarray")
    if qv.dtype != np.float64 or qv.ndim != 2:
        raise ValueError("Query Vertices must be of type double, and 2 dimensional")
    if qf.dtype != np.uint32 or qf.ndim != 2:
        raise ValueError("Query Faces must be of type uint32, and 2 dimensional")
    if qv.shape[1] != 3 or qf.shape[1] != 3:
        raise ValueError("Input must be Nx3")
    qv = np.ascontiguousarray(qv)
    qf = np.ascontiguousarray(qf)
    out = np.empty(qf.shape[0], dtype=np.uint32)
    K = N._sz(0)
    N.check(N.lib().msh_tree_intersections(tree.ptr, N.dptr(qv), qv.shape[0], N.uptr(qf), qf.shape[0], N.uptr(out),
                                            N.ctypes.byref(K)), Mesh_IntersectionsError)
    return out[:K.value].copy()


def _pairs_tree(tree, fn, kinds):
    if not isinstance(tree, N.Handle) or tree.ptr is None:
        raise TypeError("%s: expected a tree handle" % fn)
    if tree.kind not in kinds:
        raise ValueError("%s: handle is a %s tree (needs: %s)" % (fn, tree.kind, " or ".join(kinds)))
    return tree


def _first_cap(rows):
    """First guess at the pair capacity of a pair-list call; a second call is made only when K exceeds it."""
    return max(4 * rows, 4096)


def _pairs_call(rows, return_counts, call, exc_value=ValueError):
    """One call with a first guess at the capacity, a second with cap = K only when K > cap -> an owned (K, 2) uint32
    array (and the (rows,) uint32 counts).  ``call(pairs, cap, counts, K)`` returns the status."""
    counts = np.empty(rows, dtype=np.uint32) if return_counts else None
    cap = _first_cap(rows)
    K = N._sz(0)
    pairs = np.empty((cap, 2), dtype=np.uint32)
    N.check(call(pairs, cap, counts, K), exc_value)
    if K.value > cap:
        cap = K.value
        pairs = np.empty((cap, 2), dtype=np.uint32)
        N.check(call(pairs, cap, counts, K), exc_value)
    out = pairs[:K.value].copy()
    return (out, counts) if return_counts else out


def aabbtree_intersections_pairs(tree, qv, qf, return_counts=False):
    """All pairs (i, j) of a query face i of ``qv[qf]`` and a mesh face j that intersect: (K, 2) uint32 sorted by
    (i, j), and with ``return_counts`` the (Tq,) uint32 number of pairs of every query face (its exclusive scan
    indexes the pairs as CSR).  The predicate is ``aabbtree_intersections_indices``'s (closed: touching counts), so
    ``np.unique(pairs[:, 0])`` is that function's answer.  On a tree built with extra faces j also ranges over them
    (ids after the main faces).  No reference counterpart."""
    tree = _pairs_tree(tree, "aabbtree_intersections_pairs", ("triangles",))
    if not isinstance(qv, np.ndarray) or not isinstance(qf, np.ndarray):
        raise TypeError("aabbtree_intersections_pairs() arguments must be numpy.ndarray")
    if qv.dtype != np.float64 or qv.ndim != 2:
        raise ValueError("Query Vertices must be of type double, and 2 dimensional")
    if qf.dtype != np.uint32 or qf.ndim != 2:
        raise ValueError("Query Faces must be of type uint32, and 2 dimensional")
    if qv.shape[1] != 3 or qf.shape[1] != 3:
        raise ValueError("Input must be Nx3")
    qv = np.ascontiguousarray(qv)
    qf = np.ascontiguousarray(qf)
    fn = N.lib().msh_tree_intersection_pairs
    return _pairs_call(qf.shape[0], return_counts,
                       lambda pairs, cap, counts, K: fn(tree.ptr, N.dptr(qv), qv.shape[0], N.uptr(qf), qf.shape[0],
                                                        N.uptr(pairs), cap, N.uptr(counts), N.ctypes.byref(K)),
                       Mesh_IntersectionsError)


def _self_pairs(tree, return_counts):
    rows = int(tree.info().n_faces)
    fn = N.lib().msh_tree_self_intersection_pairs
    return _pairs_call(rows, return_counts,
                       lambda pairs, cap, counts, K: fn(tree.ptr, N.uptr(pairs), cap, N.uptr(counts),
                                                        N.ctypes.byref(K)))


def aabbtree_selfintersections_pairs(tree, return_counts=False):
    """All pairs (i, j), i < j, of faces of the tree's mesh that intersect and share no exactly equal vertex
    coordinate (the rule of ``aabb_normals.aabbtree_n_selfintersects``): (K, 2) uint32 sorted by (i, j), and with
    ``return_counts`` the (T,) uint32 number of pairs whose smaller face is each face.  No reference counterpart."""
    tree = _pairs_tree(tree, "aabbtree_selfintersections_pairs", ("triangles",))
    return _self_pairs(tree, return_counts)
