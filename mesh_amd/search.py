"""Drop-in for ``psbody.mesh.search`` (mesh/search.py): same class names, constructor and method
signatures, and return shapes/dtypes; the bodies are delegations to this package's GPU modules.

``AabbTree`` / ``AabbNormalsTree`` / ``CGALClosestPointTree`` apply the same input coercions as the
reference (search.py:24,29,35-36,76,95).  ``ClosestPointTree`` answers all queries with one GPU launch
over a point LBVH instead of the reference's per-query scipy KDTree loop (search.py:59-61); the nearest
vertex is the lexicographic minimum of (distance, vertex index).
"""
import numpy as np

from . import _native as N

__all__ = ['AabbTree', 'AabbNormalsTree', 'ClosestPointTree', 'CGALClosestPointTree', 'AabbTreeBatch']


def _f64c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _u32c(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


class AabbTree(object):
    """Closest-point / ray / intersection search over the triangles of ``m`` (search.py:19-49).

    Built once on the GPU (LBVH); the handle lives in ``cpp_handle`` as in the reference.
    """

    def __init__(self, m):
        from . import spatialsearch
        self.cpp_handle = spatialsearch.aabbtree_compute(_f64c(m.v).copy(), _u32c(m.f).copy())

    def nearest(self, v_samples, nearest_part=False):
        """Closest face (1,S) u32 and point (S,3) f64 for each sample.

        With ``nearest_part=True`` a third array (1,S) u32 is returned between them that classifies
        where the point lies on its triangle (a,b,c): 0 inside, 1/2/3 on edge ab/bc/ca, 4/5/6 at
        vertex a/b/c.
        """
        from . import spatialsearch
        faces, parts, pts = spatialsearch.aabbtree_nearest(self.cpp_handle, _f64c(v_samples))
        if nearest_part:
            return faces, parts, pts
        return faces, pts

    def nearest_k(self, v_samples, k, max_distance=np.inf, nearest_part=False):
        """The at most ``k`` faces within ``max_distance`` of each sample, nearest first: (faces (S,k) u32,
        points (S,k,3) f64, distances (S,k) f64), with ``nearest_part=True`` (faces, parts (S,k) u32, points,
        distances).  Ascending by (squared distance, face id), so ties go to the smaller face id, column 0 of an
        uncapped answer is ``nearest``'s, and a smaller ``k`` gives a prefix.  Ranks past the faces in range (and
        non-finite samples) hold face 0xFFFFFFFF, part 0, a NaN point and distance inf.  ``1 <= k <= 64``."""
        from . import spatialsearch
        faces, parts, pts, dist = spatialsearch.aabbtree_nearest_k(self.cpp_handle, _f64c(v_samples), k, max_distance)
        if nearest_part:
            return faces, parts, pts, dist
        return faces, pts, dist

    def within(self, v_samples, r, points=False, parts=False):
        """Every face within ``r`` of each sample, as CSR: (counts (S,) u32, faces (K,) u32, distances (K,) f64), with
        ``points=True`` also the closest points (K,3) f64 and with ``parts=True`` their part codes (K,) u32.  The
        exclusive scan of ``counts`` indexes the lists; a row's faces are sorted by (squared distance, face id), so its
        first ``k`` entries are ``nearest_k``'s and no row is truncated.  ``r`` is a scalar or (S,); ``r = inf`` lists
        every face."""
        from . import spatialsearch
        return spatialsearch.aabbtree_within(self.cpp_handle, _f64c(v_samples), r, points, parts)

    def count_within(self, v_samples, r):
        """uint32 (S,): how many faces lie within ``r`` (a scalar or (S,)) of each sample (see ``within``)."""
        from . import spatialsearch
        return spatialsearch.aabbtree_within_count(self.cpp_handle, _f64c(v_samples), r)

    def nearest_alongnormal(self, points, normals):
        """Nearest hit of the lines through ``points`` along +/-``normals``: (dist, face, point)."""
        from . import spatialsearch
        return spatialsearch.aabbtree_nearest_alongnormal(self.cpp_handle, points.astype(np.float64),
                                                          normals.astype(np.float64))

    def nearest_barycentric(self, v_samples):
        """(face (S,) u32, point (S,3) f64, barycentric weights (S,3) f64) of the closest point.

        Fused replacement of ``nearest`` followed by ``Mesh.barycentric_coordinates_for_points``
        (mesh.py:218-222, Heidrich projection, geometry/barycentric_coordinates_of_projection.py:9-49);
        the weights are computed in the traversal kernel from the winning triangle.
        """
        from . import spatialsearch
        return spatialsearch.aabbtree_nearest_barycentric(self.cpp_handle, _f64c(v_samples))

    def ray_cast(self, origins, directions, t_range=None, barycentric=False):
        """First hit of every ray ``origins[i] + t directions[i]``, ``t`` in the closed range ``t_range`` (None:
        ``[0, inf]``; a pair for every row; or (S,2)): (t (S,) f64, face (S,) u32, point (S,3) f64), with
        ``barycentric=True`` also the weights (S,3) of the point in ``f[face]``.  Directions need not be unit vectors.
        The smallest (t, face id) wins; a miss gives t = inf, face 0xFFFFFFFF and NaN point and weights."""
        from . import spatialsearch
        return spatialsearch.aabbtree_raycast(self.cpp_handle, _f64c(origins), _f64c(directions), t_range, barycentric)

    def occluded(self, origins, directions, t_range=None):
        """bool (S,): whether each ray meets any face within ``t_range`` (see ``ray_cast``)."""
        from . import spatialsearch
        return spatialsearch.aabbtree_occluded(self.cpp_handle, _f64c(origins), _f64c(directions), t_range)

    def ray_count(self, origins, directions, t_range=None):
        """uint32 (S,): how many faces each ray meets within ``t_range`` (see ``ray_cast``)."""
        from . import spatialsearch
        return spatialsearch.aabbtree_raycast_count(self.cpp_handle, _f64c(origins), _f64c(directions), t_range)

    def ray_cast_all(self, origins, directions, t_range=None, points=False, sides=False):
        """Every hit of every ray, as CSR: (counts (S,) u32, t (K,) f64, face (K,) u32), with ``points=True`` also the
        hit points (K,3) and with ``sides=True`` the side (K,) i8 each face is met from (+1 front, -1 back, 0 in its
        plane).  The exclusive scan of ``counts`` indexes the lists; a row's hits are sorted by (t, face id), so its
        first entry is ``ray_cast``'s answer."""
        from . import spatialsearch
        return spatialsearch.aabbtree_raycast_all(self.cpp_handle, _f64c(origins), _f64c(directions), t_range, points,
                                                  sides)

    def line_of_sight(self, a, b, margin=0.0):
        """bool (S,): True where the segment ``a[i] -> b[i]`` meets no face between its parameters ``margin`` and
        ``1 - margin`` (0 at ``a``, 1 at ``b``); a positive margin keeps end points that lie on the surface from
        blocking their own segment."""
        from . import spatialsearch
        a, b = _f64c(a), _f64c(b)
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != 3 or a.shape != b.shape:
            raise ValueError("line_of_sight: a and b must both be Nx3")
        margin = float(margin)
        if not 0.0 <= margin <= 0.5:
            raise ValueError("line_of_sight: margin must be in [0, 0.5], got %r" % (margin,))
        return ~spatialsearch.aabbtree_occluded(self.cpp_handle, a, b - a, (margin, 1.0 - margin))

    def orientation_info(self):
        """Topology counters of the mesh as the sign table sees it (built on first use): a dict with
        ``boundary_edges``, ``nonmanifold_edges``, ``inconsistent_edges`` and ``degenerate_faces``.  All zero:
        the mesh is a closed, consistently oriented manifold and ``signed_distance`` is exact."""
        h = self.cpp_handle
        info = h.sign_info()
        if info["state"] != "built":
            info = h.sign_build()
        return dict((k, info[k]) for k in ("boundary_edges", "nonmanifold_edges", "inconsistent_edges",
                                           "degenerate_faces"))

    def winding_number(self, v_samples, beta=None):
        """w (S,) f64: the generalised winding number of each sample -- 1 inside an outward-oriented closed mesh,
        0 outside, fractional near openings; inside iff ``w > 0.5``.  Defined on open meshes and soups too.
        ``beta``: accuracy of the far-field approximation (0 exact, larger more accurate; ``None`` the library
        default, error <= 1e-2)."""
        from . import spatialsearch
        return spatialsearch.aabbtree_winding_number(self.cpp_handle, _f64c(v_samples), beta)

    def signed_distance(self, v_samples, check=True, sign="pseudonormal"):
        """(sdist (S,) f64, face (S,) u32, point (S,3) f64): the closest face and point of ``nearest`` and the
        signed distance to it, negative inside an outward-oriented mesh (angle-weighted pseudonormal test).

        With ``check=True`` a mesh that is not a closed, consistently oriented manifold raises ValueError naming
        the counts of ``orientation_info``.  With ``check=False`` the query runs anyway: a boundary or non-manifold
        edge uses its own face's normal, an inconsistent edge the sum of both, a degenerate face a zero normal,
        and the sign is undefined near those features.

        ``sign="winding"`` takes the sign from the generalised winding number instead (negative where
        ``winding_number > 0.5``): no orientation check is made and ``check`` is ignored, so open meshes and soups
        are answered.  Magnitude, face and point are ``nearest``'s; rows at distance 0 stay +0.0, non-finite rows
        NaN."""
        from . import spatialsearch
        if sign == "winding":
            q = _f64c(v_samples)
            face, pt = self.nearest(q)
            face = face.reshape(-1)
            d = q.reshape(-1, 3) - pt
            # the sign pass's magnitude, operation for operation (msh_tree_signed_distance)
            sdist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            sdist[face == N.NO_FACE] = np.nan
            inside = (self.winding_number(q) > 0.5) & (sdist > 0)
            sdist[inside] = -sdist[inside]
            return sdist, face, pt
        if sign != "pseudonormal":
            raise ValueError("signed_distance: sign must be 'pseudonormal' or 'winding', got %r" % (sign,))
        if check:
            bad = dict((k, n) for k, n in self.orientation_info().items() if n)
            if bad:
                raise ValueError("mesh is not a closed, consistently oriented manifold: %s" %
                                 ", ".join("%d %s" % (n, k.replace("_", " ")) for k, n in sorted(bad.items())))
        sdist, face, _, pt = spatialsearch.aabbtree_signed_distance(self.cpp_handle, _f64c(v_samples))
        return sdist, face, pt

    def contains(self, v_samples, check=True, method="pseudonormal"):
        """bool (S,): whether each sample lies inside the mesh (``signed_distance < 0``; points on the surface
        and non-finite rows are not inside).  ``method="winding"``: ``winding_number > 0.5`` instead -- no
        orientation check (``check`` is ignored), defined on open meshes and soups."""
        if method == "winding":
            return self.winding_number(v_samples) > 0.5
        if method != "pseudonormal":
            raise ValueError("contains: method must be 'pseudonormal' or 'winding', got %r" % (method,))
        return self.signed_distance(v_samples, check)[0] < 0

    def intersections_indices(self, q_v, q_f):
        """Indices (ascending, u32) of the query triangles ``q_v[q_f]`` that touch the mesh.

        The reference method cannot run (its module function is unregistered and imported by an
        absolute name, search.py:46); this one is wired to the GPU triangle-triangle kernel.
        """
        from . import spatialsearch
        return spatialsearch.aabbtree_intersections_indices(self.cpp_handle, _f64c(q_v), _u32c(q_f))

    def intersections_pairs(self, q_v, q_f):
        """All (query face, mesh face) pairs of the query triangles ``q_v[q_f]`` and the mesh that touch: (K, 2) u32
        sorted by (query face, mesh face); ``intersections_indices`` is its distinct first column."""
        from . import spatialsearch
        return spatialsearch.aabbtree_intersections_pairs(self.cpp_handle, _f64c(q_v), _u32c(q_f))

    def selfintersections_pairs(self):
        """All pairs (i, j), i < j, of faces of the mesh that intersect and share no exactly equal vertex coordinate:
        (K, 2) u32 sorted by (i, j)."""
        from . import spatialsearch
        return spatialsearch.aabbtree_selfintersections_pairs(self.cpp_handle)


class ClosestPointTree(object):
    """Nearest mesh vertex for query points; faces are ignored (search.py:52-65)."""

    def __init__(self, m):
        self.v = m.v
        self._h = N.build_points(_f64c(m.v))

    def _query(self, v_samples):
        q = _f64c(v_samples).reshape(-1, 3)
        S = q.shape[0]
        idx, dist = N.empty_results(((S,), np.uint32), ((S,), np.float64))
        N.check(N.lib().msh_points_nearest(self._h.ptr, N.dptr(q), S, N.uptr(idx), N.dptr(dist)))
        return idx.astype(np.intp), dist

    def query(self, v_samples, k=1, distance_upper_bound=np.inf):
        """``scipy.spatial.KDTree.query(x, k, distance_upper_bound=...)`` on the GPU: (distances, indices) of the
        ``k`` nearest vertices of each sample within the bound, nearest first, ties by vertex index.  Shapes as scipy's:
        (S,) for ``k == 1``, else (S, k); a single (3,) point gives () / (k,).  Indices are ``np.intp``; a missing
        neighbour has index ``n`` (the number of vertices) and distance inf.  ``1 <= k <= 64``."""
        from . import spatialsearch
        q = _f64c(v_samples)
        single = q.ndim == 1
        if single:
            q = q.reshape(1, -1)
        idx, dist, _ = spatialsearch.points_nearest_k(self._h, q, k, distance_upper_bound)
        ind = idx.astype(np.intp)
        ind[idx == N.NO_FACE] = np.asarray(self.v).shape[0]
        if int(k) == 1:
            dist, ind = dist[:, 0], ind[:, 0]
        if single:
            dist, ind = dist[0], ind[0]
        return dist, ind

    def within(self, x, r):
        """Every vertex within ``r`` of each sample, as CSR: (counts (S,) u32, indices (K,) intp, distances (K,) f64);
        the exclusive scan of ``counts`` indexes the lists, and a row's neighbours come nearest first, ties by vertex
        index.  ``r`` is a scalar or (S,).  No row is truncated: the first ``k`` entries of a row are ``query``'s."""
        from . import spatialsearch
        counts, idx, dist = spatialsearch.points_within(self._h, _f64c(x).reshape(-1, 3), r)
        return counts, idx.astype(np.intp), dist

    def query_ball_point(self, x, r, p=2.0, eps=0, workers=1, return_sorted=None, return_length=False):
        """``scipy.spatial.KDTree.query_ball_point(x, r, ...)`` on the GPU: the indices of all vertices within ``r`` of
        each sample (``d2 <= r * r`` with the exact squared distance of ``query``).  A single (3,) point gives a list
        of indices (or their number with ``return_length``); (..., 3) input gives an object array of lists (or an intp
        array of lengths) of the leading shape.  ``r`` is broadcast against the samples.  ``return_sorted`` True, or
        None on multi-point input, sorts each list ascending by index; False keeps the lists nearest first, ties by
        index.  Only the Euclidean metric without approximation is supported: ``p != 2`` or ``eps != 0`` raise
        ValueError; ``workers`` is accepted and ignored."""
        from . import spatialsearch
        if float(p) != 2.0:
            raise ValueError("query_ball_point: only p = 2 (the Euclidean metric) is supported, got %r" % (p,))
        if float(eps) != 0.0:
            raise ValueError("query_ball_point: only eps = 0 (no approximation) is supported, got %r" % (eps,))
        q = _f64c(x)
        if q.ndim < 1 or q.shape[-1] != 3:
            raise ValueError("query_ball_point: x must have shape (..., 3), got %r" % (q.shape,))
        lead = q.shape[:-1]
        q = q.reshape(-1, 3)
        S = q.shape[0]
        rr = np.asarray(r, dtype=np.float64)
        if rr.ndim:
            try:
                rr = np.ascontiguousarray(np.broadcast_to(rr, lead)).reshape(-1)
            except ValueError:
                raise ValueError("query_ball_point: r of shape %r does not broadcast against the %r samples" %
                                 (np.shape(r), lead))
        if return_length:
            n = spatialsearch.points_within_count(self._h, q, rr).astype(np.intp)
            return int(n[0]) if not lead else n.reshape(lead)
        counts, idx, _ = spatialsearch.points_within(self._h, q, rr)
        idx = idx.astype(np.intp)
        if return_sorted or (return_sorted is None and lead):
            # one segmented sort over the CSR: by row, then by index
            idx = idx[np.lexsort((idx, np.repeat(np.arange(S), counts)))]
        flat = idx.tolist()
        if not lead:
            return flat
        ends = np.cumsum(counts, dtype=np.int64).tolist()
        out = np.empty(S, dtype=object)
        a = 0
        for i, b in enumerate(ends):
            out[i] = flat[a:b]
            a = b
        return out.reshape(lead)

    def nearest(self, v_samples):
        # same container types as the reference's zip(*[...]) over per-sample KDTree queries
        idx, dist = self._query(v_samples)
        return (tuple(idx), tuple(dist))

    def nearest_vertices(self, v_samples):
        # row gather by vertex index (the reference's tuple indexing breaks for >= 3 samples,
        # SURVEY.md Appendix B)
        idx, _ = self._query(v_samples)
        return self.v[idx]


class CGALClosestPointTree(object):
    """Nearest vertex through the triangle tree (search.py:68-86).

    Every vertex becomes a tiny triangle (its three corners displaced by 1e-12 along +x, +y and
    -(x+y)), so the closest face index is the closest vertex index.
    """

    def __init__(self, m):
        from . import spatialsearch
        self.v = m.v
        n = m.v.shape[0]
        ids = np.arange(n)
        tri = np.stack([ids, ids + n, ids + 2 * n], axis=1)
        d = 1e-12
        corners = np.concatenate([m.v + [d, 0.0, 0.0], m.v + [0.0, d, 0.0], m.v - [d, d, 0.0]], axis=0)
        self.cpp_handle = spatialsearch.aabbtree_compute(_f64c(corners).copy(), _u32c(tri).copy())

    def _faces(self, v_samples):
        from . import spatialsearch
        faces, _, _ = spatialsearch.aabbtree_nearest(self.cpp_handle, _f64c(v_samples))
        return faces.flatten()

    def nearest(self, v_samples):
        fi = self._faces(v_samples)
        dist = np.sqrt(np.sum((self.v[fi] - v_samples) ** 2.0, axis=1)).flatten()
        return fi, dist

    def nearest_vertices(self, v_samples):
        return self.v[self._faces(v_samples)]


class AabbNormalsTree(object):
    """Closest face under the distance + normal-agreement metric (search.py:89-100).

    The reference fixes the normal weight eps at 0.1 (search.py:94); so does this class.
    """

    EPS = 0.1

    def __init__(self, m):
        from . import aabb_normals
        self.tree_handle = aabb_normals.aabbtree_n_compute(_f64c(m.v), _u32c(m.f).copy(), self.EPS)

    def nearest(self, v_samples, n_samples):
        from . import aabb_normals
        return aabb_normals.aabbtree_n_nearest(self.tree_handle, v_samples, n_samples)

    def selfintersections_pairs(self):
        """All pairs (i, j), i < j, of faces of the mesh that intersect and share no exactly equal vertex coordinate:
        (K, 2) u32 sorted by (i, j)."""
        from . import aabb_normals
        return aabb_normals.aabbtree_n_selfintersections_pairs(self.tree_handle)


class AabbTreeBatch(object):
    """Many meshes sharing one topology, searched together (scan-to-mesh registration, BASELINE C4).

    The reference answers this with one ``AabbTree`` per mesh (search.py:21-30); ``AabbTreeBatch(v, f)``
    builds all B trees in one batched GPU build and ``nearest(q)`` answers every mesh's queries in one
    launch.  ``nearest(q)[..., b]`` equals ``AabbTree(mesh_b).nearest(q[b])`` with mesh-local face
    indices; shapes gain a leading mesh axis: face (B,S) uint32, part (B,S) uint32, point (B,S,3).
    """

    def __init__(self, v, f):
        v = _f64c(v)
        f = _u32c(f)
        if v.ndim != 3 or v.shape[2] != 3:
            raise ValueError("Vertices must be BxPx3")
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("Faces must be Tx3")
        self.n_meshes = v.shape[0]
        self.cpp_handle = N.build_batch(v, f)

    def _q(self, v_samples):
        q = _f64c(v_samples)
        if q.ndim != 3 or q.shape[0] != self.n_meshes or q.shape[2] != 3:
            raise ValueError("Queries must be BxSx3 with B = %d" % self.n_meshes)
        return q

    def nearest(self, v_samples, nearest_part=False):
        q = self._q(v_samples)
        B, S = q.shape[0], q.shape[1]
        face, part, pt = N.empty_results(((B, S), np.uint32), ((B, S), np.uint32), ((B, S, 3), np.float64))
        N.check(N.lib().msh_batch_nearest(self.cpp_handle.ptr, N.dptr(q), S, N.uptr(face), N.uptr(part),
                                          N.dptr(pt)))
        return (face, part, pt) if nearest_part else (face, pt)

    def nearest_barycentric(self, v_samples):
        """(face (B,S) u32, point (B,S,3) f64, barycentric weights (B,S,3) f64) per mesh."""
        q = self._q(v_samples)
        B, S = q.shape[0], q.shape[1]
        face, pt, bary = N.empty_results(((B, S), np.uint32), ((B, S, 3), np.float64), ((B, S, 3), np.float64))
        N.check(N.lib().msh_batch_nearest_bary(self.cpp_handle.ptr, N.dptr(q), S, N.uptr(face), N.dptr(pt),
                                               N.dptr(bary)))
        return face, pt, bary
