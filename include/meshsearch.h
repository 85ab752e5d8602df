/*
 * meshsearch.h — C ABI of the MI355X-native point-to-mesh spatial search engine (libmeshsearch.so).
 *
 * Drop-in replacement for the three CPython extensions of psbody-mesh 0.4 that wrap CGAL 4.7's
 * AABB_tree (KanaLab/mesh: mesh/src/spatialsearchmodule.cpp, mesh/src/aabb_normals.cpp,
 * mesh/src/py_visibility.cpp) and for the scipy KDTree behind search.ClosestPointTree.  Every entry
 * point takes plain pointers and sizes; no Python, numpy or torch type crosses this boundary.
 * The Python shims in mesh_amd/ (spatialsearch.py, aabb_normals.py, visibility.py, search.py) bind
 * these functions with ctypes; INTEGRATION.md shows the binding a psbody-mesh maintainer would add.
 *
 * Conventions
 *  - Arrays are C-contiguous row-major: points/normals (N,3) double, faces (T,3) uint32.
 *  - Every function returns MSH_OK (0) or an error code; msh_last_error() gives the message of the
 *    last failure on the calling thread.  MSH_EINVAL maps to ValueError (bad shape / index),
 *    MSH_EDEVICE / MSH_ENOMEM to RuntimeError (HIP failure), as the reference raises
 *    (spatialsearchmodule.cpp:82-97 ValueError; cgal_error_emulation.hpp:19-33 RuntimeError).
 *  - Host-buffer entry points (no _device suffix) copy inputs to HBM, run the HIP kernels and copy
 *    results back; they are synchronous.  *_device entry points take HBM pointers and a hipStream_t
 *    (passed as void*, NULL = the handle's own stream, a blocking stream that orders with the legacy default
 *    stream — so NULL also serves a caller whose work is queued on the default stream) and are asynchronous
 *    on that stream.
 *  - A handle owns device copies of the mesh and its BVH (the reference's TreeAndTri owns host
 *    copies, nearest_triangle.hpp:28-32); input arrays are not retained.  Calls on one handle must be
 *    serialised by the caller (host threads); on the device, launches that share a handle's scratch
 *    are ordered with an event, whatever streams they are issued on.  Different handles are
 *    independent.
 *  - Query counts per call are limited to 2^32 - 1 (device slot indices are 32-bit).
 *  - There is no CPU fallback: without a usable gfx950 device every compute entry point fails with
 *    MSH_EDEVICE.
 */
#ifndef MESHSEARCH_H_
#define MESHSEARCH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSH_OK 0
#define MSH_EINVAL 1
#define MSH_EDEVICE 2
#define MSH_ENOMEM 3

#define MSH_NO_FACE 0xFFFFFFFFu

typedef struct msh_tree msh_tree;

typedef struct msh_tree_info {
    int device;          /* HIP device ordinal holding the tree */
    int kind;            /* 0 triangles (spatialsearch), 1 normals metric (aabb_normals), 2 points */
    uint64_t n_points;   /* P: vertices of the main mesh */
    uint64_t n_faces;    /* T: leaf primitives (main + extra mesh faces, or points) */
    uint64_t n_main_faces;
    uint64_t n_nodes;    /* internal LBVH nodes (T-1) */
    uint64_t bytes;      /* device bytes owned by the handle (mesh + BVH) */
    double eps;
    float scene_lo[3], scene_hi[3];
    double build_ms;     /* GPU time of the build (Morton + radix sort + emission + re-split + oriented boxes) */
    uint64_t n_meshes;   /* meshes in a batched tree (msh_batch_build), 1 otherwise */
    uint32_t node_bytes; /* bytes of one internal node as stored in HBM (one traversal step reads it) */
    uint32_t leaf_bytes; /* bytes of one leaf record (triangle: 9 x f64 + face id; point: 3 x f64 + id) */
    int32_t max_depth;   /* upper bound of the deepest leaf below the root (sizes traversal stacks) */
} msh_tree_info;

/* Layout of a packed tree blob (msh_tree_blob_*), readable on the host without a device. */
typedef struct msh_blob_info {
    int32_t kind, max_depth;
    uint64_t n_points, n_faces, n_main_faces;
    uint64_t off_vertices, off_nodes, off_leaves, total;
    uint32_t node_bytes, leaf_bytes;
    double origin[3];
} msh_blob_info;

/* ---- library / device ---- */
const char* msh_last_error(void);
int msh_version(void);
/* Identity of the built kernels: the first 16 hex digits of the SHA-256 of mesh_amd/csrc's sources (and any
 * extra compile flags).  Profiles are keyed by it, so a measurement is only ever paired with the code it
 * measured (bench.py roofline.traffic). */
const char* msh_build_id(void);
int msh_device_count(int* n);
/* Device used by subsequent builds on the calling thread (default: current HIP device).  It also drops the
 * thread's device list (msh_set_devices / msh_set_device_list): later trees are built on this device alone. */
int msh_set_device(int device);
/* In-process multi-device handles (SURVEY §8(b) msh_set_devices; the reference's drop-in call
 * Mesh.closest_faces_and_points -> AabbTree.nearest, mesh.py:454-455 / search.py:26-30, has no device argument).
 * Trees built afterwards on the calling thread are built on the first device and replicated to the others
 * (blob pack + peer copy + unpack); the host-buffer entry points (msh_tree_nearest, _nearest_bary, _signed_distance,
 * _nearest_alongnormal, _knearest, _raycast, _occluded, msh_ntree_nearest, msh_points_nearest, msh_points_knearest:
 * contiguous row ranges;
 * msh_visibility: camera ranges) then split their rows over the devices, one host thread and one chunk pipeline per device, so each
 * device's host link carries its share.  Calls below 32 MB of rows stay on the first device.  The answers equal
 * the one-device answers bit for bit (disjoint row ranges of the same arrays).  *_device entry points, batched
 * trees and the intersection tests stay on the handle's own device.  Untested across devices: the GPU box this
 * library is tested on has one device, so the peer copy and the per-device pipelines have run only as replicas on
 * one device, and the devices' pageable <-> pinned staging copies share one host copy pool (one job at a time).
 *   msh_set_devices(G): devices d, d + 1, ..., d + G - 1 from the current device d (G = 1: one device again);
 *   msh_set_device_list(devices, G): an explicit list (an entry may repeat: several replicas on one device);
 *   msh_tree_devices: the devices of a handle (G = 1 + replicas; devices may be NULL);
 *   msh_device_plan: the row split of S rows over G devices, begins[0..G] (host only, no device needed). */
int msh_set_devices(int G);
int msh_set_device_list(const int* devices, int G);
int msh_tree_devices(const msh_tree* tree, int* devices, int cap, int* G);
int msh_device_plan(uint64_t S, int G, uint64_t* begins);

/* ---- spatialsearch (spatialsearchmodule.cpp) ---- */
/* aabbtree_compute(v, f) -> capsule: spatialsearchmodule.cpp:74-127 (TreeAndTri build :108-123).
 * GPU LBVH build: Morton codes of triangle centroids, LDS radix sort, Karras emission, subtrees of <= 2^16
 * leaves re-split top down along the surface, and 64-B nodes holding both children's oriented boxes (exact fp64
 * extents rounded outward, quantised outward); no refit pass. */
int msh_tree_build(const double* v, size_t P, const uint32_t* f, size_t T, msh_tree** out);
/* visibility_compute(v=, f=, extra_v=, extra_f=) builds over main + extra triangles:
 * py_visibility.cpp:114-163.  extra may be NULL/0. */
int msh_tree_build_ex(const double* v, size_t P, const uint32_t* f, size_t T, const double* ev, size_t EP,
                      const uint32_t* ef, size_t ET, msh_tree** out);
/* capsule destructor: spatialsearchmodule.cpp:68-72 */
void msh_tree_free(msh_tree* tree);
int msh_tree_get_info(const msh_tree* tree, msh_tree_info* info);

/* aabbtree_nearest(tree, q) -> (face (1,S) u32, part (1,S) u32, point (S,3) f64):
 * spatialsearchmodule.cpp:165-220, per query nearest_one :129-140.  part may be NULL.
 * Closest face = lexicographic minimum of (squared distance, face index); point = CGAL's
 * construction for that face (project on plane, edge, vertex); part = iev::nearest_primitive code. */
int msh_tree_nearest(msh_tree* tree, const double* q, size_t S, uint32_t* face, uint32_t* part, double* pt);
int msh_tree_nearest_device(msh_tree* tree, const double* d_q, size_t S, uint32_t* d_face, uint32_t* d_part,
                            double* d_pt, void* stream);
/* Instrumented traversal (not timed, same two-pass traversal as msh_tree_nearest_device): total internal
 * nodes popped and leaf triangles tested over the S queries, for the algorithmic-bytes figure of the
 * roofline. */
int msh_tree_nearest_stats(msh_tree* tree, const double* d_q, size_t S, uint64_t* nodes, uint64_t* leaves);
/* nearest + barycentric weights of the closest point in its face (Heidrich's projection, the reference's
 * Mesh.barycentric_coordinates_for_points, mesh.py:218-222 / barycentric_coordinates_of_projection.py:9-49,
 * as called by landmarks.py:61-62): face (S,) u32, point (S,3) f64, w (S,3) f64 for vertices f[face]. */
int msh_tree_nearest_bary(msh_tree* tree, const double* q, size_t S, uint32_t* face, double* pt, double* w);
int msh_tree_nearest_bary_device(msh_tree* tree, const double* d_q, size_t S, uint32_t* d_face, double* d_pt,
                                 double* d_w, void* stream);

/* The closest point (and part code) of each row q[i] on a GIVEN face face[i] -- the construction msh_tree_nearest
 * stores for the face it finds (CGAL's closest point on the triangle, spatialsearchmodule.cpp:129-140 /
 * nearest_point_triangle_3.h:22-154), so for rows answered with face f it reproduces the answer's point and part bit
 * for bit.  face MSH_NO_FACE (or >= T): point NaN, part 0.  The narrow multi-GPU result exchange
 * (mesh_amd/distributed.py NarrowRing) all-gathers faces only (4 B per row instead of 32) and rebuilds the other
 * ranks' points with it.  Device pointers; asynchronous on `stream`; part may be NULL. */
int msh_tree_points_from_faces_device(msh_tree* tree, const double* d_q, size_t S, const uint32_t* d_face,
                                      uint32_t* d_part, double* d_pt, void* stream);

/* ---- signed distance / inside-outside (no reference counterpart) ----
 * The sign of the distance to a closed, consistently oriented manifold mesh by the angle-weighted pseudonormal test
 * (Baerentzen and Aanaes 2005): with p the closest point of q and N the pseudonormal of the feature p lies on -- chosen
 * by the part code the traversal returns: 0 the face normal, 1/2/3 the sum of the two unit face normals at edge
 * ab/bc/ca (the face's own on a boundary edge), 4/5/6 the sum over the faces around vertex a/b/c of (angle at the
 * vertex) x (unit face normal) -- q is inside iff (q - p) . N < 0.  No rays, no parity counting.
 *
 * msh_tree_sign_build derives the table on the GPU from the face array the tree was built with (host, (T,3); T must
 * be the tree's face count): half-edges sorted by (min vertex, max vertex) give the face across every edge, corner
 * keys sorted by vertex give every vertex's faces in ascending order (no float atomics: the table is deterministic).
 * It holds fn (T,3) f64, vpn (P,3) f64, opp (T,3) u32 and f (T,3) u32: 48 B per face + 24 B per vertex.  The build
 * checks that every leaf's corners equal v[f[face]] exactly (MSH_EINVAL "faces do not match the tree") and that every
 * index is < P (MSH_EINVAL), and counts what makes the sign undefined: boundary edges (one half-edge), non-manifold
 * edges (more than two; treated as boundary), inconsistently oriented edges (two half-edges of the same direction;
 * the opposite face is still used) and degenerate faces (zero area: a zero normal).  With all four counters zero the
 * sign is exact; otherwise it is undefined near the offending features.  One limit: a closest point that falls exactly
 * on a vertex while its part code names an edge uses the edge normal.
 * Plain triangle trees only (not the normals metric, point or batched trees, nor trees built with extra faces).
 * Calling it again replaces the table; msh_tree_free frees it; it is installed on every replica of the handle
 * (msh_set_devices); blobs leave it out (an unpacked handle has none until msh_tree_sign_build is called on it). */
typedef struct msh_sign_info {
    int32_t state;                /* 0 none, 1 built */
    uint64_t boundary_edges, nonmanifold_edges, inconsistent_edges, degenerate_faces;
    uint64_t bytes;               /* device bytes of the table */
    double build_ms;              /* GPU time of its build */
} msh_sign_info;
int msh_tree_sign_build(msh_tree* tree, const uint32_t* f, size_t T);
int msh_tree_sign_info(const msh_tree* tree, msh_sign_info* info);
/* msh_tree_nearest plus sdist (S,) f64 = +-sqrt((dx dx + dy dy) + dz dz), d = q - point: negative where d . N < 0
 * (inside an outward-oriented mesh), positive otherwise, +0.0 where d is zero, NaN on rows whose face is
 * MSH_NO_FACE (non-finite queries).  face, part and point are msh_tree_nearest's, bit for bit.  part may be NULL.
 * MSH_EINVAL before msh_tree_sign_build. */
int msh_tree_signed_distance(msh_tree* tree, const double* q, size_t S, double* sdist, uint32_t* face, uint32_t* part,
                             double* pt);
int msh_tree_signed_distance_device(msh_tree* tree, const double* d_q, size_t S, double* d_sdist, uint32_t* d_face,
                                    uint32_t* d_part, double* d_pt, void* stream);
/* The sign pass alone, for given (face, part, point) rows (a caller that already holds answers, such as the narrow
 * multi-GPU exchange): d_part is required; no workspace is used.  Device pointers; asynchronous on `stream`. */
int msh_tree_sign_from_faces_device(msh_tree* tree, const double* d_q, size_t S, const uint32_t* d_face,
                                    const uint32_t* d_part, const double* d_pt, double* d_sdist, void* stream);

/* ---- generalised winding numbers: inside / outside on open meshes and soups (no reference counterpart) ----
 * w(q) = (1 / 4 pi) sum over the tree's leaf triangles (a, b, c), taken relative to q, of the solid angle
 *   2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|)        (Van Oosterom and Strackee 1983):
 * 1 inside an outward-oriented closed mesh, 0 outside, fractional near openings; a row is inside iff w > 0.5.  It
 * needs no closed, manifold or consistently oriented mesh, so it serves where the pseudonormal sign above is
 * undefined: scans with holes, templates open at the neck or wrist, clothing layers, soups.  The sum runs over every
 * leaf of the tree, the extra faces of msh_tree_build_ex included.  A row with a non-finite coordinate gets NaN; a
 * row exactly on the surface gets a finite, otherwise unspecified value (the solid angle of a triangle seen from
 * one of its own points is taken as atan2 gives it: 0 at a corner, 0 or +-2 pi in its plane).
 *
 * The walk (Barill et al. 2018, "Fast winding numbers for soups and clouds"): depth first from the root, child 0
 * before child 1.  A node farther than beta r from the row -- |q - p| > beta r, p the area-weighted centroid of the
 * node's triangles and r a radius around p that holds all their vertices -- adds its dipole (p - q) . N / (4 pi
 * |p - q|^3), N the sum of its triangles' area vectors, and is not opened; a leaf adds its exact fp64 solid angle.
 * Everything is accumulated in fp64 in visit order, one lane per row, so a row's answer depends on (tree, q, beta)
 * alone: not on the other rows of the call, their order, the device split or the entry cut.
 *   beta = 0     exact: every node is opened and every leaf evaluated (O(T) per row);
 *   beta > 0     larger is more accurate and slower; MSH_WINDING_BETA_DEFAULT keeps |w - exact| <= 1e-2 on the test
 *                meshes (DESIGN.md s14 has the table);
 *   beta = +inf  no node lies farther than that: the exact walk again;
 *   beta < 0 or NaN: MSH_EINVAL.
 * The table behind it holds one 32-B fp32 record per internal node (p, r, N; relative to the tree's origin), built on
 * the GPU from the stored nodes and leaves alone, bottom up: a node's fp64 sums are (child 0's) + (child 1's), a
 * leaf's come from its own triangle -- no float atomics, the same bytes on every build.  It is built by
 * msh_tree_winding_build or by the first query that misses it, on the handle and every replica (msh_set_devices);
 * msh_tree_free frees it; blobs leave it out (an unpacked handle builds its own).  A tree of one face has no table
 * (state stays 0, bytes 0) and is always evaluated exactly.
 * Plain triangle trees only (kind 0): normals-metric, point and batched trees and NULL handles are MSH_EINVAL.
 * S == 0 returns MSH_OK.  msh_timing_get names: "winding_build", "winding". */
#define MSH_WINDING_BETA_DEFAULT 4.0
typedef struct msh_winding_info {
    int32_t state;        /* 0 none, 1 built */
    uint32_t node_bytes;  /* bytes of one record */
    uint32_t stack_lds;   /* per-lane stack entries held in LDS before the walk spills */
    uint64_t bytes;       /* device bytes of the table */
    double build_ms;      /* GPU time of its build */
} msh_winding_info;
int msh_tree_winding_build(msh_tree* tree);                 /* idempotent; the query calls build it when missing */
int msh_tree_winding_info(const msh_tree* tree, msh_winding_info* info);
/* Host arrays: q (S,3) f64 in, w (S,) f64 out; the rows go through the pinned-slab pipeline and are split over the
 * handle's replicas as msh_tree_signed_distance's are (24 B in, 8 B out per row). */
int msh_tree_winding_number(msh_tree* tree, const double* q, size_t S, double beta, double* w);
/* Device pointers; asynchronous on `stream` -- except a first call that has to build the table, which is synchronous
 * (it waits for the build and reads its status back), like the call that builds the entry cut: a caller that
 * captures the call in a graph or needs it asynchronous calls msh_tree_winding_build first. */
int msh_tree_winding_number_device(msh_tree* tree, const double* d_q, size_t S, double beta, double* d_w, void* stream);
/* untimed, same walk: counts[0] nodes approximated, [1] nodes opened, [2] leaves evaluated, [3] deepest stack any row
 * reached (entries; beyond stack_lds the walk spilled).  d_q is a device pointer; synchronous. */
int msh_tree_winding_stats(msh_tree* tree, const double* d_q, size_t S, double beta, uint64_t counts[4]);

/* The order in which the closest-point path visits the S query rows (d_perm[slot] = row): stable by the
 * Hilbert index of each row's cell in a 256^3 grid over the tree's scene box widened by 10 % per side (the cell is
 * the top 24 bits of the row's 30-bit Morton code, mapped to the Hilbert curve of the same cells; then 3 LDS radix
 * passes of 8 bits).  No reference counterpart (test and diagnostic entry point).  Asynchronous on `stream`. */
int msh_tree_query_order(msh_tree* tree, const double* d_q, size_t S, uint32_t* d_perm, void* stream);

/* Entry cut of a triangle tree (no reference counterpart: derived acceleration data).  A grid
 * of G^3 cells over the scene box widened by 1/4, one record per cell -- its hint leaf and 7 start entries: 32 B for
 * trees of up to 2^20 faces, 64 B beyond (which also hold the radius each list covers) -- from which closest-point
 * queries start their walks instead of the root, and so do nearest_alongnormal rays (their walk first covers that
 * radius around p, and starts again from the root only when no hit lies that near); it changes where a walk starts,
 * never an answer.  It is built lazily by a closest-point or alongnormal call of the handle (msh_tree_nearest*,
 * msh_tree_nearest_bary*, msh_tree_signed_distance*, msh_tree_nearest_alongnormal*, and their _stats).  The automatic grid comes in two sizes: the
 * coarse one (about 8 cells per face, at most 2^23 cells: C3 G = 200, 256 MB, ~11 ms) once the handle's calls have
 * brought at least one row per 16 of its cells (C3: 500k rows; a few small calls on a large mesh walk from the root
 * instead of paying the build), the fine one (twice the coarse resolution: about 64 cells per face, C3 G = 400,
 * 2.05 GB) once they have brought 16 rows per fine cell (C3: ~1G rows), or at the next call after
 * msh_tree_set_entry_cut(t, -1) (a caller that keeps the tree for many batches).  The fine grid is built from the
 * coarse one (its cells' start lists and centre walks begin there); asked for with no grid installed, the coarse grid
 * is built first and freed after (C3: ~57 ms for both).  build_ms counts both.  A grid asked for with msh_tree_set_entry_cut is built by the
 * next call whatever its size.  Trees used only for visibility or the normals metric never hold it; trees of
 * < 4096 faces never get one.  The call that builds it is synchronous, also for the *_device entry points (the cut's
 * build waits for its own cell-centre queries): a caller that captures *_device calls in a graph or needs them
 * asynchronous calls msh_tree_set_entry_cut and makes one small query first (or sets G = 0).
 *   G < 0: the fine automatic grid at the next call (the default policy above until then);
 *   G = 0: no cut (frees one already built); queries start at the root;
 *   G > 0: G^3 cells.
 * Calling it (any G != 0, also the current one) makes the next closest-point call build the grid if it is not
 * built yet; changing G frees the current cut first.  A cut that cannot be built (device memory) is not an error:
 * its queries start at the root (a failed upgrade keeps the coarse grid); an automatic grid is tried again after
 * another threshold of rows (at most twice, state 0 meanwhile), then the handle records the failure (state 3), as
 * it does at once for a grid asked for with msh_tree_set_entry_cut. */
int msh_tree_set_entry_cut(msh_tree* tree, int G);
/* state: 0 not built yet, 1 built, 2 off (G = 0, or a tree it does not apply to), 3 build failed (a handle with
 * replicas reports a replica's failed or pending state over its own);
 * G: cells per axis of the built cut (0 if none); bytes: device bytes it holds; build_ms: GPU time of its
 * build (cell-centre queries + cut + hints).  Any output pointer may be NULL. */
int msh_tree_entry_cut_info(const msh_tree* tree, int* state, int* G, uint64_t* bytes, double* build_ms);
/* cells of the built cut whose start list was shortened by the build's directional rule (0 if none is built).
 * Closest-point queries use such cells like any other; aabbtree_nearest_alongnormal starts their rays at the root. */
int msh_tree_entry_cut_flagged(const msh_tree* tree, uint64_t* cells);

/* aabbtree_nearest_alongnormal(tree, p, n) -> (dist (S,) f64, face (S,) u32, point (S,3) f64):
 * spatialsearchmodule.cpp:222-323.  Nearest hit of the rays (p, n) and (p, -n); hit point = CGAL's
 * Plane_3 / Line_3 construction.  No hit: dist = 1e100 (as the reference), face = MSH_NO_FACE,
 * point = NaN (reference: uninitialised). */
int msh_tree_nearest_alongnormal(msh_tree* tree, const double* p, const double* n, size_t S, double* dist,
                                 uint32_t* face, double* pt);
int msh_tree_nearest_alongnormal_device(msh_tree* tree, const double* d_p, const double* d_n, size_t S,
                                        double* d_dist, uint32_t* d_face, double* d_pt, void* stream);
/* Instrumented ray traversals (not timed; same traversal as the entry points above): total internal nodes
 * loaded and leaf triangles tested, for the algorithmic-bytes figure of the ray roofline. */
int msh_tree_nearest_alongnormal_stats(msh_tree* tree, const double* d_p, const double* d_n, size_t S, uint64_t* nodes,
                                       uint64_t* leaves);
int msh_visibility_stats(msh_tree* tree, const double* d_cams, size_t C, double min_dist, uint64_t* nodes,
                         uint64_t* leaves);

/* aabbtree_intersections_indices(tree, qv, qf) -> ascending query-face indices (K,) u32 whose
 * triangle intersects any mesh triangle: spatialsearchmodule.cpp:326-417 (unregistered there,
 * SURVEY App. B).  out must hold Tq entries; *K receives the count. */
int msh_tree_intersections(msh_tree* tree, const double* qv, size_t Pq, const uint32_t* qf, size_t Tq, uint32_t* out,
                           size_t* K);

/* ---- intersection pair lists (no reference counterpart: the reference stops at the first hit) ----
 * Which face hits which face, for collision and interpenetration terms, contact detection and mesh repair.
 * Query mode: all (i, j) for which query face i of (qv, qf) and the tree's leaf primitive j overlap, by the closed
 * predicate msh_tree_intersections uses (touching counts, coplanar pairs included), called as overlap(query_i, mesh_j).
 * j is the face id of the leaf: on a tree built with extra faces (msh_tree_build_ex) it ranges over the main faces
 * [0, T) and the extra faces [T, T + ET), as msh_tree_intersections tests them all.  Plain triangle trees (kind 0).
 * Self mode: all (i, j), i < j, both faces of the tree, that overlap (overlap(tri_i, tri_j)) and share no exactly
 * equal vertex coordinate -- the rule of msh_ntree_selfintersects; plain and normals-metric trees (kinds 0, 1); a tree
 * built with extra faces is MSH_EINVAL.
 * pairs is (K, 2) u32 row-major, sorted ascending by (i, j), without duplicates.  counts (optional, may be NULL) gets
 * one u32 per row -- Tq rows in query mode, T in self mode, rows being face ids, not leaf positions --: the number of
 * pairs whose first member is that row, so an exclusive scan of it indexes pairs as CSR.  The same inputs give the
 * same bytes on every call (no atomics decide order or content).
 * cap protocol: *K always receives the full pair count; the first min(K, cap) pairs in sorted order are written to
 * pairs (capacity cap pairs = 2 cap u32).  cap == 0 with pairs == NULL counts only: nothing is filled or sorted.
 * Tq == 0: K = 0.  K is limited to 2^32 - 1 (MSH_EINVAL beyond, found by a 64-bit sum of the counts), Tq to 2^31 - 1.
 * Point trees, batched trees and NULL handles are MSH_EINVAL.  The host entry points check every query face index
 * (MSH_EINVAL); the device ones detect an index >= Pq on the device (MSH_EINVAL, nothing is read out of bounds, the
 * handle stays usable).
 * The *_device entry points take device pointers and are synchronous up to the moment K is known (one 24-byte
 * read-back on `stream` after the counting pass); the scan, fill and order launches after it, and the copy into
 * d_counts, are asynchronous on `stream`.  The calls stay on the handle's own device (no row split over replicas).
 * msh_timing_get names: "tritri_count" (the counting traversal), "tritri_scan" (the totals, then the offsets),
 * "tritri_fill" (the second traversal; it also orders rows of up to 32 hits) and "tritri_order" (only when a row is
 * longer: two stable radix sorts of all pairs and the interleave). */
int msh_tree_intersection_pairs(msh_tree* tree, const double* qv, size_t Pq, const uint32_t* qf, size_t Tq,
                                uint32_t* pairs, size_t cap, uint32_t* counts, size_t* K);
int msh_tree_intersection_pairs_device(msh_tree* tree, const double* d_qv, size_t Pq, const uint32_t* d_qf, size_t Tq,
                                       uint32_t* d_pairs, size_t cap, uint32_t* d_counts, size_t* K, void* stream);
int msh_tree_self_intersection_pairs(msh_tree* tree, uint32_t* pairs, size_t cap, uint32_t* counts, size_t* K);
int msh_tree_self_intersection_pairs_device(msh_tree* tree, uint32_t* d_pairs, size_t cap, uint32_t* d_counts,
                                            size_t* K, void* stream);

/* ---- aabb_normals (aabb_normals.cpp, AABB_n_tree.h) ---- */
/* aabbtree_n_compute(v, f, eps): aabb_normals.cpp:63-110 */
int msh_ntree_build(const double* v, size_t P, const uint32_t* f, size_t T, double eps, msh_tree** out);
/* aabbtree_n_nearest(tree, v, n) -> (face (1,S) u32, point (S,3) f64): aabb_normals.cpp:112-190.
 * Metric ||q - p|| + eps (1 - n_q . n_tri) (AABB_n_tree.h:40-84); lexicographic min (metric, face). */
int msh_ntree_nearest(msh_tree* tree, const double* q, const double* n, size_t S, uint32_t* face, double* pt);
/* aabbtree_n_selfintersects(tree) -> int: aabb_normals.cpp:192-207; pairs sharing an exactly equal
 * vertex coordinate are skipped (AABB_n_tree.h:107-116). */
int msh_ntree_selfintersects(msh_tree* tree, int64_t* count);

/* ---- visibility (py_visibility.cpp, visibility.cpp) ---- */
/* visibility_compute(cams, tree|v,f, n, sensors, extra_v, extra_f, min_dist) -> (vis (C,P) u32,
 * n_dot_cam (C,P) f64): py_visibility.cpp:81-219, VisibilityTask visibility.cpp:75-115.
 * Visibility is computed for the tree's main-mesh vertices.  normals (P,3) and sensors (C,9) may be
 * NULL; without normals ndc is zero-filled (reference: uninitialised).  The tree is borrowed, never
 * freed (fixes the double free at py_visibility.cpp:212). */
int msh_visibility(msh_tree* tree, const double* cams, size_t C, const double* normals, const double* sensors,
                   double min_dist, uint32_t* vis, double* ndc);
/* Device-resident shard of visibility_compute: vertices [v_begin, v_begin + v_count) of the main mesh
 * (the multi-GPU split of the (C x P) ray grid by vertex range, visibility.cpp:136-173).  d_normals is
 * indexed by global vertex (P,3); d_vis / d_ndc are (C, v_count). */
int msh_visibility_device(msh_tree* tree, const double* d_cams, size_t C, const double* d_normals,
                          const double* d_sensors, double min_dist, size_t v_begin, size_t v_count, uint32_t* d_vis,
                          double* d_ndc, void* stream);

/* ---- mesh geometry feeding the path ---- */
/* Mesh.estimate_vertex_normals (mesh.py:208-216): per vertex, the sum in ascending face order of the
 * faces' cross products (v1 - v0) x (v2 - v0) (tri_normals.py:23-24), divided by its norm (0 -> 1). */
int msh_vertex_normals(const double* v, size_t P, const uint32_t* f, size_t T, double* vn);
/* device pointers; returns when the result is in d_vn (stream may be NULL).  A face index >= P is
 * detected on the device: MSH_EINVAL, d_vn unspecified, no out-of-bounds access. */
int msh_vertex_normals_device(const double* d_v, size_t P, const uint32_t* d_f, size_t T, double* d_vn, void* stream);

/* ---- batched trees: scan-to-mesh registration over many meshes (BASELINE configs[3], C4) ----
 * The reference answers this with one AabbTree per mesh (search.py:21-30, one aabbtree_compute +
 * aabbtree_nearest per mesh).  Here B meshes sharing one topology are built in ONE batched LBVH build
 * (per-mesh Morton order, Karras emission and refit in single launches over all B*T faces) and queried
 * in one launch.  v: (B,P,3) f64, f: (T,3) u32 shared by all meshes, T >= 2.  Face indices returned
 * are mesh-local (as a per-mesh AabbTree would return). */
int msh_batch_build(const double* v, size_t B, size_t P, const uint32_t* f, size_t T, msh_tree** out);
/* q: (B,S,3) f64, S queries per mesh -> face (B,S) u32, part (B,S) u32 (may be NULL), point (B,S,3) f64;
 * per mesh identical to msh_tree_nearest on that mesh alone. */
int msh_batch_nearest(msh_tree* tree, const double* q, size_t S, uint32_t* face, uint32_t* part, double* pt);
int msh_batch_nearest_device(msh_tree* tree, const double* d_q, size_t S, uint32_t* d_face, uint32_t* d_part,
                             double* d_pt, void* stream);
/* registration-ready variant: face (B,S), point (B,S,3), barycentric weights (B,S,3) (see
 * msh_tree_nearest_bary) */
int msh_batch_nearest_bary(msh_tree* tree, const double* q, size_t S, uint32_t* face, double* pt, double* w);
int msh_batch_nearest_bary_device(msh_tree* tree, const double* d_q, size_t S, uint32_t* d_face, double* d_pt,
                                  double* d_w, void* stream);

/* ---- ClosestPointTree (search.py:52-65, scipy.spatial.KDTree) ---- */
int msh_points_build(const double* v, size_t P, msh_tree** out);
/* nearest vertex: lexicographic min (squared distance, vertex index); dist = sqrt(d2) */
int msh_points_nearest(msh_tree* tree, const double* q, size_t S, uint32_t* idx, double* dist);

/* ---- K-nearest and radius-capped queries on point trees and plain triangle trees ----
 * For row i and a tree of n primitives (the vertices of a point tree; the leaf triangles of a triangle tree, the extra
 * faces of msh_tree_build_ex included, with the ids the pair lists use), the answer is the first min(K, m_i) of the
 * primitives with d2 <= r2, ascending by the lexicographic key (d2, id):
 *   d2   the exact fp64 squared distance the 1-NN entry points compute ((dx dx + dy dy) + dz dz to a vertex; CGAL's
 *        closest-point construction on a triangle), id the vertex index or face id;
 *   r2   r_max * r_max, rounded once in fp64; r_max = +inf: no cap; r_max = 0: exact hits only;
 *   m_i  the number of primitives that qualify.
 * A row's answer is a function of (tree, q_i, K, r_max) alone -- not of the visit order, the other rows, the chunking
 * or the device split; ties on d2 are decided by id; no atomic decides content or order.  dist[i, j] = sqrt(d2).
 * Unused entries j >= count[i] hold MSH_NO_FACE, +inf, a NaN point and part 0; a row with a non-finite coordinate
 * gets count 0 and padding only.  Column 0 of an uncapped answer equals msh_points_nearest (idx, dist) and
 * msh_tree_nearest (face, part, point) bit for bit, and columns 0..K-1 of a K' > K answer equal the K answer.
 * 1 <= K <= MSH_KNEAREST_MAX and r_max >= 0 (not NaN), else MSH_EINVAL -- checked before the handle, then the handle,
 * then the pointers.  S == 0 returns MSH_OK; K > n is legal (padding); a tree of one primitive works.
 * msh_points_* take point trees, msh_tree_knearest* plain triangle trees; normals-metric and batched trees and NULL
 * handles are MSH_EINVAL.  The walk starts at the root (the entry cut is neither built nor used), one lane per row in
 * the closest-point path's slot order, depth first, nearer child first, keeping a sorted list of at most K entries and
 * pruning on its K-th.  The host entry points go through the pinned-slab pipeline and split their
 * rows over the handle's replicas; the *_device ones take device pointers and are asynchronous on `stream` -- except
 * the first msh_tree_knearest_device call with pt or part on a handle, which builds the face -> leaf map and waits
 * for it (as msh_tree_points_from_faces_device does).  count, pt and part may be NULL.
 * msh_timing_get names: "kbest" (the walk), "kbest_finish" (the pass that writes dist, pt, part and the padding). */
#define MSH_KNEAREST_MAX 64
int msh_points_knearest(msh_tree* tree, const double* q, size_t S, uint32_t K, double r_max, uint32_t* idx,
                        double* dist, uint32_t* count);
int msh_points_knearest_device(msh_tree* tree, const double* d_q, size_t S, uint32_t K, double r_max, uint32_t* d_idx,
                               double* d_dist, uint32_t* d_count, void* stream);
int msh_tree_knearest(msh_tree* tree, const double* q, size_t S, uint32_t K, double r_max, uint32_t* face, double* dist,
                      double* pt, uint32_t* part, uint32_t* count);
int msh_tree_knearest_device(msh_tree* tree, const double* d_q, size_t S, uint32_t K, double r_max, uint32_t* d_face,
                             double* d_dist, double* d_pt, uint32_t* d_part, uint32_t* d_count, void* stream);
/* untimed, same walk, point trees and plain triangle trees: counts[0] nodes visited, [1] primitives evaluated,
 * [2] list insertions, [3] deepest stack any row reached (entries).  d_q is a device pointer; synchronous. */
int msh_tree_knearest_stats(msh_tree* tree, const double* d_q, size_t S, uint32_t K, double r_max, uint64_t counts[4]);

/* ---- all primitives within a radius (scipy's query_ball_point) on point trees and plain triangle trees ----
 * Row i is a point q_i and a radius r_i.  A primitive (a vertex of a point tree; a leaf triangle of a triangle tree, the
 * extra faces of msh_tree_build_ex included) qualifies when d2 <= r2_i: d2 exactly the fp64 squared distance of the
 * K-nearest queries above, r2_i = r_i * r_i rounded once in fp64.  r = +inf takes every primitive, r = 0 exact hits only.
 *   radius  double r_max and const double* r_rows (S,): r_rows == NULL uses r_max for every row; otherwise r_rows[i] is
 *           used and r_max is ignored.  A scalar r_max that is negative or NaN is MSH_EINVAL, checked before the handle.
 *           A per-row radius that is negative or NaN gives that row count 0, as does a non-finite q_i; neither is an error.
 *   counts  msh_points_within_count, msh_tree_within_count: count (S,) u32, count[i] the number of qualifying primitives.
 *   lists   msh_points_within, msh_tree_within: the neighbours of all rows as CSR.  counts (S,) u32 (may be NULL) is as
 *           above and its exclusive scan indexes the lists; entries are sorted by (row, d2, id).  idx / face (cap,) u32 is
 *           the vertex index or face id, dist (cap,) f64 = sqrt(d2); for triangle trees pt (cap,3) f64 and part (cap,)
 *           u32 (each may be NULL) are the closest point and its part code by msh_tree_knearest's construction.
 *           So for every K' <= MSH_KNEAREST_MAX the first min(K', count[i]) entries of row i equal row i of
 *           msh_*_knearest(K', r_i) in id, dist, pt and part bit for bit, and min(count[i], K') is its count; with
 *           r = +inf entry 0 equals msh_points_nearest / msh_tree_nearest.
 * Cap protocol (that of msh_tree_raycast_all): *K always receives the full number of entries; the first min(K, cap)
 * entries in sorted order are written; cap == 0 with NULL list pointers counts only (nothing is filled or ordered);
 * counts is always complete; K > 2^32 - 1 is MSH_EINVAL, found by a 64-bit sum; S == 0 is MSH_OK with K = 0.
 * Determinism: a row's count and list are a function of (tree, q_i, r_i) alone -- not of the other rows, their order or
 * the chunking; the same inputs give the same bytes on every call; no atomic decides content or order.
 * msh_points_* take point trees, msh_tree_within* plain triangle trees: normals-metric and batched trees and NULL handles
 * are MSH_EINVAL, checked in the order handle, tree kind, row count, pointers.  The walk is msh_*_knearest's with the
 * radius as its only bound; the list call walks twice (count, fill) and orders each row: rows of at most 32 entries in
 * their own lane, longer ones through radix sorts of all K entries.
 * The counts calls go through the pinned-slab pipeline and split their rows over the handle's replicas; the list calls
 * stay on the handle's own device (the rows are uploaded whole; counts and the first min(K, cap) entries come back).
 * The *_device forms take device pointers (d_r_rows too) and are asynchronous on `stream`, except that the list calls
 * wait for the read-back of K.
 * msh_timing_get names: "within_count", "within_scan", "within_fill", "within_order" (long rows only), "within_emit". */
int msh_points_within_count(msh_tree* tree, const double* q, size_t S, double r_max, const double* r_rows,
                            uint32_t* count);
int msh_points_within_count_device(msh_tree* tree, const double* d_q, size_t S, double r_max, const double* d_r_rows,
                                   uint32_t* d_count, void* stream);
int msh_tree_within_count(msh_tree* tree, const double* q, size_t S, double r_max, const double* r_rows,
                          uint32_t* count);
int msh_tree_within_count_device(msh_tree* tree, const double* d_q, size_t S, double r_max, const double* d_r_rows,
                                 uint32_t* d_count, void* stream);
int msh_points_within(msh_tree* tree, const double* q, size_t S, double r_max, const double* r_rows, uint32_t* counts,
                      uint32_t* idx, double* dist, size_t cap, size_t* K);
int msh_points_within_device(msh_tree* tree, const double* d_q, size_t S, double r_max, const double* d_r_rows,
                             uint32_t* d_counts, uint32_t* d_idx, double* d_dist, size_t cap, size_t* K, void* stream);
int msh_tree_within(msh_tree* tree, const double* q, size_t S, double r_max, const double* r_rows, uint32_t* counts,
                    uint32_t* face, double* dist, double* pt, uint32_t* part, size_t cap, size_t* K);
int msh_tree_within_device(msh_tree* tree, const double* d_q, size_t S, double r_max, const double* d_r_rows,
                           uint32_t* d_counts, uint32_t* d_face, double* d_dist, double* d_pt, uint32_t* d_part,
                           size_t cap, size_t* K, void* stream);
/* untimed, the count walk, point trees and plain triangle trees: counts[0] nodes visited, [1] primitives evaluated,
 * [2] entries (the sum of the rows' counts), [3] deepest stack any row reached.  d_q and d_r_rows are device pointers;
 * synchronous. */
int msh_tree_within_stats(msh_tree* tree, const double* d_q, size_t S, double r_max, const double* d_r_rows,
                          uint64_t counts[4]);

/* ---- ray casting on plain triangle trees: first hit and occlusion for arbitrary rays ----
 * Row i is an origin o, a direction d and a closed range [t0, t1] of the parameter t of the point o + t d.  d may have
 * any non-zero length and is used as given (no (o + d) - o as for a CGAL Ray_3).  range is (S,2), or NULL for
 * [0, +inf] on every row; t0 < 0 is taken as 0.
 *   hit set    Leaf triangle j (face id j: the ids the pair lists use; on a tree of msh_tree_build_ex the main faces are
 *              [0, T) and the extra faces [T, T + ET)) is a hit when the closed ray-triangle predicate that
 *              nearest_alongnormal and visibility share reports a proper hit with t_j = num / den (num = n . (a - o),
 *              den = n . d, n = (b - a) x (c - a)) and t0 <= t_j <= t1, or a coplanar overlap whose parameter interval,
 *              clipped starting from [t0, t1] instead of [0, +inf], is not empty; then t_j is its lower end.
 *   first hit  msh_tree_raycast: the lexicographic minimum of (t_j, j) over the hit set.  t (S,) f64, face (S,) u32,
 *              and on request pt (S,3) and w (S,3) (either may be NULL): pt is nearest_alongnormal's construction,
 *              CGAL's intersection(Plane_3(a, b, c), Line_3(o, o + d)) for a proper hit and o + t d for a coplanar hit
 *              or where that construction's denominator is 0; w are the barycentric weights of pt that
 *              msh_tree_nearest_bary computes, in the order of f[face].  A miss gives t = +inf, face = MSH_NO_FACE, pt
 *              and w NaN.
 *   occlusion  msh_tree_occluded: hit (S,) u8 is 1 iff the hit set is not empty; the walk stops at the first hit found.
 * A row that cannot be cast -- a non-finite o or d, d = 0, a NaN in the range, t0 > t1 -- is answered as a miss; it is
 * no error.  A row's answer is a function of (tree, o, d, range) alone: not of the other rows, their order, the
 * chunking or the device split; no atomic decides an answer.
 * Relations to the reference's ray queries (tests/test_gpu_raycast.py):
 *   msh_tree_nearest_alongnormal(p, n) is the nearer, by (|pt - p|, face), of the first hits of (p, (p + n) - p) and
 *   (p, (p - n) - p);
 *   a vertex is visible to a camera iff (src, (src + dir) - src) is not occluded, src = v + min_dist dir and dir the unit
 *   vector from v to the camera as msh_visibility forms them.
 *   (One difference at the edge of fp64: a proper hit whose t_j = num / den is NaN -- a determinant overflowed -- is not
 *   in the hit set here, since t0 <= NaN fails, while msh_visibility and nearest_alongnormal accept it.)
 * Conditioning: the walk prunes by comparing fp32 box intervals of the geometric ray with the computed t; as for
 * nearest_alongnormal, its margins cover constructions whose error stays below 2^-20 (|o| + M), M the scene's
 * half-diagonal.
 * Plain triangle trees only, with or without extra faces: normals-metric, point and batched trees and NULL handles are
 * MSH_EINVAL, checked in the order handle, tree kind, row count, pointers.  S == 0 returns MSH_OK.  The walk starts at
 * the root (the entry cut is neither built nor used), one lane per ray in the slot order of the origins.  The host
 * entry points go through the pinned-slab pipeline and split their rows over the handle's replicas; the *_device ones
 * take device pointers and are asynchronous on `stream`.  msh_timing_get names: "raycast", "occluded". */
int msh_tree_raycast(msh_tree* tree, const double* o, const double* d, const double* range, size_t S, double* t,
                     uint32_t* face, double* pt, double* w);
int msh_tree_raycast_device(msh_tree* tree, const double* d_o, const double* d_d, const double* d_range, size_t S,
                            double* d_t, uint32_t* d_face, double* d_pt, double* d_w, void* stream);
int msh_tree_occluded(msh_tree* tree, const double* o, const double* d, const double* range, size_t S, uint8_t* hit);
int msh_tree_occluded_device(msh_tree* tree, const double* d_o, const double* d_d, const double* d_range, size_t S,
                             uint8_t* d_hit, void* stream);
/* untimed, the same walks (any != 0: the occlusion walk), outputs not written: *nodes internal nodes loaded, *leaves
 * leaf tests.  d_o, d_d, d_range are device pointers; synchronous. */
int msh_tree_raycast_stats(msh_tree* tree, const double* d_o, const double* d_d, const double* d_range, size_t S,
                           int any, uint64_t* nodes, uint64_t* leaves);

/* ---- ray casting on plain triangle trees: hit counts and sorted all-hits lists ----
 * Rows, ranges, castability and the hit set are exactly those of msh_tree_raycast above: row i is (o, d, [t0, t1]), d used
 * as given, t0 < 0 taken as 0; face j is in the hit set when the predicate reports a proper hit with t0 <= t_j <= t1
 * (t_j not NaN) or a coplanar overlap with a non-empty clipped interval (t_j: its lower end); a row that cannot be cast
 * has an empty hit set and is no error; the extra faces of msh_tree_build_ex are included with ids [T, T + ET).
 *   counts  msh_tree_raycast_count: count (S,) u32, count[i] the size of row i's hit set.
 *   lists   msh_tree_raycast_all: the hits of all rows as CSR.  counts (S,) u32 (may be NULL) is as above and its
 *           exclusive scan indexes the list; the list is sorted by (row, t by value, face id): -0.0 == 0.0, and equal t --
 *           shared edges and vertices, duplicated faces -- goes to the smaller face id.  t[k] is the value the predicate
 *           produced, unchanged; face[k] its face id; pt (cap,3) (may be NULL) is msh_tree_raycast's construction:
 *           CGAL's plane / line intersection for a proper hit, o + t d for a coplanar hit or a zero denominator; side (cap,)
 *           i8 (may be NULL) is +1 where den = n . d < 0 (the ray meets the front of the face, n = (b - a) x (c - a) in the
 *           order of f[face]), -1 where den > 0, 0 for a coplanar hit.
 *           So the first entry of every non-empty row equals msh_tree_raycast's (t, face, pt) bit for bit, and count > 0
 *           equals msh_tree_occluded.
 * Cap protocol (that of the pair lists): *K always receives the full number of hits; the first min(K, cap) entries in
 * sorted order are written; cap == 0 with NULL list pointers counts only (nothing is filled or ordered); counts is
 * always complete; K > 2^32 - 1 is MSH_EINVAL, found by a 64-bit sum; S == 0 is MSH_OK with K = 0.
 * Determinism: a row's count and list are a function of (tree, o, d, range) alone -- not of the other rows, their order
 * or the chunking; the same inputs give the same bytes on every call; no atomic decides content or order.
 * Plain triangle trees only: normals-metric, point and batched trees and NULL handles are MSH_EINVAL, checked in the
 * order handle, tree kind, row count, pointers.  The walk is msh_tree_occluded's without the early exit (nothing can be
 * pruned by a best t); the list call walks twice (count, fill) and orders each row's hits: rows of at most 32 hits in
 * their own lane, longer ones through radix sorts of all K entries.
 * msh_tree_raycast_count goes through the pinned-slab pipeline and splits its rows over the handle's replicas;
 * msh_tree_raycast_all stays on the handle's own device (the rays are uploaded whole; counts and the first min(K, cap)
 * entries come back).  The *_device forms take device pointers and are asynchronous on `stream`, except that
 * msh_tree_raycast_all_device waits for the read-back of K.
 * msh_timing_get names: "raycast_count", "raycast_scan", "raycast_fill", "raycast_order" (long rows only),
 * "raycast_emit". */
int msh_tree_raycast_count(msh_tree* tree, const double* o, const double* d, const double* range, size_t S,
                           uint32_t* count);
int msh_tree_raycast_count_device(msh_tree* tree, const double* d_o, const double* d_d, const double* d_range, size_t S,
                                  uint32_t* d_count, void* stream);
int msh_tree_raycast_all(msh_tree* tree, const double* o, const double* d, const double* range, size_t S,
                         uint32_t* counts, double* t, uint32_t* face, double* pt, int8_t* side, size_t cap, size_t* K);
int msh_tree_raycast_all_device(msh_tree* tree, const double* d_o, const double* d_d, const double* d_range, size_t S,
                                uint32_t* d_counts, double* d_t, uint32_t* d_face, double* d_pt, int8_t* d_side,
                                size_t cap, size_t* K, void* stream);

/* ---- multi-GPU replication (RCCL broadcast of a built BVH over xGMI) ---- */
/* Size of the flat device blob holding the mesh + BVH of a handle. */
int msh_tree_blob_size(const msh_tree* tree, size_t* bytes);
/* Pack the handle's device buffers into d_dst (HBM, on the handle's device, blob_size bytes). */
int msh_tree_blob_pack(const msh_tree* tree, void* d_dst, void* stream);
/* Create a handle on `device` from a packed blob already resident in that device's HBM
 * (e.g. after an RCCL broadcast).  The blob is copied; the caller keeps ownership of d_src. */
int msh_tree_blob_unpack(const void* d_src, size_t bytes, int device, void* stream, msh_tree** out);
/* Host-side blob header (no device): write the header of a blob for the given sizes into dst (cap
 * bytes), or parse + validate a header copied to host memory (magic, layout, version, length). */
int msh_blob_header_write(int kind, uint64_t P, uint64_t T, uint64_t T_main, void* dst, size_t cap,
                          msh_blob_info* info);
int msh_blob_header_parse(const void* src, size_t bytes, msh_blob_info* info);

/* ---- mesh files feeding the path (host parsing) ----
 * OBJ: replaces psbody.mesh.serialization.loadobj (mesh/src/py_loadobj.cpp:62-243).  sizes[9] = v rows,
 * vt rows, vt columns, vn rows, f rows, ft rows, fn rows, groups, landmarks.  Arrays are row-major
 * (rows x 3, vt rows x vt columns); groups and landmarks are enumerated in name order (std::map, as the
 * reference).  Errors: "Could not load file". */
typedef struct msh_obj msh_obj;
int msh_obj_load(const char* path, msh_obj** out);
int msh_obj_sizes(const msh_obj* obj, uint64_t* sizes);
int msh_obj_arrays(const msh_obj* obj, double* v, double* vt, double* vn, uint32_t* f, uint32_t* ft, uint32_t* fn);
const char* msh_obj_mtl_path(const msh_obj* obj);
int msh_obj_group(const msh_obj* obj, size_t k, const char** name, uint64_t* n_faces, const uint32_t** faces);
int msh_obj_landmark(const msh_obj* obj, size_t k, const char** name, uint32_t* vertex);
void msh_obj_free(msh_obj* obj);
/* PLY: replaces psbody.mesh.serialization.plyutils.read (mesh/src/plyutils.c:64-139 over rply.c).
 * sizes[4] = vertices, faces, has colour, has normals; v / colour / normals (P,3), tri (F,3) as double
 * (items 0..2 of each face list).  Errors: "Failed to open PLY file.", "plyread_mex: Bad raw header.",
 * "Read failed. <path>". */
typedef struct msh_ply msh_ply;
int msh_ply_load(const char* path, msh_ply** out);
int msh_ply_sizes(const msh_ply* ply, uint64_t* sizes);
int msh_ply_arrays(const msh_ply* ply, double* v, double* tri, double* color, double* normals);
void msh_ply_free(msh_ply* ply);

/* ---- kernel timing (HIP events on the launch stream; used by bench.py's roofline) ---- */
int msh_timing_enable(int on);
/* Total milliseconds and launch count of kernel `name` ("nearest", "sort", "morton") since reset. */
int msh_timing_get(const char* name, double* ms, int64_t* count);
int msh_timing_reset(void);

/* ---- page-locked result pool (host-buffer entry points) ----
 * Replaces nothing in the reference: its methods return fresh numpy arrays (PyArray_SimpleNew,
 * spatialsearchmodule.cpp:196-206), which the shims keep doing for small calls.  For large calls the
 * shims carve the result arrays out of one block of this pool instead, so the host-buffer entry points
 * copy results from HBM straight into them (no pinned staging copy, and no first-touch page faults of
 * fresh pages: on C3, 3.2 GB of results per call).  A block returns to the pool when the last array
 * over it dies.
 *  - msh_host_alloc: a block of >= bytes (2 MB granules), reusing a free block of at most 5/4 the
 *    size; blocks are page-locked with hipHostMalloc.  MSH_ENOMEM when the pool would outgrow its
 *    cap (MESH_AMD_PINNED_POOL_MB, default 16384; 0 disables the pool) even after releasing its free
 *    blocks: the caller then allocates ordinary pageable arrays.
 *  - msh_host_free: returns a block (any pointer msh_host_alloc gave) to the pool; NULL is ignored.
 *  - msh_host_pool_trim: releases every free block, and the idle staging slabs the host-array entry points
 *    share between handles; msh_host_pool_bytes: bytes held (live + free).
 * Host-buffer entry points recognise output arrays that lie inside one live block. */
int msh_host_alloc(size_t bytes, void** out);
void msh_host_free(void* p);
int msh_host_pool_trim(void);
size_t msh_host_pool_bytes(void);

/* ---- device memory kept between handles (no reference counterpart) ----
 * Three process-wide caches keep device memory after the handles that used it are freed, so a caller that builds
 * a tree per call (Mesh.closest_faces_and_points, mesh.py:454-455) does not reallocate it every call:
 *  - every device block the library frees (tree buffers, build temporaries, scratch) is cached for the next
 *    request of a similar size on its device, up to MESH_AMD_DEVICE_CACHE_MB (default 16384; 0 turns it off);
 *  - the query workspace of a freed triangle tree (sort keys, permutations, spill stacks, deferred lists:
 *    ~80 B per query of its largest call, ~8 GB at 100M queries), one idle workspace per device, handed to the
 *    next triangle tree built on that device;
 *  - up to two idle sets of host-call staging slabs per device (three device slabs of chunk x row bytes each,
 *    plus two page-locked host slabs).
 * msh_device_pool_trim frees all three (idle entries only: memory held by live handles stays with them);
 * msh_device_pool_bytes reports the device bytes they hold (any pointer may be NULL).  A process that
 * shares the GPU with other allocators (torch) calls the trim after freeing its handles.  A device allocation of
 * the library that fails for memory first releases the idle workspace, the idle staging slabs' device slabs and
 * the cached blocks of its device, then tries once more. */
int msh_device_pool_trim(void);
int msh_device_pool_bytes(uint64_t* workspace, uint64_t* staging, uint64_t* cached);

#ifdef __cplusplus
}
#endif
#endif /* MESHSEARCH_H_ */
