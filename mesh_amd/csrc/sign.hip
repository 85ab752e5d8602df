// Signed distance: the sign table of a triangle tree and the per-row sign pass (no reference counterpart).
//
// The side of the surface a query lies on is the sign of (q - p) . N, p the closest point and N the angle-weighted
// pseudonormal of the feature p lies on (Baerentzen and Aanaes 2005, "Signed distance computation using the angle
// weighted pseudonormal"): exact on a closed, consistently oriented manifold mesh.  The traversal already classifies
// the feature (closest_on_triangle's part code: 0 interior, 1/2/3 edge ab/bc/ca, 4/5/6 vertex a/b/c), so the table
// holds what each class needs:
//
//   k_sign_faces      one lane per leaf: its face's unit normal and three corner angles (fp64), the check that the
//                     leaf's corners are v[f[face]] bit for bit, degenerate faces counted
//   radix sort        (vertex, corner) pairs, stable: every vertex's corners in ascending face order (as geometry.hip)
//   k_sign_vertex     the first lane of each vertex's run: ordered sum of angle x unit normal -> vpn
//   radix sort x 2    half-edges keyed by (min vertex, max vertex): the max first, then a stable pass on the min
//   k_sign_edge_min   the second pass's keys (the min vertex of the half-edge now at each sorted position)
//   k_sign_edge_runs  the first lane of each run of equal edges classifies it: 1 half-edge boundary, 2 of opposite
//                     direction manifold, 2 of the same direction inconsistent (still paired), > 2 non-manifold
//                     (treated as boundary) -> opp, and the counters (integer atomics only: the table is deterministic)
//   k_sign_pass       one lane per row, caller order: N by (face, part), sdist = +-|q - p|
#include <algorithm>
#include <cmath>

#include "internal.h"

namespace msh {

enum { kCntBoundary = 0, kCntNonManifold = 1, kCntInconsistent = 2, kCntDegenerate = 3, kCntError = 4 };

__device__ inline bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

// angle between e1 and e2 (Baerentzen and Aanaes' weight): atan2(|e1 x e2|, e1 . e2)
__device__ inline double corner_angle(const D3& e1, const D3& e2) {
    const D3 c = vcross(e1, e2);
    return atan2(sqrt((c.x * c.x + c.y * c.y) + c.z * c.z), vdot(e1, e2));
}

// Face indices are checked before they index v (as k_face_normals does): a face with an index >= P raises the error
// word and gets a zero normal and zero angles.
__global__ __launch_bounds__(kBlock) void k_sign_faces(const TriRec* __restrict__ tris, const double* __restrict__ v,
                                                       size_t P, const uint32_t* __restrict__ f, size_t T,
                                                       double* __restrict__ fn, double* __restrict__ ang,
                                                       uint32_t* __restrict__ counts) {
    const size_t l = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= T) return;
    D3 a, b, c;
    uint32_t face;
    load_tri(tris, (int)l, a, b, c, face);
    if (face >= T) {
        atomicOr(&counts[kCntError], 2u);
        return;
    }
    const size_t t = face;
    const size_t i0 = f[3 * t], i1 = f[3 * t + 1], i2 = f[3 * t + 2];
    if (i0 >= P || i1 >= P || i2 >= P) {
        atomicOr(&counts[kCntError], 1u);
        return;  // fn and ang were zeroed by the launcher
    }
    const bool same = same_bits(a.x, v[3 * i0]) && same_bits(a.y, v[3 * i0 + 1]) && same_bits(a.z, v[3 * i0 + 2]) &&
                      same_bits(b.x, v[3 * i1]) && same_bits(b.y, v[3 * i1 + 1]) && same_bits(b.z, v[3 * i1 + 2]) &&
                      same_bits(c.x, v[3 * i2]) && same_bits(c.y, v[3 * i2 + 1]) && same_bits(c.z, v[3 * i2 + 2]);
    if (!same) atomicOr(&counts[kCntError], 2u);
    const D3 ab = vsub(b, a), ac = vsub(c, a), bc = vsub(c, b);
    const D3 n = vcross(ab, ac);
    const double len = sqrt((n.x * n.x + n.y * n.y) + n.z * n.z);
    if (len > 0.0 && len < INFINITY) {
        fn[3 * t] = n.x / len;
        fn[3 * t + 1] = n.y / len;
        fn[3 * t + 2] = n.z / len;
    } else {
        atomicAdd(&counts[kCntDegenerate], 1u);
    }
    ang[3 * t] = corner_angle(ab, ac);
    ang[3 * t + 1] = corner_angle(bc, D3{-ab.x, -ab.y, -ab.z});
    ang[3 * t + 2] = corner_angle(D3{-ac.x, -ac.y, -ac.z}, D3{-bc.x, -bc.y, -bc.z});
}

// keys = vertex of corner e (an index >= P becomes P, which sorts last), vals = e
__global__ __launch_bounds__(kBlock) void k_sign_corner_keys(const uint32_t* __restrict__ f, size_t n, size_t P,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    keys[e] = f[e] < P ? f[e] : (uint32_t)P;
    vals[e] = (uint32_t)e;
}

// the lane at the first position of a vertex's run sums the run in order (ascending face: the sort is stable)
__global__ __launch_bounds__(kBlock) void k_sign_vertex(const uint32_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ corners, size_t n, size_t P,
                                                        const double* __restrict__ fn, const double* __restrict__ ang,
                                                        double* __restrict__ vpn) {
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = keys[p];
    if (k >= P || (p > 0 && keys[p - 1] == k)) return;
    double x = 0.0, y = 0.0, z = 0.0;
    for (size_t j = p; j < n && keys[j] == k; ++j) {
        const size_t e = corners[j], t = e / 3u;
        const double w = ang[e];
        x += w * fn[3 * t];
        y += w * fn[3 * t + 1];
        z += w * fn[3 * t + 2];
    }
    vpn[3 * (size_t)k] = x;
    vpn[3 * (size_t)k + 1] = y;
    vpn[3 * (size_t)k + 2] = z;
}

// half-edge e = 3 t + k runs from corner k of face t to corner (k + 1) % 3: edges ab, bc, ca (part codes 1, 2, 3)
__device__ inline void half_edge(const uint32_t* __restrict__ f, size_t e, uint32_t& u, uint32_t& w) {
    const size_t t = e / 3u, k = e - 3 * t;
    u = f[e];
    w = f[3 * t + (k == 2 ? 0 : k + 1)];
}

__global__ __launch_bounds__(kBlock) void k_sign_edge_max(const uint32_t* __restrict__ f, size_t n, size_t P,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    uint32_t u, w;
    half_edge(f, e, u, w);
    const uint32_t m = u > w ? u : w;
    keys[e] = m < P ? m : (uint32_t)P;
    vals[e] = (uint32_t)e;
}

__global__ __launch_bounds__(kBlock) void k_sign_edge_min(const uint32_t* __restrict__ f, size_t n, size_t P,
                                                          const uint32_t* __restrict__ vals, uint32_t* __restrict__ keys) {
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const size_t e = vals[p];
    if (e >= n) return;
    uint32_t u, w;
    half_edge(f, e, u, w);
    const uint32_t m = u < w ? u : w;
    keys[p] = m < P ? m : (uint32_t)P;
}

__global__ __launch_bounds__(kBlock) void k_sign_edge_runs(const uint32_t* __restrict__ f, size_t n,
                                                           const uint32_t* __restrict__ sorted, uint32_t* __restrict__ opp,
                                                           uint32_t* __restrict__ counts) {
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const size_t e0 = sorted[p];
    if (e0 >= n) return;
    uint32_t u0, w0;
    half_edge(f, e0, u0, w0);
    const uint32_t lo = u0 < w0 ? u0 : w0, hi = u0 < w0 ? w0 : u0;
    auto same_edge = [&](size_t j, uint32_t& u, uint32_t& w) {
        const size_t e = sorted[j];
        if (e >= n) return false;
        half_edge(f, e, u, w);
        return (u < w ? u : w) == lo && (u < w ? w : u) == hi;
    };
    uint32_t u1 = 0, w1 = 0;
    if (p > 0 && same_edge(p - 1, u1, w1)) return;  // not the first of its run
    size_t len = 1;
    while (p + len < n && same_edge(p + len, u1, w1)) ++len;
    if (len == 2) {
        const size_t e1 = sorted[p + 1];
        opp[e0] = (uint32_t)(e1 / 3u);
        opp[e1] = (uint32_t)(e0 / 3u);
        half_edge(f, e1, u1, w1);
        if (!(u0 == w1 && w0 == u1)) atomicAdd(&counts[kCntInconsistent], 1u);
        return;
    }
    for (size_t j = 0; j < len; ++j) opp[sorted[p + j]] = MSH_NO_FACE;
    atomicAdd(&counts[len == 1 ? kCntBoundary : kCntNonManifold], 1u);
}

__global__ __launch_bounds__(kBlock) void k_sign_pass(const double* __restrict__ fn, const double* __restrict__ vpn,
                                                      const uint32_t* __restrict__ opp, const uint32_t* __restrict__ tf,
                                                      size_t T, size_t P, const double* __restrict__ q, size_t S,
                                                      const uint32_t* __restrict__ face, const uint32_t* __restrict__ part,
                                                      const double* __restrict__ pt, double* __restrict__ sdist) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= S) return;
    const size_t t = face[i];
    if (t >= T) {
        sdist[i] = NAN;
        return;
    }
    const uint32_t pc = part[i];
    const double dx = q[3 * i] - pt[3 * i], dy = q[3 * i + 1] - pt[3 * i + 1], dz = q[3 * i + 2] - pt[3 * i + 2];
    double nx = fn[3 * t], ny = fn[3 * t + 1], nz = fn[3 * t + 2];
    if (pc >= 1u && pc <= 3u) {
        const size_t o = opp[3 * t + (pc - 1u)];
        if (o < T) {
            nx += fn[3 * o];
            ny += fn[3 * o + 1];
            nz += fn[3 * o + 2];
        }
    } else if (pc >= 4u && pc <= 6u) {
        const size_t vi = tf[3 * t + (pc - 4u)];
        if (vi < P) {
            nx = vpn[3 * vi];
            ny = vpn[3 * vi + 1];
            nz = vpn[3 * vi + 2];
        }
    }
    const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
    const double side = (dx * nx + dy * ny) + dz * nz;
    sdist[i] = side < 0.0 ? -dist : dist;
}

static int bits_upto(size_t P) {  // keys are <= P (P marks an out-of-range index)
    int bits = 1;
    while (bits < 32 && ((size_t)1 << bits) <= P) ++bits;
    return bits;
}

int sign_table_build(const msh_tree* tree, const uint32_t* d_f, void* block, uint32_t* d_counts, Workspace& ws,
                     hipStream_t s) {
    const size_t T = tree->T, P = tree->P, n = 3 * T;
    if (T == 0 || n > 0xFFFFFFFFull || P > 0xFFFFFFFEull) {
        set_error("sign table: %zu faces / %zu vertices are outside the 32-bit index range", T, P);
        return MSH_EINVAL;
    }
    TimedLaunch tl("sign_build", s);
    const SignTable tab = sign_table_of(block, P, T);
    double* fn = const_cast<double*>(tab.fn);
    double* vpn = const_cast<double*>(tab.vpn);
    uint32_t* opp = const_cast<uint32_t*>(tab.opp);
    MSH_TRY(ws.out_d.reserve(n * sizeof(double)));  // corner angles (T,3)
    MSH_TRY(ws.keys.reserve(n * sizeof(uint32_t)));
    MSH_TRY(ws.vals.reserve(n * sizeof(uint32_t)));
    MSH_TRY(ws.keys_alt.reserve(n * sizeof(uint32_t)));
    MSH_TRY(ws.vals_alt.reserve(n * sizeof(uint32_t)));
    double* ang = ws.out_d.as<double>();
    uint32_t* keys = ws.keys.as<uint32_t>();
    uint32_t* vals = ws.vals.as<uint32_t>();
    MSH_HIP(hipMemsetAsync(fn, 0, (T + P) * 3 * sizeof(double), s));  // fn and vpn are adjacent
    MSH_HIP(hipMemsetAsync(ang, 0, n * sizeof(double), s));
    MSH_HIP(hipMemcpyAsync(const_cast<uint32_t*>(tab.f), d_f, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    k_sign_faces<<<blocks_for(T), kBlock, 0, s>>>(static_cast<const TriRec*>(tree->d_leaves), tree->d_v, P, d_f, T, fn, ang,
                                            d_counts);
    MSH_HIP(hipGetLastError());
    const int bits = bits_upto(P);
    // vertex pseudonormals
    k_sign_corner_keys<<<blocks_for(n), kBlock, 0, s>>>(d_f, n, P, keys, vals);
    MSH_HIP(hipGetLastError());
    MSH_TRY(radix_sort_pairs(keys, vals, ws.keys_alt.as<uint32_t>(), ws.vals_alt.as<uint32_t>(), n, bits, ws, s));
    k_sign_vertex<<<blocks_for(n), kBlock, 0, s>>>(keys, vals, n, P, fn, ang, vpn);
    MSH_HIP(hipGetLastError());
    // edge adjacency
    k_sign_edge_max<<<blocks_for(n), kBlock, 0, s>>>(d_f, n, P, keys, vals);
    MSH_HIP(hipGetLastError());
    MSH_TRY(radix_sort_pairs(keys, vals, ws.keys_alt.as<uint32_t>(), ws.vals_alt.as<uint32_t>(), n, bits, ws, s));
    k_sign_edge_min<<<blocks_for(n), kBlock, 0, s>>>(d_f, n, P, vals, keys);
    MSH_HIP(hipGetLastError());
    MSH_TRY(radix_sort_pairs(keys, vals, ws.keys_alt.as<uint32_t>(), ws.vals_alt.as<uint32_t>(), n, bits, ws, s));
    k_sign_edge_runs<<<blocks_for(n), kBlock, 0, s>>>(d_f, n, vals, opp, d_counts);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int launch_sign_pass(const SignTable& tab, size_t T, size_t P, const double* d_q, size_t S, const uint32_t* d_face,
                     const uint32_t* d_part, const double* d_pt, double* d_sdist, hipStream_t s) {
    if (S == 0) return MSH_OK;
    TimedLaunch tl("sign_pass", s);
    k_sign_pass<<<blocks_for(S), kBlock, 0, s>>>(tab.fn, tab.vpn, tab.opp, tab.f, T, P, d_q, S, d_face, d_part, d_pt, d_sdist);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

}  // namespace msh
