// K6 — triangle/triangle any-hit against the LBVH.
//   * aabbtree_intersections_indices (spatialsearchmodule.cpp:326-417; CGAL do_intersect(Triangle_3)):
//     one lane per query-mesh triangle, flag = 1 iff it touches any mesh triangle (closed test).
//   * aabbtree_n_selfintersects (aabb_normals.cpp:192-207, AABB_n_tree.h:107-116): one lane per mesh
//     triangle, pairs sharing an exactly equal vertex coordinate are skipped.
// K6b -- the same traversal without the early exit, for the pair lists (msh_tree_intersection_pairs,
// msh_tree_self_intersection_pairs; no reference counterpart).  One kernel, k_tritri_all, walks for all of them: its
// any-hit mode is K6, its count and fill modes are K6b.
// The overlap test is the orientation-predicate test of Guigue & Devillers (2003) evaluated in fp64,
// with a 2-D edge/containment test for the coplanar case.  Boxes: closed fp64 separating-axis test of
// the triangle against each child's outward-rounded oriented box, on the node frame's three axes.
#include <algorithm>

#include "internal.h"

namespace msh {

__device__ inline bool seg_seg_2d(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) {
    auto o2 = [](double px, double py, double qx, double qy, double rx, double ry) {
        return (qx - px) * (ry - py) - (qy - py) * (rx - px);
    };
    const double o1 = o2(ax, ay, bx, by, cx, cy), o2v = o2(ax, ay, bx, by, dx, dy);
    const double o3 = o2(cx, cy, dx, dy, ax, ay), o4 = o2(cx, cy, dx, dy, bx, by);
    if (((o1 > 0 && o2v < 0) || (o1 < 0 && o2v > 0)) && ((o3 > 0 && o4 < 0) || (o3 < 0 && o4 > 0))) return true;
    auto onseg = [](double px, double py, double qx, double qy, double rx, double ry) {
        return fmin(px, qx) <= rx && rx <= fmax(px, qx) && fmin(py, qy) <= ry && ry <= fmax(py, qy);
    };
    if (o1 == 0 && onseg(ax, ay, bx, by, cx, cy)) return true;
    if (o2v == 0 && onseg(ax, ay, bx, by, dx, dy)) return true;
    if (o3 == 0 && onseg(cx, cy, dx, dy, ax, ay)) return true;
    if (o4 == 0 && onseg(cx, cy, dx, dy, bx, by)) return true;
    return false;
}

__device__ inline bool pt_in_tri_2d(double px, double py, const double* t) {
    auto o2 = [](double ax, double ay, double bx, double by, double cx, double cy) {
        return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    };
    const double d0 = o2(t[0], t[1], t[2], t[3], px, py);
    const double d1 = o2(t[2], t[3], t[4], t[5], px, py);
    const double d2 = o2(t[4], t[5], t[0], t[1], px, py);
    return (d0 >= 0 && d1 >= 0 && d2 >= 0) || (d0 <= 0 && d1 <= 0 && d2 <= 0);
}

// Not inlined: the walk calls it (through tri_tri_overlap, which follows it in the code object).  aligned(256): where
// the two start relative to an instruction-cache line shows in a walk of coplanar triangles (300 coincident ones:
// +0.2 % count, +0.6 % fill when three small kernels came to lie before them, at a function's default 4 B).
__device__ __attribute__((aligned(256))) bool coplanar_tri_tri(const D3& p1, const D3& q1, const D3& r1, const D3& p2,
                                                               const D3& q2, const D3& r2, const D3& n) {
    const double ax = fabs(n.x), ay = fabs(n.y), az = fabs(n.z);
    const int drop = (ax > az && ax >= ay) ? 0 : ((ay > az && ay > ax) ? 1 : 2);
    auto pr = [drop](const D3& p, double* o) {
        if (drop == 0) { o[0] = p.y; o[1] = p.z; }
        else if (drop == 1) { o[0] = p.x; o[1] = p.z; }
        else { o[0] = p.x; o[1] = p.y; }
    };
    double t1[6], t2[6];
    pr(p1, t1); pr(q1, t1 + 2); pr(r1, t1 + 4);
    pr(p2, t2); pr(q2, t2 + 2); pr(r2, t2 + 4);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (seg_seg_2d(t1[2 * i], t1[2 * i + 1], t1[(2 * i + 2) % 6], t1[(2 * i + 3) % 6], t2[2 * j], t2[2 * j + 1],
                           t2[(2 * j + 2) % 6], t2[(2 * j + 3) % 6]))
                return true;
    if (pt_in_tri_2d(t1[0], t1[1], t2)) return true;
    if (pt_in_tri_2d(t2[0], t2[1], t1)) return true;
    return false;
}

__device__ inline bool check_min_max(const D3& p1, const D3& q1, const D3& r1, const D3& p2, const D3& q2, const D3& r2) {
    D3 n = vcross(vsub(p2, q1), vsub(p1, q1));
    if (vdot(vsub(q2, q1), n) > 0.0) return false;
    n = vcross(vsub(p2, p1), vsub(r1, p1));
    if (vdot(vsub(r2, p1), n) > 0.0) return false;
    return true;
}

__device__ bool tri_tri_3d(const D3& p1, const D3& q1, const D3& r1, const D3& p2, const D3& q2, const D3& r2, double dp2,
                           double dq2, double dr2, const D3& n1) {
    if (dp2 > 0.0) {
        if (dq2 > 0.0) return check_min_max(p1, r1, q1, r2, p2, q2);
        if (dr2 > 0.0) return check_min_max(p1, r1, q1, q2, r2, p2);
        return check_min_max(p1, q1, r1, p2, q2, r2);
    }
    if (dp2 < 0.0) {
        if (dq2 < 0.0) return check_min_max(p1, q1, r1, r2, p2, q2);
        if (dr2 < 0.0) return check_min_max(p1, q1, r1, q2, r2, p2);
        return check_min_max(p1, r1, q1, p2, q2, r2);
    }
    if (dq2 < 0.0) {
        if (dr2 >= 0.0) return check_min_max(p1, r1, q1, q2, r2, p2);
        return check_min_max(p1, q1, r1, p2, q2, r2);
    }
    if (dq2 > 0.0) {
        if (dr2 > 0.0) return check_min_max(p1, r1, q1, p2, q2, r2);
        return check_min_max(p1, q1, r1, q2, r2, p2);
    }
    if (dr2 > 0.0) return check_min_max(p1, q1, r1, r2, p2, q2);
    if (dr2 < 0.0) return check_min_max(p1, r1, q1, r2, p2, q2);
    return coplanar_tri_tri(p1, q1, r1, p2, q2, r2, n1);
}

__device__ bool tri_tri_overlap(const D3& p1, const D3& q1, const D3& r1, const D3& p2, const D3& q2, const D3& r2) {
    const D3 n2 = vcross(vsub(p2, r2), vsub(q2, r2));
    const double dp1 = vdot(vsub(p1, r2), n2), dq1 = vdot(vsub(q1, r2), n2), dr1 = vdot(vsub(r1, r2), n2);
    if (dp1 * dq1 > 0.0 && dp1 * dr1 > 0.0) return false;
    const D3 n1 = vcross(vsub(q1, p1), vsub(r1, p1));
    const double dp2 = vdot(vsub(p2, r1), n1), dq2 = vdot(vsub(q2, r1), n1), dr2 = vdot(vsub(r2, r1), n1);
    if (dp2 * dq2 > 0.0 && dp2 * dr2 > 0.0) return false;
    if (dp1 > 0.0) {
        if (dq1 > 0.0) return tri_tri_3d(r1, p1, q1, p2, r2, q2, dp2, dr2, dq2, n1);
        if (dr1 > 0.0) return tri_tri_3d(q1, r1, p1, p2, r2, q2, dp2, dr2, dq2, n1);
        return tri_tri_3d(p1, q1, r1, p2, q2, r2, dp2, dq2, dr2, n1);
    }
    if (dp1 < 0.0) {
        if (dq1 < 0.0) return tri_tri_3d(r1, p1, q1, p2, q2, r2, dp2, dq2, dr2, n1);
        if (dr1 < 0.0) return tri_tri_3d(q1, r1, p1, p2, q2, r2, dp2, dq2, dr2, n1);
        return tri_tri_3d(p1, q1, r1, p2, r2, q2, dp2, dr2, dq2, n1);
    }
    if (dq1 < 0.0) {
        if (dr1 >= 0.0) return tri_tri_3d(q1, r1, p1, p2, r2, q2, dp2, dr2, dq2, n1);
        return tri_tri_3d(p1, q1, r1, p2, q2, r2, dp2, dq2, dr2, n1);
    }
    if (dq1 > 0.0) {
        if (dr1 > 0.0) return tri_tri_3d(p1, q1, r1, p2, r2, q2, dp2, dr2, dq2, n1);
        return tri_tri_3d(q1, r1, p1, p2, q2, r2, dp2, dq2, dr2, n1);
    }
    if (dr1 > 0.0) return tri_tri_3d(r1, p1, q1, p2, q2, r2, dp2, dq2, dr2, n1);
    if (dr1 < 0.0) return tri_tri_3d(r1, p1, q1, p2, r2, q2, dp2, dr2, dq2, n1);
    return coplanar_tri_tri(p1, q1, r1, p2, q2, r2, n1);
}

// Interval of the query triangle (vertices relative to the tree origin) along each frame axis, widened
// by a 2^-40 relative margin for the fp64 projections.
struct TriProj {
    double lo[3], hi[3];
};
__device__ inline TriProj tri_proj(const FrameD& f, const D3& a, const D3& b, const D3& c) {
    TriProj r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double pa = vdot(f.a[k], a), pb = vdot(f.a[k], b), pc = vdot(f.a[k], c);
        const double lo = fmin(fmin(pa, pb), pc), hi = fmax(fmax(pa, pb), pc);
        const double m = 9.094947017729282e-13 * (fabs(lo) + fabs(hi)) + 1e-300;
        r.lo[k] = lo - m;
        r.hi[k] = hi + m;
    }
    return r;
}
// separating-axis test on the node frame's three axes: false only if the triangle and the child's oriented
// box are disjoint along one of them
__device__ inline bool obb_overlap(const TriProj& p, const float* ext) {
    return p.lo[0] <= (double)ext[3] && (double)ext[0] <= p.hi[0] && p.lo[1] <= (double)ext[4] &&
           (double)ext[1] <= p.hi[1] && p.lo[2] <= (double)ext[5] && (double)ext[2] <= p.hi[2];
}

// ---- the walk: any hit, or all hits as the (query face, mesh face) pair list ----
// Count, sum, scan, fill, order (DESIGN.md "Intersection pair lists").  k_tritri_all is one depth-first walk in three
// modes.  kTriAny stops at a row's first hit and writes flags (a.counts[i] = 1 or 0, i the query triangle's index).
// kTriCount and kTriFill walk to the end with the same body: the first counts the hits of every row, the second writes
// them at the row's offset.  There a row is the query triangle's index (query mode) or its face id (self mode: the
// queries are the tree's own leaves, in leaf order; only leaves of a larger face id are kept, so every pair appears
// once, under its smaller face, and the predicate gets the smaller face first; the any-hit mode keeps every leaf, since
// a face is flagged whatever the id order).  Nothing but a row's own lane writes its count or its segment, so the
// output does not depend on how lanes are scheduled.
enum { kTriAny = 0, kTriCount = 1, kTriFill = 2 };

struct PairArgs {
    const BNode* nodes;
    const TriRec* tris;
    size_t T;
    const TriRec* q;
    size_t Tq;
    int self_mode;
    uint32_t* counts;         // per row; written by the any-hit (flags) and the count pass, read by the fill pass
    const uint32_t* offsets;  // exclusive scan of counts (fill pass)
    uint32_t* ids;            // fill pass: mesh face of pair offsets[row] + k ...
    uint32_t* rows;           // ... and its row (nullptr when the lanes order their own rows)
    uint32_t* pairs;          // fill pass, every row <= kLaneSort hits: the output (n_emit, 2); else nullptr
    size_t n_emit;
    uint2* spill;
    int spill_depth;
    double org[3];  // tree origin
};

// self mode's filter: do the two triangles share an exactly equal vertex coordinate
__device__ inline bool shares_vertex(const D3& qa, const D3& qb, const D3& qc, const D3& a0, const D3& a1, const D3& a2) {
    return veq(qa, a0) || veq(qa, a1) || veq(qa, a2) || veq(qb, a0) || veq(qb, a1) || veq(qb, a2) || veq(qc, a0) ||
           veq(qc, a1) || veq(qc, a2);
}

// waves_per_eu(3): the any-hit walk's occupancy (162 VGPRs); without the hint the fill pass took 169, one over the step
// to 2 waves.  The modes differ by constexpr conditions inside the one body: the walk handed to the modes as a function
// template over test / done lambdas compiled to 173 VGPRs (any hit) and 10 / 22 spilled ones (count / fill).
template <int kMode>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void k_tritri_all(PairArgs a) {
    constexpr bool kAny = kMode == kTriAny, kFill = kMode == kTriFill;
    __shared__ uint2 stk[kStack * kBlock];
    const int tid = threadIdx.x;
    uint2* lds = stk + tid;
    for (size_t i = (size_t)blockIdx.x * kBlock + tid; i < a.Tq; i += (size_t)gridDim.x * kBlock) {
        uint2* spill = a.spill ? a.spill + (size_t)blockIdx.x * kBlock * (size_t)a.spill_depth + tid : nullptr;
        D3 qa, qb, qc;
        uint32_t qface;
        load_tri(a.q, (int)i, qa, qb, qc, qface);
        const uint32_t row = !kAny && a.self_mode ? qface : (uint32_t)i;
        // fill pass: this row's segment is [base, base + lim); a row without hits has nothing to walk for, and a walk
        // ends with its last hit (the count pass made the same walk to the end and found lim of them)
        uint32_t base = 0;
        uint32_t lim = 0;
        if (kFill) {
            base = a.offsets[row];
            lim = a.counts[row];
            if (lim == 0) continue;
        }
        // query vertices relative to the tree origin (node bounds are origin-relative and padded >= 1 fp32
        // ulp, far above the fp64 rounding of this subtraction)
        const D3 org = D3{a.org[0], a.org[1], a.org[2]};
        const D3 ra = vsub(qa, org), rb = vsub(qb, org), rc = vsub(qc, org);
        uint32_t n = 0;
        auto leaf_test = [&](int leaf) {
            D3 a0, a1, a2;
            uint32_t f;
            load_tri(a.tris, leaf, a0, a1, a2, f);
            if (a.self_mode) {
                if (!kAny && f <= qface) return;
                if (shares_vertex(qa, qb, qc, a0, a1, a2)) return;
            }
            if (!tri_tri_overlap(qa, qb, qc, a0, a1, a2)) return;
            if (kFill && n < lim) {  // never at or beyond the segment's end, whatever the walk meets
                a.ids[(size_t)base + n] = f;
                if (a.rows) a.rows[(size_t)base + n] = row;
            }
            ++n;
        };
        if (a.T == 1) {
            leaf_test(0);
        } else {
            int node = 0, sp = 0;
            for (size_t guard = 0; guard < a.T; ++guard) {
                const NodeV nd = load_node(a.nodes, node);
                float e0[6], e1[6];
                nd.extents(e0, e1);
                const TriProj tp = tri_proj(frame_d(nd), ra, rb, rc);
                bool h0 = obb_overlap(tp, e0);
                bool h1 = obb_overlap(tp, e1);
                const int c0 = nd.child(0), c1 = nd.child(1);
                if (h0 && c0 < 0) { leaf_test(~c0); h0 = false; if (kAny && n) break; }
                if (h1 && c1 < 0) { leaf_test(~c1); h1 = false; if (kAny && n) break; }
                if (kFill && n >= lim) break;
                if (h0 && h1) {
                    const uint2 e = make_uint2((unsigned)c1, 0u);
                    stack_put(lds, spill, sp, e);
                    ++sp;
                    node = c0;
                    continue;
                }
                if (h0) { node = c0; continue; }
                if (h1) { node = c1; continue; }
                if (sp == 0) break;
                --sp;
                node = (int)stack_get(lds, spill, sp).x;
            }
        }
        if (kAny) a.counts[i] = n ? 1u : 0u;
        if (kMode == kTriCount) a.counts[row] = n;
        // Short rows are ordered by their own lane: the face ids of a row are distinct, so pair k of the row is the
        // smallest id above pair k - 1's -- lim^2 reads of the segment the lane has just written, lim <= kLaneSort.
        if (kFill && a.pairs) {
            uint32_t last = 0;
            for (uint32_t k = 0; k < lim && (size_t)base + k < a.n_emit; ++k) {
                uint32_t best = 0xFFFFFFFFu;  // not a face id (ids < 2^31)
                for (uint32_t m = 0; m < lim; ++m) {
                    const uint32_t f = a.ids[(size_t)base + m];
                    if ((k == 0 || f > last) && f < best) best = f;
                }
                a.pairs[2 * ((size_t)base + k)] = row;
                a.pairs[2 * ((size_t)base + k) + 1] = best;
                last = best;
            }
        }
    }
}

// out[0] += the 64-bit sum of counts, out[1] = max(out[1], the largest count) (out zeroed by the caller; an integer sum
// and a maximum, so the order of the blocks' atomic operations does not show in them)
__global__ __launch_bounds__(kBlock) void k_sum_counts(const uint32_t* __restrict__ counts, size_t n,
                                                       unsigned long long* __restrict__ out) {
    __shared__ unsigned long long sh[kBlock], shm[kBlock];
    unsigned long long acc = 0, mx = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const unsigned long long c = counts[i];
        acc += c;
        mx = c > mx ? c : mx;
    }
    sh[threadIdx.x] = acc;
    shm[threadIdx.x] = mx;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh[threadIdx.x] += sh[threadIdx.x + o];
            shm[threadIdx.x] = shm[threadIdx.x + o] > shm[threadIdx.x] ? shm[threadIdx.x + o] : shm[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0]) {
        atomicAdd(out, sh[0]);
        atomicMax(out + 1, shm[0]);
    }
}

int sum_counts(const uint32_t* d_counts, size_t n, unsigned long long* d_out, unsigned nblk, hipStream_t s) {
    k_sum_counts<<<std::max(std::min(nblk, 1024u), 1u), kBlock, 0, s>>>(d_counts, n, d_out);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

// pairs (n, 2) row-major from the sorted (row, mesh face) columns
__global__ __launch_bounds__(kBlock) void k_emit_pairs(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ ids,
                                                       size_t n, uint32_t* __restrict__ pairs) {
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    pairs[2 * p] = rows[p];
    pairs[2 * p + 1] = ids[p];
}

// query triangles from device arrays, in the manner of k_pack_tris; a face with an index >= Pq becomes a zero
// triangle and sets *err (no read outside qv)
__global__ __launch_bounds__(kBlock) void k_pack_query_tris(const double* __restrict__ qv, size_t Pq,
                                                            const uint32_t* __restrict__ qf, size_t Tq,
                                                            TriRec* __restrict__ out, unsigned long long* __restrict__ err) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= Tq) return;
    const size_t i0 = qf[3 * t], i1 = qf[3 * t + 1], i2 = qf[3 * t + 2];
    const bool ok = i0 < Pq && i1 < Pq && i2 < Pq;
    const size_t vi[3] = {i0, i1, i2};
    TriRec r;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) r.v[3 * c + k] = ok ? qv[3 * vi[c] + k] : 0.0;
    r.face = (uint32_t)t;
    r.pad = 0;
    out[t] = r;
    if (!ok) atomicOr(err, 1ull);
}

// persistent grid: 5 blocks per CU at most, every lane strides over the rows
static unsigned pair_blocks(const msh_tree* tree, size_t n) { return persistent_blocks(tree->device, blocks_for(n), 5); }

// the walk's arguments (counts = d_counts) and, for a tree deeper than kStack, its spill area
static int pair_args(msh_tree* t, const TriRec* d_qtris, size_t Tq, int self_mode, unsigned nblk, uint32_t* d_counts,
                     PairArgs* out) {
    PairArgs a{};
    a.nodes = t->d_nodes;
    a.tris = static_cast<const TriRec*>(t->d_leaves);
    a.T = t->T;
    a.q = d_qtris;
    a.Tq = Tq;
    a.self_mode = self_mode;
    for (int k = 0; k < 3; ++k) a.org[k] = t->origin[k];
    a.counts = d_counts;
    MSH_TRY(plan_spill(t->ws, t->max_depth + 1, kStack, nblk, &a.spill, &a.spill_depth));
    *out = a;
    return MSH_OK;
}

int launch_tri_intersect(const msh_tree* tree, const TriRec* d_qtris, size_t Tq, int self_mode, uint32_t* d_flags,
                         hipStream_t s) {
    if (Tq == 0) return MSH_OK;
    const unsigned nblk = pair_blocks(tree, Tq);
    PairArgs a;
    MSH_TRY(pair_args(const_cast<msh_tree*>(tree), d_qtris, Tq, self_mode, nblk, d_flags, &a));
    TimedLaunch tl("tritri", s);
    k_tritri_all<kTriAny><<<nblk, kBlock, 0, s>>>(a);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

// ws.counters of a pair-list call: [0] the 64-bit sum of the counts, [1] the largest count, [2] set by
// k_pack_query_tris when a query face index is out of range
constexpr int kPairWords = 3;

int pack_query_tris(msh_tree* tree, const double* d_qv, size_t Pq, const uint32_t* d_qf, size_t Tq, hipStream_t s) {
    Workspace& ws = tree->ws;
    MSH_TRY(ws.q.reserve(Tq * sizeof(TriRec)));
    MSH_TRY(ws.counters.reserve(kPairWords * sizeof(unsigned long long)));
    MSH_HIP(hipMemsetAsync(ws.counters.ptr, 0, kPairWords * sizeof(unsigned long long), s));
    k_pack_query_tris<<<blocks_for(Tq), kBlock, 0, s>>>(
        d_qv, Pq, d_qf, Tq, ws.q.as<TriRec>(), ws.counters.as<unsigned long long>() + 2);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int launch_tri_pairs_count(msh_tree* tree, const TriRec* d_qtris, size_t Tq, int self_mode, bool packed, PairTotals* out,
                           hipStream_t s) {
    Workspace& ws = tree->ws;
    MSH_TRY(ws.flags.reserve(Tq * sizeof(uint32_t)));
    MSH_TRY(ws.counters.reserve(kPairWords * sizeof(unsigned long long)));
    unsigned long long* d_tot = ws.counters.as<unsigned long long>();
    // pack_query_tris zeroed the words on this stream already, and its kernel may have set the third
    if (!packed) MSH_HIP(hipMemsetAsync(d_tot, 0, kPairWords * sizeof(unsigned long long), s));
    const unsigned nblk = pair_blocks(tree, Tq);
    PairArgs a;
    MSH_TRY(pair_args(tree, d_qtris, Tq, self_mode, nblk, ws.flags.as<uint32_t>(), &a));
    {
        TimedLaunch tl("tritri_count", s);
        k_tritri_all<kTriCount><<<nblk, kBlock, 0, s>>>(a);
        MSH_HIP(hipGetLastError());
    }
    {
        TimedLaunch tl("tritri_scan", s);
        k_sum_counts<<<std::min(nblk, 1024u), kBlock, 0, s>>>(a.counts, Tq, d_tot);
        MSH_HIP(hipGetLastError());
    }
    unsigned long long h[kPairWords] = {0, 0, 0};
    MSH_HIP(hipMemcpyAsync(h, d_tot, sizeof(h), hipMemcpyDeviceToHost, s));
    MSH_HIP(hipStreamSynchronize(s));
    out->K = h[0];
    out->longest = h[1];
    out->bad_face = h[2] != 0;
    return MSH_OK;
}

int launch_tri_pairs_emit(msh_tree* tree, const TriRec* d_qtris, size_t Tq, int self_mode, const PairTotals& tot,
                          uint32_t* d_pairs, size_t n_emit, hipStream_t s) {
    const size_t K = (size_t)tot.K;
    if (K == 0 || n_emit == 0) return MSH_OK;
    Workspace& ws = tree->ws;
    const bool lane_order = tot.longest <= (uint64_t)kLaneSort;
    MSH_TRY(ws.ranges.reserve(Tq * sizeof(uint32_t)));
    MSH_TRY(ws.keys.reserve(K * sizeof(uint32_t)));
    if (!lane_order) {
        MSH_TRY(ws.vals.reserve(K * sizeof(uint32_t)));
        MSH_TRY(ws.keys_alt.reserve(K * sizeof(uint32_t)));
        MSH_TRY(ws.vals_alt.reserve(K * sizeof(uint32_t)));
    }
    const unsigned nblk = pair_blocks(tree, Tq);
    PairArgs a;
    MSH_TRY(pair_args(tree, d_qtris, Tq, self_mode, nblk, ws.flags.as<uint32_t>(), &a));
    uint32_t* offsets = ws.ranges.as<uint32_t>();
    {
        TimedLaunch tl("tritri_scan", s);
        MSH_HIP(hipMemcpyAsync(offsets, a.counts, Tq * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        MSH_TRY(exclusive_scan_u32(offsets, Tq, ws, s));
    }
    a.offsets = offsets;
    a.ids = ws.keys.as<uint32_t>();
    a.rows = lane_order ? nullptr : ws.vals.as<uint32_t>();
    a.pairs = lane_order ? d_pairs : nullptr;
    a.n_emit = n_emit;
    {
        TimedLaunch tl("tritri_fill", s);
        k_tritri_all<kTriFill><<<nblk, kBlock, 0, s>>>(a);
        MSH_HIP(hipGetLastError());
    }
    if (lane_order) return MSH_OK;
    // Long rows: the segments are in row order already; a stable sort of all K pairs by mesh face and then by row
    // leaves them sorted by (row, mesh face), in time linear in K however long a row is.
    TimedLaunch tl("tritri_order", s);
    uint32_t *ids = a.ids, *rows = a.rows, *ids_alt = ws.keys_alt.as<uint32_t>(), *rows_alt = ws.vals_alt.as<uint32_t>();
    bool alt = false;
    MSH_TRY(radix_sort_pairs(ids, rows, ids_alt, rows_alt, K, bits_for(tree->T), ws, s, 0, &alt));
    if (alt) { std::swap(ids, ids_alt); std::swap(rows, rows_alt); }
    alt = false;
    MSH_TRY(radix_sort_pairs(rows, ids, rows_alt, ids_alt, K, bits_for(Tq), ws, s, 0, &alt));
    if (alt) { std::swap(ids, ids_alt); std::swap(rows, rows_alt); }
    k_emit_pairs<<<blocks_for(n_emit), kBlock, 0, s>>>(rows, ids, n_emit, d_pairs);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

}  // namespace msh
