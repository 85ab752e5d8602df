// Generalised winding numbers of a triangle tree (no reference counterpart): inside / outside on open meshes and soups.
//
// w(q) = (1 / 4 pi) sum over the leaves of the solid angle the triangle subtends at q (Van Oosterom and Strackee 1983):
// 1 inside an outward-oriented closed mesh, 0 outside, fractional near openings.  The exact sum is O(T) per row; the
// walk below replaces far subtrees by their dipole (Barill, Dickson, Schmidt, Levin and Jacobson 2018, "Fast winding
// numbers for soups and clouds"): a subtree whose triangles all lie within r of its area-weighted centroid p subtends
// about (p - q) . N / |p - q|^3 at a query farther than beta r from p, N the sum of its area vectors.
//
//   k_wind_sweep  the table, bottom up from d_nodes alone: launch k computes every internal node of height k (both
//                 children are leaves or carry a stamp < k), its fp64 sums as (child 0's sums) + (child 1's sums), a
//                 leaf's from its own triangle; max_depth launches reach the root.  The association is the tree's: no
//                 float atomics, no prefix differences, the same bytes on every build.
//   k_winding     one lane per row in the closest-point path's slot order; DFS, child 0 before child 1, on the per-lane
//                 LDS stack with global spill; fp64 accumulation in visit order, so a row's answer depends on
//                 (tree, q, beta) alone.  A lane evaluates a leaf when it reaches it.  Postponing leaves until every
//                 walking lane of the wave holds one (as rays.hip traverse_along_pend) ran 4x slower: at 3.5 leaves
//                 in 500 steps per row (C3) a lane waits far longer for its neighbours than the atan2 costs
//                 (DESIGN.md s14).
#include <algorithm>
#include <cmath>

#include "internal.h"

namespace msh {

// Per-lane stack entries held in LDS (4 B each: 12 KB per block at 12); deeper entries spill.  The walk's stack is as
// deep as the number of child-0 turns on the path to the current node.
#ifndef MSH_WIND_STACK
#define MSH_WIND_STACK 12
#endif
constexpr int kWindStack = MSH_WIND_STACK;
int winding_stack_lds() { return kWindStack; }

// fp64 sums of a subtree, relative to the tree's origin: area vectors, area-weighted centroids, area, vertex box
struct WindSum {
    double n[3], c[3], area, lo[3], hi[3];
};

__device__ inline WindSum wind_leaf_sum(const TriRec* __restrict__ tris, int leaf, const D3& org) {
    D3 a, b, c;
    uint32_t face;
    load_tri(tris, leaf, a, b, c, face);
    a = vsub(a, org);
    b = vsub(b, org);
    c = vsub(c, org);
    const D3 x = vcross(vsub(b, a), vsub(c, a));
    WindSum s;
    s.n[0] = 0.5 * x.x;
    s.n[1] = 0.5 * x.y;
    s.n[2] = 0.5 * x.z;
    s.area = sqrt((s.n[0] * s.n[0] + s.n[1] * s.n[1]) + s.n[2] * s.n[2]);
    s.c[0] = s.area * (((a.x + b.x) + c.x) / 3.0);
    s.c[1] = s.area * (((a.y + b.y) + c.y) / 3.0);
    s.c[2] = s.area * (((a.z + b.z) + c.z) / 3.0);
    s.lo[0] = fmin(fmin(a.x, b.x), c.x);
    s.lo[1] = fmin(fmin(a.y, b.y), c.y);
    s.lo[2] = fmin(fmin(a.z, b.z), c.z);
    s.hi[0] = fmax(fmax(a.x, b.x), c.x);
    s.hi[1] = fmax(fmax(a.y, b.y), c.y);
    s.hi[2] = fmax(fmax(a.z, b.z), c.z);
    return s;
}

// One record per internal node, 32 B (two 16-B loads): the dipole of its subtree in fp32, relative to the tree's
// origin.  r bounds the distance from the stored (rounded) p to every vertex of the subtree: the distance to the
// farthest corner of the subtree's fp64 vertex box, rounded up.
struct alignas(16) WindRec {
    float p[3], r;
    float n[3], pad;
};
static_assert(sizeof(WindRec) == kWindRecBytes, "WindRec must be 32 B");

__device__ inline WindRec wind_record(const WindSum& s) {
    WindRec rec;
    double p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = s.c[k] / s.area;
        // no area (or an overflowed one): the box centre
        if (!(s.area > 0.0) || !(fabs(p[k]) < INFINITY)) p[k] = 0.5 * s.lo[k] + 0.5 * s.hi[k];
        rec.p[k] = (float)p[k];
        rec.n[k] = (float)s.n[k];
    }
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double d = fmax(fabs((double)rec.p[k] - s.lo[k]), fabs(s.hi[k] - (double)rec.p[k]));
        r2 += d * d;
    }
    rec.r = f32_up(sqrt(r2) * kSlack);  // NaN (non-finite vertices) never passes the walk's test: the node is opened
    rec.pad = 0.f;
    return rec;
}

// err: bit 0 = a child reference outside the tree
__global__ __launch_bounds__(kBlock) void k_wind_sweep(const BNode* __restrict__ nodes, const TriRec* __restrict__ tris,
                                                       size_t T, D3 org, uint32_t k, WindSum* __restrict__ sums,
                                                       uint32_t* __restrict__ stamp, WindRec* __restrict__ recs,
                                                       uint32_t* __restrict__ err) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= T - 1 || stamp[i] != 0u) return;
    const int2 ch = *reinterpret_cast<const int2*>(&nodes[i].f[6]);
    const int c[2] = {ch.x, ch.y};
    WindSum s[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (c[j] >= 0) {
            if ((size_t)c[j] >= T - 1) {
                atomicOr(err, 1u);
                return;
            }
            // a stamp of this launch may appear while its sums are still on their way: only earlier launches count
            const uint32_t st = stamp[c[j]];
            if (st == 0u || st >= k) return;
            s[j] = sums[c[j]];
        } else {
            if ((size_t)~c[j] >= T) {
                atomicOr(err, 1u);
                return;
            }
            s[j] = wind_leaf_sum(tris, ~c[j], org);
        }
    }
    WindSum o;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        o.n[d] = s[0].n[d] + s[1].n[d];
        o.c[d] = s[0].c[d] + s[1].c[d];
        o.lo[d] = fmin(s[0].lo[d], s[1].lo[d]);
        o.hi[d] = fmax(s[0].hi[d], s[1].hi[d]);
    }
    o.area = s[0].area + s[1].area;
    sums[i] = o;
    recs[i] = wind_record(o);
    stamp[i] = k;
}

int winding_table_build(const msh_tree* tree, void* block, uint32_t* d_err, Workspace& ws, hipStream_t s) {
    const size_t T = tree->T;
    if (T < 2 || !tree->d_nodes || T > 0x7FFFFFFFull) {
        set_error("winding table: a tree of %zu leaves has no internal nodes to describe", T);
        return MSH_EINVAL;
    }
    TimedLaunch tl("winding_build", s);
    const size_t n = T - 1;
    MSH_TRY(ws.out_d.reserve(n * sizeof(WindSum)));
    MSH_TRY(ws.flags.reserve((n + 1) * sizeof(uint32_t)));
    WindSum* sums = ws.out_d.as<WindSum>();
    uint32_t* stamp = ws.flags.as<uint32_t>();
    MSH_HIP(hipMemsetAsync(stamp, 0, (n + 1) * sizeof(uint32_t), s));
    MSH_HIP(hipMemsetAsync(block, 0, n * sizeof(WindRec), s));
    const D3 org = D3{tree->origin[0], tree->origin[1], tree->origin[2]};
    // a node of height h is computed by launch h; the root's height is the deepest leaf's depth (<= max_depth)
    const int levels = std::max(tree->max_depth, 1);
    for (int k = 1; k <= levels; ++k) {
        k_wind_sweep<<<blocks_for(n), kBlock, 0, s>>>(tree->d_nodes, static_cast<const TriRec*>(tree->d_leaves), T, org,
                                                      (uint32_t)k, sums, stamp, static_cast<WindRec*>(block), d_err);
        MSH_HIP(hipGetLastError());
    }
    // d_err[1] = the root's stamp (0: the sweeps did not reach it)
    MSH_HIP(hipMemcpyAsync(d_err + 1, stamp, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return MSH_OK;
}

// ---- the walk ----
struct WindArgs {
    const BNode* nodes;
    const WindRec* recs;
    const TriRec* tris;
    size_t T;
    const double* q;
    const uint32_t* perm;  // slot -> caller's row (nullptr: identity)
    size_t S;
    double beta;
    double* w;
    double org[3];
    uint2* spill;
    int spill_depth;
    int cap;                    // stack entries a lane may hold (LDS + spill)
    unsigned long long* stats;  // STATS launches: [0] approximated, [1] opened, [2] leaves, [3] deepest stack
};

// solid angle of (a, b, c) at q (Van Oosterom and Strackee); 0 where q is a corner (atan2(0, 0))
__device__ inline double wind_omega(const TriRec* __restrict__ tris, int leaf, const D3& q) {
    D3 a, b, c;
    uint32_t face;
    load_tri(tris, leaf, a, b, c, face);
    a = vsub(a, q);
    b = vsub(b, q);
    c = vsub(c, q);
    const double la = sqrt(vdot(a, a)), lb = sqrt(vdot(b, b)), lc = sqrt(vdot(c, c));
    const double num = vdot(a, vcross(b, c));
    const double den = la * lb * lc + vdot(a, b) * lc + vdot(b, c) * la + vdot(c, a) * lb;
    return 2.0 * atan2(num, den);
}

// The node step runs in fp32 -- the record is fp32 and the dipole's own error is ~1e-3 of its value --: the far test,
// the dipole and v_rsq_f32 for |p - q|^-3; only the sum is fp64.  (In fp64, with a divide and a square root per
// dipole, the walk ran 10 % slower on C3 and 16 % on C2 with the same errors to six digits)
template <bool STATS>
__global__ __launch_bounds__(kBlock) void k_winding(WindArgs a) {
    __shared__ uint32_t stk[kWindStack * kBlock];
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t* lds = stk + tid;
    uint2* spill = a.spill ? a.spill + (size_t)blockIdx.x * kBlock * (size_t)a.spill_depth + tid : nullptr;
    const D3 org = D3{a.org[0], a.org[1], a.org[2]};
    const bool exact = a.beta == 0.0;
    const size_t ntiles = (a.S + 63) / 64, nwaves = (size_t)gridDim.x * (kBlock / 64);
    unsigned long long n_far = 0, n_open = 0, n_leaf = 0, deepest = 0;
    // waves are independent (no block barrier): each takes every nwaves-th tile of 64 slots
    for (size_t tile = (size_t)blockIdx.x * (kBlock / 64) + (tid >> 6); tile < ntiles; tile += nwaves) {
        const size_t i = tile * 64 + lane;
        const bool live = i < a.S;
        size_t r;  // the caller's row
        const D3 q = load_slot_row(a.q, a.perm, i, live, r);
        const bool fin = live && finite3(q);
        const D3 qr = vsub(q, org);
        const float qx = (float)qr.x, qy = (float)qr.y, qz = (float)qr.z, beta = (float)a.beta;
        double acc = 0.0;  // solid angle, in visit order
        int cur = a.T == 1 ? -1 : 0, sp = 0;  // a tree of one leaf has no internal node
        bool active = fin;
        const size_t steps = 2 * a.T + 2;  // a walk visits every node at most once
        size_t guard = 0;
        while (__ballot(active) != 0ull) {
            if (!active) continue;
            if (++guard > steps) {  // a reference cycle (a corrupt tree): no answer
                acc = NAN;
                active = false;
                continue;
            }
            bool pop = true;
            if (cur < 0) {
                acc += wind_omega(a.tris, ~cur, q);
                if (STATS) ++n_leaf;
            } else {
                const float4* rp = reinterpret_cast<const float4*>(a.recs + cur);
                const float4 r0 = rp[0], r1 = rp[1];
                // beta r of inf x 0 or a NaN radius is NaN: not far, the node is opened
                const float dx = r0.x - qx, dy = r0.y - qy, dz = r0.z - qz;
                const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
                const float br = beta * r0.w;
                const bool far = !exact && d2 > br * br;
                if (far) {
                    const float rs = __builtin_amdgcn_rsqf(d2);  // v_rsq_f32, 1 ulp
                    acc += (double)(fmaf(r1.x, dx, fmaf(r1.y, dy, r1.z * dz)) * (rs * rs * rs));
                    if (STATS) ++n_far;
                } else {
                    const int2 ch = *reinterpret_cast<const int2*>(&a.nodes[cur].f[6]);
                    if (STATS) ++n_open;
                    if (sp >= a.cap) {  // deeper than the tree's recorded depth: no answer rather than a stray store
                        acc = NAN;
                        active = false;
                        continue;
                    }
                    stack_put<kWindStack>(lds, spill, sp, (uint32_t)ch.y);
                    ++sp;
                    if (STATS && (unsigned long long)sp > deepest) deepest = (unsigned long long)sp;
                    cur = ch.x;
                    pop = false;
                }
            }
            if (pop) {
                if (sp == 0) {
                    active = false;
                } else {
                    --sp;
                    cur = (int)stack_get<kWindStack>(lds, spill, sp);
                }
            }
        }
        if (!STATS && live) a.w[r] = fin ? acc * 0.07957747154594767 : NAN;  // 1 / (4 pi)
    }
    if (STATS) flush_stats4(a.stats, n_far, n_open, n_leaf, deepest);
}

template <bool STATS>
static int launch_wind(msh_tree* tree, const void* table, const QueryOrder& ord, size_t S, double beta, double* d_w,
                       unsigned long long* d_stats, hipStream_t s) {
    if (S == 0) return MSH_OK;
    WindArgs a{};
    a.nodes = tree->d_nodes;
    a.recs = static_cast<const WindRec*>(table);
    a.tris = static_cast<const TriRec*>(tree->d_leaves);
    a.T = tree->T;
    a.q = ord.q;  // the caller's rows: each lane reads row perm[slot] and stores its answer there
    a.perm = ord.perm;
    a.S = S;
    a.beta = beta;
    a.w = d_w;
    a.stats = d_stats;
    for (int k = 0; k < 3; ++k) a.org[k] = tree->origin[k];
    // persistent grid: 8 blocks per CU at most (8 KB of LDS each), every wave strides over the tiles
    const unsigned nb = persistent_blocks(tree->device, blocks_for(S), 8);
    MSH_TRY(plan_spill(tree->ws, tree->max_depth + 1, kWindStack, nb, &a.spill, &a.spill_depth));
    a.cap = kWindStack + a.spill_depth;
    if (STATS) {
        k_winding<true><<<nb, kBlock, 0, s>>>(a);
    } else {
        TimedLaunch tl("winding", s);
        k_winding<false><<<nb, kBlock, 0, s>>>(a);
    }
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int launch_winding(msh_tree* tree, const void* table, const QueryOrder& ord, size_t S, double beta, double* d_w,
                   hipStream_t s) {
    return launch_wind<false>(tree, table, ord, S, beta, d_w, nullptr, s);
}

int launch_winding_stats(msh_tree* tree, const void* table, const QueryOrder& ord, size_t S, double beta,
                         unsigned long long* d_counts, hipStream_t s) {
    return launch_wind<true>(tree, table, ord, S, beta, nullptr, d_counts, s);
}

}  // namespace msh
