// Ray casting for arbitrary rays: first hit (msh_tree_raycast) and occlusion (msh_tree_occluded) on plain triangle
// trees.  No reference counterpart; the predicate and the hit point are the ones nearest_alongnormal and visibility
// use (rays.h ray_tri, cgal_plane_line), so the two are special cases of these queries (include/meshsearch.h).
//
// Row i is an origin o, a direction d (any non-zero length, used as given) and a closed range [t0, t1] of the
// parameter t of o + t d (t0 < 0 is taken as 0).  Leaf triangle j is a hit when ray_tri(o, d, a, b, c) reports a proper
// hit at t_j = num / den within the range, or a coplanar overlap whose interval, clipped starting from [t0, t1], is not
// empty (t_j: its lower end).  First hit: the lexicographic minimum of (t_j, face id).  Occlusion: is the hit set
// non-empty.  A row that cannot be cast (non-finite o or d, d = 0, NaN in the range, t0 > t1) is a miss.
//
// Execution shape: k_raycast<ANY, STATS>, one lane per ray over 64-slot tiles, persistent blocks and k_rays' tile queue,
// the plain walk traverse_rays from the root.  Rays run in the slot order sort_queries gives for their origins (stable:
// the rays of a pinhole camera share one origin and keep the caller's raster order); each lane reads o, d and its range
// at the caller's row perm[slot] and stores its answers to that row, so a row's answer depends on the tree and the row
// alone.
//
// First-hit pruning: with L = |d| the fp32 model's parameter is s = t L.  A child's key (common.h ray_child_first_key)
// is a lower bound of s* = t* L over the real hits inside it; a child or a stack entry is kept iff key <= lim, lim =
// best_t L (1 + 2^-40) rounded up to fp32 (+inf before the first hit).  A hit that would replace the best one, ties on
// t with a smaller face id included, has t_j <= best_t, so key <= t_j L <= lim: the comparison is <=.
#include "knn.h"
#include "rays.h"

namespace msh {

// first hit in [t0, t1]; key = ray_child_first_key
struct FirstPol {
    const TriRec* __restrict__ tris;
    D3 o, d;
    double t0, t1, L;
    RayF rf;
    double best_t;
    uint32_t best_face;
    int best_leaf;  // pt and w are rebuilt from it after the walk (finish), not carried through it
    float limf;
    __device__ void relim() {
        const double s = best_t * L * kSlack;
        limf = rf.wide || !(s == s) ? INFINITY : __double2float_ru(s);
    }
    __device__ void children(const NodeV& nd, bool& h0, bool& h1, float& k0, float& k1) const {
        ray_child_first_key(nd, rf, h0, h1, k0, k1);
        h0 = h0 && k0 <= limf;
        h1 = h1 && k1 <= limf;
    }
    __device__ bool keep(float key) const { return key <= limf; }
    __device__ bool done() const { return false; }
    __device__ void test(int leaf) {
        D3 a, b, c;
        uint32_t face;
        load_tri(tris, leaf, a, b, c, face);
        double t;
        if (!ray_tri(o, d, a, b, c, t, t0, t1) || t != t) return;
        if (t < best_t || (t == best_t && face < best_face)) {
            best_t = t;
            best_face = face;
            best_leaf = leaf;
            relim();
        }
    }
    // the winning hit's point (alongnormal's construction) and its barycentric weights
    __device__ void finish(D3& pt, D3& w) const {
        pt = w = D3{NAN, NAN, NAN};
        if (best_leaf < 0) return;
        D3 a, b, c;
        uint32_t face;
        load_tri(tris, best_leaf, a, b, c, face);
        double t;
        const int kind = ray_tri(o, d, a, b, c, t, t0, t1);
        if (kind == 2 || !cgal_plane_line(o, d, a, b, c, pt)) pt = vadd(o, vscale(t, d));
        w = heidrich_bary(pt, a, b, c);
    }
};

// any hit in [t0, t1] (AnyPol with the range); key = entry parameter
struct AnyRangePol {
    const TriRec* __restrict__ tris;
    D3 o, d;
    double t0, t1;
    RayF rf;
    bool hit;
    __device__ void children(const NodeV& nd, bool& h0, bool& h1, float& k0, float& k1) const {
        ray_child_slabs(nd, rf, h0, h1, k0, k1);
    }
    __device__ bool keep(float) const { return !hit; }
    __device__ bool done() const { return hit; }
    __device__ void test(int leaf) {
        D3 a, b, c;
        uint32_t face;
        load_tri(tris, leaf, a, b, c, face);
        double t;
        if (ray_tri(o, d, a, b, c, t, t0, t1) && t == t) hit = true;
    }
};

struct RcArgs {
    const BNode* nodes;
    const TriRec* tris;
    size_t T;
    const double* o;       // the caller's rows
    const double* d;
    const double* range;   // (S,2) or nullptr: [0, +inf]
    size_t S;
    const uint32_t* perm;  // slot -> caller's row, nullptr: identity
    double* out_t;
    uint32_t* out_face;
    double* out_pt;  // nullable
    double* out_w;   // nullable
    uint8_t* out_hit;
    unsigned long long* stats;  // STATS launches: [0] nodes loaded, [1] leaf tests (outputs not written)
    unsigned* counters;
    unsigned ntiles;
    uint2* spill;
    int spill_depth;
    double org[3];
    double M;
};

// Both policies keep the plain walk traverse_rays with kStack LDS entries and no node slots.  For first hits alongnormal's
// form (rays.hip traverse_along_pend without the entry cut's phase: postponed leaf tests, the node prefetch into LDS, 48
// KB of LDS per block and 3 waves per SIMD) measured 3.56-3.58 against 2.92-2.93 ms on C5's 10M +n rays
// (profiles/raycast_walk_ab.jsonl): a ray tests 1.04 leaves, so there is little leaf work to gather into wave-wide rounds.
// 4 waves per SIMD: 123 (first hit) and 120 (occlusion) VGPRs, no scratch (DESIGN §16 has the table).
template <bool ANY, bool STATS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_raycast(RcArgs a) {
    unsigned n_nodes = 0, n_leaves = 0;
    __shared__ uint2 stk[kStack * kBlock];
    const int tid = threadIdx.x, lane = tid & 63;
    uint2* lds = stk + tid;
    uint2* spill = a.spill ? a.spill + (size_t)blockIdx.x * kBlock * (size_t)a.spill_depth + tid : nullptr;
    const unsigned group = blockIdx.x & 7u;
    const D3 org = D3{a.org[0], a.org[1], a.org[2]};
    const unsigned glo = (unsigned)(((unsigned long long)a.ntiles * group) >> 3);
    const unsigned ghi = (unsigned)(((unsigned long long)a.ntiles * (group + 1)) >> 3);
    unsigned nxt = ~0u;
    for (;;) {
        unsigned tile = 0;
        if (lane == 0) tile = (nxt != ~0u && glo + nxt < ghi) ? glo + nxt : dequeue_tile(a.counters, a.ntiles, group);
        tile = __shfl(tile, 0);
        if (tile >= a.ntiles) break;
        const size_t i = (size_t)tile * 64 + lane;
        if (lane == 0) nxt = glo < ghi ? atomicAdd(&a.counters[group * 32], 1u) : ~0u;
        if (i >= a.S) continue;
        const size_t r = a.perm ? (size_t)a.perm[i] : i;  // the caller's row
        const D3 o = D3{a.o[3 * r], a.o[3 * r + 1], a.o[3 * r + 2]};
        const D3 d = D3{a.d[3 * r], a.d[3 * r + 1], a.d[3 * r + 2]};
        double t0 = a.range ? a.range[2 * r] : 0.0;
        const double t1 = a.range ? a.range[2 * r + 1] : INFINITY;
        // rows that cannot be cast are misses (t0 <= t1 is false for a NaN in the range)
        const bool go = finite3(o) && finite3(d) && (d.x != 0.0 || d.y != 0.0 || d.z != 0.0) && t0 <= t1;
        t0 = fmax(t0, 0.0);
        double L = 0.0;
        const RayF rf = make_rayf_range(vsub(o, org), d, a.M, t0, t1, &L);
        if constexpr (ANY) {
            AnyRangePol pol{a.tris, o, d, t0, t1, rf, false};
            if (go) traverse_rays<AnyRangePol, STATS>(a.nodes, a.T, pol, lds, spill, n_nodes, n_leaves);
            if (STATS) continue;
            a.out_hit[r] = pol.hit ? 1 : 0;
        } else {
            FirstPol pol{a.tris, o, d, t0, t1, L, rf, INFINITY, MSH_NO_FACE, -1, INFINITY};
            if (go) traverse_rays<FirstPol, STATS>(a.nodes, a.T, pol, lds, spill, n_nodes, n_leaves);
            if (STATS) continue;
            a.out_t[r] = pol.best_t;  // scattered stores to the caller's row
            a.out_face[r] = pol.best_face;
            if (a.out_pt || a.out_w) {
                D3 pt, w;
                pol.finish(pt, w);
                if (a.out_pt) {
                    a.out_pt[3 * r] = pt.x;
                    a.out_pt[3 * r + 1] = pt.y;
                    a.out_pt[3 * r + 2] = pt.z;
                }
                if (a.out_w) {
                    a.out_w[3 * r] = w.x;
                    a.out_w[3 * r + 1] = w.y;
                    a.out_w[3 * r + 2] = w.z;
                }
            }
        }
    }
    if (STATS) {
        atomicAdd(&a.stats[0], (unsigned long long)n_nodes);
        atomicAdd(&a.stats[1], (unsigned long long)n_leaves);
    }
}

template <bool ANY, bool STATS>
static int launch_rc(msh_tree* tree, RcArgs a, hipStream_t s) {
    if (a.S == 0) return MSH_OK;
    for (int k = 0; k < 3; ++k) a.org[k] = tree->origin[k];
    a.M = tree->half_diag;
    a.ntiles = (unsigned)((a.S + 63) / 64);  // S <= 2^32 - 1 (the entry points' check_count)
    const unsigned nblk = persistent_blocks(tree->device, (a.ntiles + 3) / 4, 5);
    MSH_TRY(tree->ws.counters.reserve(9 * 32 * sizeof(unsigned)));
    a.counters = tree->ws.counters.as<unsigned>();
    MSH_HIP(hipMemsetAsync(a.counters, 0, 8 * 32 * sizeof(unsigned), s));
    MSH_TRY(plan_spill(tree->ws, tree->max_depth + 1, kStack, nblk, &a.spill, &a.spill_depth));
    TimedLaunch tl(STATS ? (ANY ? "occluded_stats" : "raycast_stats") : (ANY ? "occluded" : "raycast"), s);
    k_raycast<ANY, STATS><<<nblk, kBlock, 0, s>>>(a);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int launch_raycast(msh_tree* tree, const QueryOrder& ord, const double* d_range, size_t S, const RayOut& o,
                   unsigned long long* d_stats, hipStream_t s) {
    RcArgs a{};
    a.nodes = tree->d_nodes; a.tris = static_cast<const TriRec*>(tree->d_leaves); a.T = tree->T;
    a.o = ord.q; a.d = ord.n; a.range = d_range; a.S = S;
    a.perm = ord.perm;  // rays run in slot order and read and store at the caller's rows
    a.out_t = o.t; a.out_face = o.face; a.out_pt = o.pt; a.out_w = o.w; a.out_hit = o.hit;
    a.stats = d_stats;
    const bool any = o.any;
    if (d_stats) return any ? launch_rc<true, true>(tree, a, s) : launch_rc<false, true>(tree, a, s);
    return any ? launch_rc<true, false>(tree, a, s) : launch_rc<false, false>(tree, a, s);
}

}  // namespace msh
