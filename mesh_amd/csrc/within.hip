// All primitives within a radius, on point and plain triangle trees: the per-row counts (msh_points_within_count,
// msh_tree_within_count) and the sorted neighbour lists as CSR (msh_points_within, msh_tree_within).
//
// Row i is a point q_i and a radius r_i (one for all rows, or one per row).  A primitive qualifies when d2 <= r2_i: d2
// the exact fp64 squared distance of the K-nearest queries (knn.h kb_eval), r2_i = r_i * r_i rounded once.  A row with a
// non-finite point or a negative or NaN radius has none.
//
// Count, sum, scan, fill, order, emit -- the protocol of the all-hits ray lists (raycast_all.hip).  k_within is k_kbest's
// walk (one lane per row in the slot order of the rows, depth first from the root, nearer child first, the LDS stack
// with global spill) with a limit that never moves: r2_i * kSlack, so nothing but the radius prunes.  Count mode writes
// counts[r].  Fill mode makes the same walk again and writes (d2, leaf, id) of the n-th primitive met at offsets[r] + n,
// guarded by n < counts[r], and stops at the row's last entry.  Only a row's own lane writes its count and its segment;
// the walk order decides only where in its segment an entry lands, and the order step removes that: entries are sorted
// by (row, d2, id).
//   Short rows (no row above kLaneSort entries): each fill lane orders its own segment by repeated selection.
//   Long rows: order_csr_entries, the radix sorts of the all-hits lists (d2 >= 0 and never NaN in the qualifying set).
// k_within_emit, one thread per written entry, writes id and sqrt(d2), and for a triangle the point and part from the
// stored leaf by k_kbest_finish's construction, which makes a row's first K' entries equal the K'-nearest answer.
#include "knn.h"

namespace msh {

enum { kWithinCount = 0, kWithinFill = 1 };
constexpr unsigned kWithinBlocksPerCU = 4;  // k_kbest's: the stack's 16 or 32 KB of LDS per block would allow more

struct WiArgs {
    const BNode* nodes;
    const void* leaves;
    size_t T;
    const double* q;       // the caller's rows
    const uint32_t* perm;  // slot -> caller's row (nullptr: identity)
    size_t S;
    double r_max;          // the radius of every row when r_rows == nullptr
    const double* r_rows;  // (S,) per caller's row, or nullptr
    double org[3];
    double tm;
    uint2* spill;
    int spill_depth;
    uint32_t* counts;         // per caller's row; written by the count pass, read by the fill pass
    const uint32_t* offsets;  // fill: exclusive scan of counts
    double* ed2;              // fill: (K,) d2, leaf and id of entry offsets[r] + n
    uint32_t* eleaf;
    uint32_t* eid;
    uint32_t* order;  // fill, every row <= kLaneSort entries: order[p] = the entry that comes p-th; else nullptr
    size_t n_emit;    // positions >= n_emit are not ordered
    unsigned long long* stats;  // STATS launches: [0] nodes, [1] primitives, [2] entries, [3] deepest stack
};

// The leaf policy of WalkerT::step: the limit is the row's radius, fixed for the whole walk.
template <bool TRI, bool kFill>
struct WithinPol {
    const void* __restrict__ leaves;
    D3 q;
    double r2;
    float limf;
    uint32_t n, lim;  // qualifying primitives met so far; fill: the row's count
    double* ed2;      // fill: the row's segment
    uint32_t* eleaf;
    uint32_t* eid;
    __device__ double limit() const { return r2 * kSlack; }
    __device__ void relim() { limf = __double2float_ru(limit()); }
    // a fill walk ends with the row's last entry (the count pass made the same walk to the end and found lim of them)
    __device__ bool done() const { return kFill && n >= lim; }
    __device__ void test(int leaf) {
        uint32_t id;
        const double d2 = kb_eval<TRI>(leaves, leaf, q, id);
        if (!(d2 <= r2)) return;
        if (kFill && n < lim) {  // never at or beyond the segment's end, whatever the walk meets
            ed2[n] = d2;
            eleaf[n] = (uint32_t)leaf;
            eid[n] = id;
        }
        ++n;
    }
};

// E: the stack entries (Ent4 for trees of <= 2^20 leaves).  STATS: count mode only, nothing written but the counters.
template <bool TRI, int kMode, class E, bool STATS>
__global__ __launch_bounds__(kBlock) void k_within(WiArgs a) {
    constexpr bool kFill = kMode == kWithinFill;
    typedef typename E::T Ent;
    __shared__ Ent stk[kStack * kBlock];
    const int tid = threadIdx.x, lane = tid & 63;
    Ent* lds = stk + tid;
    uint2* spill = a.spill ? a.spill + (size_t)blockIdx.x * kBlock * (size_t)a.spill_depth + tid : nullptr;
    const double org[3] = {a.org[0], a.org[1], a.org[2]};
    const size_t ntiles = (a.S + 63) / 64, nwaves = (size_t)gridDim.x * (kBlock / 64);
    unsigned n_nodes = 0, n_leaves = 0;
    unsigned long long t_nodes = 0, t_leaves = 0, t_ent = 0, deepest = 0;
    // waves are independent (no block barrier): each takes every nwaves-th tile of 64 slots
    for (size_t tile = (size_t)blockIdx.x * (kBlock / 64) + (tid >> 6); tile < ntiles; tile += nwaves) {
        const size_t i = tile * 64 + lane;
        const bool live = i < a.S;
        size_t r;  // the caller's row
        const D3 q = load_slot_row(a.q, a.perm, i, live, r);
        const double rad = !live ? -1.0 : (a.r_rows ? a.r_rows[r] : a.r_max);
        bool go = live && finite3(q) && rad >= 0.0;  // false for a NaN radius
        size_t base = 0;
        uint32_t lim = 0;
        if (kFill && live) {
            base = a.offsets[r];
            lim = a.counts[r];
            go = go && lim != 0;  // nothing to walk for
        }
        WithinPol<TRI, kFill> pol;
        pol.leaves = a.leaves;
        pol.q = q;
        pol.r2 = rad * rad;
        pol.n = 0;
        pol.lim = lim;
        pol.ed2 = kFill ? a.ed2 + base : nullptr;
        pol.eleaf = kFill ? a.eleaf + base : nullptr;
        pol.eid = kFill ? a.eid + base : nullptr;
        pol.relim();
        if (go) {
            if (a.T == 1) {  // a tree of one leaf has no internal node
                pol.test(0);
                if (STATS) ++n_leaves;
            } else {
                const QF qf = make_qf(q, org, a.tm);
                WalkerT<E> w{0, 0};
                size_t steps = 0;
                // a walk enters a node at most once: more steps than nodes mean a reference cycle (a corrupt tree)
                while (w.template step<decltype(pol), STATS>(a.nodes, qf, pol, lds, spill, n_nodes, n_leaves)) {
                    if (STATS && (unsigned long long)w.sp > deepest) deepest = (unsigned long long)w.sp;
                    if (pol.done() || ++steps >= a.T) break;
                }
            }
        }
        if (STATS) {
            t_nodes += n_nodes;
            t_leaves += n_leaves;
            t_ent += pol.n;
            n_nodes = n_leaves = 0;
        } else if (!kFill) {
            if (live) a.counts[r] = pol.n;
        } else if (a.order) {
            // Short rows are ordered by their own lane: entry k of the row is the smallest (d2, id) above entry k - 1's
            // -- the pairs are distinct within a row because the ids are -- lim^2 reads of the segment the lane has just
            // written, lim <= kLaneSort.
            double last_d = 0.0;
            uint32_t last_i = 0;
            for (uint32_t k = 0; k < lim && base + k < a.n_emit; ++k) {
                double best_d = INFINITY;
                uint32_t best_i = 0xFFFFFFFFu, best_m = 0;  // not an id (ids < 2^32 - 1: MSH_NO_FACE)
                for (uint32_t m = 0; m < lim; ++m) {
                    const double d = a.ed2[base + m];
                    const uint32_t f = a.eid[base + m];
                    const bool above = k == 0 || d > last_d || (d == last_d && f > last_i);
                    if (above && (d < best_d || (d == best_d && f < best_i))) {
                        best_d = d;
                        best_i = f;
                        best_m = m;
                    }
                }
                a.order[base + k] = (uint32_t)(base + best_m);
                last_d = best_d;
                last_i = best_i;
            }
        }
    }
    if (STATS) flush_stats4(a.stats, t_nodes, t_leaves, t_ent, deepest);
}

struct WiEmit {
    const void* leaves;
    const double* q;
    size_t S;
    const uint32_t* offsets;
    const uint32_t* order;  // order[p] = the entry that comes p-th
    const double* ed2;
    const uint32_t* eleaf;
    const uint32_t* eid;
    size_t n;
    WithinOut o;
};

template <bool TRI>
__global__ __launch_bounds__(kBlock) void k_within_emit(WiEmit a) {
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    const size_t e = a.order[p];
    a.o.id[p] = a.eid[e];
    a.o.dist[p] = sqrt(a.ed2[e]);
    if constexpr (TRI) {
        if (!a.o.pt && !a.o.part) return;
        const size_t r = hit_row(a.offsets, a.S, e);
        D3 ta, tb, tc, pt;
        uint32_t face;
        int part = 0;
        load_tri(static_cast<const TriRec*>(a.leaves), (int)a.eleaf[e], ta, tb, tc, face);
        closest_on_triangle(D3{a.q[3 * r], a.q[3 * r + 1], a.q[3 * r + 2]}, ta, tb, tc, pt, part);
        if (a.o.part) a.o.part[p] = (uint32_t)part;
        if (a.o.pt) {
            a.o.pt[3 * p] = pt.x;
            a.o.pt[3 * p + 1] = pt.y;
            a.o.pt[3 * p + 2] = pt.z;
        }
    }
}

static WiArgs within_args(const msh_tree* tree, const QueryOrder& ord, double r_max, const double* d_r, size_t S) {
    WiArgs a{};
    a.nodes = tree->d_nodes;
    a.leaves = tree->d_leaves;
    a.T = tree->T;
    a.q = ord.q;  // the caller's rows: each lane reads row perm[slot]
    a.perm = ord.perm;
    a.S = S;
    a.r_max = r_max;
    a.r_rows = d_r;
    a.tm = tree_margin(tree->half_diag);
    for (int k = 0; k < 3; ++k) a.org[k] = tree->origin[k];
    return a;
}

template <int kMode, bool STATS>
static int launch_walk(msh_tree* tree, WiArgs a, hipStream_t s) {
    const bool tri = tree->kind != kPoints, e4 = tree->T <= kEnt4MaxLeaves;
    const unsigned nb = persistent_blocks(tree->device, blocks_for(a.S), kWithinBlocksPerCU);
    // the depth-first stack holds at most one entry per level of the path to the current node
    MSH_TRY(plan_spill(tree->ws, tree->max_depth + 1, kStack, nb, &a.spill, &a.spill_depth));
    TimedLaunch tl(STATS ? "within_stats" : (kMode == kWithinFill ? "within_fill" : "within_count"), s);
    if (tri) {
        if (e4) k_within<true, kMode, Ent4, STATS><<<nb, kBlock, 0, s>>>(a);
        else k_within<true, kMode, Ent8, STATS><<<nb, kBlock, 0, s>>>(a);
    } else {
        if (e4) k_within<false, kMode, Ent4, STATS><<<nb, kBlock, 0, s>>>(a);
        else k_within<false, kMode, Ent8, STATS><<<nb, kBlock, 0, s>>>(a);
    }
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int launch_within_count(msh_tree* tree, const QueryOrder& ord, double r_max, const double* d_r, size_t S,
                        uint32_t* d_counts, hipStream_t s) {
    if (S == 0) return MSH_OK;
    WiArgs a = within_args(tree, ord, r_max, d_r, S);
    a.counts = d_counts;
    return launch_walk<kWithinCount, false>(tree, a, s);
}

int launch_within_stats(msh_tree* tree, const QueryOrder& ord, double r_max, const double* d_r, size_t S,
                        unsigned long long* d_stats, hipStream_t s) {
    if (S == 0) return MSH_OK;
    WiArgs a = within_args(tree, ord, r_max, d_r, S);
    a.stats = d_stats;
    return launch_walk<kWithinCount, true>(tree, a, s);
}

int launch_within_all_count(msh_tree* tree, const QueryOrder& ord, double r_max, const double* d_r, size_t S,
                            HitTotals* out, hipStream_t s) {
    out->K = out->longest = 0;
    if (S == 0) return MSH_OK;
    Workspace& ws = tree->ws;
    MSH_TRY(ws.flags.reserve(S * sizeof(uint32_t)));
    MSH_TRY(ws.stats.reserve(2 * sizeof(unsigned long long)));
    unsigned long long* d_tot = ws.stats.as<unsigned long long>();
    MSH_HIP(hipMemsetAsync(d_tot, 0, 2 * sizeof(unsigned long long), s));
    MSH_TRY(launch_within_count(tree, ord, r_max, d_r, S, ws.flags.as<uint32_t>(), s));
    {
        TimedLaunch tl("within_scan", s);
        MSH_TRY(sum_counts(ws.flags.as<uint32_t>(), S, d_tot, persistent_blocks(tree->device, blocks_for(S), 5), s));
    }
    unsigned long long h[2] = {0, 0};
    MSH_HIP(hipMemcpyAsync(h, d_tot, sizeof(h), hipMemcpyDeviceToHost, s));
    MSH_HIP(hipStreamSynchronize(s));
    out->K = h[0];
    out->longest = h[1];
    return MSH_OK;
}

int launch_within_emit(msh_tree* tree, const QueryOrder& ord, double r_max, const double* d_r, size_t S,
                       const HitTotals& tot, const WithinOut& o, size_t n_emit, hipStream_t s) {
    const size_t K = (size_t)tot.K;
    if (K == 0 || n_emit == 0) return MSH_OK;
    Workspace& ws = tree->ws;
    const bool tri = tree->kind != kPoints;
    const bool lane_order = tot.longest <= (uint64_t)kLaneSort;
    MSH_TRY(ws.ranges.reserve(S * sizeof(uint32_t)));
    MSH_TRY(ws.out_a.reserve(K * sizeof(double)));
    MSH_TRY(ws.out_b.reserve(K * sizeof(uint32_t)));
    MSH_TRY(ws.out_c.reserve(K * sizeof(uint32_t)));
    MSH_TRY(ws.out_d.reserve(K * sizeof(uint32_t)));
    uint32_t* counts = ws.flags.as<uint32_t>();
    uint32_t* offsets = ws.ranges.as<uint32_t>();
    {
        TimedLaunch tl("within_scan", s);
        MSH_HIP(hipMemcpyAsync(offsets, counts, S * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        MSH_TRY(exclusive_scan_u32(offsets, S, ws, s));
    }
    WiArgs a = within_args(tree, ord, r_max, d_r, S);
    a.counts = counts;
    a.offsets = offsets;
    a.ed2 = ws.out_a.as<double>();
    a.eleaf = ws.out_b.as<uint32_t>();
    a.eid = ws.out_c.as<uint32_t>();
    uint32_t* idx = ws.out_d.as<uint32_t>();
    a.order = lane_order ? idx : nullptr;
    a.n_emit = n_emit;
    MSH_TRY((launch_walk<kWithinFill, false>(tree, a, s)));
    if (!lane_order) {
        TimedLaunch tl("within_order", s);
        // ids: vertex indices < P = T leaves of a point tree, face ids < T of a triangle tree
        MSH_TRY(order_csr_entries(a.ed2, a.eid, bits_for(tree->T), offsets, S, K, ws, &idx, s));
    }
    WiEmit e{tree->d_leaves, ord.q, S, offsets, idx, a.ed2, a.eleaf, a.eid, n_emit, o};
    if (!tri) e.o.pt = nullptr, e.o.part = nullptr;
    TimedLaunch tl("within_emit", s);
    if (tri) k_within_emit<true><<<blocks_for(n_emit), kBlock, 0, s>>>(e);
    else k_within_emit<false><<<blocks_for(n_emit), kBlock, 0, s>>>(e);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

}  // namespace msh
