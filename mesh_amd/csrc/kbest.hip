// K-nearest and radius-capped queries on point and plain triangle trees (msh_points_knearest, msh_tree_knearest).
//
// The answer of a row is the first min(K, m) of the primitives with d2 <= r2, ascending by the key (d2, id): d2 the
// exact fp64 squared distance of the 1-NN path (sqdist for points, closest_on_triangle for triangles), id the vertex
// index or face id.  It is a function of (tree, q, K, r_max) alone: the key is a total order on the primitives, a
// primitive is rejected only by a bound that is conservative for that order, and no atomic touches an answer.
//
//   k_kbest         one lane per row in the closest-point path's slot order; depth first from the root, nearer child
//                   first (WalkerT::step), on the per-lane LDS stack with global spill; every lane runs to completion.
//                   The lane keeps a sorted list of at most K (d2, id) entries (insertion from the tail in LDS, by
//                   bisection and a chunked shift in memory), and prunes with
//                   min(K-th d2, r2) once the list is full.  The walker compares bound <= limit, so a primitive that
//                   ties the K-th entry on d2 with a smaller id is still reached.  The list lives in a register pair
//                   (K = 1), in LDS lane columns (K <= 16) or in the workspace, wave-interleaved (larger K); at the end
//                   of a row every variant leaves it in the workspace for the finish pass.
//   k_kbest_finish  one thread per (row, rank): dist = sqrt(d2), the point and part of a triangle by the construction
//                   the 1-NN answer store runs, the count, and the padding of the unused ranks.  The walk writes no
//                   output array, so no row is ever partly filled.
#include <algorithm>
#include <cmath>

#include "knn.h"

namespace msh {

// list entries per lane kept in LDS, 12 B each in columns of stride kBlock: 24 KB per block for K <= 8 (with the 16 KB
// stack: 4 blocks per CU), 48 KB for K <= 16 (2 blocks per CU: half the waves, still ahead of the list in memory)
constexpr int kKbestLds = 8, kKbestLds2 = 16;
constexpr unsigned kKbestBlocksPerCU = 4;

struct KbArgs {
    const BNode* nodes;
    const void* leaves;
    size_t T;
    const double* q;       // the caller's rows
    const uint32_t* perm;  // slot -> caller's row (nullptr: identity)
    size_t S;
    uint32_t K;
    double r2;
    double org[3];
    double tm;
    uint2* spill;
    int spill_depth;
    // the rows' lists, wave-interleaved: entry j of slot i at ((i / 64) * K + j) * 64 + i % 64, so the accesses of a
    // wave to one rank coalesce; cnt[i] = entries of slot i
    double* ld2;
    uint32_t* lid;
    uint32_t* cnt;
    unsigned long long* stats;  // STATS launches: [0] nodes, [1] primitives, [2] insertions, [3] deepest stack
};

// The leaf policy of WalkerT::step.  CAP: 1 the list is (kd2, kid); 8 or 16: LDS columns of stride kBlock;
// 0: the workspace (ld2 / lid point at this lane's entry 0, stride 64).  (kd2, kid) is the K-th entry once the list is
// full; until then kd2 = +inf, so only the radius prunes.
template <bool TRI, int CAP, bool STATS>
struct KbPol {
    const void* __restrict__ leaves;
    D3 q;
    double r2, kd2;
    uint32_t kid, n, K;
    float limf;
    double* ld2;
    uint32_t* lid;
    unsigned n_ins;
    __device__ double limit() const { return fmin(kd2, r2) * kSlack; }
    __device__ void relim() { limf = __double2float_ru(limit()); }
    __device__ static size_t at(int j) { return (size_t)j * (CAP == 0 ? 64 : kBlock); }
    __device__ void test(int leaf) {
        uint32_t id;
        const double d2 = kb_eval<TRI>(leaves, leaf, q, id);
        // within the radius, and before the K-th entry (any entry while the list has room: kd2 = +inf, kid = ~0)
        if (!(d2 <= r2) || !(d2 < kd2 || (d2 == kd2 && id < kid))) return;
        if (STATS) ++n_ins;
        if constexpr (CAP == 1) {
            n = 1;
            kd2 = d2;
            kid = id;
        } else {
            const int m = (int)(n < K ? n : K - 1);  // entries that stay: a full list drops its last one
            int j = m;
            if constexpr (CAP == 0) {
                // the list is in memory, where every dependent access costs a round trip: find the place by bisection,
                // then move the entries above it up four at a time, the four loads in flight together
                int lo = 0;
                while (lo < j) {
                    const int mid = (lo + j) >> 1;
                    const double e = ld2[at(mid)];
                    const uint32_t f = lid[at(mid)];
                    if (e < d2 || (e == d2 && f < id)) lo = mid + 1;
                    else j = mid;
                }
                for (int top = m; top > j; top -= 4) {  // entries [top - 4, top) that lie at or above j move up by one
                    double e[4];
                    uint32_t f[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (top - 1 - c >= j) {
                            e[c] = ld2[at(top - 1 - c)];
                            f[c] = lid[at(top - 1 - c)];
                        }
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (top - 1 - c >= j) {
                            ld2[at(top - c)] = e[c];
                            lid[at(top - c)] = f[c];
                        }
                }
            } else {
                while (j > 0) {
                    const double e = ld2[at(j - 1)];
                    const uint32_t f = lid[at(j - 1)];
                    if (e < d2 || (e == d2 && f < id)) break;
                    ld2[at(j)] = e;
                    lid[at(j)] = f;
                    --j;
                }
            }
            ld2[at(j)] = d2;
            lid[at(j)] = id;
            if (n < K) ++n;
            if (n < K) return;  // still room: the limit stays the radius
            kd2 = ld2[at((int)K - 1)];
            kid = lid[at((int)K - 1)];
        }
        relim();
    }
};

// E: the stack entries (Ent4 for trees of <= 2^20 leaves)
template <bool TRI, int CAP, class E, bool STATS>
__global__ __launch_bounds__(kBlock) void k_kbest(KbArgs a) {
    typedef typename E::T Ent;
    __shared__ Ent stk[kStack * kBlock];
    __shared__ double l_d2[CAP > 1 ? CAP * kBlock : 1];
    __shared__ uint32_t l_id[CAP > 1 ? CAP * kBlock : 1];
    const int tid = threadIdx.x, lane = tid & 63;
    Ent* lds = stk + tid;
    uint2* spill = a.spill ? a.spill + (size_t)blockIdx.x * kBlock * (size_t)a.spill_depth + tid : nullptr;
    const double org[3] = {a.org[0], a.org[1], a.org[2]};
    const size_t ntiles = (a.S + 63) / 64, nwaves = (size_t)gridDim.x * (kBlock / 64);
    unsigned n_nodes = 0, n_leaves = 0;
    unsigned long long t_nodes = 0, t_leaves = 0, t_ins = 0, deepest = 0;
    // waves are independent (no block barrier): each takes every nwaves-th tile of 64 slots
    for (size_t tile = (size_t)blockIdx.x * (kBlock / 64) + (tid >> 6); tile < ntiles; tile += nwaves) {
        const size_t i = tile * 64 + lane;
        const bool live = i < a.S;
        size_t r;  // the caller's row
        const D3 q = load_slot_row(a.q, a.perm, i, live, r);
        const bool fin = live && finite3(q);
        double* const g_d2 = a.ld2 + tile * a.K * 64 + lane;  // this slot's entry 0 in the workspace
        uint32_t* const g_id = a.lid + tile * a.K * 64 + lane;
        KbPol<TRI, CAP, STATS> pol;
        pol.leaves = a.leaves;
        pol.q = q;
        pol.r2 = a.r2;
        pol.kd2 = INFINITY;
        pol.kid = 0xFFFFFFFFu;
        pol.n = 0;
        pol.K = a.K;
        pol.ld2 = CAP == 0 ? g_d2 : l_d2 + tid;
        pol.lid = CAP == 0 ? g_id : l_id + tid;
        pol.n_ins = 0;
        pol.relim();
        if (fin) {
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
                    if (++steps >= a.T) break;
                }
            }
        }
        if (live) {
            a.cnt[i] = pol.n;
            if constexpr (CAP == 1) {
                if (pol.n) {
                    g_d2[0] = pol.kd2;
                    g_id[0] = pol.kid;
                }
            } else if constexpr (CAP != 0) {
                for (uint32_t j = 0; j < pol.n; ++j) {
                    g_d2[(size_t)j * 64] = pol.ld2[pol.at(j)];
                    g_id[(size_t)j * 64] = pol.lid[pol.at(j)];
                }
            }
        }
        if (STATS) {
            t_nodes += n_nodes;
            t_leaves += n_leaves;
            t_ins += pol.n_ins;
            n_nodes = n_leaves = 0;
        }
    }
    if (STATS) flush_stats4(a.stats, t_nodes, t_leaves, t_ins, deepest);
}

struct KbFinish {
    const void* leaves;
    const uint32_t* inv;  // face -> leaf (triangle trees with pt or part)
    size_t T;
    const double* q;
    const uint32_t* perm;
    size_t S;
    uint32_t K;
    const double* ld2;
    const uint32_t* lid;
    const uint32_t* cnt;
    KbOut o;
};

// thread t handles the list entry at index t: ((slot / 64) * K + rank) * 64 + slot % 64
template <bool TRI>
__global__ __launch_bounds__(kBlock) void k_kbest_finish(KbFinish f) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t per = (size_t)f.K * 64;
    const size_t tile = t / per, rem = t - tile * per;
    const uint32_t j = (uint32_t)(rem >> 6);
    const size_t i = tile * 64 + (rem & 63);
    if (i >= f.S) return;
    const size_t r = f.perm ? (size_t)f.perm[i] : i;
    const uint32_t n = f.cnt[i];
    const bool have = j < n;
    const double d2 = have ? f.ld2[t] : INFINITY;
    const uint32_t id = have ? f.lid[t] : MSH_NO_FACE;
    const size_t at = r * f.K + j;
    f.o.id[at] = id;
    f.o.dist[at] = sqrt(d2);
    if (j == 0 && f.o.count) f.o.count[r] = n;
    if constexpr (TRI) {
        if (!f.o.pt && !f.o.part) return;
        D3 p = D3{NAN, NAN, NAN};
        int pc = 0;
        if (have && id < f.T) {
            D3 ta, tb, tc;
            uint32_t ff;
            load_tri(static_cast<const TriRec*>(f.leaves), (int)f.inv[id], ta, tb, tc, ff);
            closest_on_triangle(D3{f.q[3 * r], f.q[3 * r + 1], f.q[3 * r + 2]}, ta, tb, tc, p, pc);
        }
        if (f.o.part) f.o.part[at] = (uint32_t)pc;
        if (f.o.pt) {
            f.o.pt[3 * at] = p.x;
            f.o.pt[3 * at + 1] = p.y;
            f.o.pt[3 * at + 2] = p.z;
        }
    }
}

template <bool TRI, class E, bool STATS>
static void kbest_walk(const KbArgs& a, unsigned nb, hipStream_t s) {
    if (a.K == 1)
        k_kbest<TRI, 1, E, STATS><<<nb, kBlock, 0, s>>>(a);
    else if (a.K <= (uint32_t)kKbestLds)
        k_kbest<TRI, kKbestLds, E, STATS><<<nb, kBlock, 0, s>>>(a);
    else if (a.K <= (uint32_t)kKbestLds2)
        k_kbest<TRI, kKbestLds2, E, STATS><<<nb, kBlock, 0, s>>>(a);
    else
        k_kbest<TRI, 0, E, STATS><<<nb, kBlock, 0, s>>>(a);
}

template <bool STATS>
static int launch_kb(msh_tree* tree, const QueryOrder& ord, size_t S, uint32_t K, double r_max, const KbOut& o,
                     const uint32_t* d_inv, unsigned long long* d_stats, hipStream_t s) {
    if (S == 0) return MSH_OK;
    const bool tri = tree->kind != kPoints;
    Workspace& ws = tree->ws;
    const size_t ntiles = (S + 63) / 64, slots = ntiles * 64;
    KbArgs a{};
    a.nodes = tree->d_nodes;
    a.leaves = tree->d_leaves;
    a.T = tree->T;
    a.q = ord.q;  // the caller's rows: each lane reads row perm[slot]
    a.perm = ord.perm;
    a.S = S;
    a.K = K;
    a.r2 = r_max * r_max;
    a.tm = tree_margin(tree->half_diag);
    a.stats = d_stats;
    for (int k = 0; k < 3; ++k) a.org[k] = tree->origin[k];
    MSH_TRY(ws.res.reserve(slots * K * sizeof(double)));
    MSH_TRY(ws.res_w.reserve(slots * K * sizeof(uint32_t)));
    MSH_TRY(ws.flags.reserve(slots * sizeof(uint32_t)));
    a.ld2 = ws.res.as<double>();
    a.lid = ws.res_w.as<uint32_t>();
    a.cnt = ws.flags.as<uint32_t>();
    const bool e4 = tree->T <= kEnt4MaxLeaves;
    // persistent grid: every wave strides over the tiles; as many blocks per CU as their LDS (stack + list) lets
    // reside in its 160 KB, at most kKbestBlocksPerCU
    const size_t cap = K == 1 ? 0 : (K <= (uint32_t)kKbestLds ? kKbestLds : (K <= (uint32_t)kKbestLds2 ? kKbestLds2 : 0));
    const size_t lds = (size_t)kBlock * (kStack * (e4 ? sizeof(Ent4::T) : sizeof(Ent8::T)) + cap * 12);
    const unsigned per_cu = std::min<unsigned>(kKbestBlocksPerCU, (unsigned)(((size_t)160 << 10) / lds));
    const unsigned nb = persistent_blocks(tree->device, blocks_for(S), per_cu);
    // the depth-first stack holds at most one entry per level of the path to the current node
    MSH_TRY(plan_spill(ws, tree->max_depth + 1, kStack, nb, &a.spill, &a.spill_depth));
    {
        TimedLaunch tl(STATS ? "kbest_stats" : "kbest", s);
        if (tri) {
            if (e4) kbest_walk<true, Ent4, STATS>(a, nb, s);
            else kbest_walk<true, Ent8, STATS>(a, nb, s);
        } else {
            if (e4) kbest_walk<false, Ent4, STATS>(a, nb, s);
            else kbest_walk<false, Ent8, STATS>(a, nb, s);
        }
        MSH_HIP(hipGetLastError());
    }
    if (STATS) return MSH_OK;
    KbFinish f{};
    f.leaves = tree->d_leaves;
    f.inv = d_inv;
    f.T = tree->T;
    f.q = ord.q;
    f.perm = ord.perm;
    f.S = S;
    f.K = K;
    f.ld2 = a.ld2;
    f.lid = a.lid;
    f.cnt = a.cnt;
    f.o = o;
    if (!d_inv) f.o.pt = nullptr, f.o.part = nullptr;
    const size_t nthr = slots * K;
    TimedLaunch tl("kbest_finish", s);
    if (tri)
        k_kbest_finish<true><<<blocks_for(nthr), kBlock, 0, s>>>(f);
    else
        k_kbest_finish<false><<<blocks_for(nthr), kBlock, 0, s>>>(f);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int launch_kbest(msh_tree* tree, const QueryOrder& ord, size_t S, uint32_t K, double r_max, const KbOut& o,
                 const uint32_t* d_inv, hipStream_t s) {
    return launch_kb<false>(tree, ord, S, K, r_max, o, d_inv, nullptr, s);
}

int launch_kbest_stats(msh_tree* tree, const QueryOrder& ord, size_t S, uint32_t K, double r_max,
                       unsigned long long* d_counts, hipStream_t s) {
    return launch_kb<true>(tree, ord, S, K, r_max, KbOut{}, nullptr, d_counts, s);
}

}  // namespace msh
