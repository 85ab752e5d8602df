// Ray casting, all hits: per-ray hit counts (msh_tree_raycast_count) and the sorted hit lists as CSR
// (msh_tree_raycast_all) on plain triangle trees.  Rows, ranges, castability and the hit set are raycast.hip's: leaf
// triangle j is a hit of row (o, d, [t0, t1]) when ray_tri reports kind 1 or 2 in the range and its t is not NaN.
//
// Count, sum, scan, fill, order, emit -- the protocol of the pair lists (tritri.hip).  k_raycast_all is k_raycast's
// tile loop (one lane per ray, slot order of the origins, reads and stores at the caller's row perm[slot]) over
// traverse_rays with a policy that never prunes: the ranged slab test picks the children, every taken leaf is tested.
// Count mode writes counts[r].  Fill mode makes the same walk again and writes (t, leaf, face) of hit n at offsets[r] +
// n, guarded by n < counts[r], and stops after the row's last hit.  Only a row's own lane writes its count and its
// segment, so the content does not depend on how lanes are scheduled; the walk order decides only where in its segment
// a hit lands, and the order step removes that: entries are sorted by (row, t by value, face id).
//   Short rows (no row above kLaneSort hits): each fill lane orders its own segment by repeated selection of the next
//   (t, face) above the previous one -- the pairs are distinct within a row because the face ids are -- and writes the
//   sorted positions to `order`.
//   Long rows: stable LSD radix sorts of an index over all K entries, keys face id, the low and high words of
//   allhits_t_key(t), then the row.
// k_hit_emit, one thread per written entry, then rebuilds what the walk did not carry: it loads the leaf's triangle and
// writes t, face and on request pt (FirstPol::finish's construction) and side (the sign of den = n . d as ray_tri forms
// it).  An entry's row is found by bisection of the offsets.
#include "knn.h"
#include "rays.h"

namespace msh {

enum { kHitCount = 0, kHitFill = 1 };

// all hits in [t0, t1]; no key, nothing is pruned (AnyRangePol's node test and acceptance)
template <bool kFill>
struct AllPol {
    const TriRec* __restrict__ tris;
    D3 o, d;
    double t0, t1;
    RayF rf;
    uint32_t n, lim;  // hits met so far; fill: the row's count
    double* ht;       // fill: the row's segment of t, leaf and face
    uint32_t* hl;
    uint32_t* hf;
    __device__ void children(const NodeV& nd, bool& h0, bool& h1, float& k0, float& k1) const {
        ray_child_slabs(nd, rf, h0, h1, k0, k1);
    }
    __device__ bool keep(float) const { return true; }
    // a fill walk ends with the row's last hit (the count pass made the same walk to the end and found lim of them)
    __device__ bool done() const { return kFill && n >= lim; }
    __device__ void test(int leaf) {
        D3 a, b, c;
        uint32_t face;
        load_tri(tris, leaf, a, b, c, face);
        double t;
        if (!ray_tri(o, d, a, b, c, t, t0, t1) || t != t) return;
        if (kFill && n < lim) {  // never at or beyond the segment's end, whatever the walk meets
            ht[n] = t;
            hl[n] = (uint32_t)leaf;
            hf[n] = face;
        }
        ++n;
    }
};

struct RcAllArgs {
    const BNode* nodes;
    const TriRec* tris;
    size_t T;
    const double* o;       // the caller's rows
    const double* d;
    const double* range;   // (S,2) or nullptr: [0, +inf]
    size_t S;
    const uint32_t* perm;  // slot -> caller's row, nullptr: identity
    uint32_t* counts;      // per caller's row; written by the count pass, read by the fill pass
    const uint32_t* offsets;  // fill: exclusive scan of counts
    double* ht;            // fill: (K,) t, leaf and face of entry offsets[r] + n
    uint32_t* hl;
    uint32_t* hf;
    uint32_t* order;       // fill, every row <= kLaneSort hits: order[p] = the entry that comes p-th; else nullptr
    size_t n_emit;         // positions >= n_emit are not ordered
    unsigned* counters;
    unsigned ntiles;
    uint2* spill;
    int spill_depth;
    double org[3];
    double M;
};

// k_raycast's shape: kStack LDS entries per lane, no node slots, 4 waves per SIMD (DESIGN §17 has the resource table).
template <int kMode>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_raycast_all(RcAllArgs a) {
    constexpr bool kFill = kMode == kHitFill;
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
        size_t base = 0;
        uint32_t lim = 0;
        if (kFill) {
            base = a.offsets[r];
            lim = a.counts[r];
            if (lim == 0) continue;  // nothing to walk for (rows that cannot be cast among them)
        }
        const D3 o = D3{a.o[3 * r], a.o[3 * r + 1], a.o[3 * r + 2]};
        const D3 d = D3{a.d[3 * r], a.d[3 * r + 1], a.d[3 * r + 2]};
        double t0 = a.range ? a.range[2 * r] : 0.0;
        const double t1 = a.range ? a.range[2 * r + 1] : INFINITY;
        // rows that cannot be cast have an empty hit set (t0 <= t1 is false for a NaN in the range)
        const bool go = finite3(o) && finite3(d) && (d.x != 0.0 || d.y != 0.0 || d.z != 0.0) && t0 <= t1;
        t0 = fmax(t0, 0.0);
        double L = 0.0;
        const RayF rf = make_rayf_range(vsub(o, org), d, a.M, t0, t1, &L);
        AllPol<kFill> pol{a.tris, o, d, t0, t1, rf, 0u, lim, kFill ? a.ht + base : nullptr, kFill ? a.hl + base : nullptr,
                          kFill ? a.hf + base : nullptr};
        if (go) traverse_rays<AllPol<kFill>, false>(a.nodes, a.T, pol, lds, spill, n_nodes, n_leaves);
        if (!kFill) {
            a.counts[r] = pol.n;
            continue;
        }
        // Short rows are ordered by their own lane: entry k of the row is the smallest (t, face) above entry k - 1's --
        // lim^2 reads of the segment the lane has just written, lim <= kLaneSort.  t is compared by value.
        if (a.order) {
            double last_t = 0.0;
            uint32_t last_f = 0;
            for (uint32_t k = 0; k < lim && base + k < a.n_emit; ++k) {
                double best_t = INFINITY;
                uint32_t best_f = 0xFFFFFFFFu, best_m = 0;  // not a face id (ids < 2^31)
                for (uint32_t m = 0; m < lim; ++m) {
                    const double t = a.ht[base + m];
                    const uint32_t f = a.hf[base + m];
                    const bool above = k == 0 || t > last_t || (t == last_t && f > last_f);
                    if (above && (t < best_t || (t == best_t && f < best_f))) {
                        best_t = t;
                        best_f = f;
                        best_m = m;
                    }
                }
                a.order[base + k] = (uint32_t)(base + best_m);
                last_t = best_t;
                last_f = best_f;
            }
        }
    }
}

// keys[p] of the entry idx[p] (idx == nullptr: p itself, and idx_out[p] = p) for one of the order's four sorts
enum { kKeyFace = 0, kKeyTLo = 1, kKeyTHi = 2, kKeyRow = 3 };
template <int kKey>
__global__ __launch_bounds__(kBlock) void k_hit_keys(const uint32_t* __restrict__ idx, size_t n,
                                                     const double* __restrict__ ht, const uint32_t* __restrict__ hf,
                                                     const uint32_t* __restrict__ offsets, size_t S,
                                                     uint32_t* __restrict__ keys, uint32_t* __restrict__ idx_out) {
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const size_t e = idx ? (size_t)idx[p] : p;
    if (!idx) idx_out[p] = (uint32_t)p;
    uint32_t key;
    if (kKey == kKeyFace) key = hf[e];
    else if (kKey == kKeyTLo) key = (uint32_t)allhits_t_key(ht[e]);
    else if (kKey == kKeyTHi) key = (uint32_t)(allhits_t_key(ht[e]) >> 32);
    else key = (uint32_t)hit_row(offsets, S, e);
    keys[p] = key;
}

struct EmitArgs {
    const TriRec* tris;
    const double* o;
    const double* d;
    const double* range;
    size_t S;
    const uint32_t* offsets;
    const uint32_t* order;  // order[p] = the entry that comes p-th
    const double* ht;
    const uint32_t* hl;
    size_t n;
    double* out_t;
    uint32_t* out_face;
    double* out_pt;   // nullable
    int8_t* out_side; // nullable
};

__global__ __launch_bounds__(kBlock) void k_hit_emit(EmitArgs a) {
    const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    const size_t e = a.order[p];
    const double t = a.ht[e];
    D3 ta, tb, tc;
    uint32_t face;
    load_tri(a.tris, (int)a.hl[e], ta, tb, tc, face);
    a.out_t[p] = t;
    a.out_face[p] = face;
    if (!a.out_pt && !a.out_side) return;
    const size_t r = hit_row(a.offsets, a.S, e);
    const D3 o = D3{a.o[3 * r], a.o[3 * r + 1], a.o[3 * r + 2]};
    const D3 d = D3{a.d[3 * r], a.d[3 * r + 1], a.d[3 * r + 2]};
    const double t0 = fmax(a.range ? a.range[2 * r] : 0.0, 0.0);
    const double t1 = a.range ? a.range[2 * r + 1] : INFINITY;
    double tt = t;
    const int kind = ray_tri(o, d, ta, tb, tc, tt, t0, t1);  // the walk's own evaluation again: tt == t
    if (a.out_pt) {
        D3 pt;
        if (kind == 2 || !cgal_plane_line(o, d, ta, tb, tc, pt)) pt = vadd(o, vscale(tt, d));
        a.out_pt[3 * p] = pt.x;
        a.out_pt[3 * p + 1] = pt.y;
        a.out_pt[3 * p + 2] = pt.z;
    }
    if (a.out_side) {
        const double den = vdot(vcross(vsub(tb, ta), vsub(tc, ta)), d);
        a.out_side[p] = kind == 2 ? 0 : (den < 0.0 ? 1 : (den > 0.0 ? -1 : 0));
    }
}

static RcAllArgs all_args(const msh_tree* tree, const QueryOrder& ord, const double* d_range, size_t S) {
    RcAllArgs a{};
    a.nodes = tree->d_nodes; a.tris = static_cast<const TriRec*>(tree->d_leaves); a.T = tree->T;
    a.o = ord.q; a.d = ord.n; a.range = d_range; a.S = S;
    a.perm = ord.perm;  // rays run in slot order and read and store at the caller's rows
    for (int k = 0; k < 3; ++k) a.org[k] = tree->origin[k];
    a.M = tree->half_diag;
    a.ntiles = (unsigned)((S + 63) / 64);  // S <= 2^32 - 1 (the entry points' check_count)
    return a;
}

template <int kMode>
static int launch_all(msh_tree* tree, RcAllArgs a, hipStream_t s) {
    const unsigned nblk = persistent_blocks(tree->device, (a.ntiles + 3) / 4, 5);
    MSH_TRY(tree->ws.counters.reserve(9 * 32 * sizeof(unsigned)));
    a.counters = tree->ws.counters.as<unsigned>();
    MSH_HIP(hipMemsetAsync(a.counters, 0, 8 * 32 * sizeof(unsigned), s));
    MSH_TRY(plan_spill(tree->ws, tree->max_depth + 1, kStack, nblk, &a.spill, &a.spill_depth));
    TimedLaunch tl(kMode == kHitFill ? "raycast_fill" : "raycast_count", s);
    k_raycast_all<kMode><<<nblk, kBlock, 0, s>>>(a);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int launch_raycast_count(msh_tree* tree, const QueryOrder& ord, const double* d_range, size_t S, uint32_t* d_counts,
                         hipStream_t s) {
    if (S == 0) return MSH_OK;
    RcAllArgs a = all_args(tree, ord, d_range, S);
    a.counts = d_counts;
    return launch_all<kHitCount>(tree, a, s);
}

int launch_raycast_all_count(msh_tree* tree, const QueryOrder& ord, const double* d_range, size_t S, HitTotals* out,
                             hipStream_t s) {
    out->K = out->longest = 0;
    if (S == 0) return MSH_OK;
    Workspace& ws = tree->ws;
    MSH_TRY(ws.flags.reserve(S * sizeof(uint32_t)));
    MSH_TRY(ws.stats.reserve(2 * sizeof(unsigned long long)));
    unsigned long long* d_tot = ws.stats.as<unsigned long long>();
    MSH_HIP(hipMemsetAsync(d_tot, 0, 2 * sizeof(unsigned long long), s));
    MSH_TRY(launch_raycast_count(tree, ord, d_range, S, ws.flags.as<uint32_t>(), s));
    {
        TimedLaunch tl("raycast_scan", s);
        MSH_TRY(sum_counts(ws.flags.as<uint32_t>(), S, d_tot, persistent_blocks(tree->device, blocks_for(S), 5), s));
    }
    unsigned long long h[2] = {0, 0};
    MSH_HIP(hipMemcpyAsync(h, d_tot, sizeof(h), hipMemcpyDeviceToHost, s));
    MSH_HIP(hipStreamSynchronize(s));
    out->K = h[0];
    out->longest = h[1];
    return MSH_OK;
}

int launch_raycast_all_emit(msh_tree* tree, const QueryOrder& ord, const double* d_range, size_t S, const HitTotals& tot,
                            const HitOut& o, size_t n_emit, hipStream_t s) {
    const size_t K = (size_t)tot.K;
    if (K == 0 || n_emit == 0) return MSH_OK;
    Workspace& ws = tree->ws;
    const bool lane_order = tot.longest <= (uint64_t)kLaneSort;
    MSH_TRY(ws.ranges.reserve(S * sizeof(uint32_t)));
    MSH_TRY(ws.out_a.reserve(K * sizeof(double)));
    MSH_TRY(ws.out_b.reserve(K * sizeof(uint32_t)));
    MSH_TRY(ws.out_c.reserve(K * sizeof(uint32_t)));
    MSH_TRY(ws.out_d.reserve(K * sizeof(uint32_t)));
    uint32_t* counts = ws.flags.as<uint32_t>();
    uint32_t* offsets = ws.ranges.as<uint32_t>();
    {
        TimedLaunch tl("raycast_scan", s);
        MSH_HIP(hipMemcpyAsync(offsets, counts, S * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        MSH_TRY(exclusive_scan_u32(offsets, S, ws, s));
    }
    RcAllArgs a = all_args(tree, ord, d_range, S);
    a.counts = counts;
    a.offsets = offsets;
    a.ht = ws.out_a.as<double>();
    a.hl = ws.out_b.as<uint32_t>();
    a.hf = ws.out_c.as<uint32_t>();
    uint32_t* idx = ws.out_d.as<uint32_t>();
    a.order = lane_order ? idx : nullptr;
    a.n_emit = n_emit;
    MSH_TRY(launch_all<kHitFill>(tree, a, s));
    if (!lane_order) {
        TimedLaunch tl("raycast_order", s);
        MSH_TRY(order_csr_entries(a.ht, a.hf, bits_for(tree->T), offsets, S, K, ws, &idx, s));
    }
    EmitArgs e{a.tris, a.o, a.d, d_range, S, offsets, idx, a.ht, a.hl, n_emit, o.t, o.face, o.pt, o.side};
    TimedLaunch tl("raycast_emit", s);
    k_hit_emit<<<blocks_for(n_emit), kBlock, 0, s>>>(e);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

// Long rows: stable sorts of an index over all K entries, least significant key first, leave it sorted by
// (row, key by value, id) in time linear in K however long a row is (internal.h order_csr_entries).
int order_csr_entries(const double* d_key, const uint32_t* d_id, int id_bits, const uint32_t* d_offsets, size_t S,
                      size_t K, Workspace& ws, uint32_t** idx_io, hipStream_t s) {
    MSH_TRY(ws.keys.reserve(K * sizeof(uint32_t)));
    MSH_TRY(ws.keys_alt.reserve(K * sizeof(uint32_t)));
    MSH_TRY(ws.vals_alt.reserve(K * sizeof(uint32_t)));
    uint32_t *keys = ws.keys.as<uint32_t>(), *keys_alt = ws.keys_alt.as<uint32_t>(), *idx_alt = ws.vals_alt.as<uint32_t>();
    uint32_t* idx = *idx_io;
    const unsigned nb = blocks_for(K);
    const int bits[4] = {id_bits, 32, 32, bits_for(S)};
    for (int pass = 0; pass < 4; ++pass) {
        const uint32_t* in = pass ? idx : nullptr;
        if (pass == kKeyFace) k_hit_keys<kKeyFace><<<nb, kBlock, 0, s>>>(in, K, d_key, d_id, d_offsets, S, keys, idx);
        else if (pass == kKeyTLo) k_hit_keys<kKeyTLo><<<nb, kBlock, 0, s>>>(in, K, d_key, d_id, d_offsets, S, keys, idx);
        else if (pass == kKeyTHi) k_hit_keys<kKeyTHi><<<nb, kBlock, 0, s>>>(in, K, d_key, d_id, d_offsets, S, keys, idx);
        else k_hit_keys<kKeyRow><<<nb, kBlock, 0, s>>>(in, K, d_key, d_id, d_offsets, S, keys, idx);
        MSH_HIP(hipGetLastError());
        bool alt = false;
        MSH_TRY(radix_sort_pairs(keys, idx, keys_alt, idx_alt, K, bits[pass], ws, s, 0, &alt));
        if (alt) { std::swap(keys, keys_alt); std::swap(idx, idx_alt); }
    }
    *idx_io = idx;
    return MSH_OK;
}

}  // namespace msh
