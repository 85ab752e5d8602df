// K2 + K3 — closest-point traversal with fused fp64 refinement (replaces
// spatialsearchmodule.cpp:165-220 aabbtree_nearest and CGAL's closest_point_and_primitive), plus the
// normal-weighted metric variant (K7, aabb_normals.cpp:112-190), the vertex nearest-neighbour variant
// (K8, search.ClosestPointTree) and the barycentric variant (K9: nearest + Heidrich weights of the
// closest point, mesh.py:218-222 / geometry/barycentric_coordinates_of_projection.py:9-49).
//
// Query pipeline (sorted launches):
//   k_query_morton -> radix sort (both sort.hip) -> the closest-point traversal reads query row perm[i] for slot
//   i straight from the caller's array and stores its answer straight to the caller's row perm[i] (face,
//   part, point: scattered 4 + 4 + 24-B stores); only the leader phases also write a 32-B slot-order
//   record, because followers take their hints from them.  The ray, normals-metric and point-tree paths
//   gather the rows into slot order (k_gather_rows) and restore the caller's order from slot-order records
//   (k_unpermute).  Unsorted launches read and write the caller's arrays directly.
//
// Execution shape (gfx950):
//   Pass 1 (k_knn_list, k_knn_queue, k_knn_lean): persistent grid; each WAVE dequeues 64-query tiles from one of 8 XCD-group
//     counters (group = blockIdx % 8 labels the blocks sharing an XCD; each counter owns a contiguous
//     eighth of the Morton-sorted queries, so an XCD's L2 serves one region of the BVH; exhausted
//     groups steal).  One lane per query, near-child-first depth-first traversal: one 64-B node read
//     bounds both children by their fp32 oriented boxes; the far child is pushed (16-entry LDS stack
//     per lane, [depth][lane] layout, deeper entries spill to a lane-interleaved global area sized
//     from the tree depth).  Leaf children that survive the bound go to the wave leaf list, a ring in LDS
//     the wave evaluates in full rounds of 64 with CGAL's exact fp64 construction (postponed leaves,
//     Aila & Laine, dealt to every lane of the wave).  Pass 1 runs over super-leader slots, then leader
//     slots, then followers, each starting from the leaf of its nearest leader's answer.
//     The fp32 pruning radius is cached per lane and refreshed only when the best distance changes.
//     The cut-started unled launch of a sorted call (the headline) runs k_knn_lean.
//     A lane that exceeds `budget` node steps stops and appends its query (with its exact best so far)
//     to a deferred list: queries near the centre of a closed surface are equidistant from most of it
//     and would otherwise hold their whole wave for ~10^6 steps.
//   Pass 2 (k_knn_coop): one WAVE per deferred query, dealt from an atomic counter.  The wave walks a
//     last-in-first-out list of subtrees in LDS, 64 entries at a time (one per lane): children within the
//     bound are pushed back (compacted by ballot), leaf children are tested on the spot, and the wave
//     shares the best bound (wave min) after every round.  A list that would outgrow LDS is dealt to the
//     lanes' own stacks for depth-first walks.
// Ties: the lexicographic minimum of (squared distance, face index) — deterministic and independent of
// traversal order or of how the work was split (every box within best*(1+2^-40) is visited).
// Retired A/B switches (their shipped sides are the code; records under profiles/): MSH_TILE_PF
// (r06_c3_tile_prefetch_ab.jsonl), MSH_RESUME (r05_ab_leaders_sort_resume.jsonl), MSH_KNN_LEAN, MSH_LEAN_COLD,
// MSH_LEAN_STEP and MSH_LEAN_STATE (r07_c3_knn_lean_ab.jsonl, r07_knn_lean_isa.txt), and MSH_FOLLOW_CELL (followers
// also testing their cell's hint leaf: never shipped, no record kept).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "knn.h"


namespace msh {

// ---- pass 1: what the instrumented launches (STATS) add, shared by the list and the queue kernel ----
// a lane's counters, added to KnnArgs::stats when its wave runs out of tiles (the wave iterations: lane 0's)
__device__ inline void add_knn_stats(unsigned long long* stats, int lane, unsigned n_nodes, unsigned n_leaves,
                                     unsigned n_impr, unsigned n_hinted, unsigned n_hint_won, unsigned long long u_trav_it,
                                     unsigned long long u_trav_lanes, unsigned long long u_leaf_it,
                                     unsigned long long u_leaf_lanes) {
    atomicAdd(&stats[0], (unsigned long long)n_nodes);
    atomicAdd(&stats[1], (unsigned long long)n_leaves);
    atomicAdd(&stats[36], (unsigned long long)n_impr);
    atomicAdd(&stats[37], (unsigned long long)n_hinted);
    atomicAdd(&stats[38], (unsigned long long)n_hint_won);
    if (lane == 0) {
        atomicAdd(&stats[2], u_trav_it);
        atomicAdd(&stats[3], u_trav_lanes);
        atomicAdd(&stats[4], u_leaf_it);
        atomicAdd(&stats[5], u_leaf_lanes);
    }
}

// per-tile step profile of the launch's phase (stats[8 + 9 * phase slot ...]); tot = this lane's node steps
__device__ inline void tile_step_stats(const KnnArgs& a, unsigned tot, int lane) {
    unsigned mx = tot, sm = tot;
    for (int o = 32; o > 0; o >>= 1) {
        mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
        sm += (unsigned)__shfl_xor((int)sm, o);
    }
    unsigned long long* h = a.stats + 8 + 9 * (a.phase == 3 ? 0 : ((a.phase == 1 || a.phase == 4) ? 1 : 2));
    if (lane == 0) {
        atomicAdd(h + 0, 1ull);
        atomicAdd(h + 1, (unsigned long long)mx);
        atomicAdd(h + 2, (unsigned long long)sm);
        atomicAdd(h + 3, (unsigned long long)min(mx, 128u));
        atomicAdd(h + 4, (unsigned long long)min(mx, 256u));
        atomicAdd(h + 5, (unsigned long long)min(mx, 512u));
    }
    if (tot > 128) atomicAdd(h + 6, 1ull);
    if (tot > 256) atomicAdd(h + 7, 1ull);
    if (tot > 512) atomicAdd(h + 8, 1ull);
}

// The record that hands slot i, past its budget with pol's best so far, to pass 2 (no resume entries yet: pass 2 would
// start at the root), and the launch's largest deferred best raised to it (k_p2_plan's threshold)
template <class Pol>
__device__ inline DeferRec defer_rec(const KnnArgs& a, size_t i, const Pol& pol) {
    DeferRec r;
    r.slot = (uint32_t)i;
    r.face = pol.best_face;
    r.leaf = pol.best_leaf;
    r.roff = 0;
    r.best = pol.best;
    r.rcnt = 0;
    r.sbound = 0x7F800000u;  // +inf
    if (a.max_best) atomicMax(a.max_best, (unsigned long long)__double_as_longlong(pol.best));
    return r;
}

// ---- pass 1: the kernels ----
// k_knn_list and k_knn_queue were one kernel.  They share the record of a deferred query (defer_rec) and what the
// instrumented launches add (tile_step_stats, add_knn_stats).  The rest of what they have in common is written out in
// both: the tile claim with its prefetch, the tile's start (slot, query, start hint, the T == 1 case) and a deferred
// leader's published hint.  Each of these as a function both call changes the register allocation or the schedule of
// non-instrumented kernels (profiles/knn_split_isa_diff.txt), so a change to one goes into the other by hand.

// The list kernel (closest-point modes, trees of < 2^26 leaves): leaf children that survive the bound go to the wave
// leaf list.
// PF (trees of <= 2^20 leaves): 4-B stack entries (Ent4) and each lane's next node prefetched into LDS
// (node_prefetch); the 16 KB the node slots take per block come out of the stack.  C3: 1889 -> 1945 M q/s in one
// session, wave-cycles waiting on memory 55.7 -> 46.7 % at +10 VALU instructions per query
// (profiles/r04_c3_node_prefetch_lds_ab.jsonl).
template <int MODE, bool STATS, bool PF>
__global__ __launch_bounds__(kBlock) MSH_KNN_ATTR void k_knn_list(KnnArgs a) {
    static_assert(MODE == 0 || MODE == 3, "closest-point modes");
    typedef typename std::conditional<PF, Ent4, Ent8>::type E;
    __shared__ typename E::T stk[kStack * kBlock];
    __shared__ float4 nbuf[PF ? 4 * kBlock : 1];
    __shared__ uint32_t lsh[4 * (kRing + 64 * 4)];  // per wave: ring + bd/bfl (u64 per lane each)
    const int tid = threadIdx.x, lane = tid & 63;
    typename E::T* lds = stk + tid;
    // the wave's node slots (PF): LDS byte address from a wave-uniform wave index, so M0 is set by scalar code
    const int wv_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wsl = (uint32_t)(size_t)(__attribute__((address_space(3))) float4*)(nbuf + (PF ? wv_u * 256 : 0));
    const float4* nb = nbuf + (PF ? (tid >> 6) * 256 + lane : 0);
    uint2* spill = a.spill ? a.spill + (size_t)blockIdx.x * kBlock * (size_t)a.spill_depth + tid : nullptr;
    const unsigned group = blockIdx.x & 7u;
    unsigned long long u_trav_it = 0, u_trav_lanes = 0, u_leaf_it = 0, u_leaf_lanes = 0;  // STATS: wave iterations
    unsigned n_nodes = 0, n_leaves = 0;
    unsigned n_impr = 0, n_hinted = 0, n_hint_won = 0;  // STATS: improving leaf tests, hinted queries, hint = answer
    // lane 0 claims the wave's next tile of its own group while the current one's rows load (an atomic whose return
    // is waited for with the tile's first loads), instead of at the next tile's start
    const unsigned glo = (unsigned)(((unsigned long long)a.ntiles * group) >> 3);
    const unsigned ghi = (unsigned)(((unsigned long long)a.ntiles * (group + 1)) >> 3);
    unsigned nxt = ~0u;
    for (;;) {
        unsigned tile = 0;
        if (lane == 0) tile = (nxt != ~0u && glo + nxt < ghi) ? glo + nxt : dequeue_tile(a.counters, a.ntiles, group);
        tile = __shfl(tile, 0);
        if (tile >= a.ntiles) break;
        // every lane of the wave stays in the tile's loops (the leaf rounds deal entries to all 64 lanes);
        // a lane without a query (past the phase's units, or a non-finite row) only helps
        const size_t k = (size_t)tile * 64 + lane;
        size_t i = 0;
        bool live = k < a.nunits;
        if (live) {
            i = slot_of(a, k);
            live = i < a.S;
        }
        const D3 q = live ? load_q(a, i) : D3{0.0, 0.0, 0.0};
        if (lane == 0) nxt = glo < ghi ? atomicAdd(&a.counters[group * 32], 1u) : ~0u;
        if (live && a.inv_w && !a.direct) a.inv_w[a.qperm[i]] = (uint32_t)i;
        auto pol = make_pol<MODE>(a, i, q);
        const bool fin = live && finite3(q);
        if (live && !fin) {  // no distance is defined: NO_FACE / NaN, no traversal
            if (!STATS || a.res) write_result<MODE>(a, i, q, pol);
        }
        int hint_leaf = -1;  // STATS
        const size_t cell = fin ? cut_cell(a, q) : kNoCell;
        if (a.cut && cell != kNoCell && a.phase != 2) {
            // slots without a leader (super-leaders, leaders, unled launches) inside the grid: the cell's hint
            // leaf (the closest face found for its centre), within U(c) + r of q's own answer
            const int lf = cut_hint_leaf(cut_rec(a, cell)[0]);
            if (STATS) hint_leaf = lf;
            if (lf >= 0) {
                pol.test(lf);
                if (STATS) {
                    ++n_leaves;
                    ++n_hinted;
                }
            }
        } else if (fin && (a.phase == 2 || a.phase == 1)) {
            const int lf = a.phase == 2 ? leader_leaf(a, i, q, kFWin, kLead) : leader_leaf(a, i, q, kLWin * kLead2, kLead2);
            if (STATS) hint_leaf = lf;
            if (lf >= 0) {
                pol.test(lf);
                if (STATS) {
                    ++n_leaves;
                    ++n_hinted;
                }
            }
        }
        if (a.T == 1) {
            if (fin) {
                pol.test(0);
                if (STATS) ++n_leaves;
                if (!STATS || a.res) write_result<MODE>(a, i, q, pol);
            }
            continue;
        }
        QF qf;
        const int root = query_root(a, i, q, qf);
        WalkerT<E> w{root, 0};
        bool start = fin;
        if (cell != kNoCell) start = cut_start(a, cell, pol, w, lds, spill);
        if (PF && start && w.node >= 0) node_prefetch(a.nodes, w.node, wsl);
        uint32_t* ring = lsh + (tid >> 6) * (kRing + 64 * 4);
        unsigned long long* bd = reinterpret_cast<unsigned long long*>(ring + kRing);  // per owner: d2 bits
        unsigned long long* bfl = bd + 64;                                              // (face << 32 | leaf)
        bool active = start, want_defer = false, deferred = false;
        int nq = 0;              // this lane's leaves appended since all of them were last evaluated (a bound)
        unsigned last_pos = 0;   // ring counter of this lane's newest entry
        unsigned head = 0, tail = 0;  // wave-uniform ring counters: entries [head, tail) wait
        unsigned steps = 0;
        const unsigned max_steps = (unsigned)min(a.T, (size_t)UINT_MAX);
        const unsigned budget = a.budget;
        unsigned tot = 0;  // STATS: node steps of this lane, restarts included
        // Evaluate ring entries [head, upto) in rounds of 64, one per lane: each lane tests its entry's leaf
        // against its owner's query (ds_bpermute); the owners publish their best before each round and take
        // the round's lexicographic (d2, face) minimum back from LDS.
        auto run_rounds = [&](unsigned upto) {
            while (head != upto) {
                const unsigned n = min(64u, upto - head);
                bd[lane] = (unsigned long long)__double_as_longlong(pol.best);
                bfl[lane] = ~0ull;
                const bool valid = (unsigned)lane < n;
                const uint32_t en = ring[(head + (valid ? (unsigned)lane : 0u)) & (kRing - 1)];
                const int src = (int)(en & 63u);
                const int leaf = (int)(en >> 6);
                const D3 x = D3{__shfl(pol.q.x, src), __shfl(pol.q.y, src), __shfl(pol.q.z, src)};
                uint32_t f;
                const double d2 = pol.eval(leaf, x, f);
                const unsigned long long kb = (unsigned long long)__double_as_longlong(d2);
                asm volatile("" ::: "memory");
                if (valid) atomicMin(&bd[src], kb);
                asm volatile("" ::: "memory");
                if (valid && bd[src] == kb) atomicMin(&bfl[src], ((unsigned long long)f << 32) | (unsigned)leaf);
                asm volatile("" ::: "memory");
                const unsigned long long nb = bd[lane], nf = bfl[lane];
                const double nd = __longlong_as_double((long long)nb);
                const uint32_t nface = (uint32_t)(nf >> 32);
                if (nf != ~0ull && (nd < pol.best || (nd == pol.best && nface < pol.best_face))) {
                    pol.best = nd;
                    pol.best_face = nface;
                    pol.best_leaf = (int)(uint32_t)nf;
                    pol.relim();
                    if (STATS) ++n_impr;
                }
                asm volatile("" ::: "memory");
                if (STATS) {
                    if (valid) ++n_leaves;
                    if (lane == 0) {
                        ++u_leaf_it;
                        u_leaf_lanes += n;
                    }
                }
                head += n;
            }
            if ((int)(last_pos - head) < 0) nq = 0;  // every entry of this lane is evaluated
        };
        unsigned dslot = ~0u;  // this lane's deferred-list slot (deferred)
        for (;;) {
            // a lane past its budget defers once its own leaves are evaluated (pass 2 then owns the query); its
            // records are written after the tile's loop, so the loop holds no copy of the construction
            if (want_defer && nq == 0) {
                want_defer = false;
                dslot = atomicAdd(a.n_deferred, 1u);
                if (dslot < a.max_deferred) {
                    active = false;
                    deferred = true;
                }
                // deferred list full: finish here without a budget
            }
            const bool can = active && !want_defer && nq < (MSH_LIST_RESERVE ? kPend - 1 : kPend);
            const bool any = __ballot(can) != 0ull;
            if (!any && tail == head) break;  // nothing queued and nobody can move: the tile is done
            if (STATS) {
                const int nt = __popcll(__ballot(can));
                if (lane == 0 && any) {
                    ++u_trav_it;
                    u_trav_lanes += nt;
                }
            }
            int l0 = -1, l1 = -1;
            if (can) {
                active = w.template step_collect<decltype(pol), STATS, PF>(a.nodes, qf, pol, lds, spill, n_nodes,
                                                                              l0, l1, kPend - nq, nb, wsl);
                ++steps;
                if (STATS) ++tot;
                if (active && steps >= max_steps) active = false;  // each node is entered once: corrupt tree
                if (active && steps == budget) want_defer = true;
            }
            // append this step's leaves (at most two per lane) to the ring, in lane order
            if (l0 < 0) {
                l0 = l1;
                l1 = -1;
            }
            const unsigned long long m1 = __ballot(l0 >= 0), m2 = __ballot(l1 >= 0);
            const unsigned pos = tail + lanes_below(m1) + lanes_below(m2);
            if (l0 >= 0) {
                ring[pos & (kRing - 1)] = ((uint32_t)l0 << 6) | (uint32_t)lane;
                last_pos = pos;
                ++nq;
            }
            if (l1 >= 0) {
                ring[(pos + 1) & (kRing - 1)] = ((uint32_t)l1 << 6) | (uint32_t)lane;
                last_pos = pos + 1;
                ++nq;
            }
            tail += (unsigned)(__popcll(m1) + __popcll(m2));
            // full rounds while lanes can move; everything once nobody can
            const unsigned upto = any ? head + ((tail - head) & ~63u) : tail;
            if (upto != head) run_rounds(upto);
        }
        if (deferred) {
            if ((a.phase == 1 || a.phase == 3 || a.phase == 4) && a.res) {
                // later phases take hints from this slot before pass 2 answers it: publish the closest point of
                // the best face so far (a point on the mesh), or NO_FACE when it has none yet
                D3 o = D3{NAN, NAN, NAN};
                uint32_t f = MSH_NO_FACE;
                if (pol.best_leaf >= 0) {
                    D3 ta, tb, tc;
                    int part;
                    load_tri(static_cast<const TriRec*>(a.leaves), pol.best_leaf, ta, tb, tc, f);
                    closest_on_triangle(q, ta, tb, tc, o, part);
                }
                store_qres(a.res + i, f, (uint32_t)pol.best_leaf, o.x, o.y, o.z);
            }
            DeferRec r = defer_rec(a, i, pol);
            if (a.resume) {
                // what is left of this walk: the pending entry (w.node, not yet visited: bound 0) above the stack
                const unsigned cnt = (unsigned)w.sp + 1;
                const unsigned off = atomicAdd(a.n_resume, cnt);
                if (off + cnt <= a.resume_cap) {
                    uint2* dst = a.resume + off;
                    for (int j = 0; j < w.sp; ++j) {
                        const typename E::T e = stack_get(lds, spill, j);
                        dst[j] = make_uint2((uint32_t)E::ref(e), __float_as_uint(E::bound(e)));
                    }
                    dst[w.sp] = make_uint2((uint32_t)w.node, 0u);
                    r.roff = off;
                    r.rcnt = cnt;
                }
            }
            a.deferred[dslot] = r;
        }
        if (STATS) tile_step_stats(a, tot, lane);
        if (STATS && fin && hint_leaf >= 0 && pol.best_leaf == hint_leaf) ++n_hint_won;
        if (deferred) continue;
        if (fin && (!STATS || a.res)) write_result<MODE>(a, i, q, pol);
    }
    // a lane that stopped (deferred) may still have a node prefetch in flight: it lands before the block's LDS is
    // released
    if constexpr (PF) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (STATS)
        add_knn_stats(a.stats, lane, n_nodes, n_leaves, n_impr, n_hinted, n_hint_won, u_trav_it, u_trav_lanes, u_leaf_it,
                      u_leaf_lanes);
}

// The queue kernel (the closest-point modes on trees of >= 2^26 leaves, and the normals-metric and point modes): per-lane
// leaf queues (kLeafQ), dealt to the wave in the closest-point modes, tested by their own lanes otherwise.  No entry cut.
// Its tile claim, tile start and hint publish are k_knn_list's, statement for statement (see above).
template <int MODE, bool STATS>
__global__ __launch_bounds__(kBlock) MSH_KNN_ATTR void k_knn_queue(KnnArgs a) {
    constexpr bool kCompact = MODE == 0 || MODE == 3;  // per-lane queues dealt to the wave (else: per-lane rounds)
    __shared__ uint2 stk[kStack * kBlock];
    // compacted leaf phases: kLeafQ entries per lane
    __shared__ uint32_t lsh[kCompact ? (size_t)kBlock * kLeafQ * 2 : 1];
    uint2* lent = reinterpret_cast<uint2*>(lsh);
    const int tid = threadIdx.x, lane = tid & 63;
    uint2* lds = stk + tid;
    uint2* ent = lent + (kCompact ? (tid >> 6) * 64 * kLeafQ : 0);
    uint2* spill = a.spill ? a.spill + (size_t)blockIdx.x * kBlock * (size_t)a.spill_depth + tid : nullptr;
    const unsigned group = blockIdx.x & 7u;
    unsigned long long u_trav_it = 0, u_trav_lanes = 0, u_leaf_it = 0, u_leaf_lanes = 0;  // STATS: wave iterations
    unsigned n_nodes = 0, n_leaves = 0;
    unsigned n_impr = 0, n_hinted = 0, n_hint_won = 0;  // STATS: improving leaf tests, hinted queries, hint = answer
    // lane 0 claims the wave's next tile of its own group while the current one's rows load (an atomic whose return
    // is waited for with the tile's first loads), instead of at the next tile's start
    const unsigned glo = (unsigned)(((unsigned long long)a.ntiles * group) >> 3);
    const unsigned ghi = (unsigned)(((unsigned long long)a.ntiles * (group + 1)) >> 3);
    unsigned nxt = ~0u;
    for (;;) {
        unsigned tile = 0;
        if (lane == 0) tile = (nxt != ~0u && glo + nxt < ghi) ? glo + nxt : dequeue_tile(a.counters, a.ntiles, group);
        tile = __shfl(tile, 0);
        if (tile >= a.ntiles) break;
        // every lane of the wave stays in the tile's loops (compacted leaf phases deal entries to all 64 lanes);
        // a lane without a query (past the phase's units, or a non-finite row) only helps
        const size_t k = (size_t)tile * 64 + lane;
        size_t i = 0;
        bool live = k < a.nunits;
        if (live) {
            i = slot_of(a, k);
            live = i < a.S;
        }
        const D3 q = live ? load_q(a, i) : D3{0.0, 0.0, 0.0};
        if (lane == 0) nxt = glo < ghi ? atomicAdd(&a.counters[group * 32], 1u) : ~0u;
        if (live && a.inv_w && !a.direct) a.inv_w[a.qperm[i]] = (uint32_t)i;
        auto pol = make_pol<MODE>(a, i, q);
        const bool fin = live && finite3(q);
        if (live && !fin) {  // no distance is defined: NO_FACE / NaN, no traversal
            if (!STATS || a.res) write_result<MODE>(a, i, q, pol);
        }
        int hint_leaf = -1;  // STATS
        if constexpr (MODE == 0 || MODE == 3) {
            if (fin && (a.phase == 2 || a.phase == 1)) {
                const int lf = a.phase == 2 ? leader_leaf(a, i, q, kFWin, kLead) : leader_leaf(a, i, q, kLWin * kLead2, kLead2);
                if (STATS) hint_leaf = lf;
                if (lf >= 0) {
                    pol.test(lf);
                    if (STATS) {
                        ++n_leaves;
                        ++n_hinted;
                    }
                }
            }
        }
        if (a.T == 1) {
            if (fin) {
                pol.test(0);
                if (STATS) ++n_leaves;
                if (!STATS || a.res) write_result<MODE>(a, i, q, pol);
            }
            continue;
        }
        QF qf;
        const int root = query_root(a, i, q, qf);
        Walker w{root, 0};
        bool active = fin, deferred = false;
        // leaf children waiting for a wave-wide leaf phase: a per-lane queue of up to kLeafQ leaves
        int q0 = -1, q1 = -1, q2 = -1, q3 = -1, nq = 0;
        // a shift register (no dynamic index, so the queue stays in VGPRs, not in scratch)
        auto enqueue = [&](int x) {
            if (x < 0) return;
            if (kLeafQ > 3) q3 = q2;
            q2 = q1;
            q1 = q0;
            q0 = x;
            ++nq;
        };
        // tests up to `most` queued leaves, newest first (one copy of the fp64 construction in the code: a
        // loop over the queue, not one per entry)
        auto test_queue = [&](int most) {
            const int n = min(nq, most);
#pragma nounroll
            for (int k = 0; k < n; ++k) {
                pol.test(q0);
                q0 = q1;
                q1 = q2;
                if (kLeafQ > 3) q2 = q3;
            }
            nq -= n;
        };
        unsigned steps = 0;
        const unsigned max_steps = (unsigned)min(a.T, (size_t)UINT_MAX);
        unsigned tot = 0;  // STATS: node steps of this lane, restarts included
        // Wave-synchronous loop.  Lanes that reach leaves queue them; a lane keeps traversing while
        // its queue has room for one more leaf.  Leaf tests run as soon as one lane is blocked (or nobody
        // can traverse), so the expensive fp64 leaf path executes for many lanes at once instead of
        // stalling the wave on one lane every iteration (Aila & Laine 2009, "postponed leaf" while-while).
        for (;;) {
            const bool can = active && nq <= kLeafQ - 1;
            const bool has = nq > 0;
            const unsigned long long bl = __ballot(has);
            const unsigned long long bt = __ballot(can);
            if ((bl | bt) == 0ull) break;
            const bool flush = bt == 0ull || __ballot(has && !can) != 0ull;
            if (bl != 0ull && flush) {
                if constexpr (kCompact) {
                    // Compacted leaf phase: the wave's queued leaves (newest first per lane) are dealt to
                    // its 64 lanes, one (leaf, owner) entry each; a lane tests its entry against the
                    // owner's query (ds_bpermute) and each owner takes its entries' (d2, face) back.  The
                    // fp64 construction then runs with (nearly) every lane busy instead of only the
                    // lanes that hold leaves.
                    const unsigned long long lt = (1ull << lane) - 1ull;
                    const unsigned long long m1 = bl, m2 = __ballot(nq >= 2), m3 = __ballot(nq >= 3),
                                             m4 = kLeafQ > 3 ? __ballot(nq >= 4) : 0ull;
                    const int pos = __popcll(m1 & lt) + __popcll(m2 & lt) + __popcll(m3 & lt) + __popcll(m4 & lt);
                    const int E = __popcll(m1) + __popcll(m2) + __popcll(m3) + __popcll(m4);
                    if (nq >= 1) ent[pos] = make_uint2((unsigned)q0, (unsigned)lane);
                    if (nq >= 2) ent[pos + 1] = make_uint2((unsigned)q1, (unsigned)lane);
                    if (nq >= 3) ent[pos + 2] = make_uint2((unsigned)q2, (unsigned)lane);
                    if (kLeafQ > 3 && nq >= 4) ent[pos + 3] = make_uint2((unsigned)q3, (unsigned)lane);
                    asm volatile("" ::: "memory");  // the wave's LDS accesses run in order
                    bool better = false;
                    for (int base = 0; base < E; base += 64) {
                        const uint2 en = ent[min(base + lane, E - 1)];  // lanes past E repeat the last entry
                        const int src = (int)en.y;
                        const D3 x = D3{__shfl(pol.q.x, src), __shfl(pol.q.y, src), __shfl(pol.q.z, src)};
                        uint32_t f;
                        const double d2 = pol.eval((int)en.x, x, f);
                        if (STATS && base + lane < E) ++n_leaves;
#pragma unroll
                        for (int e = 0; e < kLeafQ; ++e) {
                            const int at = pos + e - base;
                            const bool mine = e < nq && at >= 0 && at < 64;
                            const int from = mine ? at : lane;
                            const double dk = __shfl(d2, from);
                            const uint32_t fk = (uint32_t)__shfl((int)f, from);
                            if (mine) {
                                const bool b = pol.offer(dk, fk, e == 0 ? q0 : (e == 1 ? q1 : (e == 2 ? q2 : q3)));
                                better |= b;
                                if (STATS && b) ++n_impr;
                            }
                        }
                    }
                    asm volatile("" ::: "memory");
                    if (better) pol.relim();
                    if (STATS && lane == 0) {
                        u_leaf_it += (unsigned long long)((E + 63) / 64);
                        u_leaf_lanes += (unsigned long long)E;
                    }
                    nq = 0;
                } else {
                    if (STATS && lane == 0) {
                        ++u_leaf_it;
                        u_leaf_lanes += __popcll(bl);
                    }
                    if (has) {
                        if (STATS) n_leaves += min(nq, kLeafRound);
                        test_queue(kLeafRound);
                    }
                }
                continue;
            }
            if (STATS && lane == 0) {
                ++u_trav_it;
                u_trav_lanes += __popcll(bt);
            }
            if (can) {
                int l0 = -1, l1 = -1;
                active = w.step_collect<decltype(pol), STATS>(a.nodes, qf, pol, lds, spill, n_nodes, l0, l1,
                                                              kLeafQ - nq);
                enqueue(l0);
                enqueue(l1);
                ++steps;
                if (STATS) ++tot;
                if (active && steps >= max_steps) active = false;  // each node is entered once: corrupt tree
                if (active && steps == a.budget) {
                    const unsigned slot = atomicAdd(a.n_deferred, 1u);
                    if (slot < a.max_deferred) {
                        if (STATS) n_leaves += nq;
                        test_queue(kLeafQ);
                        if ((a.phase == 1 || a.phase == 3 || a.phase == 4) && a.res) {
                            // later phases take hints from this slot before pass 2 answers it: publish the
                            // closest point of the best face so far (a point on the mesh, so a valid upper
                            // bound for its neighbours), or NO_FACE when it has none yet
                            if constexpr (MODE == 0 || MODE == 3) {
                                D3 o = D3{NAN, NAN, NAN};
                                uint32_t f = MSH_NO_FACE;
                                if (pol.best_leaf >= 0) {
                                    D3 ta, tb, tc;
                                    int part;
                                    load_tri(static_cast<const TriRec*>(a.leaves), pol.best_leaf, ta, tb, tc, f);
                                    closest_on_triangle(q, ta, tb, tc, o, part);
                                }
                                store_qres(a.res + i, f, (uint32_t)pol.best_leaf, o.x, o.y, o.z);
                            } else {
                                store_qres(a.res + i, MSH_NO_FACE, 0u, NAN, NAN, NAN);
                            }
                        }
                        a.deferred[slot] = defer_rec(a, i, pol);
                        active = false;
                        deferred = true;  // pass 2 owns this query
                    }
                    // deferred list full: finish here without a budget
                }
            }
        }
        if (STATS) tile_step_stats(a, tot, lane);
        if (deferred) continue;
        if (STATS && fin && hint_leaf >= 0 && pol.best_leaf == hint_leaf) ++n_hint_won;
        if (fin && (!STATS || a.res)) write_result<MODE>(a, i, q, pol);
    }
    if (STATS)
        add_knn_stats(a.stats, lane, n_nodes, n_leaves, n_impr, n_hinted, n_hint_won, u_trav_it, u_trav_lanes, u_leaf_it,
                      u_leaf_lanes);
}

// Lean pass-1 kernel: the headline launch -- phase 0 over every slot of a sorted call, a single tree of > 1 and
// <= 2^20 leaves with a narrow entry cut, direct stores (launch_knn's pass1 checks all of it).  It is k_knn_list's
// path with the node prefetch, written out without the leader / follower starts, the T == 1 path, wide cut records,
// slot-order records, the inv_w store and the instrumented counters.  Its cold arguments are read from the kernarg
// segment after the tile's wave loop (cold_arg), its node step keeps two ring places free and puts the deep stack
// behind one wave-uniform test (WalkerT::step_list), and a lane's walk state is one register.  The walk does not queue
// the cell's hint leaf, evaluated before it starts, a second time (step_list; profiles/r10_*).  Against k_knn_list: 80 SGPR
// spills -> 3, none in the loop; C3 100M 2.533-2.557 -> 2.592-2.610 G q/s (profiles/r07_knn_lean_isa.txt,
// r07_c3_knn_lean_ab.jsonl).  The tile claim, the ring code (run_rounds, the append) and the resume
// append are k_knn_list's, statement for statement, and the deferral record is defer_rec's with max_best read cold: as
// functions shared with it each changes this kernel's code (profiles/knn_split_isa_diff.txt).
template <int MODE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(MSH_KNN_WAVES))) void k_knn_lean(KnnArgs a) {
    static_assert(MODE == 0 || MODE == 3, "closest-point modes");
    typedef Ent4 E;
    __shared__ uint32_t stk[kStack * kBlock];
    __shared__ float4 nbuf[4 * kBlock];
    __shared__ uint32_t lsh[4 * (kRing + 64 * 4)];  // per wave: ring + bd/bfl (u64 per lane each)
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t* lds = stk + tid;
    // the wave's node slots: LDS byte address from a wave-uniform wave index, so M0 is set by scalar code
    const int wv_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wsl = (uint32_t)(size_t)(__attribute__((address_space(3))) float4*)(nbuf + wv_u * 256);
    const float4* nb = nbuf + (tid >> 6) * 256 + lane;
    const unsigned group = blockIdx.x & 7u;
    // the tile claim with its prefetch, as in k_knn_list
    const unsigned glo = (unsigned)(((unsigned long long)a.ntiles * group) >> 3);
    const unsigned ghi = (unsigned)(((unsigned long long)a.ntiles * (group + 1)) >> 3);
    unsigned nxt = ~0u;
    for (;;) {
        unsigned tile = 0;
        if (lane == 0) tile = (nxt != ~0u && glo + nxt < ghi) ? glo + nxt : dequeue_tile(a.counters, a.ntiles, group);
        tile = __shfl(tile, 0);
        if (tile >= a.ntiles) break;
        const size_t k = (size_t)tile * 64 + lane;  // phase 0: unit k is slot k
        size_t i = 0;
        bool live = k < a.S;
        if (live) {
            i = k;
            live = i < a.S;
        }
        const D3 q = live ? load_q(a, i) : D3{0.0, 0.0, 0.0};
        if (lane == 0) nxt = glo < ghi ? atomicAdd(&a.counters[group * 32], 1u) : ~0u;
        auto pol = make_pol<MODE>(a, i, q);
        const bool fin = live && finite3(q);
        // the sorted path's direct stores to the caller's row, their arguments fetched here (cold_arg)
        auto write = [&]() {
            write_direct<MODE>(static_cast<const TriRec*>(a.leaves), (size_t)MSH_COLD_ARG(perm)[i], q, pol,
                               MSH_COLD_ARG(out_face), MSH_COLD_ARG(out_part), MSH_COLD_ARG(out_pt),
                               MSH_COLD_ARG(out_w));
        };
        if (live && !fin) write();  // no distance is defined: NO_FACE / NaN, no traversal
        const size_t cell = fin ? cut_cell(a, q) : kNoCell;
        if (cell != kNoCell) {  // the cell's hint leaf (the closest face found for its centre)
            const int lf = cut_hint_leaf(a.cut[cell * 8]);
            if (lf >= 0) pol.test(lf);
        }
        const int hint = pol.best_leaf;  // evaluated: the walk does not queue it again (step_list; -1: none)
        QF qf;
        const double o[3] = {a.org[0], a.org[1], a.org[2]};  // single tree
        qf = make_qf(q, o, a.tm);
        WalkerT<E> w{0, 0};
        bool start = fin;
        if (cell != kNoCell) start = cut_start_narrow(a.cut, cell, pol, w, lds);
        // the lane's global spill column, worked out only where a deep stack needs it
        auto spill_col = [&]() -> uint2* {
            return MSH_COLD_ARG(spill) + (size_t)blockIdx.x * kBlock * (size_t)MSH_COLD_ARG(spill_depth) + tid;
        };
        if (start && w.node >= 0) node_prefetch(a.nodes, w.node, wsl);
        uint32_t* ring = lsh + (tid >> 6) * (kRing + 64 * 4);
        unsigned long long* bd = reinterpret_cast<unsigned long long*>(ring + kRing);  // per owner: d2 bits
        unsigned long long* bfl = bd + 64;                                              // (face << 32 | leaf)
        bool active = start, deferred = false;  // (active: the last step's result only)
        // the lane's walk state, one VGPR (three lane masks would be kept by scalar code at every iteration): idle,
        // walking, past its budget (its own leaves still wait), deferred
        enum { kIdle = 0, kWalk = 1, kPast = 2, kDeferred = 3 };
        int st = start ? kWalk : kIdle;
        int nq = 0;              // this lane's leaves appended since all of them were last evaluated (a bound)
        unsigned last_pos = 0;   // ring counter of this lane's newest entry
        unsigned head = 0, tail = 0;  // wave-uniform ring counters: entries [head, tail) wait
        unsigned steps = 0;
        const unsigned max_steps = (unsigned)min(a.T, (size_t)UINT_MAX);
        unsigned budget = a.budget;
        // held in an SGPR (left alone, the compiler reloads it from the kernarg segment at every step and waits for it)
        asm volatile("" : "+s"(budget));
        auto run_rounds = [&](unsigned upto) {  // k_knn_list's, without the counters
            while (head != upto) {
                const unsigned n = min(64u, upto - head);
                bd[lane] = (unsigned long long)__double_as_longlong(pol.best);
                bfl[lane] = ~0ull;
                const bool valid = (unsigned)lane < n;
                const uint32_t en = ring[(head + (valid ? (unsigned)lane : 0u)) & (kRing - 1)];
                const int src = (int)(en & 63u);
                const int leaf = (int)(en >> 6);
                const D3 x = D3{__shfl(pol.q.x, src), __shfl(pol.q.y, src), __shfl(pol.q.z, src)};
                uint32_t f;
                const double d2 = pol.eval(leaf, x, f);
                const unsigned long long kb = (unsigned long long)__double_as_longlong(d2);
                asm volatile("" ::: "memory");
                if (valid) atomicMin(&bd[src], kb);
                asm volatile("" ::: "memory");
                if (valid && bd[src] == kb) atomicMin(&bfl[src], ((unsigned long long)f << 32) | (unsigned)leaf);
                asm volatile("" ::: "memory");
                const unsigned long long nb = bd[lane], nf = bfl[lane];
                const double nd = __longlong_as_double((long long)nb);
                const uint32_t nface = (uint32_t)(nf >> 32);
                if (nf != ~0ull && (nd < pol.best || (nd == pol.best && nface < pol.best_face))) {
                    pol.best = nd;
                    pol.best_face = nface;
                    pol.best_leaf = (int)(uint32_t)nf;
                    pol.relim();
                }
                asm volatile("" ::: "memory");
                head += n;
            }
            if ((int)(last_pos - head) < 0) nq = 0;  // every entry of this lane is evaluated
        };
        unsigned dslot = ~0u;  // this lane's deferred-list slot
    walk:
        for (;;) {
            // a lane past its budget defers once its own leaves are evaluated (pass 2 then owns the query); its slot is
            // claimed and its records are written after the loop, so the loop holds no copy of the construction
            if (st == kPast && nq == 0) st = kDeferred;
            // two ring places stay free, so a step hands back both leaf children (step_list)
            const bool can = st == kWalk && nq < kPend - 1;
            const bool any = __ballot(can) != 0ull;
            if (!any && tail == head) break;  // nothing queued and nobody can move: the tile is done
            int l0 = -1, l1 = -1;
            if (can) {
                active = w.step_list(a.nodes, qf, pol, lds, spill_col, l0, l1, nb, wsl, hint);
                ++steps;
                if (active && steps >= max_steps) active = false;  // each node is entered once: corrupt tree
                st = !active ? kIdle : (steps == budget ? kPast : kWalk);
            }
            // append this step's leaves (at most two per lane) to the ring, in lane order
            if (l0 < 0) {
                l0 = l1;
                l1 = -1;
            }
            const unsigned long long m1 = __ballot(l0 >= 0), m2 = __ballot(l1 >= 0);
            const unsigned pos = tail + lanes_below(m1) + lanes_below(m2);
            if (l0 >= 0) {
                ring[pos & (kRing - 1)] = ((uint32_t)l0 << 6) | (uint32_t)lane;
                last_pos = pos;
                ++nq;
            }
            if (l1 >= 0) {
                ring[(pos + 1) & (kRing - 1)] = ((uint32_t)l1 << 6) | (uint32_t)lane;
                last_pos = pos + 1;
                ++nq;
            }
            tail += (unsigned)(__popcll(m1) + __popcll(m2));
            // full rounds while lanes can move; everything once nobody can
            const unsigned upto = any ? head + ((tail - head) & ~63u) : tail;
            if (upto != head) run_rounds(upto);
        }
        {
            // claim the deferred lanes' list slots; with the list full a lane takes its walk up again where it
            // stopped (its pending node is still prefetched), now without a budget: steps is past it
            bool again = false;
            const unsigned max_deferred = MSH_COLD_ARG(max_deferred);
            deferred = st == kDeferred;
            if (deferred && dslot == ~0u) {
                dslot = atomicAdd(MSH_COLD_ARG(n_deferred), 1u);
                if (dslot >= max_deferred) {
                    deferred = false;
                    active = true;
                    st = kWalk;
                    again = true;
                }
            }
            if (__ballot(again) != 0ull) goto walk;
            // only a lane that holds a slot of the list is deferred: steps is past the budget after a refused claim,
            // so the walk state does not ask to defer a second time
            deferred = deferred && dslot < max_deferred;
        }
        // defer_rec written out (through it max_best is no cold_arg: 8 more instructions), then k_knn_list's resume append
        if (deferred) {
            DeferRec r;
            r.slot = (uint32_t)i;
            r.face = pol.best_face;
            r.leaf = pol.best_leaf;
            r.roff = 0;
            r.best = pol.best;
            r.rcnt = 0;
            r.sbound = 0x7F800000u;  // +inf
            unsigned long long* const max_best = MSH_COLD_ARG(max_best);
            if (max_best) atomicMax(max_best, (unsigned long long)__double_as_longlong(pol.best));
            uint2* const resume = MSH_COLD_ARG(resume);
            if (resume) {
                const unsigned cnt = (unsigned)w.sp + 1;
                const unsigned off = atomicAdd(MSH_COLD_ARG(n_resume), cnt);
                if (off + cnt <= MSH_COLD_ARG(resume_cap)) {
                    uint2* dst = resume + off;
                    const uint2* sp_col = w.sp > kStack ? spill_col() : nullptr;
                    for (int j = 0; j < w.sp; ++j) {
                        const uint32_t e = stack_get(lds, sp_col, j);
                        dst[j] = make_uint2((uint32_t)E::ref(e), __float_as_uint(E::bound(e)));
                    }
                    dst[w.sp] = make_uint2((uint32_t)w.node, 0u);
                    r.roff = off;
                    r.rcnt = cnt;
                }
            }
            MSH_COLD_ARG(deferred)[dslot] = r;
            continue;
        }
        if (fin) write();
    }
    // a lane that stopped (deferred) may still have a node prefetch in flight: it lands before the block's LDS is
    // released
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

constexpr int kFront = 512;  // pass 2: 2 kFront work-list entries per wave (LDS)

template <int MODE, bool STATS>
__global__ __launch_bounds__(kBlock) void k_knn_coop(KnnArgs a) {
    __shared__ uint2 stk[kStack * kBlock];
    __shared__ uint2 front[4][2][kFront];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint2* lds = stk + tid;
    uint2* spill = a.spill ? a.spill + (size_t)blockIdx.x * kBlock * (size_t)a.spill_depth + tid : nullptr;
    const unsigned total = min(*a.n_deferred, a.max_deferred);
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    unsigned n_nodes = 0, n_leaves = 0;
    unsigned* next_item = a.n_deferred + 32;  // items are dealt dynamically: their costs vary widely
    // work units: the heavy items' K parts first (consecutive units: the parts run side by side), then every item in
    // order, the heavy ones skipped
    constexpr unsigned K = (MODE == 0 || MODE == 3) ? kP2Split : 1u;
    const unsigned nsplit = (K > 1 && a.cand) ? min(*a.n_heavy, kP2SplitItems) : 0u;
    const unsigned nunit = nsplit * K + total;
    for (;;) {
        unsigned unit = 0;
        if (lane == 0) unit = atomicAdd(next_item, 1u);
        unit = __shfl(unit, 0);
        if (unit >= nunit) break;
        const bool split = unit < nsplit * K;
        const unsigned hidx = split ? unit / K : 0u;
        const unsigned item = split ? a.heavy[hidx] : unit - nsplit * K;
        const unsigned part = split ? unit % K : 0u, kk = split ? K : 1u;
        if (!split && nsplit && a.deferred[item].sbound != kP2Whole) continue;  // a heavy item: its parts ran above
        const unsigned item_nodes0 = n_nodes, item_leaves0 = n_leaves;
        const DeferRec r = a.deferred[item];
        const size_t i = r.slot;
        const D3 q = load_q(a, i);
        QF qf;
        const int root = query_root(a, i, q, qf);
        auto pol = make_pol<MODE>(a, i, q);
        pol.shared = r.best;  // pass-1 best: an upper bound of the final best
        unsigned rounds = 0;
        // an item's parts share their bound: every 8th round a part publishes its own and takes the others'
        auto share = [&]() {
            if (!split || (++rounds & 7u) != 0u) return;
            unsigned old = 0;
            if (lane == 0) old = atomicMin(&a.deferred[item].sbound, __float_as_uint(__double2float_ru(pol.shared)));
            old = (unsigned)__shfl((int)old, 0);
            pol.shared = fmin(pol.shared, (double)__uint_as_float(old));
        };
        if (lane == 0) {
            pol.best = r.best;
            pol.best_face = r.face;
            pol.best_leaf = r.leaf;
        }
        pol.relim();
        // Subtree work list, last in first out, expanded 64 entries at a time (one per lane): children
        // within the bound go back on the list (compacted by ballot), leaf children are tested on the spot.
        // Taking the 64 newest entries keeps the walk deep-first, so good leaves (and the shared bound)
        // come early.  Most items finish here at full wave width; a list that would outgrow LDS is dealt
        // to the lanes' own stacks for depth-first walks.
        uint2* W = &front[wv][0][0];  // kWork contiguous entries
        constexpr int kWork = 2 * kFront;
        // pass 1's unexplored entries (oldest first, its pending node on top), or the root
        // (a split item's part p: entries p, p + K, p + 2K, ... in their order; the root, when pass 1 left none, to part 0)
        const int rc = (int)r.rcnt;
        int top = 1;
        if (rc > 0 && rc <= kWork - 128) {
            const int cnt = rc > (int)part ? (rc - (int)part + (int)kk - 1) / (int)kk : 0;
            for (int m = lane; m < cnt; m += 64) W[m] = a.resume[r.roff + part + (unsigned)m * kk];
            top = cnt;
        } else if (part != 0) {
            top = 0;
        } else if (lane == 0) {
            W[0] = make_uint2((unsigned)root, 0u);
        }
        __builtin_amdgcn_wave_barrier();
        while (top > 0 && top <= kWork - 128) {
            const int nt = min(64, top);
            const int base = top - nt;
            bool k0 = false, k1 = false;
            uint2 e0, e1;
            int lf0 = -1, lf1 = -1;  // leaves to test: a resumed leaf entry, or leaf children within the bound
            if (lane < nt) {
                const uint2 e = W[base + lane];
                if (__uint_as_float(e.y) <= pol.limf) {
                    if ((int)e.x < 0) {
                        lf0 = ~(int)e.x;
                    } else {
                        const NodeV nd = load_node(a.nodes, (int)e.x);
                        ++n_nodes;
                        float d0, d1;
                        node_child_bounds(nd, qf, d0, d1);
                        const int c0 = nd.child(0), c1 = nd.child(1);
                        if (d0 <= pol.limf) {
                            if (c0 < 0) lf0 = ~c0;
                            else { k0 = true; e0 = make_uint2((unsigned)c0, __float_as_uint(d0)); }
                        }
                        if (d1 <= pol.limf) {
                            if (c1 < 0) lf1 = ~c1;
                            else { k1 = true; e1 = make_uint2((unsigned)c1, __float_as_uint(d1)); }
                        }
                    }
                }
            }
#pragma nounroll
            for (int j = 0; j < 2; ++j) {  // one call site of the construction
                const int lf = j == 0 ? lf0 : lf1;
                if (lf >= 0) {
                    pol.test(lf);
                    ++n_leaves;
                }
            }
            __builtin_amdgcn_wave_barrier();
            const unsigned long long b0 = __ballot(k0), b1 = __ballot(k1);
            const int p0 = base + __popcll(b0 & lt) + __popcll(b1 & lt);
            if (k0) W[p0] = e0;
            if (k1) W[p0 + (k0 ? 1 : 0)] = e1;
            top = base + __popcll(b0) + __popcll(b1);
            __builtin_amdgcn_wave_barrier();
            pol.shared = fmin(pol.shared, wave_min(pol.best));
            share();
            pol.relim();
        }
        // overflow: deal the list to the lanes (entry j -> lane j % 64), then depth-first walks
        const int n = top;
        Walker w{0, 0};
        if (lane < n)
            for (int j = lane + ((n - 1 - lane) / 64) * 64; j >= lane; j -= 64) w.push(W[j].x, W[j].y, lds, spill);
        bool active = w.pop(pol, lds, spill);
        while (__any(active)) {
            if (active) active = w.step<decltype(pol), false>(a.nodes, qf, pol, lds, spill, n_nodes, n_leaves);
            pol.shared = fmin(pol.shared, wave_min(pol.best));
            share();
            pol.relim();
        }
        double best = pol.best;
        uint32_t face = pol.best_face;
        int leaf = pol.best_leaf;
        wave_lexmin(best, face, leaf);
        if (split) {  // the part's candidate; k_knn_combine merges the item's parts and writes the answer
            if (lane == 0 && !STATS) a.cand[(size_t)hidx * K + part] = P2Cand{best, face, leaf};
        } else if (lane == 0 && !STATS) {
            pol.best = best;
            pol.best_face = face;
            pol.best_leaf = leaf;
            write_result<MODE>(a, i, q, pol);
        }
        if (STATS) {  // per-item work: stats[44] sum and stats[45] max of node + leaf visits over the wave
            unsigned w = (n_nodes - item_nodes0) + (n_leaves - item_leaves0);
            for (int o = 32; o > 0; o >>= 1) w += (unsigned)__shfl_xor((int)w, o);
            if (lane == 0) {
                atomicAdd(&a.stats[44], (unsigned long long)w);
                atomicMax(&a.stats[45], (unsigned long long)w);
                atomicAdd(&a.stats[46], 1ull);
                a.deferred[item].sbound = w;  // development dump (MESH_AMD_P2_DUMP): the item's visits
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (STATS) {
        atomicAdd(&a.stats[0], (unsigned long long)n_nodes);
        atomicAdd(&a.stats[1], (unsigned long long)n_leaves);
        if (lane == 0) atomicAdd(&a.stats[6], 1ull);  // waves x deferred items (pass-2 work units)
    }
}

// pass 2's plan: the deferred items whose pass-1 distance is within kP2Heavy of the largest are listed in heavy[]
// (sbound +inf, the parts' shared bound); every other item is marked to run whole (sbound kP2Whole)
__global__ __launch_bounds__(kBlock) void k_p2_plan(KnnArgs a) {
    const unsigned total = min(*a.n_deferred, a.max_deferred);
    const double mb = __longlong_as_double((long long)*a.max_best);
    const double thr = mb * (kP2Heavy * kP2Heavy);
    for (unsigned k = blockIdx.x * kBlock + threadIdx.x; k < total; k += gridDim.x * kBlock) {
        uint32_t mark = kP2Whole;
        if (a.deferred[k].best >= thr) {
            const unsigned h = atomicAdd(a.n_heavy, 1u);
            if (h < kP2SplitItems) {
                a.heavy[h] = k;
                mark = 0x7F800000u;
            }
        }
        a.deferred[k].sbound = mark;
    }
}

// the answers of the split pass-2 items: the lexicographic (d2, face) minimum of their parts' candidates (each
// part starts from the pass-1 candidate, so every part holds a real one)
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_knn_combine(KnnArgs a) {
    if constexpr (MODE == 0 || MODE == 3) {
        const unsigned nsplit = min(*a.n_heavy, kP2SplitItems);
        const unsigned h = blockIdx.x * kBlock + threadIdx.x;
        if (h >= nsplit) return;
        const DeferRec r = a.deferred[a.heavy[h]];
        const size_t i = r.slot;
        const D3 q = load_q(a, i);
        auto pol = make_pol<MODE>(a, i, q);
        pol.best = r.best;
        pol.best_face = r.face;
        pol.best_leaf = r.leaf;
#pragma unroll
        for (unsigned p = 0; p < kP2Split; ++p) {
            const P2Cand c = a.cand[(size_t)h * kP2Split + p];
            if (c.leaf >= 0) pol.offer(c.best, c.face, c.leaf);
        }
        write_result<MODE>(a, i, q, pol);
    }
}

#ifndef MSH_BUDGET
#define MSH_BUDGET 512
#endif
constexpr unsigned kBudget = MSH_BUDGET;  // pass-1 node steps per lane before a query is deferred
// super-leaders: their launch has few tiles (C3: 6104 for 8192 wave slots), so its slowest tile sets its
// length; with 256 steps the launch takes 1.4 instead of 2.9 ms and pass 2 gets ~18k more (cheap) items
// (+0.4 ms).  A deferred super-leader publishes its best point so far as its leaders' hint.
constexpr unsigned kBudget3 = 256;
constexpr unsigned kBudget1 = MSH_BUDGET;  // leaders (C3: 13.8 -> 12.6 ms, pass 2 +0.5 ms)
constexpr unsigned kKnnBlocksPerCU = 4;  // resident pass-1 blocks per CU (persistent grid)

// Common launch: grid, counters, spill area, deferred list; pass 1 then pass 2 (both also in STATS
// mode, so the instrumented counts describe the traversal that is timed).
template <int MODE, bool STATS>
static int launch_knn(msh_tree* tree, KnnArgs a, hipStream_t s, const char* timer) {
    if (a.S == 0) return MSH_OK;
    for (int k = 0; k < 3; ++k) a.org[k] = tree->origin[k];
    const unsigned ncu = (unsigned)device_cus(tree->device);
    Workspace& ws = tree->ws;
    // counters: 8 group counters (one 128-B line each) + the deferred count + pass 2's item counter + the resume arena's
    // + the largest deferred best + the heavy items' count
    MSH_TRY(ws.counters.reserve(13 * 32 * sizeof(unsigned)));
    a.counters = ws.counters.as<unsigned>();
    a.n_deferred = a.counters + 8 * 32;
    a.n_resume = a.counters + 10 * 32;
    MSH_HIP(hipMemsetAsync(a.counters, 0, 13 * 32 * sizeof(unsigned), s));  // + the pass-2 item counter
    const size_t n_lead = (a.S + kLead - 1) / kLead;
    const unsigned max_tiles = (unsigned)((a.S + 63) / 64);
    const unsigned nblk_max = std::min<unsigned>((max_tiles + 3) / 4, ncu * kKnnBlocksPerCU);
    // pass 2 lanes carry up to 2 kFront/64 dealt subtrees on top of a depth-first path
    const unsigned nblk2 = ncu * 2;  // pass 2: 2 blocks per CU
    const int need = tree->max_depth + 1 + 2 * kFront / 64 + 1 + (a.cut ? kCutK : 0);
    MSH_TRY(plan_spill(ws, need, kStack, std::max(nblk_max, nblk2), &a.spill, &a.spill_depth));
    a.budget = kBudget;
    bool list_pf = false;  // list path with the LDS node prefetch and 4-B stack entries (k_knn_list PF)
    {
        // test hook: 0 per-lane leaf queues (the path of trees of >= 2^26 leaves), 2 the list without the node
        // prefetch (the path of trees of more than 2^20 leaves)
        const char* e = getenv("MESH_AMD_LEAF_LIST");
        const int hook = e ? atoi(e) : 1;
        a.list = (MODE == 0 || MODE == 3) && hook != 0 && tree->B * tree->T < kListMaxLeaves;
        list_pf = a.list && hook != 2 && tree->B * tree->T <= kEnt4MaxLeaves;
    }
    // leader ordering: closest-point launches over a sorted slot order (records in a.res); leader phases only for
    // trees of >= kLeadMinLeaves leaves (on a small tree the hint saves little and the three dependent launches
    // serialise their slowest tiles: C1 0.56 -> 0.29 ms), and only without the entry cut's cell hints: every query inside the cut's grid starts from its cell's entries
    // with the hint leaf of the cell centre, and the leader launch's hints for the followers no longer pay for the
    // launch (C3 100M: 1985-1990 -> 2150-2179 M q/s without leader phases; one N = 8 shard of 12.5M rows 9.0 ->
    // 7.55 ms, profiles/r05_ab_leaders_sort_resume.jsonl); batched trees and trees without a cut keep them
    static_assert(kLead > 1 && kLead2 == 256, "the leader phases below: leaders, and super-leaders among them");
    const bool lead = (MODE == 0 || MODE == 3) && a.res != nullptr && a.S >= 64 * (size_t)kLead &&
                      a.T >= kLeadMinLeaves && !(a.list && a.cut);
    a.max_deferred = (unsigned)std::min<size_t>(a.S, (a.S / 16) + 65536);
    // test hook: a shorter deferred list, so that a few rows past their budget fill it (a lane that finds it full
    // finishes its walk in pass 1 without a budget)
    if (const char* e = getenv("MESH_AMD_MAX_DEFERRED"))
        a.max_deferred = std::min<unsigned>(a.max_deferred, (unsigned)std::max(1, atoi(e)));
    DevBuf& dbuf = ws.flags;
    MSH_TRY(dbuf.reserve((size_t)a.max_deferred * sizeof(DeferRec)));
    a.deferred = dbuf.as<DeferRec>();
    a.resume = nullptr;
    a.resume_cap = 0;
    a.cand = nullptr;
    a.heavy = nullptr;
    a.n_heavy = a.counters + 12 * 32;
    a.max_best = reinterpret_cast<unsigned long long*>(a.counters + 11 * 32);
    const unsigned split_cap = std::min<unsigned>(a.max_deferred, kP2SplitItems);
    if (kP2Split > 1 && (MODE == 0 || MODE == 3) && !STATS) {
        MSH_TRY(ws.p2cand.reserve((size_t)split_cap * (kP2Split * sizeof(P2Cand) + sizeof(unsigned))));
        a.cand = ws.p2cand.as<P2Cand>();
        a.heavy = reinterpret_cast<unsigned*>(a.cand + (size_t)split_cap * kP2Split);
    }
    if (a.list) {  // resume arena: ~48 entries per expected deferral (C3: 75k deferred of 100M queries), >= 1M entries
        const size_t cap = std::min<size_t>((size_t)1 << 26, std::max<size_t>((size_t)1 << 20, 48 * (a.S / 1024 + 1024)));
        MSH_TRY(ws.resume.reserve(cap * sizeof(uint2)));
        a.resume = ws.resume.as<uint2>();
        a.resume_cap = (unsigned)cap;
    }
    // the lean kernel takes the cut-started unled launch (k_knn_lean); test hook MESH_AMD_KNN_LEAN=0: the generic one
    bool lean = false;
    if constexpr (!STATS && (MODE == 0 || MODE == 3)) {
        const char* e = getenv("MESH_AMD_KNN_LEAN");
        lean = (!e || atoi(e) != 0) && a.list && list_pf && a.cut && !a.cut_wide && a.direct && a.T > 1 &&
               !a.orgs;
    }
    auto pass1 = [&](int phase, size_t nunits, const char* name) -> int {
        a.phase = phase;
        a.budget = phase == 3 ? kBudget3 : ((phase == 1 || phase == 4) ? kBudget1 : kBudget);
        // small trees: a query that walks T/16 nodes (the centre of a coarse closed mesh) goes to the
        // wave-cooperative pass 2 instead of holding its tile for up to T serial steps (C1, 840 faces:
        // traversal 1.15 -> 0.56 ms; with no leader phases below, 0.29 ms)
        a.budget = std::min<unsigned>(a.budget, (unsigned)std::max<size_t>(64, a.T / 16));
        a.nunits = nunits;
        a.ntiles = (unsigned)((nunits + 63) / 64);
        const unsigned nblk = std::min<unsigned>((a.ntiles + 3) / 4, ncu * kKnnBlocksPerCU);
        if (nblk == 0) return MSH_OK;
        const bool take_lean = lean && phase == 0;
        TimedLaunch t1(take_lean ? "knn_lean" : name, s);  // its own timer name: tests tell the two kernels apart
        if (take_lean) {  // (lean is false in the other modes and in instrumented launches)
            if constexpr (!STATS && (MODE == 0 || MODE == 3)) k_knn_lean<MODE><<<nblk, kBlock, 0, s>>>(a);
        } else if (a.list) {  // (false in the other modes)
            if constexpr (MODE == 0 || MODE == 3) {
                if (list_pf)
                    k_knn_list<MODE, STATS, true><<<nblk, kBlock, 0, s>>>(a);
                else
                    k_knn_list<MODE, STATS, false><<<nblk, kBlock, 0, s>>>(a);
            }
        } else {
            k_knn_queue<MODE, STATS><<<nblk, kBlock, 0, s>>>(a);
        }
        MSH_HIP(hipGetLastError());
        return MSH_OK;
    };
    {
        TimedLaunch tl(timer, s);
        {
            TimedLaunch t1(STATS ? "knn_pass1_stats" : "knn_pass1", s);
            if (lead) {
                if (a.list && a.cut) {
                    // cell hints serve every leader inside the entry cut's grid, so the super-leaders would only
                    // hint leaders outside it: one leader launch over every leader slot (phase 4; outside the
                    // grid unhinted) instead of a super-leader launch the chip cannot fill
                    MSH_TRY(pass1(4, n_lead, STATS ? "knn_lead_stats" : "knn_lead"));
                } else {
                    const size_t n_super = (a.S + kLead2 - 1) / kLead2;
                    MSH_TRY(pass1(3, n_super, STATS ? "knn_lead2_stats" : "knn_lead2"));
                    MSH_HIP(hipMemsetAsync(a.counters, 0, 8 * 32 * sizeof(unsigned), s));
                    MSH_TRY(pass1(1, n_lead - n_super, STATS ? "knn_lead_stats" : "knn_lead"));
                }
                MSH_HIP(hipMemsetAsync(a.counters, 0, 8 * 32 * sizeof(unsigned), s));  // group counters only
                MSH_TRY(pass1(2, a.S - n_lead, STATS ? "knn_follow_stats" : "knn_follow"));
            } else {
                MSH_TRY(pass1(0, a.S, STATS ? "knn_all_stats" : "knn_all"));
            }
        }
        {
            TimedLaunch t2(STATS ? "knn_pass2_stats" : "knn_pass2", s);
            if (a.cand) {
                k_p2_plan<<<64, kBlock, 0, s>>>(a);
                MSH_HIP(hipGetLastError());
            }
            k_knn_coop<MODE, STATS><<<nblk2, kBlock, 0, s>>>(a);
            MSH_HIP(hipGetLastError());
            if (a.cand) {
                k_knn_combine<MODE><<<blocks_for(split_cap), kBlock, 0, s>>>(a);
                MSH_HIP(hipGetLastError());
            }
        }
        if (STATS && getenv("MESH_AMD_P2_DUMP")) {  // development: the deferred items with their pass-2 visits
            unsigned nd = 0;
            MSH_HIP(hipMemcpyAsync(&nd, a.n_deferred, sizeof(unsigned), hipMemcpyDeviceToHost, s));
            MSH_HIP(hipStreamSynchronize(s));
            nd = std::min(nd, a.max_deferred);
            std::vector<DeferRec> h(nd);
            if (nd) MSH_HIP(hipMemcpy(h.data(), a.deferred, nd * sizeof(DeferRec), hipMemcpyDeviceToHost));
            if (FILE* f = fopen(getenv("MESH_AMD_P2_DUMP"), "wb")) {
                fwrite(h.data(), sizeof(DeferRec), nd, f);
                fclose(f);
            }
        }
    }
    return MSH_OK;
}


// Slot-order plumbing shared by the point-query launchers: with a permutation the kernels write 32-B
// records (plus nw weights) into the workspace and k_unpermute scatters them to the caller's arrays.
template <int MODE, bool STATS>
static int run_knn(msh_tree* tree, KnnArgs a, const QueryOrder& ord, const SlotOut& o, int nw, hipStream_t s,
                   const char* timer) {
    if (a.S == 0) return MSH_OK;
    a.q = ord.q;
    a.perm = ord.perm;
    if (!ord.gathered) {
        a.qperm = ord.perm;
        a.inv_w = const_cast<uint32_t*>(ord.inv);
    }
    Workspace& ws = tree->ws;
    if (ord.perm) {  // STATS launches keep the records too: followers take their hints from them
        MSH_TRY(ws.res.reserve(a.S * sizeof(QRes)));
        a.res = ws.res.as<QRes>();
        a.direct = !STATS && (MODE == 0 || MODE == 3);
        a.rec_leaf = a.direct || STATS;
        if (nw && !a.direct) {
            MSH_TRY(ws.res_w.reserve(a.S * (size_t)nw * sizeof(double)));
            a.res_w = ws.res_w.as<double>();
        }
        if (a.direct) {
            a.out_face = o.face;
            a.out_part = o.part;
            a.out_pt = o.pt;
            a.out_dist = o.dist;
            a.out_w = o.w;
        }
    } else {
        a.out_face = o.face;
        a.out_part = o.part;
        a.out_pt = o.pt;
        a.out_dist = o.dist;
        a.out_w = o.w;
    }
    MSH_TRY((launch_knn<MODE, STATS>(tree, a, s, timer)));
    if (ord.perm && !STATS && !a.direct) MSH_TRY(unpermute_results(a.res, a.res_w, nw, ord.inv, a.S, o, s));
    return MSH_OK;
}

static KnnArgs tree_args(const msh_tree* tree, size_t S) {
    KnnArgs a{};
    a.nodes = tree->d_nodes;
    a.leaves = tree->d_leaves;
    a.T = tree->T;
    a.S = S;
    a.tm = tree_margin(tree->half_diag);
    return a;
}

// the entry cut of a single tree (list path of the closest-point modes)
static void cut_args(const msh_tree* tree, KnnArgs& a) {
    if (!tree->d_cut || tree->B != 1) return;
    a.cut = tree->d_cut;
    a.cut_wide = tree->cut_wide;
    a.cut_G = tree->cut_G;
    for (int k = 0; k < 3; ++k) {
        a.cut_lo[k] = tree->cut_lo[k];
        a.cut_iw[k] = tree->cut_iw[k];
    }
}

int launch_nearest(const msh_tree* tree, const QueryOrder& ord, size_t S, const SlotOut& o, hipStream_t s) {
    KnnArgs a = tree_args(tree, S);
    cut_args(tree, a);
    SlotOut oo = o;
    oo.dist = nullptr;
    if (o.w) {
        oo.part = nullptr;
        return run_knn<3, false>(const_cast<msh_tree*>(tree), a, ord, oo, 3, s, "nearest");
    }
    return run_knn<0, false>(const_cast<msh_tree*>(tree), a, ord, oo, 0, s, "nearest");
}

int launch_nearest_batch(const msh_tree* tree, const QueryOrder& ord, size_t n, size_t S, const SlotOut& o,
                         hipStream_t s, size_t mesh0) {
    KnnArgs a = tree_args(tree, n);
    a.orgs = tree->d_orgs + 3 * mesh0;
    a.qper = S;
    a.npm = tree->T - 1;
    a.root0 = mesh0 * a.npm;
    SlotOut oo = o;
    oo.dist = nullptr;
    if (o.w) {
        oo.part = nullptr;
        return run_knn<3, false>(const_cast<msh_tree*>(tree), a, ord, oo, 3, s, "nearest_batch");
    }
    return run_knn<0, false>(const_cast<msh_tree*>(tree), a, ord, oo, 0, s, "nearest_batch");
}

int launch_nearest_stats(const msh_tree* tree, const QueryOrder& ord, size_t S, unsigned long long* d_counts,
                         hipStream_t s) {
    KnnArgs a = tree_args(tree, S);
    cut_args(tree, a);
    a.stats = d_counts;
    return run_knn<0, true>(const_cast<msh_tree*>(tree), a, ord, SlotOut{}, 0, s, "nearest_stats");
}

int launch_nnearest(const msh_tree* tree, const QueryOrder& ord, size_t S, const SlotOut& o, hipStream_t s) {
    KnnArgs a = tree_args(tree, S);
    a.n = ord.n;
    a.eps = tree->eps;
    SlotOut oo = o;
    oo.part = nullptr;
    oo.dist = nullptr;
    oo.w = nullptr;
    return run_knn<1, false>(const_cast<msh_tree*>(tree), a, ord, oo, 0, s, "nnearest");
}

int launch_points_nearest(const msh_tree* tree, const QueryOrder& ord, size_t S, const SlotOut& o, hipStream_t s) {
    KnnArgs a = tree_args(tree, S);
    SlotOut oo{};
    oo.face = o.face;
    oo.dist = o.dist;
    return run_knn<2, false>(const_cast<msh_tree*>(tree), a, ord, oo, 0, s, "points_nearest");
}

}  // namespace msh
