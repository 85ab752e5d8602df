// The shared vocabulary of the closest-point kernels (nearest.hip: pass 1 and pass 2; cutbuild.hip packs the entry
// cut's records with Ent4): the launch arguments, the deferred-query records, the leaf policies, the stack entries and
// the per-lane walker, the result writes, the leader and entry-cut starts, and pass 1's tuning constants.  The
// pipeline and the execution shape are described at the head of nearest.hip.
#pragma once
#include <cstddef>
#include <type_traits>

#include "internal.h"

namespace msh {

struct DeferRec {
    uint32_t slot;
    uint32_t face;
    int32_t leaf;
    uint32_t roff;   // first of the query's resume entries (KnnArgs::resume)
    double best;
    uint32_t rcnt;   // resume entries: pass 1's unexplored work (0: pass 2 starts at the root)
    uint32_t sbound; // pass 2, an item split over waves: their shared bound, fp32 bits rounded up (atomicMin)
};
static_assert(sizeof(DeferRec) == 32, "DeferRec must be 32 B");

// Pass 2 ends with its longest item: on C3 every deferred query lies near the sphere's centre, and their walks grow
// steeply as they approach it (12.5M shard: 8,239 items of 250 node visits on average, the longest 19,688;
// profiles/r06_c3_shard_pass2_r5_vs_r6.jsonl, r06_c3_p2_items.json).  So the items whose pass-1 distance is within
// kP2Heavy of the largest one (k_p2_plan) are split over kP2Split waves, dealt before the others: part p takes every
// kP2Split-th of the item's resume entries, the parts share their bound through DeferRec::sbound, and k_knn_combine
// merges their candidates.  (Splitting every item: 12.5M shard pass 2 0.63 -> 0.50 ms at 2 parts, 0.68 at 4; 100M
// 1.14 -> 3.2 ms at 4: the parts' fixed costs.)
#ifndef MSH_P2_SPLIT
#define MSH_P2_SPLIT 8
#endif
#ifndef MSH_P2_HEAVY
#define MSH_P2_HEAVY 0.97
#endif
constexpr unsigned kP2Split = MSH_P2_SPLIT;
constexpr double kP2Heavy = MSH_P2_HEAVY;      // split items with sqrt(best) >= kP2Heavy sqrt(the largest best)
constexpr unsigned kP2SplitItems = 1u << 16;  // at most this many items split: 8 MB of candidates
constexpr uint32_t kP2Whole = 0xFFFFFFFFu;    // DeferRec::sbound of an item run whole (k_p2_plan)
struct P2Cand {
    double best;
    uint32_t face;
    int32_t leaf;
};

// MODE: 0 closest point (face, part, point), 1 normals metric (face, point), 2 vertex NN (index,
// distance), 3 closest point + barycentric weights (face, point, weights)
struct KnnArgs {
    const BNode* nodes;
    const void* leaves;
    size_t T;
    const double* q;       // query rows in slot order (Morton-sorted copy, or the caller's array)
    const double* n;       // MODE 1: query normals in slot order
    const uint32_t* perm;  // slot -> caller's query index (nullptr: identity)
    const uint32_t* qperm; // non-null: q holds the caller's rows and slot i reads row qperm[i]
    uint32_t* inv_w;       // with qperm: pass 1 records inv_w[qperm[i]] = i
    size_t S;
    QRes* res;             // slot-order records (sorted path); nullptr: write the caller's arrays below
    double* res_w;         // MODE 3 slot-order barycentric weights (3 per slot)
    uint32_t* out_face;
    uint32_t* out_part;
    double* out_pt;
    double* out_dist;
    double* out_w;
    double eps;
    double org[3];  // tree origin: fp32 node bounds are relative to it
    double tm;      // tree_margin(tree->half_diag): the node bounds' share of the query margin (make_qf)
    // batched trees (msh_batch_build): slot i belongs to mesh i / qper (the batched sort is mesh-major),
    // whose root is node mesh * npm and whose origin is orgs[3 * mesh]; orgs == nullptr: single tree
    const double* orgs;
    size_t qper;
    size_t npm;
    size_t root0;  // batched trees: root of the launch's first mesh (a launch over meshes [mesh0, ...): mesh0 * npm)
    unsigned* counters;
    unsigned ntiles;
    uint2* spill;
    int spill_depth;
    unsigned long long* stats;
    unsigned budget;
    // leader / follower ordering (sorted closest-point launches, MODE 0 and 3): phase 0 = every slot,
    // unhinted; phase 1 = leader slots (i % kLead == 0); phase 2 = the other slots, each starting from the
    // leaf of the nearest leader's closest point in its 64-slot window (see leader_leaf)
    int phase;
    // direct: the sorted path writes each answer straight to the caller's row perm[i] (no k_unpermute);
    // slot-order records are kept only for the leader phases, whose records are the followers' hints
    bool direct;
    // rec_leaf: slot-order records are hints only (direct stores, or instrumented launches), so their part
    // field carries the winner's leaf index instead of its part code (leader_leaf)
    bool rec_leaf;
    bool list;      // closest-point modes: wave leaf list (trees of < 2^26 leaves) instead of per-lane queues
    // entry cut (list path; single trees): a query inside the grid starts from its cell's record -- the cell's hint
    // leaf and up to kCutK start entries -- instead of the root (build_entry_cut); nullptr: from the root
    const uint32_t* cut;
    int cut_wide;  // records of 64 B with 8-B entries (trees of > 2^20 leaves); else 32 B with 4-B entries
    int cut_G;
    double cut_lo[3], cut_iw[3];
    size_t nunits;  // work units of this phase (slots it covers)
    DeferRec* deferred;
    unsigned* n_deferred;
    unsigned max_deferred;
    // pass-1 work a deferred query leaves (list path): its pending node and its stack as (ref, fp32 bound bits),
    // appended to one arena, from which pass 2 resumes instead of walking again from the root; a query that does
    // not fit keeps rcnt = 0
    uint2* resume;
    unsigned* n_resume;
    unsigned resume_cap;
    // pass 2: the heavy items (k_p2_plan: heavy[0, *n_heavy)) run as kP2Split parts whose candidates go to cand
    // (k_knn_combine); max_best: pass 1's largest deferred best (d2 bits)
    P2Cand* cand;
    unsigned* heavy;
    unsigned* n_heavy;
    unsigned long long* max_best;
};

// root node and fp32 query of slot i (batched trees: its mesh's root and origin)
__device__ inline int query_root(const KnnArgs& a, size_t i, const D3& q, QF& qf) {
    if (a.orgs) {
        const size_t mb = i / a.qper;
        const double o[3] = {a.orgs[3 * mb], a.orgs[3 * mb + 1], a.orgs[3 * mb + 2]};
        qf = make_qf(q, o, a.tm);
        return (int)(a.root0 + mb * a.npm);
    }
    const double o[3] = {a.org[0], a.org[1], a.org[2]};
    qf = make_qf(q, o, a.tm);
    return 0;
}

// ---- leaf policies ----
// limit(): squared radius (in box-distance units) inside which a primitive can still beat or tie the
// best.  `shared` is a bound published by other lanes working on the same query (pass 2); it is always
// >= the final best, so pruning with min(best, shared) keeps the result exact.  limf caches
// limit() rounded up to fp32 (the unit of the node bounds); relim() refreshes it whenever best or
// shared changes, so a traversal step compares against a register instead of re-deriving it.
struct TriPol {
    const TriRec* __restrict__ tris;
    D3 q;
    double best, shared;
    uint32_t best_face;
    int best_leaf;
    float limf;
    __device__ double limit() const { return fmin(best, shared) * kSlack; }
    __device__ void relim() { limf = __double2float_ru(limit()); }
    // CGAL's exact fp64 construction for every leaf that passed its node's oriented-box bound.  (An fp32
    // Ericson pretest before it, tri_d2_lo, rejected some leaves early but cost more than it saved: C3
    // pass 1 137 -> 117 ms without it.)
    __device__ void test(int leaf) {
        uint32_t face;
        const double d2 = eval(leaf, q, face);
        if (offer(d2, face, leaf)) relim();
    }
    // exact squared distance from x (this lane's query or another lane's) to the leaf's triangle
    __device__ double eval(int leaf, const D3& x, uint32_t& face) const {
        D3 a, b, c;
        load_tri(tris, leaf, a, b, c, face);
        D3 o;
        int part;
        return closest_on_triangle(x, a, b, c, o, part);
    }
    // lexicographic (d2, face) update; the caller refreshes limf
    __device__ bool offer(double d2, uint32_t face, int leaf) {
        if (d2 < best || (d2 == best && face < best_face)) {
            best = d2;
            best_face = face;
            best_leaf = leaf;
            return true;
        }
        return false;
    }
};

// metric = ||q - p|| + eps (1 - n_q . n_tri)  (AABB_n_tree.h:40-84).  The penalty is bounded below by
// pmin = min(eps(1-|n_q|), eps(1+|n_q|)), so a face can only win inside the ball of radius best - pmin.
struct NrmPol {
    const TriRec* __restrict__ tris;
    D3 q, qn;
    double eps, pmin;
    double best, shared;
    uint32_t best_face;
    int best_leaf;
    float limf;
    __device__ double limit() const {
        const double b = fmin(best, shared);
        if (b == INFINITY) return INFINITY;
        double r = b - pmin;
        r += 1e-12 * (fabs(b) + fabs(pmin));
        if (r < 0.0) r = 0.0;
        return r * r * kSlack;
    }
    __device__ void relim() { limf = __double2float_ru(limit()); }
    __device__ void test(int leaf) {
        D3 a, b, c;
        uint32_t face;
        load_tri(tris, leaf, a, b, c, face);
        D3 o;
        int part;
        const double d2 = closest_on_triangle(q, a, b, c, o, part);
        double pa, pb, pc, pd;
        plane_of(a, b, c, pa, pb, pc, pd);
        const double sn = sqrt(pa * pa + pb * pb + pc * pc);
        const D3 tn = D3{pa / sn, pb / sn, pc / sn};
        const double met = sqrt(d2) + eps * (1 - vdot(qn, tn));
        if (met < best || (met == best && face < best_face)) {
            best = met;
            best_face = face;
            best_leaf = leaf;
            relim();
        }
    }
};

struct PtPol {
    const PtRec* __restrict__ pts;
    D3 q;
    double best, shared;
    uint32_t best_face;
    int best_leaf;
    float limf;
    __device__ double limit() const { return fmin(best, shared) * kSlack; }
    __device__ void relim() { limf = __double2float_ru(limit()); }
    __device__ void test(int leaf) {
        const double2* p = reinterpret_cast<const double2*>(pts + leaf);
        const double2 x0 = p[0], x1 = p[1];
        const uint32_t idx = (uint32_t)__double_as_longlong(x1.y);
        const double d2 = sqdist(q, D3{x0.x, x0.y, x1.x});
        if (d2 < best || (d2 == best && idx < best_face)) {
            best = d2;
            best_face = idx;
            best_leaf = leaf;
            relim();
        }
    }
};

// exact squared distance from q to a leaf of a triangle (TRI) or point tree, and the leaf's id: the d2 of the K-nearest
// and the radius lists (kbest.hip, within.hip)
template <bool TRI>
__device__ inline double kb_eval(const void* __restrict__ leaves, int leaf, const D3& q, uint32_t& id) {
    if constexpr (TRI) {
        D3 a, b, c, o;
        int part;
        load_tri(static_cast<const TriRec*>(leaves), leaf, a, b, c, id);
        return closest_on_triangle(q, a, b, c, o, part);
    } else {
        const double2* p = reinterpret_cast<const double2*>(static_cast<const PtRec*>(leaves) + leaf);
        const double2 x0 = p[0], x1 = p[1];
        id = (uint32_t)__double_as_longlong(x1.y);
        return sqdist(q, D3{x0.x, x0.y, x1.x});
    }
}

// Stack entries (node or ~leaf ref, fp32 bound bits): 8 B, or 4 B for trees of <= 2^20 leaves — the bound's top
// 11 bits (sign 0, exponent, 2 mantissa bits: the bound truncated, so still a lower bound; a pop it fails to prune
// only visits a node whose children are then bounded exactly) over the ref's 21 bits, one v_bfi to pack, a v_and
// and a v_bfe to unpack.
struct Ent8 {
    typedef uint2 T;
    __device__ static T make(uint32_t ref, uint32_t bb) { return make_uint2(ref, bb); }
    __device__ static int ref(T e) { return (int)e.x; }
    __device__ static float bound(T e) { return __uint_as_float(e.y); }
};
struct Ent4 {
    typedef uint32_t T;
    __device__ static T make(uint32_t ref, uint32_t bb) { return (bb & 0xFFE00000u) | (ref & 0x001FFFFFu); }
    __device__ static int ref(T e) { return __builtin_amdgcn_sbfe((int)e, 0, 21); }
    __device__ static float bound(T e) { return __uint_as_float(e & 0xFFE00000u); }
};

// Per-lane depth-first walker.  lds: this lane's column of the LDS stack (stride kBlock).
template <class E = Ent8>
struct WalkerT {
    typedef typename E::T Ent;
    int node;
    int sp;
    __device__ inline void push(uint32_t ref, uint32_t bb, Ent* __restrict__ lds, uint2* __restrict__ spill) {
        stack_put(lds, spill, sp, E::make(ref, bb));
        ++sp;
    }
    // pop until an entry survives the current limit; false when the stack is exhausted
    template <class Pol>
    __device__ inline bool pop(const Pol& pol, Ent* __restrict__ lds, uint2* __restrict__ spill) {
        while (sp > 0) {
            --sp;
            const Ent e = stack_get(lds, spill, sp);
            if (E::bound(e) <= pol.limf) {
                node = E::ref(e);
                return true;
            }
        }
        return false;
    }
    // Visit `node`: bound its two children by their fp32 oriented boxes (node_child_bounds), test leaf
    // children, descend into the nearer internal child and push the farther one.  Returns false when the
    // traversal is complete.
    template <class Pol, bool STATS>
    __device__ inline bool step(const BNode* __restrict__ nodes, const QF& qf, Pol& pol, Ent* __restrict__ lds,
                                uint2* __restrict__ spill, unsigned& n_nodes, unsigned& n_leaves) {
        const NodeV nd = load_node(nodes, node);
        if (STATS) ++n_nodes;
        float d0, d1;
        node_child_bounds(nd, qf, d0, d1);
        const int c0 = nd.child(0), c1 = nd.child(1);
        bool h0 = d0 <= pol.limf, h1 = d1 <= pol.limf;
        if (h0 && c0 < 0) {
            pol.test(~c0);
            if (STATS) ++n_leaves;
            h0 = false;
        }
        if (h1 && c1 < 0) {
            pol.test(~c1);
            if (STATS) ++n_leaves;
            h1 = false;
        }
        h0 = h0 && d0 <= pol.limf;
        h1 = h1 && d1 <= pol.limf;
        if (h0 && h1) {
            int nearc = c0, farc = c1;
            float dfar = d1;
            if (d1 < d0) { nearc = c1; farc = c0; dfar = d0; }
            push((unsigned)farc, __float_as_uint(dfar), lds, spill);
            node = nearc;
            return true;
        }
        if (h0) { node = c0; return true; }
        if (h1) { node = c1; return true; }
        return pop(pol, lds, spill);
    }
    // As step(), but leaf children that survive the bound are handed back in p0/p1 instead of being
    // tested here, so the caller can run leaf tests for many lanes of the wave at once.  `room` = leaves the
    // caller can still queue (>= 1): when a node has two leaf children and there is room for one, the farther
    // leaf is parked on the stack as an entry (~leaf, bound); a parked leaf popped later becomes `node`
    // (negative) and is handed back by the next step without a node load.  So a lane keeps traversing while
    // its queue has room for one leaf, instead of stopping as soon as a node could add two.
    // One push site and one pop site (each is a divergent loop or branch in the wave-synchronous caller, so
    // every extra copy runs serially for the lanes that take it); a parked leaf goes straight to `node`,
    // since the stack entry it would get is the one the following pop returns.
    // PF: the node was prefetched into this lane's LDS slot (nb; node_prefetch), and the next one is prefetched
    // before returning
    // The query's best leaf is never handed back: pol.best_leaf is only ever set from an exact evaluation of that leaf
    // for this query (the hint test, a round's merge, a deferral record), so a second one could only offer the
    // (d2, face) the query already holds, a duplicate in a lexicographic minimum.  With no best yet (-1) the ref
    // compared against is 0, which no leaf ref (negative) equals.  A node whose two leaf children include it queues
    // the other and parks nothing.
    template <class Pol, bool STATS, bool PF = false>
    __device__ inline bool step_collect(const BNode* __restrict__ nodes, const QF& qf, const Pol& pol,
                                        Ent* __restrict__ lds, uint2* __restrict__ spill, unsigned& n_nodes, int& p0,
                                        int& p1, int room = 2, const float4* nb = nullptr, uint32_t wsl = 0) {
        bool more = false;  // `node` holds the next entry; otherwise pop
        const int seen = ~pol.best_leaf;  // the best leaf's ref: already evaluated for this query (0 while there is none)
        if (node < 0) {
            if (node != seen) p0 = ~node;
        } else {
            const NodeV nd = PF ? node_from_lds(nb) : load_node(nodes, node);
            if (STATS) ++n_nodes;
            float d0, d1;
            node_child_bounds(nd, qf, d0, d1);
            const int c0 = nd.child(0), c1 = nd.child(1);
            const float lim = pol.limf;
            const bool h0 = d0 <= lim, h1 = d1 <= lim;
            // leaf children within the bound, but for the best leaf
            const bool l0 = h0 && c0 < 0 && c0 != seen, l1 = h1 && c1 < 0 && c1 != seen;
            const bool i0 = h0 && c0 >= 0, i1 = h1 && c1 >= 0;  // internal children within the bound
            const bool first1 = d1 < d0;                         // child 1 is the nearer
            if (l0 && l1) {
                if (room < 2) {  // two leaves, room for one: queue the nearer, park the farther
                    p0 = first1 ? ~c1 : ~c0;
                    node = first1 ? c0 : c1;
                    more = true;
                } else {
                    p0 = ~c0;
                    p1 = ~c1;
                }
            } else {
                if (l0) p0 = ~c0;
                if (l1) p0 = ~c1;
                if (i0 && i1) push((unsigned)(first1 ? c0 : c1), __float_as_uint(first1 ? d0 : d1), lds, spill);
                if (i0 || i1) {
                    node = (i0 && i1) ? (first1 ? c1 : c0) : (i0 ? c0 : c1);
                    more = true;
                }
            }
        }
        const bool r = more || pop(pol, lds, spill);
        if (PF && r && node >= 0) node_prefetch(nodes, node, wsl);
        return r;
    }
    // step_collect<PF = true> of the lean pass-1 kernel (k_knn_lean).  The caller keeps two ring places free, so
    // both leaf children are always handed back and no leaf is parked by the step itself (`node < 0` still enters:
    // cut records hold ~leaf refs).  One wave-uniform test covers the deep stack: when no lane of the step holds
    // kStack entries or more, the push writes LDS (index sp < kStack) and every pop reads it (indices < sp <= kStack),
    // so the common step carries no spill branch; spill_of() yields this lane's global spill column, only when needed.
    // `seen` is the cell's hint leaf (-1: none), which the kernel evaluates before the walk: a leaf child equal to it is
    // not handed back, since a second construction could only offer the (d2, face) already offered.  Here that covers
    // step_collect's best-leaf rule and more: every other leaf is evaluated after the walk hands it back, and the walk
    // enters a node once, so the best leaf can be reached again only while it is still the hint -- and the hint is
    // dropped also after a better leaf replaced it.  Two compares per step; a ~leaf cut entry equal to the hint is
    // dropped once, by cut_start_narrow.
    template <class Pol, class SpillOf>
    __device__ inline bool step_list(const BNode* __restrict__ nodes, const QF& qf, const Pol& pol, Ent* __restrict__ lds,
                                     SpillOf&& spill_of, int& p0, int& p1, const float4* nb, uint32_t wsl, int seen) {
        const bool deep = __ballot(sp >= kStack) != 0ull;
        bool more = false;
        if (node < 0) {
            p0 = ~node;  // a cut entry (nothing parks a leaf here), and never the hint leaf: cut_start_narrow
        } else {
            const NodeV nd = node_from_lds(nb);
            float d0, d1;
            node_child_bounds(nd, qf, d0, d1);
            const int c0 = nd.child(0), c1 = nd.child(1);
            const float lim = pol.limf;
            const bool h0 = d0 <= lim, h1 = d1 <= lim;
            const int f0 = ~c0, f1 = ~c1;
            const bool l0 = h0 && c0 < 0 && f0 != seen, l1 = h1 && c1 < 0 && f1 != seen;
            const bool i0 = h0 && c0 >= 0, i1 = h1 && c1 >= 0;
            const bool first1 = d1 < d0;
            if (l0) p0 = f0;
            if (l1) p1 = f1;
            if (i0 && i1) {
                const Ent e = E::make((unsigned)(first1 ? c0 : c1), __float_as_uint(first1 ? d0 : d1));
                if (!deep)
                    lds[sp * kBlock] = e;
                else
                    stack_put(lds, spill_of(), sp, e);
                ++sp;
            }
            if (i0 || i1) {
                node = (i0 && i1) ? (first1 ? c1 : c0) : (i0 ? c0 : c1);
                more = true;
            }
        }
        if (!more) {
            if (!deep) {
                while (sp > 0) {
                    --sp;
                    const Ent e = lds[sp * kBlock];
                    if (E::bound(e) <= pol.limf) {
                        node = E::ref(e);
                        more = true;
                        break;
                    }
                }
            } else {
                more = pop(pol, lds, spill_of());
            }
        }
        if (more && node >= 0) node_prefetch(nodes, node, wsl);
        return more;
    }
};
typedef WalkerT<Ent8> Walker;

// Heidrich's barycentric coordinates of p's projection into triangle (a, b, c), with the operation
// order of the reference's numpy code (barycentric_coordinates_of_projection.py:31-47, called with
// q = a, u = b - a, v = c - a by mesh.py:222): n = u x v, s = n.n (0 -> numpy.spacing(1)),
// b2 = ((u x w).n) / s, b1 = ((w x v).n) / s with w = p - a, weights (1 - b1 - b2, b1, b2).
__device__ inline D3 heidrich_bary(const D3& p, const D3& a, const D3& b, const D3& c) {
    const D3 u = vsub(b, a), v = vsub(c, a);
    const D3 n = vcross(u, v);
    double s = n.x * n.x + n.y * n.y + n.z * n.z;
    if (s == 0.0) s = 2.220446049250313e-16;  // numpy.spacing(1)
    const double inv = 1.0 / s;
    const D3 w = vsub(p, a);
    const double b2 = vdot(vcross(u, w), n) * inv;
    const double b1 = vdot(vcross(w, v), n) * inv;
    return D3{1.0 - b1 - b2, b1, b2};
}

// Outputs of slot i from its policy (winner's leaf -> point / part recomputed exactly).
template <int MODE, class Pol>
__device__ inline void write_result(const KnnArgs& a, size_t i, const D3& q, const Pol& pol) {
    const bool rec = a.res && (!a.direct || a.phase == 1 || a.phase == 3 || a.phase == 4);  // slot-order record
    const bool out = !a.res || a.direct;                                      // caller's arrays
    const size_t r = a.res ? (size_t)a.perm[i] : i;                           // caller's row
    if constexpr (MODE == 2) {
        const double dist = pol.best_leaf >= 0 ? sqrt(pol.best) : NAN;
        if (rec) store_qres(a.res + i, pol.best_face, 0u, dist, 0.0, 0.0);
        if (out) {
            a.out_face[r] = pol.best_face;
            a.out_dist[r] = dist;
        }
        return;
    }
    const TriRec* tris = static_cast<const TriRec*>(a.leaves);
    D3 ta, tb, tc, o = D3{NAN, NAN, NAN}, w = D3{NAN, NAN, NAN};
    uint32_t face = MSH_NO_FACE;
    int part = 0;
    if (pol.best_leaf >= 0) {  // < 0 only for a non-finite query
        load_tri(tris, pol.best_leaf, ta, tb, tc, face);
        closest_on_triangle(q, ta, tb, tc, o, part);
        if (MODE == 3) w = heidrich_bary(o, ta, tb, tc);
    }
    if (rec) {
        store_qres(a.res + i, face, a.rec_leaf ? (uint32_t)pol.best_leaf : (uint32_t)part, o.x, o.y, o.z);
        if (MODE == 3 && !a.direct) {
            a.res_w[3 * i] = w.x;
            a.res_w[3 * i + 1] = w.y;
            a.res_w[3 * i + 2] = w.z;
        }
    }
    if (!out) return;
    a.out_face[r] = face;
    if (MODE == 0 && a.out_part) a.out_part[r] = (uint32_t)part;
    a.out_pt[3 * r] = o.x;
    a.out_pt[3 * r + 1] = o.y;
    a.out_pt[3 * r + 2] = o.z;
    if (MODE == 3) {
        a.out_w[3 * r] = w.x;
        a.out_w[3 * r + 1] = w.y;
        a.out_w[3 * r + 2] = w.z;
    }
}

// write_result of the lean pass-1 kernel (k_knn_lean): the sorted path's direct stores to the caller's row r, and
// nothing else (no slot-order record, no unsorted form).
template <int MODE, class Pol>
__device__ inline void write_direct(const TriRec* __restrict__ tris, size_t r, const D3& q, const Pol& pol,
                                    uint32_t* out_face, uint32_t* out_part, double* out_pt, double* out_w) {
    D3 ta, tb, tc, o = D3{NAN, NAN, NAN}, w = D3{NAN, NAN, NAN};
    uint32_t face = MSH_NO_FACE;
    int part = 0;
    if (pol.best_leaf >= 0) {  // < 0 only for a non-finite query
        load_tri(tris, pol.best_leaf, ta, tb, tc, face);
        closest_on_triangle(q, ta, tb, tc, o, part);
        if (MODE == 3) w = heidrich_bary(o, ta, tb, tc);
    }
    out_face[r] = face;
    if (MODE == 0 && out_part) out_part[r] = (uint32_t)part;
    out_pt[3 * r] = o.x;
    out_pt[3 * r + 1] = o.y;
    out_pt[3 * r + 2] = o.z;
    if (MODE == 3) {
        out_w[3 * r] = w.x;
        out_w[3 * r + 1] = w.y;
        out_w[3 * r + 2] = w.z;
    }
}

// A kernel argument read from the kernarg segment at the point of use (the lean pass-1 kernel's cold fields: the
// deferral, resume and spill-area arguments and the output pointers, used once per tile after its wave loop).  The
// empty asm hides the segment's address from the optimiser, which otherwise loads every field of the by-value
// KnnArgs at kernel entry and keeps it in SGPRs (or in lanes of a spill VGPR) across the loop.  KnnArgs is the
// kernel's only argument, so a field's kernarg offset is its offsetof.
static_assert(std::is_standard_layout<KnnArgs>::value && std::is_trivially_copyable<KnnArgs>::value &&
                  alignof(KnnArgs) <= 8,
              "cold_arg reads KnnArgs fields at their offsetof from the start of the kernarg segment");
template <class T>
__device__ inline T cold_arg(size_t off) {
    typedef __attribute__((address_space(4))) const char* KP;
    KP p = (KP)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(__attribute__((address_space(4))) const T*)(p + off);
}
#define MSH_COLD_ARG(f) cold_arg<decltype(KnnArgs::f)>(offsetof(KnnArgs, f))

template <int MODE>
struct PolOf { using T = TriPol; };
template <>
struct PolOf<1> { using T = NrmPol; };
template <>
struct PolOf<2> { using T = PtPol; };

template <int MODE>
__device__ inline typename PolOf<MODE>::T make_pol(const KnnArgs& a, size_t i, const D3& q) {
    typename PolOf<MODE>::T pol;
    if constexpr (MODE == 2) {
        pol.pts = static_cast<const PtRec*>(a.leaves);
    } else {
        pol.tris = static_cast<const TriRec*>(a.leaves);
    }
    pol.q = q;
    if constexpr (MODE == 1) {
        pol.qn = D3{a.n[3 * i], a.n[3 * i + 1], a.n[3 * i + 2]};
        const double nq = sqrt(vdot(pol.qn, pol.qn));
        pol.eps = a.eps;
        pol.pmin = fmin(a.eps * (1 - nq), a.eps * (1 + nq));
    }
    pol.best = INFINITY;
    pol.shared = INFINITY;
    pol.best_face = MSH_NO_FACE;
    pol.best_leaf = -1;
    pol.limf = INFINITY;
    return pol;
}


__device__ inline D3 load_q(const KnnArgs& a, size_t i) {
    const size_t r = a.qperm ? (size_t)a.qperm[i] : i;
    return D3{a.q[3 * r], a.q[3 * r + 1], a.q[3 * r + 2]};
}

// ---- pass-1 constants (each measured on C3 100M; A/B records in profiles/r02_*_ab.jsonl, r03_*_ab.jsonl) ----
// Leader ordering: one leader slot per kLead slots (4: -4 %, 16: -1 %, none: -22 %; with the entry cut and the node
// prefetch, 16: -1.5 %, 16 with 128-slot follower windows: -1.5 to -2 %, profiles/r04_c3_prefetch_asm_lead_ab.jsonl), one super-leader per kLead2
// slots; super-leaders run first and unhinted, leaders take their hint from the kLWin super-leaders of their
// window (4: -1.1 %), followers from the leaders of their kFWin-slot window (32: +-0, 128: -3 %).
#ifndef MSH_KLEAD
#define MSH_KLEAD 8  // at least 2, and a divisor of kLead2 (launch_knn always runs leader phases where they apply)
#endif
#ifndef MSH_KFWIN
#define MSH_KFWIN 64
#endif
constexpr unsigned kLead = MSH_KLEAD;
constexpr unsigned kLead2 = 256;
constexpr size_t kFWin = MSH_KFWIN;
constexpr size_t kLWin = 8;
static_assert(kLead2 % kLead == 0 && kLead2 / kLead >= 2, "kLead2: a multiple of kLead");
// Per-lane leaf queues (the path of trees with >= 2^26 leaves, and of the normals-metric and point modes): up
// to kLeafQ leaves per lane, a lane traverses while its queue has room for one more (a second leaf child is
// parked on its stack); leaf phases run as soon as one lane is blocked; the uncompacted phases (MODE 1, 2) test
// at most kLeafRound leaves per lane each.
constexpr int kLeafQ = 4;
constexpr int kLeafRound = 2;

// slot of work unit k in the launch's phase: 3 super-leaders, 1 leaders (without the super-leaders), 4 every leader
// (trees with cell hints: no super-leader launch), 2 followers, 0 every slot
__device__ inline size_t slot_of(const KnnArgs& a, size_t k) {
    if (a.phase == 3) return k * kLead2;
    if (a.phase == 4) return k * kLead;
    if (a.phase == 1) {
        constexpr size_t r = kLead2 / kLead;
        return kLead * (k + k / (r - 1) + 1);
    }
    if (a.phase == 2) {
        const size_t g = k / (kLead - 1);
        return g * kLead + (k - g * (kLead - 1)) + 1;
    }
    return k;
}

// The leaf holding the closest point p_L of the leader (at slots base, base + stride, ... < base + window of
// the window containing i) nearest to q, or -1.  A hinted slot starts by testing that leaf exactly, as if the
// traversal had reached it first: a real candidate (d^2, face, leaf), so no hint can be too tight, and its
// exact distance is at most |q - p_L| (host model: 14 % fewer leaf tests than a |q - p_L| bound; C3: the
// hint leaf is the answer for 17 % of the followers).  Leaders of another mesh (batched trees) and deferred
// leaders (NO_FACE until pass 2 answers them) are skipped.
__device__ inline int leader_leaf(const KnnArgs& a, size_t i, const D3& q, size_t window, size_t stride) {
    const size_t base = (i / window) * window;
    const size_t mesh = a.orgs ? i / a.qper : 0;
    double h = INFINITY;
    int leaf = -1;
    for (size_t L = 0; L < window; L += stride) {
        const size_t li = base + L;
        if (li >= a.S) break;
        if (a.orgs && li / a.qper != mesh) continue;
        const uint4 r0 = reinterpret_cast<const uint4*>(a.res + li)[0];
        if (r0.x == MSH_NO_FACE) continue;
        const double2 r1 = reinterpret_cast<const double2*>(a.res + li)[1];
        const double x = __longlong_as_double((long long)(((unsigned long long)r0.w << 32) | r0.z));
        const double dx = q.x - x, dy = q.y - r1.x, dz = q.z - r1.y;
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 < h) {
            h = d2;
            leaf = (int)r0.y;
        }
    }
    return leaf;
}

// number of set bits of m below this lane (v_mbcnt: no per-lane mask register)
__device__ inline unsigned lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Wave leaf list (closest-point modes): lanes append the leaf children that survive their node's bound to a
// ring of (leaf << 6 | owner lane) entries in LDS shared by the wave, and the wave evaluates them in rounds of
// 64 — one entry per lane, every round full except when nobody can move — instead of per-lane queues flushed
// part-empty.  A lane stops traversing while kPend of its leaves wait.  Each round's results reach their
// owners through LDS: an atomic min of the squared distance's bits per owner, then an atomic min of
// (face << 32 | leaf) among the entries that reached it: the lexicographic (d2, face) rule.
// kPend (C3, M q/s): 3: 1236, 4: 1346, 8: 1593, 16: 1677, 32: 1706, unbounded: 1689; per-lane queues 1541.
#ifndef MSH_KPEND
#define MSH_KPEND 32
#endif
constexpr int kPend = MSH_KPEND;
// Tile prefetch: a wave claims its next tile while the current one's rows load, instead of paying dequeue_tile's two
// dependent round trips at every tile start with the wave idle (C3 100M pass 1 38.4-39.5 -> 36.3-36.4 ms,
// profiles/r06_c3_tile_prefetch_ab.jsonl).
// MSH_LIST_RESERVE 1 (a counting build, not shipped): the generic list kernel keeps the two ring places free too, so
// its step never parks a leaf and it visits what the lean kernel visits; instrumented launches (msh_tree_nearest_stats)
// run the generic kernel, and this is how the reserve's effect on the node and leaf counts is measured.
#ifndef MSH_LIST_RESERVE
#define MSH_LIST_RESERVE 0
#endif

constexpr unsigned kRing = 256;     // ring entries per wave: < 64 left after full rounds + <= 128 per step
constexpr size_t kListMaxLeaves = (size_t)1 << 26;  // leaf index bits of a ring entry
constexpr size_t kLeadMinLeaves = 4096;  // smaller trees skip the leader phases (C1: 0.56 -> 0.29 ms)

// Pass 1 runs 4 waves per SIMD (not the normals metric, MODE 1, whose larger live set would spill in the node
// step): the register budget drops from 139 to 128 VGPRs at the cost of a few spills of loop-invariant values
// outside the node step (C3: +10 % over the compiler's 3 waves; 5 waves spill in the loop: -30 %; 5 waves also
// need <= 32 KB of LDS per block).
#ifndef MSH_KNN_WAVES
#define MSH_KNN_WAVES 4
#endif
#define MSH_KNN_ATTR __attribute__((amdgpu_waves_per_eu(MODE == 1 ? 1 : MSH_KNN_WAVES)))
// Entry cut.  The grid cell of q (centre c, half-diagonal r) holds up to kCutK tree entries (node or ~leaf)
// whose bound from c is within (d(c) + 2r)^2, d(c) = c's exact distance to the mesh, and which together cover
// every such subtree; any other subtree lies farther than d(c) + 2r from c, so farther than d(c) + r >= d(q)
// from q, and can hold neither q's closest face nor a tie.  Each entry carries max(s, 0)^2 rounded down,
// s = sqrt(bound from c) - r: a lower bound of the squared distance from q to its subtree.  The entries go
// on the stack with it, nearest to c popped first, and the walk starts from the first entry within the
// current limit.  false: no entry survives the hint's bound (the hint is the answer).
constexpr size_t kNoCell = ~(size_t)0;
// grid cell of q, or kNoCell outside the grid (or without a cut)
__device__ inline size_t cut_cell(const KnnArgs& a, const D3& q) {
    if (!a.cut) return kNoCell;
    const double G = (double)a.cut_G;
    const double ux = (q.x - a.cut_lo[0]) * a.cut_iw[0], uy = (q.y - a.cut_lo[1]) * a.cut_iw[1],
                 uz = (q.z - a.cut_lo[2]) * a.cut_iw[2];
    if (!(ux >= 0.0 && ux < G && uy >= 0.0 && uy < G && uz >= 0.0 && uz < G)) return kNoCell;
    return ((size_t)(unsigned)uz * (size_t)a.cut_G + (unsigned)uy) * (size_t)a.cut_G + (unsigned)ux;
}
// the cell's record: word 0 its hint leaf (-1: none), then kCutK entries nearest-first -- 4-B entries in the stack's
// own packing (Ent4: the bound's top 11 bits over a 21-bit ref; empty entries have the sign bit set) in a 32-B
// record, or (ref, bound bits) pairs from word 2 of a 64-B record (empty: ref kCutEmpty)
// (kCutDirFlag in word 0: a directional drop shortened the list, internal.h -- the closest-point walks only mask it)
__device__ inline int cut_hint_leaf(uint32_t w0) { return (int)w0 < 0 ? -1 : (int)(w0 & ~kCutDirFlag); }
__device__ inline const uint32_t* cut_rec(const KnnArgs& a, size_t cell) {
    return a.cut + cell * (a.cut_wide ? 16 : 8);
}
template <class Pol, class W>
__device__ inline bool cut_start(const KnnArgs& a, size_t cell, const Pol& pol, W& w, typename W::Ent* __restrict__ lds,
                                 uint2* __restrict__ spill) {
    const uint32_t* r = cut_rec(a, cell);
    if (a.cut_wide) {
        const uint4* c = reinterpret_cast<const uint4*>(r);
        uint4 e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = c[j];
        auto put = [&](uint32_t ref, uint32_t sb) {
            if (ref != kCutEmpty) w.push(ref, sb, lds, spill);
        };
#pragma unroll
        for (int j = 3; j >= 1; --j) {
            put(e[j].z, e[j].w);
            put(e[j].x, e[j].y);
        }
        put(e[0].z, e[0].w);  // entry 0 (words 2, 3)
    } else {
        const uint4* c = reinterpret_cast<const uint4*>(r);
        const uint4 e0 = c[0], e1 = c[1];
        const uint32_t e[kCutK] = {e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
        for (int j = kCutK - 1; j >= 0; --j)
            if ((int)e[j] >= 0) w.push((uint32_t)Ent4::ref(e[j]), e[j] & 0xFFE00000u, lds, spill);
    }
    return w.pop(pol, lds, spill);
}
// cut_start of the lean pass-1 kernel: 32-B records only, and the walk starts with an empty stack, so the kCutK
// entries and the pop that follows stay in LDS
static_assert(kCutK <= kStack, "a cut record's entries fit the LDS stack");
template <class Pol, class W>
__device__ inline bool cut_start_narrow(const uint32_t* __restrict__ cut, size_t cell, const Pol& pol, W& w,
                                        uint32_t* __restrict__ lds) {
    const uint4* c = reinterpret_cast<const uint4*>(cut + cell * 8);
    const uint4 e0 = c[0], e1 = c[1];
    const uint32_t e[kCutK] = {e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
    // the cell's hint leaf, evaluated before the walk (pol.best_leaf), is not entered again as a ~leaf entry: whatever
    // the best is when its turn comes, its construction could not change it.  Without a hint nothing matches: entries
    // are node refs too (0 is the root), and INT_MIN is no 21-bit ref
    const int seen = pol.best_leaf >= 0 ? ~pol.best_leaf : INT_MIN;
#pragma unroll
    for (int j = kCutK - 1; j >= 0; --j)
        if ((int)e[j] >= 0 && Ent4::ref(e[j]) != seen) {
            lds[w.sp * kBlock] = Ent4::make((uint32_t)Ent4::ref(e[j]), e[j] & 0xFFE00000u);
            ++w.sp;
        }
    while (w.sp > 0) {
        --w.sp;
        const uint32_t t = lds[w.sp * kBlock];
        if (Ent4::bound(t) <= pol.limf) {
            w.node = Ent4::ref(t);
            return true;
        }
    }
    return false;
}

// lexicographic min of (best, face) over the wave; every lane ends with the winner
__device__ inline void wave_lexmin(double& best, uint32_t& face, int& leaf) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double b2 = __shfl_xor(best, o, 64);
        const uint32_t f2 = (uint32_t)__shfl_xor((int)face, o, 64);
        const int l2 = __shfl_xor(leaf, o, 64);
        if (b2 < best || (b2 == best && f2 < face)) {
            best = b2;
            face = f2;
            leaf = l2;
        }
    }
}

__device__ inline double wave_min(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = fmin(x, __shfl_xor(x, o, 64));
    return x;
}

}  // namespace msh
