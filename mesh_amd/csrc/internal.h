// Host-side internals of libmeshsearch: the handle, device buffers, error plumbing and the kernel
// launchers implemented in the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/meshsearch.h"
#include "common.h"

namespace msh {

void set_error(const char* fmt, ...);

#define MSH_HIP(expr)                                                                           \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            ::msh::set_error("HIP error %s at %s:%d: %s", hipGetErrorName(_e), __FILE__, __LINE__, #expr); \
            return (_e == hipErrorOutOfMemory) ? MSH_ENOMEM : MSH_EDEVICE;                       \
        }                                                                                       \
    } while (0)

#define MSH_TRY(expr)               \
    do {                            \
        int _s = (expr);            \
        if (_s != MSH_OK) return _s; \
    } while (0)

// Device allocations through the library's cache (devmem.cpp DevCache): dfree keeps the block for the next request of a
// similar size on its device (after waiting for the device, as hipFree does).
hipError_t dmalloc_raw(void** p, size_t bytes);
hipError_t dfree(void* p);
template <class T>
inline hipError_t dmalloc(T** p, size_t bytes) {
    void* v = nullptr;
    const hipError_t e = dmalloc_raw(&v, bytes);
    *p = static_cast<T*>(v);
    return e;
}
size_t dcache_trim();
size_t dcache_bytes();

// Grow-only device scratch buffer.  Owning and move-only: a scope's buffers are freed when it ends (hipFree
// waits for the device, so a buffer still read by queued launches is not released under them).
struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            ptr = o.ptr;
            bytes = o.bytes;
            o.ptr = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t need);
    void release();
    template <class T>
    T* as() const { return static_cast<T*>(ptr); }
};

// Reusable per-handle scratch (query keys / permutation / sort temporaries / slot-order queries and
// results / staging).
struct Workspace {
    DevBuf keys, vals, keys_alt, vals_alt, hist, scan, q, n, out_a, out_b, out_c, out_d, flags, counters, spill, stats,
        ranges, qs, ns, inv, res, res_w, resume, p2cand, sgn;
    void release();
    size_t bytes() const;
};

enum Kind { kTriangles = 0, kNormals = 1, kPoints = 2 };

// 32-B slot-order result record written (coalesced) by the traversal kernels: face / index, part code,
// point (or distance in x for point trees).
struct alignas(16) QRes {
    uint32_t face, part;
    double x, y, z;
};
static_assert(sizeof(QRes) == 32, "QRes must be 32 B");
// one record as two 16-B stores
__device__ inline void store_qres(QRes* r, uint32_t face, uint32_t part, double x, double y, double z) {
    const unsigned long long xb = (unsigned long long)__double_as_longlong(x);
    reinterpret_cast<uint4*>(r)[0] = make_uint4(face, part, (uint32_t)xb, (uint32_t)(xb >> 32));
    reinterpret_cast<double2*>(r)[1] = make_double2(y, z);
}

// Caller-order output arrays of a point query (nullptr = not wanted).  w: per-row extra doubles
// (barycentric weights, or the ray distance).
struct SlotOut {
    uint32_t* face;
    uint32_t* part;
    double* pt;
    double* dist;
    double* w;
};

// Order in which a launch visits its queries: q (and n) are the rows in slot order; perm maps a slot
// to the caller's row and inv back (both nullptr: identity, the caller's arrays are used directly).
// gathered == false: q (and n) are still the caller's rows; the traversal reads row perm[i] for slot i
// and records inv itself (closest-point launches)
struct QueryOrder {
    const double* q;
    const double* n;
    const uint32_t* perm;
    const uint32_t* inv;
    bool gathered = true;
};

// Staging slabs of one pipelined host call (hostpipe.cpp): two pinned host slabs of hbytes, a ring of three device
// slabs of dbytes.  A plain value: the handle holds the set it leased, the pool (StagePool) the idle ones.
struct StageSet {
    void* h[2] = {nullptr, nullptr};
    void* d[3] = {nullptr, nullptr, nullptr};
    size_t hbytes = 0, dbytes = 0;  // host slabs hold the inputs only when results go straight into pinned arrays
    void free_host();    // hostpipe.cpp
    void free_device();  // (the caller is on the slabs' device)
};

}  // namespace msh

struct msh_tree {
    int device = 0;
    int kind = msh::kTriangles;
    double eps = 0.0;
    size_t P = 0;        // main-mesh vertices
    size_t T = 0;        // leaf primitives
    size_t T_main = 0;   // main-mesh faces (visibility: extra faces follow)
    size_t B = 1;        // meshes in a batched tree (msh_batch_build; P, T are per mesh); 1 otherwise
    double* d_v = nullptr;         // (P,3) main vertices (visibility sources)
    msh::BNode* d_nodes = nullptr; // T-1 internal nodes (nullptr when T == 1)
    void* d_leaves = nullptr;      // T TriRec or PtRec in Morton order
    float scene_lo[3] = {0, 0, 0}, scene_hi[3] = {0, 0, 0};  // bbox of all primitives
    double origin[3] = {0, 0, 0};  // fp64 scene-box centre: all fp32 node bounds are relative to it
    double half_diag = 0.0;        // largest half-diagonal of the (per-mesh) boxes around their origins
    double* d_orgs = nullptr;      // (B,3) per-mesh origins on the device (B = 1: a copy of origin)
    double* d_boxes = nullptr;     // (B,6) per-mesh boxes (batched trees: query Morton codes)
    uint32_t* d_vorder = nullptr;  // Morton order of the main vertices (lazily built for visibility)
    uint32_t* d_vorder_shard = nullptr;  // Morton order of vertices [vshard_v0, +vshard_nv) (last shard asked for)
    size_t vshard_v0 = 0, vshard_nv = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ws_done = nullptr;  // recorded after the last launch that used `ws` (stream ordering)
    // host-call staging (hostpipe.cpp pipelined()): the slab set leased from the pool for one call, and the copy
    // streams and their events (lazily created)
    msh::StageSet stage;
    hipStream_t s_up = nullptr, s_down = nullptr;
    hipEvent_t e_up[3] = {nullptr, nullptr, nullptr}, e_run[3] = {nullptr, nullptr, nullptr},
               e_down[3] = {nullptr, nullptr, nullptr};
    double build_ms = 0.0;
    int max_depth = 0;             // bound of the deepest leaf (root children = 1): k_karras prefix lengths
    // entry cut (single triangle trees; entrycut.cpp build_entry_cut): a G^3 grid over the scene box widened by 1/4, one
    // record per cell -- its hint leaf and kCutK start entries, 32 B (4-B entries, trees of <= 2^20 leaves) or 64 B
    // (cut_wide) --; d_cut == nullptr: every query starts at the root
    uint32_t* d_cut = nullptr;
    int cut_wide = 0;
    uint32_t* d_face_leaf = nullptr;  // face -> leaf (msh_tree_points_from_faces_device; built on first use)
    // sign table (msh_tree_sign_build; sign.hip): one device block holding fn (T,3) f64, vpn (P,3) f64, opp (T,3) u32
    // and f (T,3) u32 in that order; nullptr until built (blobs leave it out)
    void* d_sign = nullptr;
    msh_sign_info sign = {0, 0, 0, 0, 0, 0, 0.0};
    // winding table (msh_tree_winding_build; winding.hip): T - 1 dipole records of kWindRecBytes; nullptr until built
    // (lazily, by the first winding-number query; trees of one leaf never hold one; blobs leave it out)
    void* d_wind = nullptr;
    msh_winding_info wind = {0, 0, 0, 0, 0.0};
    int cut_G = 0;
    // lazily built on the first closest-point query (msh_tree_set_entry_cut): requested grid (< 0 automatic,
    // 0 off), state (0 pending, 1 built, 2 off / not applicable, 3 failed), GPU build time
    int cut_req = -1;
    int cut_state = 0;
    bool cut_force = false;   // msh_tree_set_entry_cut was called: build at the next query, whatever its size
    uint64_t cut_rows = 0;    // closest-point rows answered while the automatic cut waits (ensure_entry_cut)
    int cut_fails = 0;        // failed automatic builds (retried after another threshold of rows, at most twice)
    bool cut_fine = false;    // the built grid is the fine automatic one (or a requested one): no upgrade
    double cut_ms = 0.0;
    uint64_t cut_flagged = 0;  // cells of the built grid whose record a directional drop shortened (k_cut_level)
    double cut_lo[3] = {0, 0, 0}, cut_iw[3] = {0, 0, 0};
    msh::Workspace ws;
    // copies of this tree on the other devices of msh_set_devices / msh_set_device_list (owned; freed with it):
    // host-buffer calls split their rows over this handle and its replicas
    std::vector<msh_tree*> replicas;
    // batched builds return before their last kernels finish (api.cpp msh_batch_build): the build's temporaries
    // (device pointers and its workspace) are freed, and build_ms read, once pend_done has passed (finish_pending)
    bool pending = false;
    std::vector<void*> pend_free;
    msh::Workspace pend_ws;
    hipEvent_t pend_e0 = nullptr, pend_done = nullptr;
};

namespace msh {

// ---- radix sort (sort.hip): stable LSD sort of (u32 key, u32 value) pairs on the low `bits` bits.
// Result ends in keys/vals (the alt buffers are temporaries) — or, with in_alt and an odd number of
// passes, in keys_alt/vals_alt (*in_alt = true) without the copy back.  lo_bit: first key bit sorted.
int radix_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* keys_alt, uint32_t* vals_alt, size_t n, int bits,
                     Workspace& ws, hipStream_t s, int lo_bit = 0, bool* in_alt = nullptr);
// exclusive scan of u32 (in place), n elements
int exclusive_scan_u32(uint32_t* data, size_t n, Workspace& ws, hipStream_t s);

// ---- LBVH build (build.hip) ----
// prim_lo/prim_hi: (T,3) fp64 bounds per primitive on device.  Builds nodes and the Morton order
// `order` (sorted position -> primitive id).  scene box written to tree.
int build_lbvh(msh_tree* tree, const double* d_prim_lo, const double* d_prim_hi, size_t T, uint32_t* d_order);
// Batched LBVH over tree->B meshes of T primitives each (bounds (B*T,3), mesh b's primitives at
// [bT, (b+1)T)): per-mesh boxes/origins, Morton codes, two-phase stable radix sort (Morton, then mesh),
// per-mesh Karras emission with global child references, refit.
int build_lbvh_batch(msh_tree* tree, const double* d_prim_lo, const double* d_prim_hi, size_t T, uint32_t* d_order);
int tri_bounds_batch(const double* d_v, size_t P, const uint32_t* d_f, size_t B, size_t T, double* d_lo, double* d_hi,
                     hipStream_t s);
int pack_tri_leaves_batch(const double* d_v, size_t P, const uint32_t* d_f, const uint32_t* d_order, size_t B, size_t T,
                          TriRec* d_out, hipStream_t s);
// Morton codes of (B*S,3) queries in their mesh's box (query i belongs to mesh mesh0 + i / S) + iota values.
int query_morton_batch(const msh_tree* tree, const double* d_q, size_t n, size_t S, uint32_t* keys, uint32_t* vals,
                       hipStream_t s, size_t mesh0 = 0);
// keys[j] = vals[j] / per (the mesh of element vals[j]), for the second, per-mesh sort phase
int mesh_keys(const uint32_t* vals, size_t n, size_t per, uint32_t* keys, hipStream_t s);
// largest distance from origin to a corner of box (lo xyz, hi xyz): msh_tree::half_diag
double half_diagonal(const double* box, const double* origin);
// device copy of tree->origin (single-mesh trees; blob unpack)
int upload_origin(msh_tree* tree, hipStream_t s);
// Top-down re-split of every LBVH subtree over at most 2^log2K leaves (refine.hip): the same node ids,
// ranges and leaf-order conventions as build_lbvh, which it must follow (triangle trees; before leaf packing).
int resplit_tree(msh_tree* tree, const double* d_v, const uint32_t* d_f, size_t T, uint32_t* d_order, int log2K);
// Oriented-box pass over the packed leaves (needs the node ranges recorded by build_lbvh).  defer: leave its
// temporaries to tree->pend_free instead of synchronising and freeing them (asynchronous batched builds).
int build_obb(msh_tree* tree, bool triangles, bool defer = false);
int tri_bounds(const double* d_v, const uint32_t* d_f, size_t T, double* d_lo, double* d_hi, hipStream_t s);
int pack_tri_leaves(const double* d_v, const uint32_t* d_f, const uint32_t* d_order, size_t T, uint32_t face_base,
                    TriRec* d_out, hipStream_t s);
int pack_point_leaves(const double* d_v, const uint32_t* d_order, size_t P, PtRec* d_out, hipStream_t s);
int point_bounds(const double* d_v, size_t P, double* d_lo, double* d_hi, hipStream_t s);

// ---- query ordering (sort.hip) ----
// 30-bit Morton codes of query points in the tree's scene box + iota values.
int query_morton(const msh_tree* tree, const double* d_q, size_t S, uint32_t* keys, uint32_t* vals, hipStream_t s);
// the box query Morton codes are taken in: the scene box widened by 10 % of its extent per side
void query_box(const msh_tree* tree, float* lo, float* hi);
// Query order: the S rows stably sorted by the top 30 - lo_bit bits (<= 24) of their Morton codes in the
// box lo..hi; the permutation (slot -> row) ends in ws.vals.  Uses ws.keys, ws.keys_alt, ws.vals_alt, ws.hist.
int query_sort(const float* lo, const float* hi, const double* d_q, size_t S, int lo_bit, Workspace& ws, hipStream_t s);
// slot i <- rows perm[i] of a (and b when non-null); inv[perm[i]] = i
int gather_rows(const double* d_a, const double* d_b, const uint32_t* d_perm, size_t S, double* d_as, double* d_bs,
                uint32_t* d_inv, hipStream_t s);
// caller row j <- slot inv[j] (record fields + nw doubles per row from d_w)
int unpermute_results(const QRes* d_res, const double* d_w, int nw, const uint32_t* d_inv, size_t S, const SlotOut& o,
                      hipStream_t s);
// ---- entry cut, build time (cutbuild.hip) ----
// Entry cut of a single triangle tree (k_cut_level): the records of a G^3 grid from the cell centres' exact
// answers (closest points d_pts, their leaves d_hint); e4: 32-B records of 4-B entries (trees of <= 2^20 leaves), else 64-B records.
// kCutK start entries per cell (the hint takes the record's eighth word; round 5: 8 entries of 8 B + a separate hint;
// 4 entries: 1773-1800 M q/s against 8, 16: 1285, C3, profiles/r03_c3_entry_cut_ab.jsonl)
constexpr int kCutK = 7;
constexpr uint32_t kCutEmpty = 0x7FFFFFFFu;  // empty 64-B record entry: not a node id (ids < T - 1 <= 2^31 - 2) nor a ~leaf
constexpr size_t kEnt4MaxLeaves = (size_t)1 << 20;  // 4-B stack / cut entries: refs in [-2^20, 2^20), 21 bits
// k_cut_level's directional drop (cutbuild.hip cut_dir_drop) and the mark of a record it shortened: bit 30 of word 0
// (the hint leaf; leaves < 2^26) in 32-B records -- 64-B records zero their radius word instead.  The alongnormal
// walks start at the root in a marked cell (rays.hip); the closest-point walks mask the bit.
constexpr uint32_t kCutDirFlag = 0x40000000u;
int cut_centres(int G, const double* lo, const double* w, double* d_q, hipStream_t s);
// d_half: the records of the G/2 grid over the same box (same record size), each cell then starts from its enclosing
// half-resolution cell's entries instead of the root; nullptr: from the root.  subdiv >= 0: also apply the
// directional drop, proved on sub-cells down to that depth (0: whole cells only; at most kCutSubdiv; the test hook
// MESH_AMD_CUT_SUBDIV = 0 / 1 / 2 overrides it); < 0: the ball rule alone.  d_nflag (nullable): incremented by the
// number of records the drop shortened
constexpr int kCutSubdiv = 2;         // the deepest split of a cell into octants
constexpr int kCutSubdivDefault = 2;  // the depth of a grid the caller asked for (entrycut.cpp ensure_entry_cut)
int cut_level(const msh_tree* tree, int G, const double* lo, const double* w, const double* d_pts, const int* d_hint,
              uint32_t* d_rec, bool e4, hipStream_t s, const uint32_t* d_half = nullptr,
              unsigned long long* d_nflag = nullptr, int subdiv = 0);
// d_inv[face] = the leaf holding it (T words)
int face_leaf_map(const msh_tree* tree, uint32_t* d_inv, hipStream_t s);
// closest point (and part) of each row q[i] on face d_face[i] (the traversal's answer construction); d_inv from
// face_leaf_map
int points_from_faces(const msh_tree* tree, const uint32_t* d_inv, const double* d_q, size_t S, const uint32_t* d_face,
                      uint32_t* d_part, double* d_pt, hipStream_t s);
// d_hint[cell] = the leaf holding face d_face[cell] (d_inv: T scratch words)
int cut_hints(const msh_tree* tree, const uint32_t* d_face, size_t n, uint32_t* d_inv, int* d_hint, hipStream_t s);
// ---- closest-point queries (nearest.hip) ----
// closest point: o.face, o.part (nullable), o.pt; with o.w (3 per row) the barycentric variant (part unused)
int launch_nearest(const msh_tree* tree, const QueryOrder& ord, size_t S, const SlotOut& o, hipStream_t s);
// batched trees: n = (meshes) * S queries, slot i answered on mesh mesh0 + i / S (the batched sort is mesh-major)
int launch_nearest_batch(const msh_tree* tree, const QueryOrder& ord, size_t n, size_t S, const SlotOut& o,
                         hipStream_t s, size_t mesh0 = 0);
int launch_nearest_stats(const msh_tree* tree, const QueryOrder& ord, size_t S, unsigned long long* d_counts,
                         hipStream_t s);
// normals metric: o.face, o.pt; ord.n = query normals in slot order
int launch_nnearest(const msh_tree* tree, const QueryOrder& ord, size_t S, const SlotOut& o, hipStream_t s);
// vertex NN: o.face (index), o.dist
int launch_points_nearest(const msh_tree* tree, const QueryOrder& ord, size_t S, const SlotOut& o, hipStream_t s);

// ---- rays (rays.hip) ----
// alongnormal: ord.q / ord.n = sources / normals in slot order; o.w = distance (1 per row), o.face, o.pt
int launch_alongnormal(const msh_tree* tree, const QueryOrder& ord, size_t S, const SlotOut& o, hipStream_t s);
// visibility of vertices [v0, v0 + nv) from C cameras: vis / ndc are (C, nv)
int launch_visibility(const msh_tree* tree, const double* d_cams, size_t C, const double* d_normals,
                      const double* d_sensors, double min_dist, size_t v0, size_t nv, uint32_t* d_vis, double* d_ndc,
                      hipStream_t s);

// instrumented (untimed, outputs not written): d_counts[0] += internal nodes loaded, [1] += leaf tests
int launch_alongnormal_stats(const msh_tree* tree, const QueryOrder& ord, size_t S, unsigned long long* d_counts,
                             hipStream_t s);
int launch_visibility_stats(const msh_tree* tree, const double* d_cams, size_t C, double min_dist,
                            unsigned long long* d_counts, hipStream_t s);

// ---- ray casting (raycast.hip) ----
// Caller-order outputs of S rays.  First hit (any == false): t (S,), face (S,), and pt (S,3), w (S,3), which may be
// nullptr; occlusion (any == true): hit (S,) alone.
struct RayOut {
    bool any;
    double* t;
    uint32_t* face;
    double* pt;
    double* w;
    uint8_t* hit;
};
// ord.q / ord.n: the caller's origins and directions with the slot order of the origins (ord.perm, or identity);
// d_range: (S,2) caller rows, or nullptr for [0, +inf].  Plain triangle trees; the walks start at the root.  d_stats ==
// nullptr: the timed query ("raycast" / "occluded").  Otherwise the same walks, untimed, no output written: d_stats[0]
// += internal nodes loaded, [1] += leaf tests.  Uses ws.counters and ws.spill.  Asynchronous on s.
int launch_raycast(msh_tree* tree, const QueryOrder& ord, const double* d_range, size_t S, const RayOut& o,
                   unsigned long long* d_stats, hipStream_t s);

// ---- ray casting, all hits (raycast_all.hip) ----
// d_counts[r] = the size of row r's hit set (launch_raycast's rows, ranges and hit set).  Uses ws.counters and ws.spill.
// Asynchronous on s; msh_timing_get name "raycast_count".
int launch_raycast_count(msh_tree* tree, const QueryOrder& ord, const double* d_range, size_t S, uint32_t* d_counts,
                         hipStream_t s);
// The hit lists as CSR, sorted by (row, t by value, face id), in the two steps of the pair lists:
//   count  launch_raycast_count into ws.flags (the counts stay valid until emit) and their totals, read back on s
//          (synchronous);
//   emit   scan, fill, order, emit: the first n_emit <= K entries in sorted order to o (t and face; pt (n_emit,3) and
//          side (n_emit,) may be nullptr); asynchronous on s.  K <= 2^32 - 1.  When no row is longer than kLaneSort the
//          fill lanes order their own rows; otherwise all K entries go through stable radix sorts (face, t, row).
// ord must stay valid between the two (ws.vals holds its permutation).  Uses ws.flags, ranges, stats, out_a, out_b,
// out_c, and for long rows keys, keys_alt, out_d, hist, scan.
struct HitTotals {
    uint64_t K;        // 64-bit sum of the counts
    uint64_t longest;  // the largest count
};
struct HitOut {
    double* t;
    uint32_t* face;
    double* pt;
    int8_t* side;
};
int launch_raycast_all_count(msh_tree* tree, const QueryOrder& ord, const double* d_range, size_t S, HitTotals* out,
                             hipStream_t s);
int launch_raycast_all_emit(msh_tree* tree, const QueryOrder& ord, const double* d_range, size_t S, const HitTotals& tot,
                            const HitOut& o, size_t n_emit, hipStream_t s);
// The long-row ordering of a CSR list of K entries over S rows (the all-hits lists and the radius lists): on return
// (*idx)[p] is the entry that comes p-th by (row, d_key by value, d_id).  d_key (K,) is >= 0 and never NaN (its radix
// key is allhits_t_key), d_id (K,) < 2^id_bits is distinct within a row, d_offsets (S,) the exclusive scan of the
// counts.  In: *idx a buffer of K words; out: that buffer or ws.vals_alt.  Four stable LSD radix sorts of the index
// (id, key low, key high, row).  Uses ws.keys, keys_alt, vals_alt, hist, scan.  Asynchronous on s.
int order_csr_entries(const double* d_key, const uint32_t* d_id, int id_bits, const uint32_t* d_offsets, size_t S,
                      size_t K, Workspace& ws, uint32_t** idx, hipStream_t s);

// ---- all primitives within a radius (within.hip) ----
// Row r is (q[r], radius): d_r == nullptr: r_max for every row, else d_r[r] in the caller's row order.  A primitive
// qualifies when d2 <= radius * radius, d2 the K-nearest queries' exact squared distance (knn.h kb_eval); a row with a
// non-finite point or a negative or NaN radius has none.  Point trees and plain triangle trees; ord: the rows' slot order
// (lazy: ord.q are the caller's rows).  Every walk uses ws.spill and is asynchronous on s.
// d_counts[r] = the number of qualifying primitives; msh_timing_get name "within_count".
int launch_within_count(msh_tree* tree, const QueryOrder& ord, double r_max, const double* d_r, size_t S,
                        uint32_t* d_counts, hipStream_t s);
// the count walk, untimed, nothing written: d_stats[0] += nodes visited, [1] += primitives evaluated, [2] += entries,
// [3] = max(the deepest stack any row reached)
int launch_within_stats(msh_tree* tree, const QueryOrder& ord, double r_max, const double* d_r, size_t S,
                        unsigned long long* d_stats, hipStream_t s);
// The lists as CSR, sorted by (row, d2, id), in the two steps of the all-hits lists (HitTotals; the same buffers of ws):
// count into ws.flags and the totals read back on s (synchronous); then scan, fill, order, emit of the first n_emit <= K
// entries to o (asynchronous).  id and dist (n_emit,); pt (n_emit,3) and part (n_emit,) may be nullptr (triangle trees).
struct WithinOut {
    uint32_t* id;
    double* dist;
    double* pt;
    uint32_t* part;
};
int launch_within_all_count(msh_tree* tree, const QueryOrder& ord, double r_max, const double* d_r, size_t S,
                            HitTotals* out, hipStream_t s);
int launch_within_emit(msh_tree* tree, const QueryOrder& ord, double r_max, const double* d_r, size_t S,
                       const HitTotals& tot, const WithinOut& o, size_t n_emit, hipStream_t s);

// ---- triangle-triangle (tritri.hip) ----
constexpr int kLaneSort = 32;  // rows of up to this many hits are ordered by their own lane (k_tritri_all, k_raycast_all)
// out[0] += the 64-bit sum of counts[0..n), out[1] = max(out[1], the largest count); out zeroed by the caller
int sum_counts(const uint32_t* d_counts, size_t n, unsigned long long* d_out, unsigned nblk, hipStream_t s);
// flags[i] = 1 iff query triangle i intersects any tree triangle (self: skip shared-vertex pairs and
// the query triangles are the tree's own leaves in face order).
int launch_tri_intersect(const msh_tree* tree, const TriRec* d_qtris, size_t Tq, int self_mode, uint32_t* d_flags,
                         hipStream_t s);
// All hits as a pair list (row, mesh face), sorted by (row, mesh face).  A row is the query triangle's index, or in self
// mode (d_qtris = the tree's leaves, Tq = T) its face id, with only pairs row < mesh face kept.  Two steps, both using
// tree->ws (flags: the per-row counts, which stay valid between them; counters, ranges, the four sort buffers, spill):
//   count  the per-row counts and their totals, read back on s (synchronous).  packed: pack_query_tris ran before
//          on s, and bad_face says whether it met a face index >= Pq;
//   emit   scan, fill, order: the first n_emit <= K pairs to d_pairs (n_emit, 2); asynchronous on s.  K <= 2^32 - 1.
//          When no row is longer than tritri.hip's kLaneSort the fill lanes order their own rows and write the pairs;
//          otherwise all K pairs go through two stable radix sorts (mesh face, then row).
struct PairTotals {
    uint64_t K;        // 64-bit sum of the counts
    uint64_t longest;  // the largest count
    bool bad_face;
};
int launch_tri_pairs_count(msh_tree* tree, const TriRec* d_qtris, size_t Tq, int self_mode, bool packed, PairTotals* out,
                           hipStream_t s);
int launch_tri_pairs_emit(msh_tree* tree, const TriRec* d_qtris, size_t Tq, int self_mode, const PairTotals& tot,
                          uint32_t* d_pairs, size_t n_emit, hipStream_t s);
// query triangles of device arrays qv (Pq,3), qf (Tq,3) into tree->ws.q (TriRec, face = row)
int pack_query_tris(msh_tree* tree, const double* d_qv, size_t Pq, const uint32_t* d_qf, size_t Tq, hipStream_t s);

// ---- mesh geometry (geometry.hip) ----
// area-weighted vertex normals of (P,3) v over (T,3) f: sum of the faces' cross products in ascending
// face order per vertex, normalised (mesh.py:208-216)
// d_err (device u32, zeroed by the caller) is set when a face index is >= P (those faces are ignored)
int vertex_normals(const double* d_v, size_t P, const uint32_t* d_f, size_t T, double* d_vn, Workspace& ws,
                   hipStream_t s, uint32_t* d_err);

// ---- signed distance (sign.hip) ----
// The sign table of a triangle tree: unit face normals, the face across each edge (k = 0/1/2 for ab/bc/ca, the part
// codes 1/2/3), the face array and the angle-weighted vertex pseudonormals (Baerentzen and Aanaes 2005).
struct SignTable {
    const double* fn;     // (T,3) unit face normals (zero for a zero-area face)
    const double* vpn;    // (P,3) sum over incident faces of (angle at the vertex) x (unit face normal)
    const uint32_t* opp;  // (T,3) face across edge k, MSH_NO_FACE on a boundary or non-manifold edge
    const uint32_t* f;    // (T,3)
};
inline size_t sign_table_bytes(size_t P, size_t T) { return 48 * T + 24 * P; }
// the sections of a block of sign_table_bytes(P, T) bytes (256-B aligned base)
inline SignTable sign_table_of(void* block, size_t P, size_t T) {
    char* b = static_cast<char*>(block);
    return SignTable{reinterpret_cast<const double*>(b), reinterpret_cast<const double*>(b + 24 * T),
                     reinterpret_cast<const uint32_t*>(b + 24 * T + 24 * P),
                     reinterpret_cast<const uint32_t*>(b + 24 * T + 24 * P + 12 * T)};
}
// Fills `block` from the faces d_f (T,3) on the device, checked against the tree's leaves and vertices.
// d_counts (5 u32, zeroed by the caller): boundary, non-manifold and inconsistent edges, degenerate faces, and an error
// word (bit 0: a face index >= P, bit 1: a leaf's corners differ from v[f[face]]).  Asynchronous on s.
int sign_table_build(const msh_tree* tree, const uint32_t* d_f, void* block, uint32_t* d_counts, Workspace& ws,
                     hipStream_t s);
// sdist[i] = +-|q[i] - pt[i]|, negative where (q - pt) . N < 0 for the pseudonormal N of (face[i], part[i]);
// NaN for face >= T
int launch_sign_pass(const SignTable& tab, size_t T, size_t P, const double* d_q, size_t S, const uint32_t* d_face,
                     const uint32_t* d_part, const double* d_pt, double* d_sdist, hipStream_t s);

// ---- generalised winding numbers (winding.hip) ----
// The winding table of a triangle tree: one 32-B record per internal node, the dipole of its subtree (area-weighted
// centroid, a radius around it that holds the subtree's vertices, the sum of the area vectors; fp32, relative to the
// tree's origin).
constexpr size_t kWindRecBytes = 32;
inline size_t winding_table_bytes(size_t T) { return T > 1 ? (T - 1) * kWindRecBytes : 0; }
// per-lane stack entries the walk keeps in LDS before it spills
int winding_stack_lds();
// Fills `block` (winding_table_bytes(T), 16-B aligned) from d_nodes and the leaves alone: max_depth sweeps, each
// computing the nodes whose children are done.  d_err (2 u32, zeroed by the caller): [0] bit 0 = a child reference
// outside the tree, [1] = the root's sweep (0: never reached, the tree is deeper than max_depth).  Asynchronous on s.
int winding_table_build(const msh_tree* tree, void* block, uint32_t* d_err, Workspace& ws, hipStream_t s);
// w[row] = the winding number of q[row] (NaN for a non-finite row); ord: the rows' slot order (lazy: ord.q are the
// caller's rows).  beta = 0: every node is opened.  table: the tree's records (unused when T == 1).  Uses ws.spill.
int launch_winding(msh_tree* tree, const void* table, const QueryOrder& ord, size_t S, double beta, double* d_w,
                   hipStream_t s);
// the same walk, untimed, no answers: d_counts[0] += nodes approximated, [1] += nodes opened, [2] += leaves evaluated,
// [3] = max(the deepest stack any row reached)
int launch_winding_stats(msh_tree* tree, const void* table, const QueryOrder& ord, size_t S, double beta,
                         unsigned long long* d_counts, hipStream_t s);

// ---- K-nearest and radius-capped queries (kbest.hip) ----
// Caller-order outputs of S rows of K ranks: id (S,K) vertex index or face id, dist (S,K); triangle trees also pt
// (S,K,3) and part (S,K); count (S,).  pt, part and count may be nullptr.
struct KbOut {
    uint32_t* id;
    double* dist;
    double* pt;
    uint32_t* part;
    uint32_t* count;
};
// The first min(K, m) primitives within r_max of each row, ascending by (d2, id); unused ranks hold MSH_NO_FACE, +inf,
// NaN and part 0.  Point trees and plain triangle trees, 1 <= K <= MSH_KNEAREST_MAX, r_max >= 0 (the caller checked).
// ord: the rows' slot order (lazy: ord.q are the caller's rows).  d_inv: face -> leaf (face_leaf_map), needed for pt and
// part.  Uses ws.res, ws.res_w, ws.flags and ws.spill.  Asynchronous on s.
int launch_kbest(msh_tree* tree, const QueryOrder& ord, size_t S, uint32_t K, double r_max, const KbOut& o,
                 const uint32_t* d_inv, hipStream_t s);
// the same walk, untimed, no answers: d_counts[0] += nodes visited, [1] += primitives evaluated, [2] += list
// insertions, [3] = max(the deepest stack any row reached)
int launch_kbest_stats(msh_tree* tree, const QueryOrder& ord, size_t S, uint32_t K, double r_max,
                       unsigned long long* d_counts, hipStream_t s);

// ---- timing (devmem.cpp) ----
struct TimedLaunch {
    const char* name;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    TimedLaunch(const char* n, hipStream_t st);
    ~TimedLaunch();
};
// host-side intervals under the same names (msh_timing_get): the host pipeline's copies and waits
void host_time(const char* name, std::chrono::steady_clock::time_point t0);

// ---- the host layer: devmem.cpp (device state, the handle), entrycut.cpp, blob.cpp; hostpipe.h has the pipeline ----
extern thread_local std::string g_err;          // msh_last_error
extern thread_local int g_device;               // msh_set_device (-1: the runtime's current device)
extern thread_local std::vector<int> g_devices;  // devices of the trees built next on this thread (msh_set_devices)
int use_device(int dev);
int current_device(int* dev);
int device_cus(int dev);  // compute units of a device (cached; 256 when unknown): sizes the persistent grids
// blocks of a grid with one thread per element
inline unsigned blocks_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
// blocks of a persistent grid: the `wanted` ones, at most per_cu resident on each compute unit of the device
inline unsigned persistent_blocks(int dev, size_t wanted, unsigned per_cu) {
    return (unsigned)std::min<size_t>(wanted, (size_t)device_cus(dev) * per_cu);
}
// bits that hold the values 0 .. n - 1 (at most 32): the key width of a radix sort
inline int bits_for(size_t n) {
    int b = 0;
    while (b < 32 && ((size_t)1 << b) < n) ++b;
    return b;
}
// The spill area of a launch of nblk blocks whose lanes keep lds_depth stack entries in LDS (common.h stack_put) and
// may hold `need`: nothing for need <= lds_depth, else ws.spill grown to *depth = need - lds_depth + 1 entries per lane
// (block b's share starts at entry b * kBlock * *depth; a lane's entry sp >= lds_depth lies (sp - lds_depth) * kBlock
// behind its first).  The one place that sizes it: a lane that pushes beyond lds_depth + *depth entries writes outside
// the buffer.
int plan_spill(Workspace& ws, int need, int lds_depth, unsigned nblk, uint2** spill, int* depth);
// query workspaces handed from a freed triangle tree to the next one built on the device (devmem.cpp WsPool)
void ws_pool_take(int dev, Workspace& ws);
size_t ws_pool_trim();
size_t ws_pool_bytes();
int new_tree(int kind, msh_tree** out);
void free_tree(msh_tree* t);
int return_tree(msh_tree* t, int st, msh_tree** out);  // end of a build: *out = t, or t freed and the build's error kept
int finish_pending(msh_tree* t);  // end of an asynchronous batched build

template <class T>
inline int upload(DevBuf& buf, const T* host, size_t n, hipStream_t s) {
    MSH_TRY(buf.reserve(n * sizeof(T)));
    if (n) MSH_HIP(hipMemcpyAsync(buf.ptr, host, n * sizeof(T), hipMemcpyHostToDevice, s));
    return MSH_OK;
}

// Stream ordering of the handle's workspace: every launch sequence that uses `ws` first waits for the
// previous one (whatever stream it ran on) and then marks its own end, so a *_device call on a
// caller's stream followed by any other call on the same handle cannot overwrite scratch still in use.
struct WsOrder {
    msh_tree* t;
    hipStream_t s;
    WsOrder(msh_tree* tree, hipStream_t st) : t(tree), s(st) {
        if (t->ws_done) (void)hipStreamWaitEvent(s, t->ws_done, 0);
    }
    ~WsOrder() {
        if (t->ws_done) (void)hipEventRecord(t->ws_done, s);
    }
};

// frees a buffer the handle's launches read (entry cut, sign and winding tables) once none may still read it
template <class T>
inline void free_after_use(msh_tree* t, T*& p) {
    if (p) {
        (void)hipSetDevice(t->device);
        if (t->ws_done) (void)hipEventSynchronize(t->ws_done);
        (void)dfree(p);
    }
    p = nullptr;
}

// entry cut (entrycut.cpp): states of msh_tree::cut_state, and the policy's entry points
enum { kCutPending = 0, kCutBuilt = 1, kCutOff = 2, kCutFailed = 3 };
bool cut_applies(const msh_tree* t);
void free_entry_cut(msh_tree* t);
void ensure_entry_cut(msh_tree* t, size_t S);  // before a closest-point or alongnormal call of S rows

// copies of a freshly built tree on the other devices of the calling thread's device list (blob.cpp)
int replicate_tree(msh_tree* t);

}  // namespace msh
