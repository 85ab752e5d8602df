// libmeshsearch C ABI (include/meshsearch.h): the extern "C" entry points -- validation, error mapping, tree builds
// and the launch sequences around the HIP kernels -- and the helpers only they use.  Device state is devmem.cpp's, the
// host-buffer pipeline hostpipe.cpp's, the entry cut entrycut.cpp's, the blob blob.cpp's.  Mirrors the entry points of
// the reference's extensions:
//   spatialsearch  (mesh/src/spatialsearchmodule.cpp)   aabbtree_compute / _nearest / _nearest_alongnormal
//                                                         / _intersections_indices
//   aabb_normals   (mesh/src/aabb_normals.cpp)          aabbtree_n_compute / _n_nearest / _n_selfintersects
//   visibility     (mesh/src/py_visibility.cpp)         visibility_compute
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hostpipe.h"
#include "internal.h"

namespace msh {

static int check_faces(const uint32_t* f, size_t T, size_t P, const char* what) {
    for (size_t i = 0; i < 3 * T; ++i) {
        if (f[i] >= P) {
            set_error("%s: face %zu references vertex %u but only %zu vertices were given", what, i / 3, f[i], P);
            return MSH_EINVAL;
        }
    }
    return MSH_OK;
}

// queries, rays and permutation slots are 32-bit indices on the device
static int check_count(size_t S, const char* fn) {
    if (S > (size_t)0xFFFFFFFFull) {
        set_error("%s: %zu queries exceed the 32-bit index range of one call (split the batch)", fn, S);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

// Triangle tree over v (P rows) and f (T rows, indices into v).
// Subtrees of the LBVH over at most 2^kResplitLog2 leaves are rebuilt top down along the surface (refine.hip;
// C3: 2^12 and 2^17 measured slower, profiles/r03_c3_resplit_ab.jsonl)
constexpr int kResplitLog2 = 16;

static int build_triangles(msh_tree* t, const double* v, size_t Pall, const uint32_t* f, size_t T) {
    hipStream_t s = t->stream;
    hipEvent_t e0, e1;
    MSH_HIP(hipEventCreate(&e0));
    MSH_HIP(hipEventCreate(&e1));
    MSH_HIP(dmalloc(&t->d_v, std::max<size_t>(Pall, 1) * 3 * sizeof(double)));
    MSH_HIP(hipMemcpyAsync(t->d_v, v, Pall * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    DevBuf dF, dLo, dHi, dOrder;
    int st = MSH_OK;
    do {
        if ((st = upload(dF, f, 3 * T, s)) != MSH_OK) break;
        if ((st = dLo.reserve(3 * T * sizeof(double))) != MSH_OK) break;
        if ((st = dHi.reserve(3 * T * sizeof(double))) != MSH_OK) break;
        if ((st = dOrder.reserve(T * sizeof(uint32_t))) != MSH_OK) break;
        if (T > 1) {
            hipError_t e = dmalloc(&t->d_nodes, (T - 1) * sizeof(BNode));
            if (e != hipSuccess) { set_error("hipMalloc nodes: %s", hipGetErrorString(e)); st = MSH_ENOMEM; break; }
        }
        hipError_t e = dmalloc(&t->d_leaves, T * sizeof(TriRec));
        if (e != hipSuccess) { set_error("hipMalloc leaves: %s", hipGetErrorString(e)); st = MSH_ENOMEM; break; }
        (void)hipEventRecord(e0, s);
        if ((st = tri_bounds(t->d_v, dF.as<uint32_t>(), T, dLo.as<double>(), dHi.as<double>(), s)) != MSH_OK) break;
        if ((st = build_lbvh(t, dLo.as<double>(), dHi.as<double>(), T, dOrder.as<uint32_t>())) != MSH_OK) break;
        if ((st = resplit_tree(t, t->d_v, dF.as<uint32_t>(), T, dOrder.as<uint32_t>(), kResplitLog2)) != MSH_OK) break;
        if ((st = pack_tri_leaves(t->d_v, dF.as<uint32_t>(), dOrder.as<uint32_t>(), T, 0u,
                                  static_cast<TriRec*>(t->d_leaves), s)) != MSH_OK)
            break;
        if ((st = build_obb(t, true)) != MSH_OK) break;
        (void)hipEventRecord(e1, s);
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_error("LBVH build failed: %s", hipGetErrorString(e)); st = MSH_EDEVICE; break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        t->build_ms = ms;
    } while (0);
    (void)hipStreamSynchronize(s);
    dF.release(); dLo.release(); dHi.release(); dOrder.release();
    t->ws.release();  // build scratch (sort buffers, parents, ranges) is not needed by queries
    // a freed tree's query workspace, if one is idle (free_tree gives it back)
    if (st == MSH_OK) ws_pool_take(t->device, t->ws);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return st;
}

static const size_t kSortMin = 4096;  // below this the query Morton sort costs more than it saves

// Query order for S point rows (device): below kSortMin the caller's arrays are used as they are;
// otherwise Morton codes + radix sort give the permutation (ws.vals).  With allow_lazy (closest-point
// launches, and alongnormal rays with their normals) the traversal reads row perm[i] itself (and the
// closest-point one writes the inverse permutation, ws.inv); otherwise (the normals-metric queries) the rows and
// normals are gathered once into slot order (ws.qs / ws.ns) with the inverse permutation (gathering the
// closest-point rows too measured 3 % slower on C3; the C5 rays 0.5 ms slower, profiles/r06_c5_along_lazy_ab.jsonl).
// Queries are ordered by the Hilbert index of their cell of a 256^3 grid (the top 24 bits of their 30-bit Morton
// code, mapped through sort.hip's Hilbert state table; 3 radix passes): C3's 100M queries put ~6 in a cell, and the
// traversal runs the same node counts as with the full code.  The order within a cell is the caller's (stable sort).
constexpr int kQuerySortLo = 6;
static int sort_queries(msh_tree* t, const double* d_q, const double* d_n, size_t S, hipStream_t s,
                        QueryOrder* ord, bool allow_lazy = false) {
    *ord = QueryOrder{d_q, d_n, nullptr, nullptr};
    if (S < kSortMin) return MSH_OK;
    Workspace& ws = t->ws;
    MSH_TRY(ws.inv.reserve(S * sizeof(uint32_t)));
    float lo[3], hi[3];
    query_box(t, lo, hi);
    MSH_TRY(query_sort(lo, hi, d_q, S, kQuerySortLo, ws, s));
    if (allow_lazy) {
        *ord = QueryOrder{d_q, d_n, ws.vals.as<uint32_t>(), ws.inv.as<uint32_t>(), false};
        return MSH_OK;
    }
    MSH_TRY(ws.qs.reserve(3 * S * sizeof(double)));
    if (d_n) MSH_TRY(ws.ns.reserve(3 * S * sizeof(double)));
    MSH_TRY(gather_rows(d_q, d_n, ws.vals.as<uint32_t>(), S, ws.qs.as<double>(), d_n ? ws.ns.as<double>() : nullptr,
                        ws.inv.as<uint32_t>(), s));
    *ord = QueryOrder{ws.qs.as<double>(), d_n ? ws.ns.as<double>() : nullptr, ws.vals.as<uint32_t>(),
                      ws.inv.as<uint32_t>()};
    return MSH_OK;
}

// Batched trees: Morton order inside each mesh, meshes in order (two stable passes), then the gather.
static int sort_batch_queries(msh_tree* t, const double* d_q, size_t n, size_t S, hipStream_t s, QueryOrder* ord,
                              size_t mesh0 = 0) {
    *ord = QueryOrder{d_q, nullptr, nullptr, nullptr};
    if (n < kSortMin) return MSH_OK;
    Workspace& ws = t->ws;
    MSH_TRY(ws.keys.reserve(n * sizeof(uint32_t)));
    MSH_TRY(ws.vals.reserve(n * sizeof(uint32_t)));
    MSH_TRY(ws.keys_alt.reserve(n * sizeof(uint32_t)));
    MSH_TRY(ws.vals_alt.reserve(n * sizeof(uint32_t)));
    MSH_TRY(ws.qs.reserve(3 * n * sizeof(double)));
    MSH_TRY(ws.inv.reserve(n * sizeof(uint32_t)));
    uint32_t* keys = ws.keys.as<uint32_t>();
    uint32_t* vals = ws.vals.as<uint32_t>();
    MSH_TRY(query_morton_batch(t, d_q, n, S, keys, vals, s, mesh0));
    MSH_TRY(radix_sort_pairs(keys, vals, ws.keys_alt.as<uint32_t>(), ws.vals_alt.as<uint32_t>(), n, 30, ws, s));
    const size_t meshes = n / S;  // of this launch
    if (meshes > 1) {
        MSH_TRY(mesh_keys(vals, n, S, keys, s));
        MSH_TRY(radix_sort_pairs(keys, vals, ws.keys_alt.as<uint32_t>(), ws.vals_alt.as<uint32_t>(), n, bits_for(meshes),
                                 ws, s));
    }
    MSH_TRY(gather_rows(d_q, nullptr, vals, n, ws.qs.as<double>(), nullptr, ws.inv.as<uint32_t>(), s));
    *ord = QueryOrder{ws.qs.as<double>(), nullptr, vals, ws.inv.as<uint32_t>()};
    return MSH_OK;
}

static int check_tree(const msh_tree* t, int want_kind, const char* fn) {
    if (!t) {
        set_error("%s: null tree handle", fn);
        return MSH_EINVAL;
    }
    if (want_kind == kPoints ? t->kind != kPoints : t->kind == kPoints) {
        set_error("%s: wrong handle kind %d", fn, t->kind);
        return MSH_EINVAL;
    }
    // any batched handle (also B == 1: its bounds are relative to the per-mesh origins)
    if (t->B != 1 || t->d_boxes) {
        set_error("%s: batched tree handle (use the msh_batch_* entry points)", fn);
        return MSH_EINVAL;
    }
    return use_device(t->device);
}

// point trees (want kPoints) or plain triangle trees (want kTriangles): the K-nearest and ray-casting entry points;
// what: the query as the refusal of a normals-metric handle names it
static int check_plain_tree(const msh_tree* t, int want, const char* fn, const char* what) {
    MSH_TRY(check_tree(t, want, fn));
    if (t->kind == kNormals) {
        set_error("%s: normals-metric tree handle (%s a plain triangle tree)", fn, what);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

static int check_batch(const msh_tree* t, const char* fn) {
    if (!t) {
        set_error("%s: null tree handle", fn);
        return MSH_EINVAL;
    }
    if (!t->d_boxes) {
        set_error("%s: not a batched tree handle (build it with msh_batch_build)", fn);
        return MSH_EINVAL;
    }
    return use_device(t->device);
}

static hipStream_t pick(msh_tree* t, void* stream) { return stream ? static_cast<hipStream_t>(stream) : t->stream; }

// the handle's face -> leaf map (msh_tree_points_from_faces_device, msh_tree_knearest*), built on first use; that
// call waits for it, so the map is complete before any stream reads it
static int ensure_face_leaf(msh_tree* t, hipStream_t s) {
    if (t->d_face_leaf) return MSH_OK;
    uint32_t* inv = nullptr;
    MSH_HIP(dmalloc(&inv, t->T * sizeof(uint32_t)));
    const int st = face_leaf_map(t, inv, s);
    if (st != MSH_OK) {
        (void)hipStreamSynchronize(s);
        (void)dfree(inv);
        return st;
    }
    MSH_HIP(hipStreamSynchronize(s));
    t->d_face_leaf = inv;
    return MSH_OK;
}

// An instrumented launch on the handle's own stream: the rows' slot order (d_q == nullptr: the launch takes none),
// `zeroed` counter words of ws.stats cleared, launch(ord, d_counts, s), the first `nread` words read back into h.
template <class Launch>
static int stats_call(msh_tree* t, const double* d_q, const double* d_n, size_t S, size_t zeroed, unsigned long long* h,
                      size_t nread, Launch launch) {
    hipStream_t s = t->stream;
    {
        WsOrder order(t, s);
        QueryOrder ord{nullptr, nullptr, nullptr, nullptr};
        if (d_q) MSH_TRY(sort_queries(t, d_q, d_n, S, s, &ord, true));
        MSH_TRY(t->ws.stats.reserve(zeroed * sizeof(*h)));
        MSH_HIP(hipMemsetAsync(t->ws.stats.ptr, 0, zeroed * sizeof(*h), s));
        MSH_TRY(launch(ord, t->ws.stats.as<unsigned long long>(), s));
        MSH_HIP(hipMemcpyAsync(h, t->ws.stats.ptr, nread * sizeof(*h), hipMemcpyDeviceToHost, s));
    }
    MSH_HIP(hipStreamSynchronize(s));
    return MSH_OK;
}

// The table of one handle (sign, winding): a device block of `bytes` filled by build(block, d_counts, ws, s) on the
// handle's stream with scratch of its own, between two timing events; the N counter words are zeroed before and read
// back after, and install(h, block, ms) interprets them -- it sets the error and returns its status, or installs the
// block.  The block is freed unless install took it.  fn: the entry point's name in the messages.  Synchronous.
template <size_t N, class Build, class Install>
static int build_table(msh_tree* t, const char* fn, size_t bytes, Build build, Install install) {
    hipStream_t s = t->stream;
    void* block = nullptr;
    MSH_HIP(dmalloc(&block, bytes));
    Workspace ws;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    uint32_t h[N] = {};
    float ms = 0.f;
    int st = MSH_OK;
    do {
        hipError_t e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        if (e == hipSuccess && (st = ws.counters.reserve(sizeof(h))) != MSH_OK) break;
        if (e == hipSuccess) e = hipMemsetAsync(ws.counters.ptr, 0, sizeof(h), s);
        if (e == hipSuccess) e = hipEventRecord(e0, s);
        if (e != hipSuccess) { set_error("%s: %s", fn, hipGetErrorString(e)); st = MSH_EDEVICE; break; }
        if ((st = build(block, ws.counters.as<uint32_t>(), ws, s)) != MSH_OK) break;
        e = hipEventRecord(e1, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h, ws.counters.ptr, sizeof(h), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_error("%s: %s", fn, hipGetErrorString(e)); st = MSH_EDEVICE; break; }
        (void)hipEventElapsedTime(&ms, e0, e1);
    } while (0);
    (void)hipStreamSynchronize(s);  // the scratch is released on return
    ws.release();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st == MSH_OK) st = install(h, block, ms);
    if (st != MSH_OK) (void)dfree(block);
    return st;
}

// a table over the handle and its replicas: all or none (the host entry points split their rows over every replica)
template <class One, class Drop>
static int build_on_replicas(msh_tree* t, One one, Drop drop) {
    int st = one(t);
    for (size_t g = 0; g < t->replicas.size() && st == MSH_OK; ++g) st = one(t->replicas[g]);
    if (st != MSH_OK) {
        const std::string keep = g_err;
        drop(t);
        for (msh_tree* r : t->replicas) drop(r);
        g_err = keep;
    }
    (void)use_device(t->device);
    return st;
}

// flags[i] = whether query triangle i of n meets the tree (launch_tri_intersect), on the host.  up: the query triangles,
// uploaded first; nullptr: the tree's own leaves (self mode).  what: the call's name in a copy error.
static int intersect_flags(msh_tree* t, const std::vector<TriRec>* up, size_t n, int self_mode, const char* what,
                           std::vector<uint32_t>& flags) {
    hipStream_t s = t->stream;
    DevBuf dq, df;
    int st = MSH_OK;
    flags.resize(n);
    do {
        WsOrder order(t, s);
        if (up && (st = upload(dq, up->data(), n, s)) != MSH_OK) break;
        if ((st = df.reserve(n * sizeof(uint32_t))) != MSH_OK) break;
        const TriRec* d_q = up ? dq.as<TriRec>() : static_cast<const TriRec*>(t->d_leaves);
        if ((st = launch_tri_intersect(t, d_q, n, self_mode, df.as<uint32_t>(), s)) != MSH_OK) break;
        hipError_t e;
        if ((e = hipMemcpyAsync(flags.data(), df.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s)) != hipSuccess ||
            (e = hipStreamSynchronize(s)) != hipSuccess) {
            set_error("%s: %s", what, hipGetErrorString(e));
            st = MSH_EDEVICE;
        }
    } while (0);
    (void)hipStreamSynchronize(s);  // the buffers are released (DevBuf destructors) on return
    return st;
}

}  // namespace msh

using namespace msh;

extern "C" {

const char* msh_last_error(void) { return g_err.c_str(); }

int msh_version(void) { return 2; }

#ifndef MSH_SRC_HASH
#define MSH_SRC_HASH "unknown"
#endif
const char* msh_build_id(void) { return MSH_SRC_HASH; }

int msh_device_count(int* n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return MSH_EDEVICE;
    }
    *n = c;
    return MSH_OK;
}

// the calling thread's device, without touching its device list (msh_set_device_list selects its first entry here)
static int select_device(int device) {
    int c = 0;
    MSH_TRY(msh_device_count(&c));
    if (device < 0 || device >= c) {
        set_error("device %d out of range (%d devices)", device, c);
        return MSH_EINVAL;
    }
    g_device = device;
    return use_device(device);
}

// One device: the device list of msh_set_devices / msh_set_device_list is dropped too, so later trees are built
// on `device` alone and never replicated onto devices the caller no longer asked for.
int msh_set_device(int device) {
    MSH_TRY(select_device(device));
    g_devices.clear();
    return MSH_OK;
}

int msh_set_device_list(const int* devices, int G) {
    if (G < 0 || (G > 0 && !devices) || G > 64) { set_error("msh_set_device_list: bad device list (G = %d)", G); return MSH_EINVAL; }
    int c = 0;
    MSH_TRY(msh_device_count(&c));
    for (int g = 0; g < G; ++g)
        if (devices[g] < 0 || devices[g] >= c) {
            set_error("msh_set_device_list: device %d out of range (%d devices)", devices[g], c);
            return MSH_EINVAL;
        }
    if (G <= 1) {
        g_devices.clear();
        return G == 1 ? select_device(devices[0]) : MSH_OK;
    }
    MSH_TRY(select_device(devices[0]));
    g_devices.assign(devices, devices + G);
    return MSH_OK;
}

int msh_set_devices(int G) {
    int c = 0, d = 0;
    MSH_TRY(msh_device_count(&c));
    MSH_TRY(current_device(&d));
    if (G < 1 || d + G > c) {
        set_error("msh_set_devices: %d devices from device %d (%d visible)", G, d, c);
        return MSH_EINVAL;
    }
    std::vector<int> list(G);
    for (int g = 0; g < G; ++g) list[g] = d + g;
    return msh_set_device_list(list.data(), G);
}

int msh_tree_devices(const msh_tree* t, int* devices, int cap, int* G) {
    if (!t || !G) { set_error("msh_tree_devices: null argument"); return MSH_EINVAL; }
    *G = 1 + (int)t->replicas.size();
    if (devices && cap > 0) devices[0] = t->device;
    for (int g = 1; g < *G && g < cap; ++g)
        if (devices) devices[g] = t->replicas[g - 1]->device;
    return MSH_OK;
}

int msh_device_plan(uint64_t S, int G, uint64_t* begins) {
    if (G < 1 || !begins) { set_error("msh_device_plan: bad argument"); return MSH_EINVAL; }
    for (int g = 0; g < G; ++g) {
        size_t r0, n;
        shard_rows((size_t)S, (size_t)G, (size_t)g, &r0, &n);
        begins[g] = r0;
    }
    begins[G] = S;
    return MSH_OK;
}

int msh_tree_build_ex(const double* v, size_t P, const uint32_t* f, size_t T, const double* ev, size_t EP,
                      const uint32_t* ef, size_t ET, msh_tree** out) {
    if (!out) { set_error("null output handle"); return MSH_EINVAL; }
    *out = nullptr;
    if (T + ET == 0) { set_error("cannot build a tree over an empty mesh (0 faces)"); return MSH_EINVAL; }
    if (P > 0xFFFFFFFFull || T + ET > 0x7FFFFFFFull) { set_error("mesh too large"); return MSH_EINVAL; }
    MSH_TRY(check_faces(f, T, P, "faces"));
    if (ET) MSH_TRY(check_faces(ef, ET, EP, "extra faces"));
    msh_tree* t = nullptr;
    MSH_TRY(new_tree(kTriangles, &t));
    t->P = P;
    t->T = T + ET;
    t->T_main = T;
    int st;
    if (ET == 0) {
        st = build_triangles(t, v, P, f, T);
    } else {
        std::vector<double> vall(3 * (P + EP));
        std::memcpy(vall.data(), v, 3 * P * sizeof(double));
        std::memcpy(vall.data() + 3 * P, ev, 3 * EP * sizeof(double));
        std::vector<uint32_t> fall(3 * (T + ET));
        std::memcpy(fall.data(), f, 3 * T * sizeof(uint32_t));
        for (size_t i = 0; i < 3 * ET; ++i) fall[3 * T + i] = ef[i] + (uint32_t)P;
        st = build_triangles(t, vall.data(), P + EP, fall.data(), T + ET);
    }
    if (st == MSH_OK) st = replicate_tree(t);
    return return_tree(t, st, out);
}

int msh_tree_build(const double* v, size_t P, const uint32_t* f, size_t T, msh_tree** out) {
    return msh_tree_build_ex(v, P, f, T, nullptr, 0, nullptr, 0, out);
}

int msh_ntree_build(const double* v, size_t P, const uint32_t* f, size_t T, double eps, msh_tree** out) {
    MSH_TRY(msh_tree_build_ex(v, P, f, T, nullptr, 0, nullptr, 0, out));
    for (msh_tree* h : {*out}) {
        h->kind = kNormals;  // the normals metric starts at the root: no entry cut is ever built
        h->eps = eps;
        for (msh_tree* r : h->replicas) {
            r->kind = kNormals;
            r->eps = eps;
        }
    }
    return MSH_OK;
}

int msh_points_build(const double* v, size_t P, msh_tree** out) {
    if (!out) { set_error("null output handle"); return MSH_EINVAL; }
    *out = nullptr;
    if (P == 0) { set_error("cannot build a point tree over 0 vertices"); return MSH_EINVAL; }
    if (P > 0x7FFFFFFFull) { set_error("too many points"); return MSH_EINVAL; }
    msh_tree* t = nullptr;
    MSH_TRY(new_tree(kPoints, &t));
    t->P = P;
    t->T = P;
    t->T_main = P;
    hipStream_t s = t->stream;
    int st = MSH_OK;
    DevBuf dLo, dHi, dOrder;
    do {
        hipError_t e = dmalloc(&t->d_v, P * 3 * sizeof(double));
        if (e != hipSuccess) { set_error("hipMalloc: %s", hipGetErrorString(e)); st = MSH_ENOMEM; break; }
        e = hipMemcpyAsync(t->d_v, v, P * 3 * sizeof(double), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { set_error("H2D: %s", hipGetErrorString(e)); st = MSH_EDEVICE; break; }
        if ((st = dLo.reserve(3 * P * sizeof(double))) != MSH_OK) break;
        if ((st = dHi.reserve(3 * P * sizeof(double))) != MSH_OK) break;
        if ((st = dOrder.reserve(P * sizeof(uint32_t))) != MSH_OK) break;
        if (P > 1) {
            e = dmalloc(&t->d_nodes, (P - 1) * sizeof(BNode));
            if (e != hipSuccess) { set_error("hipMalloc nodes: %s", hipGetErrorString(e)); st = MSH_ENOMEM; break; }
        }
        e = dmalloc(&t->d_leaves, P * sizeof(PtRec));
        if (e != hipSuccess) { set_error("hipMalloc leaves: %s", hipGetErrorString(e)); st = MSH_ENOMEM; break; }
        if ((st = point_bounds(t->d_v, P, dLo.as<double>(), dHi.as<double>(), s)) != MSH_OK) break;
        if ((st = build_lbvh(t, dLo.as<double>(), dHi.as<double>(), P, dOrder.as<uint32_t>())) != MSH_OK) break;
        if ((st = pack_point_leaves(t->d_v, dOrder.as<uint32_t>(), P, static_cast<PtRec*>(t->d_leaves), s)) != MSH_OK)
            break;
        if ((st = build_obb(t, false)) != MSH_OK) break;
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_error("point LBVH build failed: %s", hipGetErrorString(e)); st = MSH_EDEVICE; break; }
    } while (0);
    (void)hipStreamSynchronize(s);
    dLo.release(); dHi.release(); dOrder.release();
    t->ws.release();
    if (st == MSH_OK) st = replicate_tree(t);
    return return_tree(t, st, out);
}

void msh_tree_free(msh_tree* tree) { free_tree(tree); }

int msh_tree_query_order(msh_tree* t, const double* d_q, size_t S, uint32_t* d_perm, void* stream) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_query_order"));
    MSH_TRY(check_count(S, "msh_tree_query_order"));
    if (S == 0) return MSH_OK;
    if (!d_q || !d_perm) { set_error("msh_tree_query_order: null argument"); return MSH_EINVAL; }
    hipStream_t s = pick(t, stream);
    WsOrder order(t, s);
    Workspace& ws = t->ws;
    float lo[3], hi[3];
    query_box(t, lo, hi);
    MSH_TRY(query_sort(lo, hi, d_q, S, kQuerySortLo, ws, s));
    MSH_HIP(hipMemcpyAsync(d_perm, ws.vals.ptr, S * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return MSH_OK;
}

int msh_tree_set_entry_cut(msh_tree* t, int G) {
    if (!t) { set_error("msh_tree_set_entry_cut: null tree handle"); return MSH_EINVAL; }
    if (G > 4096) { set_error("msh_tree_set_entry_cut: G = %d cells per axis (at most 4096)", G); return MSH_EINVAL; }
    const int want = G < 0 ? -1 : G;
    for (msh_tree* r : t->replicas) MSH_TRY(msh_tree_set_entry_cut(r, G));
    // the same grid again: a pending grid is built by the next call whatever its size (an automatic request on a
    // handle holding the coarse automatic grid asks for the fine one, below)
    if (want == t->cut_req && t->cut_state != kCutFailed && !(want < 0 && t->cut_state == kCutBuilt && !t->cut_fine)) {
        t->cut_force = true;
        return MSH_OK;
    }
    free_entry_cut(t);
    t->cut_req = want;
    t->cut_state = kCutPending;
    t->cut_force = true;
    return MSH_OK;
}

int msh_tree_entry_cut_info(const msh_tree* t, int* state, int* G, uint64_t* bytes, double* build_ms) {
    if (!t) { set_error("msh_tree_entry_cut_info: null tree handle"); return MSH_EINVAL; }
    const uint64_t n = t->d_cut ? (uint64_t)t->cut_G * t->cut_G * t->cut_G : 0;
    auto shown = [](const msh_tree* h) { return h->cut_state == kCutPending && !cut_applies(h) ? kCutOff : h->cut_state; };
    if (state) {
        // the handle's state, or the worst of its replicas' (failed, then still pending) when one differs
        *state = shown(t);
        for (const msh_tree* r : t->replicas) {
            const int rs = shown(r);
            if (rs == kCutFailed || (rs == kCutPending && *state != kCutFailed)) *state = rs;
        }
    }
    if (G) *G = t->d_cut ? t->cut_G : 0;
    if (bytes) *bytes = n * (t->cut_wide ? 64 : 32);
    if (build_ms) *build_ms = t->cut_ms;
    return MSH_OK;
}

int msh_tree_entry_cut_flagged(const msh_tree* t, uint64_t* cells) {
    if (!t || !cells) { set_error("msh_tree_entry_cut_flagged: null argument"); return MSH_EINVAL; }
    *cells = t->d_cut ? t->cut_flagged : 0;
    return MSH_OK;
}

int msh_tree_get_info(const msh_tree* t, msh_tree_info* info) {
    if (!t || !info) { set_error("null argument"); return MSH_EINVAL; }
    MSH_TRY(finish_pending(const_cast<msh_tree*>(t)));  // an asynchronous batched build: its GPU time
    info->device = t->device;
    info->kind = t->kind;
    info->n_points = t->P;
    info->n_faces = t->T;
    info->n_main_faces = t->T_main;
    info->n_nodes = t->T > 0 ? t->B * (t->T - 1) : 0;
    info->n_meshes = t->B;
    const size_t leaf = t->kind == kPoints ? sizeof(PtRec) : sizeof(TriRec);
    info->bytes = info->n_nodes * sizeof(BNode) + t->B * t->T * leaf;
    info->eps = t->eps;
    for (int k = 0; k < 3; ++k) {
        info->scene_lo[k] = t->scene_lo[k];
        info->scene_hi[k] = t->scene_hi[k];
    }
    info->build_ms = t->build_ms;
    info->node_bytes = (uint32_t)sizeof(BNode);
    info->leaf_bytes = (uint32_t)leaf;
    info->max_depth = t->max_depth;
    return MSH_OK;
}

// ---------------------------------------------------------------------------------------------
// one sorted closest-point launch over d_q (validated; the entry cut already settled by the caller)
static int nearest_run(msh_tree* t, const double* d_q, size_t S, const SlotOut& o, hipStream_t s) {
    WsOrder order(t, s);
    QueryOrder ord;
    MSH_TRY(sort_queries(t, d_q, nullptr, S, s, &ord, true));
    return launch_nearest(t, ord, S, o, s);
}

int msh_tree_nearest_device(msh_tree* t, const double* d_q, size_t S, uint32_t* d_face, uint32_t* d_part, double* d_pt,
                            void* stream) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_nearest_device"));
    MSH_TRY(check_count(S, "msh_tree_nearest_device"));
    if (S == 0) return MSH_OK;
    if (!d_q || !d_face || !d_pt) { set_error("msh_tree_nearest_device: null argument"); return MSH_EINVAL; }
    ensure_entry_cut(t, S);
    return nearest_run(t, d_q, S, SlotOut{d_face, d_part, d_pt, nullptr, nullptr}, pick(t, stream));
}

int msh_tree_points_from_faces_device(msh_tree* t, const double* d_q, size_t S, const uint32_t* d_face, uint32_t* d_part,
                                      double* d_pt, void* stream) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_points_from_faces_device"));
    MSH_TRY(check_count(S, "msh_tree_points_from_faces_device"));
    if (S == 0) return MSH_OK;
    if (!d_q || !d_face || !d_pt) { set_error("msh_tree_points_from_faces_device: null argument"); return MSH_EINVAL; }
    hipStream_t s = pick(t, stream);
    MSH_TRY(ensure_face_leaf(t, s));
    // no workspace is used (tree leaves and the map only), so no WsOrder: a rebuild of other ranks' points on a side
    // stream overlaps the next batch's traversal
    return points_from_faces(t, t->d_face_leaf, d_q, S, d_face, d_part, d_pt, s);
}

int msh_tree_nearest_bary_device(msh_tree* t, const double* d_q, size_t S, uint32_t* d_face, double* d_pt, double* d_w,
                                 void* stream) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_nearest_bary_device"));
    MSH_TRY(check_count(S, "msh_tree_nearest_bary_device"));
    if (S == 0) return MSH_OK;
    if (!d_q || !d_face || !d_pt || !d_w) { set_error("msh_tree_nearest_bary_device: null argument"); return MSH_EINVAL; }
    ensure_entry_cut(t, S);
    return nearest_run(t, d_q, S, SlotOut{d_face, nullptr, d_pt, nullptr, d_w}, pick(t, stream));
}

// The host-buffer entry points declare their columns once (hostpipe.h host_call) and read a chunk's slabs by column.
constexpr bool kSettleCut = true, kNoCut = false;  // whether the call's rows settle each handle's entry cut first

int msh_tree_nearest(msh_tree* t, const double* q, size_t S, uint32_t* face, uint32_t* part, double* pt) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_nearest"));
    MSH_TRY(check_count(S, "msh_tree_nearest"));
    if (S == 0) return MSH_OK;
    if (!q || !face || !pt) { set_error("msh_tree_nearest: null argument"); return MSH_EINVAL; }
    HostCols c;  // part keeps its slab when the caller wants none (nothing is written to or downloaded from it)
    const auto cq = c.in(q, 3);
    const auto cface = c.out(face, 1), cpart = c.out(part, 1);
    const auto cpt = c.out(pt, 3);
    return host_call(t, S, c, kSettleCut, [&](msh_tree* h, size_t n, const Slabs& d) {
        return nearest_run(h, d[cq], n, SlotOut{d[cface], part ? d[cpart] : nullptr, d[cpt], nullptr, nullptr}, h->stream);
    });
}

int msh_tree_nearest_bary(msh_tree* t, const double* q, size_t S, uint32_t* face, double* pt, double* w) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_nearest_bary"));
    MSH_TRY(check_count(S, "msh_tree_nearest_bary"));
    if (S == 0) return MSH_OK;
    if (!q || !face || !pt || !w) { set_error("msh_tree_nearest_bary: null argument"); return MSH_EINVAL; }
    HostCols c;
    const auto cq = c.in(q, 3);
    const auto cface = c.out(face, 1);
    const auto cpt = c.out(pt, 3), cw = c.out(w, 3);
    return host_call(t, S, c, kSettleCut, [&](msh_tree* h, size_t n, const Slabs& d) {
        return nearest_run(h, d[cq], n, SlotOut{d[cface], nullptr, d[cpt], nullptr, d[cw]}, h->stream);
    });
}

int msh_tree_nearest_stats(msh_tree* t, const double* d_q, size_t S, uint64_t* nodes, uint64_t* leaves) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_nearest_stats"));
    MSH_TRY(check_count(S, "msh_tree_nearest_stats"));
    *nodes = 0;
    *leaves = 0;
    if (S == 0) return MSH_OK;
    ensure_entry_cut(t, S);
    unsigned long long h[48] = {0};
    MSH_TRY(stats_call(t, d_q, nullptr, S, 48, h, 48, [&](const QueryOrder& ord, unsigned long long* d, hipStream_t s) {
        return launch_nearest_stats(t, ord, S, d, s);
    }));
    *nodes = h[0];
    *leaves = h[1];
    if (getenv("MESH_AMD_STATS_DUMP")) {  // development: wave-iteration utilisation of pass 1
        fprintf(stderr, "[msh stats] S=%zu nodes=%llu leaves=%llu trav_it=%llu trav_lanes=%llu leaf_it=%llu "
                        "leaf_lanes=%llu pass2_items=%llu\n", S, h[0], h[1], h[2], h[3], h[4], h[5], h[6]);
        // per phase: tiles, sum of per-tile max node steps, sum of lane steps, sum of min(tile max, 128 / 256 /
        // 512), lanes over 128 / 256 / 512 steps
        const char* nm[3] = {"super", "lead", "follow"};
        for (int p = 0; p < 3; ++p) {
            const unsigned long long* x = h + 8 + 9 * p;
            fprintf(stderr, "[msh tiles] %s tiles=%llu sum_max=%llu sum_steps=%llu cap128=%llu cap256=%llu "
                            "cap512=%llu over128=%llu over256=%llu over512=%llu\n", nm[p], x[0], x[1], x[2], x[3],
                    x[4], x[5], x[6], x[7], x[8]);
        }
        fprintf(stderr, "[msh pass2] waves=%llu items=%llu visits_sum=%llu visits_max_item=%llu\n", h[6], h[46], h[44],
                h[45]);
        fprintf(stderr, "[msh leaves] improving_phase_tests=%llu hinted=%llu hint_leaf_won=%llu\n", h[36], h[37], h[38]);
    }
    return MSH_OK;
}

// ---- signed distance (sign.hip) ----
// plain triangle trees only: the table's faces are the tree's leaves, one to one
static int check_sign_tree(const msh_tree* t, const char* fn) {
    MSH_TRY(check_tree(t, kTriangles, fn));
    if (t->kind != kTriangles) {
        set_error("%s: normals-metric tree handle (signed distance needs a plain triangle tree)", fn);
        return MSH_EINVAL;
    }
    if (t->T != t->T_main) {
        set_error("%s: the tree was built with extra faces (%zu of %zu leaves are the main mesh's)", fn, t->T_main, t->T);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

static int check_sign_built(const msh_tree* t, const char* fn) {
    if (!t->d_sign) {
        set_error("%s: the tree has no sign table (call msh_tree_sign_build first)", fn);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

static void free_sign_table(msh_tree* t) {
    free_after_use(t, t->d_sign);
    t->sign = msh_sign_info{0, 0, 0, 0, 0, 0, 0.0};
}

// the table of one handle (its own device and stream): the faces are uploaded, and the new table replaces an old one
static int sign_build_one(msh_tree* t, const uint32_t* f) {
    MSH_TRY(use_device(t->device));
    const size_t bytes = sign_table_bytes(t->P, t->T);
    DevBuf dF;  // read by the build: released after build_table's final synchronisation
    MSH_TRY(upload(dF, f, 3 * t->T, t->stream));
    auto build = [&](void* block, uint32_t* d_counts, Workspace& ws, hipStream_t s) {
        return sign_table_build(t, dF.as<uint32_t>(), block, d_counts, ws, s);
    };
    return build_table<5>(t, "msh_tree_sign_build", bytes, build, [&](const uint32_t* h, void* block, float ms) {
        if (h[4] & 1u) {
            set_error("msh_tree_sign_build: face index out of range (>= %zu vertices)", t->P);
            return MSH_EINVAL;
        }
        if (h[4] & 2u) {
            set_error("msh_tree_sign_build: faces do not match the tree (a leaf's corners differ from v[f[face]])");
            return MSH_EINVAL;
        }
        free_sign_table(t);
        t->d_sign = block;
        t->sign = msh_sign_info{1, h[0], h[1], h[2], h[3], bytes, ms};
        return MSH_OK;
    });
}

int msh_tree_sign_build(msh_tree* t, const uint32_t* f, size_t T) {
    MSH_TRY(check_sign_tree(t, "msh_tree_sign_build"));
    if (!f) { set_error("msh_tree_sign_build: null faces"); return MSH_EINVAL; }
    if (T != t->T) {
        set_error("msh_tree_sign_build: %zu faces given, the tree holds %zu", T, t->T);
        return MSH_EINVAL;
    }
    return build_on_replicas(t, [&](msh_tree* h) { return sign_build_one(h, f); }, free_sign_table);
}

int msh_tree_sign_info(const msh_tree* t, msh_sign_info* info) {
    if (!t || !info) { set_error("msh_tree_sign_info: null argument"); return MSH_EINVAL; }
    *info = t->sign;
    return MSH_OK;
}

// the closest-point launch of nearest_run, then the sign pass over its answers in caller order (part codes from
// workspace scratch when the caller wants none)
static int signed_run(msh_tree* t, const double* d_q, size_t S, double* d_sdist, uint32_t* d_face, uint32_t* d_part,
                      double* d_pt, hipStream_t s) {
    WsOrder order(t, s);
    if (!d_part) {
        MSH_TRY(t->ws.sgn.reserve(S * sizeof(uint32_t)));
        d_part = t->ws.sgn.as<uint32_t>();
    }
    QueryOrder ord;
    MSH_TRY(sort_queries(t, d_q, nullptr, S, s, &ord, true));
    MSH_TRY(launch_nearest(t, ord, S, SlotOut{d_face, d_part, d_pt, nullptr, nullptr}, s));
    return launch_sign_pass(sign_table_of(t->d_sign, t->P, t->T), t->T, t->P, d_q, S, d_face, d_part, d_pt, d_sdist, s);
}

int msh_tree_signed_distance_device(msh_tree* t, const double* d_q, size_t S, double* d_sdist, uint32_t* d_face,
                                    uint32_t* d_part, double* d_pt, void* stream) {
    MSH_TRY(check_sign_tree(t, "msh_tree_signed_distance_device"));
    MSH_TRY(check_count(S, "msh_tree_signed_distance_device"));
    MSH_TRY(check_sign_built(t, "msh_tree_signed_distance_device"));
    if (S == 0) return MSH_OK;
    if (!d_q || !d_sdist || !d_face || !d_pt) {
        set_error("msh_tree_signed_distance_device: null argument");
        return MSH_EINVAL;
    }
    ensure_entry_cut(t, S);
    return signed_run(t, d_q, S, d_sdist, d_face, d_part, d_pt, pick(t, stream));
}

int msh_tree_sign_from_faces_device(msh_tree* t, const double* d_q, size_t S, const uint32_t* d_face,
                                    const uint32_t* d_part, const double* d_pt, double* d_sdist, void* stream) {
    MSH_TRY(check_sign_tree(t, "msh_tree_sign_from_faces_device"));
    MSH_TRY(check_count(S, "msh_tree_sign_from_faces_device"));
    MSH_TRY(check_sign_built(t, "msh_tree_sign_from_faces_device"));
    if (S == 0) return MSH_OK;
    if (!d_q || !d_face || !d_part || !d_pt || !d_sdist) {
        set_error("msh_tree_sign_from_faces_device: null argument");
        return MSH_EINVAL;
    }
    // no workspace is used (the table only), so no WsOrder, as msh_tree_points_from_faces_device
    return launch_sign_pass(sign_table_of(t->d_sign, t->P, t->T), t->T, t->P, d_q, S, d_face, d_part, d_pt, d_sdist,
                            pick(t, stream));
}

int msh_tree_signed_distance(msh_tree* t, const double* q, size_t S, double* sdist, uint32_t* face, uint32_t* part,
                             double* pt) {
    MSH_TRY(check_sign_tree(t, "msh_tree_signed_distance"));
    MSH_TRY(check_count(S, "msh_tree_signed_distance"));
    MSH_TRY(check_sign_built(t, "msh_tree_signed_distance"));
    for (const msh_tree* r : t->replicas) MSH_TRY(check_sign_built(r, "msh_tree_signed_distance"));
    if (S == 0) return MSH_OK;
    if (!q || !sdist || !face || !pt) { set_error("msh_tree_signed_distance: null argument"); return MSH_EINVAL; }
    HostCols c;  // the part slab serves the sign pass also when the caller wants no parts
    const auto cq = c.in(q, 3);
    const auto csd = c.out(sdist, 1);
    const auto cface = c.out(face, 1), cpart = c.out(part, 1);
    const auto cpt = c.out(pt, 3);
    return host_call(t, S, c, kSettleCut, [&](msh_tree* h, size_t n, const Slabs& d) {
        return signed_run(h, d[cq], n, d[csd], d[cface], d[cpart], d[cpt], h->stream);
    });
}

// ---- generalised winding numbers (winding.hip) ----
// plain triangle trees (extra faces included: the sum runs over every leaf)
static int check_wind_tree(const msh_tree* t, const char* fn) {
    MSH_TRY(check_tree(t, kTriangles, fn));
    if (t->kind != kTriangles) {
        set_error("%s: normals-metric tree handle (winding numbers need a plain triangle tree)", fn);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

static int check_beta(double beta, const char* fn) {
    if (!(beta >= 0.0)) {
        set_error("%s: beta must be >= 0 (0: exact), got %g", fn, beta);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

static void free_wind_table(msh_tree* t) {
    free_after_use(t, t->d_wind);
    t->wind = msh_winding_info{0, 0, 0, 0, 0.0};
}

// the table of one handle, if it needs one and has none (its own device and stream)
static int wind_build_one(msh_tree* t) {
    if (t->d_wind || t->T < 2 || !t->d_nodes) return MSH_OK;
    MSH_TRY(use_device(t->device));
    const size_t bytes = winding_table_bytes(t->T);
    auto build = [&](void* block, uint32_t* d_err, Workspace& ws, hipStream_t s) {
        return winding_table_build(t, block, d_err, ws, s);
    };
    return build_table<2>(t, "msh_tree_winding_build", bytes, build, [&](const uint32_t* h, void* block, float ms) {
        if (h[0] & 1u) {
            set_error("msh_tree_winding_build: a node's child reference lies outside the tree (corrupt tree)");
            return MSH_EDEVICE;
        }
        if (h[1] == 0u) {
            set_error("msh_tree_winding_build: the tree is deeper than its recorded depth %d (corrupt tree)", t->max_depth);
            return MSH_EDEVICE;
        }
        t->d_wind = block;
        t->wind = msh_winding_info{1, (uint32_t)kWindRecBytes, (uint32_t)winding_stack_lds(), bytes, ms};
        return MSH_OK;
    });
}

static int wind_build_all(msh_tree* t) { return build_on_replicas(t, wind_build_one, free_wind_table); }

int msh_tree_winding_build(msh_tree* t) {
    MSH_TRY(check_wind_tree(t, "msh_tree_winding_build"));
    return wind_build_all(t);
}

int msh_tree_winding_info(const msh_tree* t, msh_winding_info* info) {
    if (!t || !info) { set_error("msh_tree_winding_info: null argument"); return MSH_EINVAL; }
    *info = t->wind;
    info->node_bytes = (uint32_t)kWindRecBytes;
    info->stack_lds = (uint32_t)winding_stack_lds();
    return MSH_OK;
}

// one launch over d_q in the closest-point path's slot order (the table is built)
static int winding_run(msh_tree* t, const double* d_q, size_t S, double beta, double* d_w, hipStream_t s) {
    WsOrder order(t, s);
    QueryOrder ord;
    MSH_TRY(sort_queries(t, d_q, nullptr, S, s, &ord, true));
    return launch_winding(t, t->d_wind, ord, S, beta, d_w, s);
}

int msh_tree_winding_number_device(msh_tree* t, const double* d_q, size_t S, double beta, double* d_w, void* stream) {
    MSH_TRY(check_beta(beta, "msh_tree_winding_number_device"));  // before the handle: a bad beta is refused on any of them
    MSH_TRY(check_wind_tree(t, "msh_tree_winding_number_device"));
    MSH_TRY(check_count(S, "msh_tree_winding_number_device"));
    if (S == 0) return MSH_OK;
    if (!d_q || !d_w) { set_error("msh_tree_winding_number_device: null argument"); return MSH_EINVAL; }
    MSH_TRY(wind_build_one(t));
    return winding_run(t, d_q, S, beta, d_w, pick(t, stream));
}

int msh_tree_winding_number(msh_tree* t, const double* q, size_t S, double beta, double* w) {
    MSH_TRY(check_beta(beta, "msh_tree_winding_number"));  // before the handle: a bad beta is refused on any of them
    MSH_TRY(check_wind_tree(t, "msh_tree_winding_number"));
    MSH_TRY(check_count(S, "msh_tree_winding_number"));
    if (S == 0) return MSH_OK;
    if (!q || !w) { set_error("msh_tree_winding_number: null argument"); return MSH_EINVAL; }
    MSH_TRY(wind_build_all(t));
    HostCols c;
    const auto cq = c.in(q, 3);
    const auto cw = c.out(w, 1);
    return host_call(t, S, c, kNoCut, [&](msh_tree* h, size_t n, const Slabs& d) {
        return winding_run(h, d[cq], n, beta, d[cw], h->stream);
    });
}

int msh_tree_winding_stats(msh_tree* t, const double* d_q, size_t S, double beta, uint64_t counts[4]) {
    MSH_TRY(check_beta(beta, "msh_tree_winding_stats"));  // before the handle: a bad beta is refused on any of them
    MSH_TRY(check_wind_tree(t, "msh_tree_winding_stats"));
    MSH_TRY(check_count(S, "msh_tree_winding_stats"));
    if (!counts) { set_error("msh_tree_winding_stats: null argument"); return MSH_EINVAL; }
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    if (S == 0) return MSH_OK;
    if (!d_q) { set_error("msh_tree_winding_stats: null argument"); return MSH_EINVAL; }
    MSH_TRY(wind_build_one(t));
    unsigned long long h[4] = {0, 0, 0, 0};
    MSH_TRY(stats_call(t, d_q, nullptr, S, 4, h, 4, [&](const QueryOrder& ord, unsigned long long* d, hipStream_t s) {
        return launch_winding_stats(t, t->d_wind, ord, S, beta, d, s);
    }));
    for (int k = 0; k < 4; ++k) counts[k] = h[k];
    return MSH_OK;
}

// the rays' walks start from the tree's entry cut (built by the automatic policy on these rows too: rays_cut)
static int along_run(msh_tree* t, const double* d_p, const double* d_n, size_t S, double* d_dist, uint32_t* d_face,
                     double* d_pt, hipStream_t s) {
    WsOrder order(t, s);
    QueryOrder ord;
    MSH_TRY(sort_queries(t, d_p, d_n, S, s, &ord, true));
    return launch_alongnormal(t, ord, S, SlotOut{d_face, nullptr, d_pt, nullptr, d_dist}, s);
}

int msh_tree_nearest_alongnormal_device(msh_tree* t, const double* d_p, const double* d_n, size_t S, double* d_dist,
                                        uint32_t* d_face, double* d_pt, void* stream) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_nearest_alongnormal_device"));
    MSH_TRY(check_count(S, "msh_tree_nearest_alongnormal_device"));
    if (S == 0) return MSH_OK;
    ensure_entry_cut(t, S);
    return along_run(t, d_p, d_n, S, d_dist, d_face, d_pt, pick(t, stream));
}

int msh_tree_nearest_alongnormal_stats(msh_tree* t, const double* d_p, const double* d_n, size_t S, uint64_t* nodes,
                                       uint64_t* leaves) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_nearest_alongnormal_stats"));
    MSH_TRY(check_count(S, "msh_tree_nearest_alongnormal_stats"));
    if (!nodes || !leaves) { set_error("msh_tree_nearest_alongnormal_stats: null argument"); return MSH_EINVAL; }
    *nodes = *leaves = 0;
    if (S == 0) return MSH_OK;
    ensure_entry_cut(t, S);
    unsigned long long h[2] = {0, 0};
    MSH_TRY(stats_call(t, d_p, d_n, S, 8, h, 2, [&](const QueryOrder& ord, unsigned long long* d, hipStream_t s) {
        return launch_alongnormal_stats(t, ord, S, d, s);
    }));
    *nodes = h[0];
    *leaves = h[1];
    return MSH_OK;
}

int msh_visibility_stats(msh_tree* t, const double* d_cams, size_t C, double min_dist, uint64_t* nodes,
                         uint64_t* leaves) {
    MSH_TRY(check_tree(t, kTriangles, "msh_visibility_stats"));
    if (!nodes || !leaves || (C && !d_cams)) { set_error("msh_visibility_stats: null argument"); return MSH_EINVAL; }
    *nodes = *leaves = 0;
    if (C == 0 || t->P == 0) return MSH_OK;
    unsigned long long h[2] = {0, 0};
    MSH_TRY(stats_call(t, nullptr, nullptr, C, 8, h, 2, [&](const QueryOrder&, unsigned long long* d, hipStream_t s) {
        return launch_visibility_stats(t, d_cams, C, min_dist, d, s);
    }));
    *nodes = h[0];
    *leaves = h[1];
    return MSH_OK;
}

int msh_tree_nearest_alongnormal(msh_tree* t, const double* p, const double* n, size_t S, double* dist, uint32_t* face,
                                 double* pt) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_nearest_alongnormal"));
    MSH_TRY(check_count(S, "msh_tree_nearest_alongnormal"));
    if (S == 0) return MSH_OK;
    if (!p || !n || !dist || !face || !pt) { set_error("msh_tree_nearest_alongnormal: null argument"); return MSH_EINVAL; }
    HostCols c;
    const auto cp = c.in(p, 3), cn = c.in(n, 3);
    const auto cdist = c.out(dist, 1);
    const auto cface = c.out(face, 1);
    const auto cpt = c.out(pt, 3);
    return host_call(t, S, c, kSettleCut, [&](msh_tree* h, size_t rows, const Slabs& d) {
        return along_run(h, d[cp], d[cn], rows, d[cdist], d[cface], d[cpt], h->stream);
    });
}

// ---- ray casting: first hit and occlusion for arbitrary rays (raycast.hip) ----

// one launch over the rays in the slot order of their origins, from the root (no entry cut)
static int raycast_run(msh_tree* t, const double* d_o, const double* d_d, const double* d_range, size_t S,
                       const RayOut& o, hipStream_t s) {
    WsOrder order(t, s);
    QueryOrder ord;
    MSH_TRY(sort_queries(t, d_o, d_d, S, s, &ord, true));
    return launch_raycast(t, ord, d_range, S, o, nullptr, s);
}

int msh_tree_raycast_device(msh_tree* t, const double* d_o, const double* d_d, const double* d_range, size_t S,
                            double* d_t, uint32_t* d_face, double* d_pt, double* d_w, void* stream) {
    MSH_TRY(check_plain_tree(t, kTriangles, "msh_tree_raycast_device", "ray casting needs"));
    MSH_TRY(check_count(S, "msh_tree_raycast_device"));
    if (S == 0) return MSH_OK;
    if (!d_o || !d_d || !d_t || !d_face) { set_error("msh_tree_raycast_device: null argument"); return MSH_EINVAL; }
    return raycast_run(t, d_o, d_d, d_range, S, RayOut{false, d_t, d_face, d_pt, d_w, nullptr}, pick(t, stream));
}

int msh_tree_raycast(msh_tree* t, const double* o, const double* d, const double* range, size_t S, double* tt,
                     uint32_t* face, double* pt, double* w) {
    MSH_TRY(check_plain_tree(t, kTriangles, "msh_tree_raycast", "ray casting needs"));
    MSH_TRY(check_count(S, "msh_tree_raycast"));
    if (S == 0) return MSH_OK;
    if (!o || !d || !tt || !face) { set_error("msh_tree_raycast: null argument"); return MSH_EINVAL; }
    HostCols c;  // a NULL range and the outputs the caller did not ask for take no slab space
    const auto co = c.in(o, 3), cd = c.in(d, 3);
    const auto cr = c.in(range, range ? 2 : 0);
    const auto ct = c.out(tt, 1);
    const auto cpt = c.out(pt, pt ? 3 : 0);
    const auto cw = c.out(w, w ? 3 : 0);
    const auto cface = c.out(face, 1);  // the 4-B column last: the fp64 columns stay 8-B aligned in a slab of odd rows
    return host_call(t, S, c, kNoCut, [&](msh_tree* h, size_t n, const Slabs& s) {
        return raycast_run(h, s[co], s[cd], range ? s[cr] : nullptr, n,
                           RayOut{false, s[ct], s[cface], pt ? s[cpt] : nullptr, w ? s[cw] : nullptr, nullptr},
                           h->stream);
    });
}

int msh_tree_occluded_device(msh_tree* t, const double* d_o, const double* d_d, const double* d_range, size_t S,
                             uint8_t* d_hit, void* stream) {
    MSH_TRY(check_plain_tree(t, kTriangles, "msh_tree_occluded_device", "ray casting needs"));
    MSH_TRY(check_count(S, "msh_tree_occluded_device"));
    if (S == 0) return MSH_OK;
    if (!d_o || !d_d || !d_hit) { set_error("msh_tree_occluded_device: null argument"); return MSH_EINVAL; }
    return raycast_run(t, d_o, d_d, d_range, S, RayOut{true, nullptr, nullptr, nullptr, nullptr, d_hit},
                       pick(t, stream));
}

int msh_tree_occluded(msh_tree* t, const double* o, const double* d, const double* range, size_t S, uint8_t* hit) {
    MSH_TRY(check_plain_tree(t, kTriangles, "msh_tree_occluded", "ray casting needs"));
    MSH_TRY(check_count(S, "msh_tree_occluded"));
    if (S == 0) return MSH_OK;
    if (!o || !d || !hit) { set_error("msh_tree_occluded: null argument"); return MSH_EINVAL; }
    HostCols c;
    const auto co = c.in(o, 3), cd = c.in(d, 3);
    const auto cr = c.in(range, range ? 2 : 0);
    const auto chit = c.out(hit, 1);
    return host_call(t, S, c, kNoCut, [&](msh_tree* h, size_t n, const Slabs& s) {
        return raycast_run(h, s[co], s[cd], range ? s[cr] : nullptr, n,
                           RayOut{true, nullptr, nullptr, nullptr, nullptr, s[chit]}, h->stream);
    });
}

int msh_tree_raycast_stats(msh_tree* t, const double* d_o, const double* d_d, const double* d_range, size_t S, int any,
                           uint64_t* nodes, uint64_t* leaves) {
    MSH_TRY(check_plain_tree(t, kTriangles, "msh_tree_raycast_stats", "ray casting needs"));
    MSH_TRY(check_count(S, "msh_tree_raycast_stats"));
    if (!nodes || !leaves) { set_error("msh_tree_raycast_stats: null argument"); return MSH_EINVAL; }
    *nodes = *leaves = 0;
    if (S == 0) return MSH_OK;
    if (!d_o || !d_d) { set_error("msh_tree_raycast_stats: null argument"); return MSH_EINVAL; }
    unsigned long long h[2] = {0, 0};
    MSH_TRY(stats_call(t, d_o, d_d, S, 2, h, 2, [&](const QueryOrder& ord, unsigned long long* d, hipStream_t s) {
        return launch_raycast(t, ord, d_range, S, RayOut{any != 0, nullptr, nullptr, nullptr, nullptr, nullptr}, d, s);
    }));
    *nodes = h[0];
    *leaves = h[1];
    return MSH_OK;
}

// ---- ray casting: hit counts and sorted all-hits lists (raycast_all.hip) ----

static int raycast_count_run(msh_tree* t, const double* d_o, const double* d_d, const double* d_range, size_t S,
                             uint32_t* d_count, hipStream_t s) {
    WsOrder order(t, s);
    QueryOrder ord;
    MSH_TRY(sort_queries(t, d_o, d_d, S, s, &ord, true));
    return launch_raycast_count(t, ord, d_range, S, d_count, s);
}

int msh_tree_raycast_count_device(msh_tree* t, const double* d_o, const double* d_d, const double* d_range, size_t S,
                                  uint32_t* d_count, void* stream) {
    MSH_TRY(check_plain_tree(t, kTriangles, "msh_tree_raycast_count_device", "ray casting needs"));
    MSH_TRY(check_count(S, "msh_tree_raycast_count_device"));
    if (S == 0) return MSH_OK;
    if (!d_o || !d_d || !d_count) { set_error("msh_tree_raycast_count_device: null argument"); return MSH_EINVAL; }
    return raycast_count_run(t, d_o, d_d, d_range, S, d_count, pick(t, stream));
}

int msh_tree_raycast_count(msh_tree* t, const double* o, const double* d, const double* range, size_t S,
                           uint32_t* count) {
    MSH_TRY(check_plain_tree(t, kTriangles, "msh_tree_raycast_count", "ray casting needs"));
    MSH_TRY(check_count(S, "msh_tree_raycast_count"));
    if (S == 0) return MSH_OK;
    if (!o || !d || !count) { set_error("msh_tree_raycast_count: null argument"); return MSH_EINVAL; }
    HostCols c;
    const auto co = c.in(o, 3), cd = c.in(d, 3);
    const auto cr = c.in(range, range ? 2 : 0);
    const auto ccount = c.out(count, 1);
    return host_call(t, S, c, kNoCut, [&](msh_tree* h, size_t n, const Slabs& s) {
        return raycast_count_run(h, s[co], s[cd], range ? s[cr] : nullptr, n, s[ccount], h->stream);
    });
}

// Count, read K back, then scan / fill / order / emit the first min(K, cap) entries (launch_raycast_all_*).  host_out:
// the outputs are host arrays -- the list comes through device buffers of its own and the call returns after the
// download; otherwise they are device arrays and everything after the read-back of K is left queued on s.
static int raycast_all_run(msh_tree* t, const double* d_o, const double* d_d, const double* d_range, size_t S,
                           bool host_out, uint32_t* counts, const HitOut& out, size_t cap, size_t* K, hipStream_t s,
                           const char* fn) {
    DevBuf dt, dface, dpt, dside;
    int st = MSH_OK;
    do {
        WsOrder order(t, s);
        QueryOrder ord;
        if ((st = sort_queries(t, d_o, d_d, S, s, &ord, true)) != MSH_OK) break;
        HitTotals tot{};
        if ((st = launch_raycast_all_count(t, ord, d_range, S, &tot, s)) != MSH_OK) break;
        // the 64-bit sum is the detector: the 32-bit scan below is never run on counts it would wrap on
        if (tot.K > 0xFFFFFFFFull) {
            set_error("%s: %llu hits exceed the 32-bit offset range of one call (split the rays)", fn,
                      (unsigned long long)tot.K);
            st = MSH_EINVAL;
            break;
        }
        *K = (size_t)tot.K;
        const size_t n = std::min<size_t>((size_t)tot.K, cap);
        HitOut d = out;
        if (host_out && n) {
            if ((st = dt.reserve(n * sizeof(double))) != MSH_OK) break;
            if ((st = dface.reserve(n * sizeof(uint32_t))) != MSH_OK) break;
            if (out.pt && (st = dpt.reserve(3 * n * sizeof(double))) != MSH_OK) break;
            if (out.side && (st = dside.reserve(n * sizeof(int8_t))) != MSH_OK) break;
            d = HitOut{dt.as<double>(), dface.as<uint32_t>(), out.pt ? dpt.as<double>() : nullptr,
                       out.side ? dside.as<int8_t>() : nullptr};
        }
        if ((st = launch_raycast_all_emit(t, ord, d_range, S, tot, d, n, s)) != MSH_OK) break;
        hipError_t e = hipSuccess;
        const hipMemcpyKind kind = host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (counts) e = hipMemcpyAsync(counts, t->ws.flags.ptr, S * sizeof(uint32_t), kind, s);
        if (host_out && n) {
            if (e == hipSuccess) e = hipMemcpyAsync(out.t, d.t, n * sizeof(double), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(out.face, d.face, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && out.pt)
                e = hipMemcpyAsync(out.pt, d.pt, 3 * n * sizeof(double), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && out.side)
                e = hipMemcpyAsync(out.side, d.side, n * sizeof(int8_t), hipMemcpyDeviceToHost, s);
        }
        if (e == hipSuccess && host_out) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error("%s: %s", fn, hipGetErrorString(e));
            st = MSH_EDEVICE;
        }
    } while (0);
    if (host_out || st != MSH_OK) (void)hipStreamSynchronize(s);
    dt.release(); dface.release(); dpt.release(); dside.release();
    return st;
}

static int check_raycast_all(msh_tree* t, size_t S, const double* tt, const uint32_t* face, const double* pt,
                             const int8_t* side, size_t cap, size_t* K, const char* fn) {
    MSH_TRY(check_plain_tree(t, kTriangles, fn, "ray casting needs"));
    MSH_TRY(check_count(S, fn));
    if (!K || (cap && (!tt || !face))) {
        set_error("%s: null argument", fn);
        return MSH_EINVAL;
    }
    *K = 0;
    return MSH_OK;
}

int msh_tree_raycast_all_device(msh_tree* t, const double* d_o, const double* d_d, const double* d_range, size_t S,
                                uint32_t* d_counts, double* d_t, uint32_t* d_face, double* d_pt, int8_t* d_side,
                                size_t cap, size_t* K, void* stream) {
    const char* fn = "msh_tree_raycast_all_device";
    MSH_TRY(check_raycast_all(t, S, d_t, d_face, d_pt, d_side, cap, K, fn));
    if (S == 0) return MSH_OK;
    if (!d_o || !d_d) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    return raycast_all_run(t, d_o, d_d, d_range, S, false, d_counts, HitOut{d_t, d_face, d_pt, d_side}, cap, K,
                           pick(t, stream), fn);
}

int msh_tree_raycast_all(msh_tree* t, const double* o, const double* d, const double* range, size_t S, uint32_t* counts,
                         double* tt, uint32_t* face, double* pt, int8_t* side, size_t cap, size_t* K) {
    const char* fn = "msh_tree_raycast_all";
    MSH_TRY(check_raycast_all(t, S, tt, face, pt, side, cap, K, fn));
    if (S == 0) return MSH_OK;
    if (!o || !d) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    // the list stays on the handle's own device, as the pair lists do: the rays are uploaded whole
    hipStream_t s = t->stream;
    DevBuf dov, ddv, drv;
    int st = upload(dov, o, 3 * S, s);
    if (st == MSH_OK) st = upload(ddv, d, 3 * S, s);
    if (st == MSH_OK && range) st = upload(drv, range, 2 * S, s);
    if (st == MSH_OK)
        st = raycast_all_run(t, dov.as<double>(), ddv.as<double>(), range ? drv.as<double>() : nullptr, S, true, counts,
                             HitOut{tt, face, pt, side}, cap, K, s, fn);
    (void)hipStreamSynchronize(s);
    dov.release(); ddv.release(); drv.release();
    return st;
}

static void host_tris(const double* v, const uint32_t* f, size_t T, std::vector<TriRec>& out) {
    out.resize(T);
    for (size_t t = 0; t < T; ++t) {
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 3; ++k) out[t].v[3 * c + k] = v[3 * (size_t)f[3 * t + c] + k];
        out[t].face = (uint32_t)t;
        out[t].pad = 0;
    }
}

int msh_tree_intersections(msh_tree* t, const double* qv, size_t Pq, const uint32_t* qf, size_t Tq, uint32_t* out,
                           size_t* K) {
    MSH_TRY(check_tree(t, kTriangles, "msh_tree_intersections"));
    *K = 0;
    if (Tq == 0) return MSH_OK;
    MSH_TRY(check_count(Tq, "msh_tree_intersections"));
    MSH_TRY(check_faces(qf, Tq, Pq, "query faces"));
    std::vector<TriRec> ht;
    host_tris(qv, qf, Tq, ht);
    std::vector<uint32_t> flags;
    MSH_TRY(intersect_flags(t, &ht, Tq, 0, "intersections", flags));
    size_t k = 0;
    for (size_t i = 0; i < Tq; ++i)
        if (flags[i]) out[k++] = (uint32_t)i;
    *K = k;
    return MSH_OK;
}

// ---- intersection pair lists (tritri.hip k_tritri_all) ----
static int check_pairs_tree(const msh_tree* t, bool self, const char* fn) {
    MSH_TRY(check_tree(t, kTriangles, fn));
    if (!self && t->kind != kTriangles) {
        set_error("%s: wrong handle kind %d (a plain triangle tree is needed)", fn, t->kind);
        return MSH_EINVAL;
    }
    if (self && t->T != t->T_main) {
        set_error("%s: the tree was built with %zu extra faces (self mode needs the main mesh alone)", fn,
                  t->T - t->T_main);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

static int check_pairs_args(const uint32_t* pairs, size_t cap, size_t* K, size_t rows, const char* fn) {
    if (!K || (cap && !pairs)) {
        set_error("%s: null argument", fn);
        return MSH_EINVAL;
    }
    *K = 0;
    // rows index the packed triangle records as int on the device
    if (rows > (size_t)0x7FFFFFFFull) {
        set_error("%s: %zu query faces exceed the 31-bit index range of one call (split the query mesh)", fn, rows);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

// Count, read K back, then scan / fill / order the first min(K, cap) pairs (launch_tri_pairs_*).  host_out: pairs and
// counts are host arrays -- the pairs come through a device buffer of their own and the call returns after the
// download; otherwise they are device arrays and everything after the read-back of K is left queued on s.
static int pairs_run(msh_tree* t, const TriRec* d_q, size_t rows, int self_mode, bool packed, bool host_out,
                     uint32_t* pairs, size_t cap, uint32_t* counts, size_t* K, hipStream_t s, const char* fn) {
    DevBuf dp;
    int st = MSH_OK;
    do {
        WsOrder order(t, s);
        PairTotals tot{};
        if ((st = launch_tri_pairs_count(t, d_q, rows, self_mode, packed, &tot, s)) != MSH_OK) break;
        const uint64_t k = tot.K;
        if (tot.bad_face) {
            set_error("%s: query face index out of range (>= the number of query vertices)", fn);
            st = MSH_EINVAL;
            break;
        }
        // the 64-bit sum is the detector: the 32-bit scan below is never run on counts it would wrap on
        if (k > 0xFFFFFFFFull) {
            set_error("%s: %llu pairs exceed the 32-bit offset range of one call (split the query mesh)", fn,
                      (unsigned long long)k);
            st = MSH_EINVAL;
            break;
        }
        *K = (size_t)k;
        const size_t n = std::min<size_t>((size_t)k, cap);
        uint32_t* d_pairs = pairs;
        if (host_out && n) {
            if ((st = dp.reserve(2 * n * sizeof(uint32_t))) != MSH_OK) break;
            d_pairs = dp.as<uint32_t>();
        }
        if ((st = launch_tri_pairs_emit(t, d_q, rows, self_mode, tot, d_pairs, n, s)) != MSH_OK) break;
        hipError_t e = hipSuccess;
        const hipMemcpyKind kind = host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (counts) e = hipMemcpyAsync(counts, t->ws.flags.ptr, rows * sizeof(uint32_t), kind, s);
        if (e == hipSuccess && host_out && n)
            e = hipMemcpyAsync(pairs, d_pairs, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && host_out) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error("%s: %s", fn, hipGetErrorString(e));
            st = MSH_EDEVICE;
        }
    } while (0);
    if (host_out || st != MSH_OK) (void)hipStreamSynchronize(s);
    dp.release();
    return st;
}

int msh_tree_intersection_pairs(msh_tree* t, const double* qv, size_t Pq, const uint32_t* qf, size_t Tq, uint32_t* pairs,
                                size_t cap, uint32_t* counts, size_t* K) {
    const char* fn = "msh_tree_intersection_pairs";
    MSH_TRY(check_pairs_tree(t, false, fn));
    MSH_TRY(check_pairs_args(pairs, cap, K, Tq, fn));
    if (Tq == 0) return MSH_OK;
    if (!qv || !qf) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    MSH_TRY(check_faces(qf, Tq, Pq, "query faces"));
    hipStream_t s = t->stream;
    std::vector<TriRec> ht;
    host_tris(qv, qf, Tq, ht);
    DevBuf dq;
    int st = upload(dq, ht.data(), Tq, s);
    if (st == MSH_OK) st = pairs_run(t, dq.as<TriRec>(), Tq, 0, false, true, pairs, cap, counts, K, s, fn);
    (void)hipStreamSynchronize(s);
    dq.release();
    return st;
}

int msh_tree_intersection_pairs_device(msh_tree* t, const double* d_qv, size_t Pq, const uint32_t* d_qf, size_t Tq,
                                       uint32_t* d_pairs, size_t cap, uint32_t* d_counts, size_t* K, void* stream) {
    const char* fn = "msh_tree_intersection_pairs_device";
    MSH_TRY(check_pairs_tree(t, false, fn));
    MSH_TRY(check_pairs_args(d_pairs, cap, K, Tq, fn));
    if (Tq == 0) return MSH_OK;
    if (!d_qv || !d_qf) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    hipStream_t s = pick(t, stream);
    {
        // the packed triangles live in the workspace too: order them after the handle's previous call (pairs_run's
        // own WsOrder then waits for an event this stream has already passed)
        WsOrder order(t, s);
        MSH_TRY(pack_query_tris(t, d_qv, Pq, d_qf, Tq, s));
    }
    return pairs_run(t, t->ws.q.as<TriRec>(), Tq, 0, true, false, d_pairs, cap, d_counts, K, s, fn);
}

int msh_tree_self_intersection_pairs(msh_tree* t, uint32_t* pairs, size_t cap, uint32_t* counts, size_t* K) {
    const char* fn = "msh_tree_self_intersection_pairs";
    MSH_TRY(check_pairs_tree(t, true, fn));
    MSH_TRY(check_pairs_args(pairs, cap, K, t->T, fn));
    return pairs_run(t, static_cast<const TriRec*>(t->d_leaves), t->T, 1, false, true, pairs, cap, counts, K, t->stream,
                     fn);
}

int msh_tree_self_intersection_pairs_device(msh_tree* t, uint32_t* d_pairs, size_t cap, uint32_t* d_counts, size_t* K,
                                            void* stream) {
    const char* fn = "msh_tree_self_intersection_pairs_device";
    MSH_TRY(check_pairs_tree(t, true, fn));
    MSH_TRY(check_pairs_args(d_pairs, cap, K, t->T, fn));
    return pairs_run(t, static_cast<const TriRec*>(t->d_leaves), t->T, 1, false, false, d_pairs, cap, d_counts, K,
                     pick(t, stream), fn);
}

int msh_ntree_nearest(msh_tree* t, const double* q, const double* n, size_t S, uint32_t* face, double* pt) {
    MSH_TRY(check_tree(t, kNormals, "msh_ntree_nearest"));
    MSH_TRY(check_count(S, "msh_ntree_nearest"));
    if (S == 0) return MSH_OK;
    if (!q || !n || !face || !pt) { set_error("msh_ntree_nearest: null argument"); return MSH_EINVAL; }
    HostCols c;  // chunked like msh_tree_nearest
    const auto cq = c.in(q, 3), cn = c.in(n, 3);
    const auto cface = c.out(face, 1);
    const auto cpt = c.out(pt, 3);
    return host_call(t, S, c, kNoCut, [&](msh_tree* h, size_t rows, const Slabs& d) {
        hipStream_t s = h->stream;
        WsOrder order(h, s);
        QueryOrder ord;
        MSH_TRY(sort_queries(h, d[cq], d[cn], rows, s, &ord));
        return launch_nnearest(h, ord, rows, SlotOut{d[cface], nullptr, d[cpt], nullptr, nullptr}, s);
    });
}

int msh_ntree_selfintersects(msh_tree* t, int64_t* count) {
    MSH_TRY(check_tree(t, kNormals, "msh_ntree_selfintersects"));
    *count = 0;
    std::vector<uint32_t> flags;
    MSH_TRY(intersect_flags(t, nullptr, t->T, 1, "selfintersects", flags));
    int64_t c = 0;
    for (uint32_t x : flags) c += x ? 1 : 0;
    *count = c;
    return MSH_OK;
}

int msh_visibility_device(msh_tree* t, const double* d_cams, size_t C, const double* d_normals, const double* d_sensors,
                          double min_dist, size_t v_begin, size_t v_count, uint32_t* d_vis, double* d_ndc, void* stream) {
    MSH_TRY(check_tree(t, kTriangles, "msh_visibility_device"));
    if (v_begin > t->P || v_count > t->P - v_begin) {
        set_error("msh_visibility_device: vertex range [%zu, %zu) outside the %zu main-mesh vertices", v_begin,
                  v_begin + v_count, t->P);
        return MSH_EINVAL;
    }
    if (C * v_count == 0) return MSH_OK;
    hipStream_t s = pick(t, stream);
    WsOrder order(t, s);
    return launch_visibility(t, d_cams, C, d_normals, d_sensors, min_dist, v_begin, v_count, d_vis, d_ndc, s);
}

// cameras [0, C) of one handle: its cameras, normals and sensors are uploaded once, outside the pipeline; out: the
// (C, P) output columns of those cameras
static int visibility_host(msh_tree* t, const double* cams, size_t C, const double* normals, const double* sensors,
                           double min_dist, const HostCols& out, Col<uint32_t> cvis, Col<double> cndc) {
    MSH_TRY(use_device(t->device));
    const size_t P = t->P;
    hipStream_t s = t->stream;
    DevBuf dc, dn, ds;
    int st = MSH_OK;
    do {
        if ((st = upload(dc, cams, 3 * C, s)) != MSH_OK) break;
        if (normals && (st = upload(dn, normals, 3 * P, s)) != MSH_OK) break;
        if (sensors && (st = upload(ds, sensors, 9 * C, s)) != MSH_OK) break;
        const std::vector<size_t> plan = {std::max<size_t>(1, ((size_t)16 << 20) / P)};  // ~16M rays a chunk
        st = pipelined(t, C, out, [&](size_t c0, size_t nc, const Slabs& d) {
            return msh_visibility_device(t, dc.as<double>() + 3 * c0, nc, normals ? dn.as<double>() : nullptr,
                                         sensors ? ds.as<double>() + 9 * c0 : nullptr, min_dist, 0, P, d[cvis], d[cndc], s);
        }, &plan);
    } while (0);
    (void)hipStreamSynchronize(s);
    return st;
}

// Host arrays: the cameras, normals and sensors are uploaded once; the (C, P) outputs come back through the pinned
// pipeline a few cameras at a time (hostpipe.cpp pipelined(): rows = cameras), so the downloads of earlier cameras
// (C5: 30 MB per camera, 1.92 GB in all) overlap the rays of later ones, and land straight in page-locked pool arrays
// when the caller's arrays are carved from it.  With replicas (msh_set_devices) each device casts a camera range.
int msh_visibility(msh_tree* t, const double* cams, size_t C, const double* normals, const double* sensors,
                   double min_dist, uint32_t* vis, double* ndc) {
    MSH_TRY(check_tree(t, kTriangles, "msh_visibility"));
    const size_t P = t->P;
    if (C * P == 0) return MSH_OK;
    if (!cams || !vis || !ndc) { set_error("msh_visibility: null argument"); return MSH_EINVAL; }
    HostCols c;  // rows = cameras
    const auto cvis = c.out(vis, P);
    const auto cndc = c.out(ndc, P);
    return fan_out(t, C, c.row(), [&](msh_tree* h, size_t c0, size_t nc) {
        return visibility_host(h, cams + 3 * c0, nc, normals, sensors ? sensors + 9 * c0 : nullptr, min_dist,
                               c.shard(c0), cvis, cndc);
    });
}

int msh_points_nearest(msh_tree* t, const double* q, size_t S, uint32_t* idx, double* dist) {
    MSH_TRY(check_tree(t, kPoints, "msh_points_nearest"));
    MSH_TRY(check_count(S, "msh_points_nearest"));
    if (S == 0) return MSH_OK;
    if (!q || !idx || !dist) { set_error("msh_points_nearest: null argument"); return MSH_EINVAL; }
    HostCols c;  // chunked like msh_tree_nearest
    const auto cq = c.in(q, 3);
    const auto cidx = c.out(idx, 1);
    const auto cdist = c.out(dist, 1);
    return host_call(t, S, c, kNoCut, [&](msh_tree* h, size_t rows, const Slabs& d) {
        hipStream_t s = h->stream;
        WsOrder order(h, s);
        QueryOrder ord;
        MSH_TRY(sort_queries(h, d[cq], nullptr, rows, s, &ord));
        return launch_points_nearest(h, ord, rows, SlotOut{d[cidx], nullptr, nullptr, d[cdist], nullptr}, s);
    });
}

// ---- K-nearest and radius-capped queries (kbest.hip) ----
static const char* const kKbestNeeds = "K-nearest queries need";
static int check_kbest_args(uint32_t K, double r_max, const char* fn) {
    if (K < 1 || K > MSH_KNEAREST_MAX) {
        set_error("%s: K must be in 1..%d, got %u", fn, MSH_KNEAREST_MAX, K);
        return MSH_EINVAL;
    }
    if (!(r_max >= 0.0)) {
        set_error("%s: r_max must be >= 0 (+inf: no cap), got %g", fn, r_max);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

// one launch over d_q in the closest-point path's slot order, from the root (no entry cut)
static int kbest_run(msh_tree* t, const double* d_q, size_t S, uint32_t K, double r_max, const KbOut& o, hipStream_t s) {
    const bool rebuild = t->kind == kTriangles && (o.pt || o.part);  // points and parts go through the face's leaf
    if (rebuild) MSH_TRY(ensure_face_leaf(t, s));
    WsOrder order(t, s);
    QueryOrder ord;
    MSH_TRY(sort_queries(t, d_q, nullptr, S, s, &ord, true));
    return launch_kbest(t, ord, S, K, r_max, o, rebuild ? t->d_face_leaf : nullptr, s);
}

int msh_points_knearest_device(msh_tree* t, const double* d_q, size_t S, uint32_t K, double r_max, uint32_t* d_idx,
                               double* d_dist, uint32_t* d_count, void* stream) {
    MSH_TRY(check_kbest_args(K, r_max, "msh_points_knearest_device"));  // before the handle, as winding's beta
    MSH_TRY(check_plain_tree(t, kPoints, "msh_points_knearest_device", kKbestNeeds));
    MSH_TRY(check_count(S, "msh_points_knearest_device"));
    if (S == 0) return MSH_OK;
    if (!d_q || !d_idx || !d_dist) { set_error("msh_points_knearest_device: null argument"); return MSH_EINVAL; }
    return kbest_run(t, d_q, S, K, r_max, KbOut{d_idx, d_dist, nullptr, nullptr, d_count}, pick(t, stream));
}

int msh_points_knearest(msh_tree* t, const double* q, size_t S, uint32_t K, double r_max, uint32_t* idx, double* dist,
                        uint32_t* count) {
    MSH_TRY(check_kbest_args(K, r_max, "msh_points_knearest"));
    MSH_TRY(check_plain_tree(t, kPoints, "msh_points_knearest", kKbestNeeds));
    MSH_TRY(check_count(S, "msh_points_knearest"));
    if (S == 0) return MSH_OK;
    if (!q || !idx || !dist) { set_error("msh_points_knearest: null argument"); return MSH_EINVAL; }
    HostCols c;  // count keeps its slab when the caller wants none (nothing is downloaded from it)
    const auto cq = c.in(q, 3);
    const auto cidx = c.out(idx, K);
    const auto cdist = c.out(dist, K);
    const auto ccnt = c.out(count, 1);
    return host_call(t, S, c, kNoCut, [&](msh_tree* h, size_t n, const Slabs& d) {
        return kbest_run(h, d[cq], n, K, r_max, KbOut{d[cidx], d[cdist], nullptr, nullptr, count ? d[ccnt] : nullptr},
                         h->stream);
    });
}

int msh_tree_knearest_device(msh_tree* t, const double* d_q, size_t S, uint32_t K, double r_max, uint32_t* d_face,
                             double* d_dist, double* d_pt, uint32_t* d_part, uint32_t* d_count, void* stream) {
    MSH_TRY(check_kbest_args(K, r_max, "msh_tree_knearest_device"));
    MSH_TRY(check_plain_tree(t, kTriangles, "msh_tree_knearest_device", kKbestNeeds));
    MSH_TRY(check_count(S, "msh_tree_knearest_device"));
    if (S == 0) return MSH_OK;
    if (!d_q || !d_face || !d_dist) { set_error("msh_tree_knearest_device: null argument"); return MSH_EINVAL; }
    return kbest_run(t, d_q, S, K, r_max, KbOut{d_face, d_dist, d_pt, d_part, d_count}, pick(t, stream));
}

int msh_tree_knearest(msh_tree* t, const double* q, size_t S, uint32_t K, double r_max, uint32_t* face, double* dist,
                      double* pt, uint32_t* part, uint32_t* count) {
    MSH_TRY(check_kbest_args(K, r_max, "msh_tree_knearest"));
    MSH_TRY(check_plain_tree(t, kTriangles, "msh_tree_knearest", kKbestNeeds));
    MSH_TRY(check_count(S, "msh_tree_knearest"));
    if (S == 0) return MSH_OK;
    if (!q || !face || !dist) { set_error("msh_tree_knearest: null argument"); return MSH_EINVAL; }
    HostCols c;  // only the columns the caller asked for take slab space: at K = 64 a row's points are 1.5 KB
    const auto cq = c.in(q, 3);
    const auto cface = c.out(face, K);
    const auto cdist = c.out(dist, K);
    const auto cpt = c.out(pt, pt ? 3 * (size_t)K : 0);
    const auto cpart = c.out(part, part ? K : 0);
    const auto ccnt = c.out(count, count ? 1 : 0);
    return host_call(t, S, c, kNoCut, [&](msh_tree* h, size_t n, const Slabs& d) {
        return kbest_run(h, d[cq], n, K, r_max,
                         KbOut{d[cface], d[cdist], pt ? d[cpt] : nullptr, part ? d[cpart] : nullptr,
                               count ? d[ccnt] : nullptr},
                         h->stream);
    });
}

int msh_tree_knearest_stats(msh_tree* t, const double* d_q, size_t S, uint32_t K, double r_max, uint64_t counts[4]) {
    MSH_TRY(check_kbest_args(K, r_max, "msh_tree_knearest_stats"));
    if (!t) { set_error("msh_tree_knearest_stats: null tree handle"); return MSH_EINVAL; }
    MSH_TRY(check_plain_tree(t, t->kind == kPoints ? kPoints : kTriangles, "msh_tree_knearest_stats", kKbestNeeds));
    MSH_TRY(check_count(S, "msh_tree_knearest_stats"));
    if (!counts) { set_error("msh_tree_knearest_stats: null argument"); return MSH_EINVAL; }
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    if (S == 0) return MSH_OK;
    if (!d_q) { set_error("msh_tree_knearest_stats: null argument"); return MSH_EINVAL; }
    unsigned long long h[4] = {0, 0, 0, 0};
    MSH_TRY(stats_call(t, d_q, nullptr, S, 4, h, 4, [&](const QueryOrder& ord, unsigned long long* d, hipStream_t s) {
        return launch_kbest_stats(t, ord, S, K, r_max, d, s);
    }));
    for (int k = 0; k < 4; ++k) counts[k] = h[k];
    return MSH_OK;
}

// ---- all primitives within a radius: counts and sorted CSR lists (within.hip) ----
static const char* const kWithinNeeds = "radius queries need";
// the scalar radius, checked before the handle as check_kbest_args does (a per-row radius that is negative or NaN is no
// error: that row is empty)
static int check_within_radius(double r_max, const double* r_rows, const char* fn) {
    if (!r_rows && !(r_max >= 0.0)) {
        set_error("%s: r_max must be >= 0 (+inf: every primitive), got %g", fn, r_max);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

static int within_count_run(msh_tree* t, const double* d_q, double r_max, const double* d_r, size_t S,
                            uint32_t* d_count, hipStream_t s) {
    WsOrder order(t, s);
    QueryOrder ord;
    MSH_TRY(sort_queries(t, d_q, nullptr, S, s, &ord, true));
    return launch_within_count(t, ord, r_max, d_r, S, d_count, s);
}

static int within_count_device(msh_tree* t, int kind, const double* d_q, size_t S, double r_max, const double* d_r,
                               uint32_t* d_count, void* stream, const char* fn) {
    MSH_TRY(check_within_radius(r_max, d_r, fn));
    MSH_TRY(check_plain_tree(t, kind, fn, kWithinNeeds));
    MSH_TRY(check_count(S, fn));
    if (S == 0) return MSH_OK;
    if (!d_q || !d_count) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    return within_count_run(t, d_q, r_max, d_r, S, d_count, pick(t, stream));
}

static int within_count_host(msh_tree* t, int kind, const double* q, size_t S, double r_max, const double* r_rows,
                             uint32_t* count, const char* fn) {
    MSH_TRY(check_within_radius(r_max, r_rows, fn));
    MSH_TRY(check_plain_tree(t, kind, fn, kWithinNeeds));
    MSH_TRY(check_count(S, fn));
    if (S == 0) return MSH_OK;
    if (!q || !count) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    HostCols c;
    const auto cq = c.in(q, 3);
    const auto cr = c.in(r_rows, r_rows ? 1 : 0);
    const auto ccount = c.out(count, 1);
    return host_call(t, S, c, kNoCut, [&](msh_tree* h, size_t n, const Slabs& d) {
        return within_count_run(h, d[cq], r_max, r_rows ? d[cr] : nullptr, n, d[ccount], h->stream);
    });
}

int msh_points_within_count(msh_tree* t, const double* q, size_t S, double r_max, const double* r_rows,
                            uint32_t* count) {
    return within_count_host(t, kPoints, q, S, r_max, r_rows, count, "msh_points_within_count");
}
int msh_points_within_count_device(msh_tree* t, const double* d_q, size_t S, double r_max, const double* d_r_rows,
                                   uint32_t* d_count, void* stream) {
    return within_count_device(t, kPoints, d_q, S, r_max, d_r_rows, d_count, stream, "msh_points_within_count_device");
}
int msh_tree_within_count(msh_tree* t, const double* q, size_t S, double r_max, const double* r_rows, uint32_t* count) {
    return within_count_host(t, kTriangles, q, S, r_max, r_rows, count, "msh_tree_within_count");
}
int msh_tree_within_count_device(msh_tree* t, const double* d_q, size_t S, double r_max, const double* d_r_rows,
                                 uint32_t* d_count, void* stream) {
    return within_count_device(t, kTriangles, d_q, S, r_max, d_r_rows, d_count, stream, "msh_tree_within_count_device");
}

// raycast_all_run's shape: count, read K back, then scan / fill / order / emit the first min(K, cap) entries.  host_out:
// the outputs are host arrays -- the list comes through device buffers of its own and the call returns after the
// download; otherwise they are device arrays and everything after the read-back of K is left queued on s.
static int within_run(msh_tree* t, const double* d_q, double r_max, const double* d_r, size_t S, bool host_out,
                      uint32_t* counts, const WithinOut& out, size_t cap, size_t* K, hipStream_t s, const char* fn) {
    DevBuf did, ddist, dpt, dpart;
    int st = MSH_OK;
    do {
        WsOrder order(t, s);
        QueryOrder ord;
        if ((st = sort_queries(t, d_q, nullptr, S, s, &ord, true)) != MSH_OK) break;
        HitTotals tot{};
        if ((st = launch_within_all_count(t, ord, r_max, d_r, S, &tot, s)) != MSH_OK) break;
        // the 64-bit sum is the detector: the 32-bit scan below is never run on counts it would wrap on
        if (tot.K > 0xFFFFFFFFull) {
            set_error("%s: %llu entries exceed the 32-bit offset range of one call (split the rows)", fn,
                      (unsigned long long)tot.K);
            st = MSH_EINVAL;
            break;
        }
        *K = (size_t)tot.K;
        const size_t n = std::min<size_t>((size_t)tot.K, cap);
        WithinOut d = out;
        if (host_out && n) {
            if ((st = did.reserve(n * sizeof(uint32_t))) != MSH_OK) break;
            if ((st = ddist.reserve(n * sizeof(double))) != MSH_OK) break;
            if (out.pt && (st = dpt.reserve(3 * n * sizeof(double))) != MSH_OK) break;
            if (out.part && (st = dpart.reserve(n * sizeof(uint32_t))) != MSH_OK) break;
            d = WithinOut{did.as<uint32_t>(), ddist.as<double>(), out.pt ? dpt.as<double>() : nullptr,
                          out.part ? dpart.as<uint32_t>() : nullptr};
        }
        if ((st = launch_within_emit(t, ord, r_max, d_r, S, tot, d, n, s)) != MSH_OK) break;
        hipError_t e = hipSuccess;
        const hipMemcpyKind kind = host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (counts) e = hipMemcpyAsync(counts, t->ws.flags.ptr, S * sizeof(uint32_t), kind, s);
        if (host_out && n) {
            if (e == hipSuccess) e = hipMemcpyAsync(out.id, d.id, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(out.dist, d.dist, n * sizeof(double), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && out.pt)
                e = hipMemcpyAsync(out.pt, d.pt, 3 * n * sizeof(double), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && out.part)
                e = hipMemcpyAsync(out.part, d.part, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        }
        if (e == hipSuccess && host_out) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error("%s: %s", fn, hipGetErrorString(e));
            st = MSH_EDEVICE;
        }
    } while (0);
    if (host_out || st != MSH_OK) (void)hipStreamSynchronize(s);
    did.release(); ddist.release(); dpt.release(); dpart.release();
    return st;
}

static int check_within(msh_tree* t, int kind, double r_max, const double* r_rows, size_t S, const uint32_t* id,
                        const double* dist, size_t cap, size_t* K, const char* fn) {
    MSH_TRY(check_within_radius(r_max, r_rows, fn));
    MSH_TRY(check_plain_tree(t, kind, fn, kWithinNeeds));
    MSH_TRY(check_count(S, fn));
    if (!K || (cap && (!id || !dist))) {
        set_error("%s: null argument", fn);
        return MSH_EINVAL;
    }
    *K = 0;
    return MSH_OK;
}

static int within_device(msh_tree* t, int kind, const double* d_q, size_t S, double r_max, const double* d_r,
                         uint32_t* d_counts, const WithinOut& o, size_t cap, size_t* K, void* stream, const char* fn) {
    MSH_TRY(check_within(t, kind, r_max, d_r, S, o.id, o.dist, cap, K, fn));
    if (S == 0) return MSH_OK;
    if (!d_q) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    return within_run(t, d_q, r_max, d_r, S, false, d_counts, o, cap, K, pick(t, stream), fn);
}

static int within_host(msh_tree* t, int kind, const double* q, size_t S, double r_max, const double* r_rows,
                       uint32_t* counts, const WithinOut& o, size_t cap, size_t* K, const char* fn) {
    MSH_TRY(check_within(t, kind, r_max, r_rows, S, o.id, o.dist, cap, K, fn));
    if (S == 0) return MSH_OK;
    if (!q) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    // the list stays on the handle's own device, as the all-hits lists do: the rows are uploaded whole
    hipStream_t s = t->stream;
    DevBuf dq, dr;
    int st = upload(dq, q, 3 * S, s);
    if (st == MSH_OK && r_rows) st = upload(dr, r_rows, S, s);
    if (st == MSH_OK)
        st = within_run(t, dq.as<double>(), r_max, r_rows ? dr.as<double>() : nullptr, S, true, counts, o, cap, K, s, fn);
    (void)hipStreamSynchronize(s);
    dq.release(); dr.release();
    return st;
}

int msh_points_within(msh_tree* t, const double* q, size_t S, double r_max, const double* r_rows, uint32_t* counts,
                      uint32_t* idx, double* dist, size_t cap, size_t* K) {
    return within_host(t, kPoints, q, S, r_max, r_rows, counts, WithinOut{idx, dist, nullptr, nullptr}, cap, K,
                       "msh_points_within");
}
int msh_points_within_device(msh_tree* t, const double* d_q, size_t S, double r_max, const double* d_r_rows,
                             uint32_t* d_counts, uint32_t* d_idx, double* d_dist, size_t cap, size_t* K, void* stream) {
    return within_device(t, kPoints, d_q, S, r_max, d_r_rows, d_counts, WithinOut{d_idx, d_dist, nullptr, nullptr}, cap,
                         K, stream, "msh_points_within_device");
}
int msh_tree_within(msh_tree* t, const double* q, size_t S, double r_max, const double* r_rows, uint32_t* counts,
                    uint32_t* face, double* dist, double* pt, uint32_t* part, size_t cap, size_t* K) {
    return within_host(t, kTriangles, q, S, r_max, r_rows, counts, WithinOut{face, dist, pt, part}, cap, K,
                       "msh_tree_within");
}
int msh_tree_within_device(msh_tree* t, const double* d_q, size_t S, double r_max, const double* d_r_rows,
                           uint32_t* d_counts, uint32_t* d_face, double* d_dist, double* d_pt, uint32_t* d_part,
                           size_t cap, size_t* K, void* stream) {
    return within_device(t, kTriangles, d_q, S, r_max, d_r_rows, d_counts, WithinOut{d_face, d_dist, d_pt, d_part}, cap,
                         K, stream, "msh_tree_within_device");
}

int msh_tree_within_stats(msh_tree* t, const double* d_q, size_t S, double r_max, const double* d_r_rows,
                          uint64_t counts[4]) {
    const char* fn = "msh_tree_within_stats";
    MSH_TRY(check_within_radius(r_max, d_r_rows, fn));
    if (!t) { set_error("%s: null tree handle", fn); return MSH_EINVAL; }
    MSH_TRY(check_plain_tree(t, t->kind == kPoints ? kPoints : kTriangles, fn, kWithinNeeds));
    MSH_TRY(check_count(S, fn));
    if (!counts) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    if (S == 0) return MSH_OK;
    if (!d_q) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    unsigned long long h[4] = {0, 0, 0, 0};
    MSH_TRY(stats_call(t, d_q, nullptr, S, 4, h, 4, [&](const QueryOrder& ord, unsigned long long* d, hipStream_t s) {
        return launch_within_stats(t, ord, r_max, d_r_rows, S, d, s);
    }));
    for (int k = 0; k < 4; ++k) counts[k] = h[k];
    return MSH_OK;
}

// ---- mesh geometry ----
int msh_vertex_normals_device(const double* d_v, size_t P, const uint32_t* d_f, size_t T, double* d_vn, void* stream) {
    if (P && (!d_v || !d_vn)) { set_error("msh_vertex_normals_device: null argument"); return MSH_EINVAL; }
    if (T && !d_f) { set_error("msh_vertex_normals_device: null faces"); return MSH_EINVAL; }
    if (P > 0xFFFFFFFFull) { set_error("msh_vertex_normals_device: too many vertices"); return MSH_EINVAL; }
    int dev = 0;
    MSH_TRY(current_device(&dev));
    MSH_TRY(use_device(dev));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Workspace ws;
    int st = ws.flags.reserve(sizeof(uint32_t));
    uint32_t h_err = 0;
    if (st == MSH_OK && hipMemsetAsync(ws.flags.ptr, 0, sizeof(uint32_t), s) != hipSuccess) st = MSH_EDEVICE;
    if (st == MSH_OK) st = vertex_normals(d_v, P, d_f, T, d_vn, ws, s, ws.flags.as<uint32_t>());
    if (st == MSH_OK && hipMemcpyAsync(&h_err, ws.flags.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess)
        st = MSH_EDEVICE;
    hipError_t e = hipStreamSynchronize(s);  // the scratch below is released on return
    ws.release();
    if (st == MSH_OK && e != hipSuccess) {
        set_error("vertex normals: %s", hipGetErrorString(e));
        st = MSH_EDEVICE;
    }
    if (st == MSH_OK && h_err) {
        set_error("msh_vertex_normals_device: face index out of range (>= %zu vertices)", P);
        st = MSH_EINVAL;
    }
    return st;
}

int msh_vertex_normals(const double* v, size_t P, const uint32_t* f, size_t T, double* vn) {
    if (P && (!v || !vn)) { set_error("msh_vertex_normals: null argument"); return MSH_EINVAL; }
    MSH_TRY(check_faces(f, T, P, "msh_vertex_normals"));
    if (P == 0) return MSH_OK;
    int dev = 0;
    MSH_TRY(current_device(&dev));
    MSH_TRY(use_device(dev));
    hipStream_t s = nullptr;
    MSH_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    DevBuf dv, df, dn;
    int st = MSH_OK;
    do {
        if ((st = upload(dv, v, 3 * P, s)) != MSH_OK) break;
        if ((st = upload(df, f, 3 * T, s)) != MSH_OK) break;
        if ((st = dn.reserve(3 * P * sizeof(double))) != MSH_OK) break;
        if ((st = msh_vertex_normals_device(dv.as<double>(), P, df.as<uint32_t>(), T, dn.as<double>(), s)) != MSH_OK)
            break;
        hipError_t e;
        if ((e = hipMemcpyAsync(vn, dn.ptr, 3 * P * sizeof(double), hipMemcpyDeviceToHost, s)) != hipSuccess ||
            (e = hipStreamSynchronize(s)) != hipSuccess) {
            set_error("vertex normals: %s", hipGetErrorString(e));
            st = MSH_EDEVICE;
        }
    } while (0);
    (void)hipStreamSynchronize(s);
    dv.release(); df.release(); dn.release();
    (void)hipStreamDestroy(s);
    return st;
}

// ---- device pools (msh_timing_* are devmem.cpp's, msh_host_* hostpipe.cpp's) ----
int msh_device_pool_trim(void) {
    ws_pool_trim();
    stage_pool_trim();
    dcache_trim();  // last: the workspaces and slabs above were returned to it
    return MSH_OK;
}

int msh_device_pool_bytes(uint64_t* workspace, uint64_t* staging, uint64_t* cached) {
    if (workspace) *workspace = ws_pool_bytes();
    if (staging) *staging = stage_pool_device_bytes();
    if (cached) *cached = dcache_bytes();
    return MSH_OK;
}

// ---- batched trees (C4: B meshes sharing one topology) ----
int msh_batch_build(const double* v, size_t B, size_t P, const uint32_t* f, size_t T, msh_tree** out) {
    if (!out) { set_error("msh_batch_build: null output"); return MSH_EINVAL; }
    *out = nullptr;
    if (!v || !f || B == 0 || P == 0 || T < 2) {
        set_error("msh_batch_build: need B >= 1 meshes of P >= 1 vertices and T >= 2 faces (got B=%zu P=%zu T=%zu)",
                  B, P, T);
        return MSH_EINVAL;
    }
    if (B * T > (size_t)0x7FFFFFFF) {
        set_error("msh_batch_build: %zu x %zu faces exceed the 31-bit leaf index range", B, T);
        return MSH_EINVAL;
    }
    MSH_TRY(check_faces(f, T, P, "msh_batch_build"));
    msh_tree* t = nullptr;
    MSH_TRY(new_tree(kTriangles, &t));
    t->B = B;
    t->P = P;
    t->T = T;
    t->T_main = T;
    hipStream_t s = t->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DevBuf dF, dLo, dHi, dOrder;
    int st = MSH_OK;
    do {
        hipError_t e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        if (e == hipSuccess) e = dmalloc(&t->d_v, B * P * 3 * sizeof(double));
        if (e == hipSuccess) e = dmalloc(&t->d_nodes, B * (T - 1) * sizeof(BNode));
        if (e == hipSuccess) e = dmalloc(&t->d_leaves, B * T * sizeof(TriRec));
        if (e != hipSuccess) { set_error("msh_batch_build: %s", hipGetErrorString(e)); st = MSH_ENOMEM; break; }
        // the vertices (C4: 496 MB) through the pinned staging pipeline, a chunk of meshes at a time (one pageable
        // hipMemcpy of them ran well below the host link's rate)
        // chunks of ~32 MB, so the host's copies into the pinned slabs overlap the uploads
        HostCols va;  // rows = meshes
        const auto cv = va.in(v, P * 3);
        const std::vector<size_t> vplan = {std::max<size_t>(1, ((size_t)32 << 20) / (P * 3 * sizeof(double)))};
        st = pipelined(t, B, va, [&](size_t m0, size_t nm, const Slabs& d) {
            MSH_HIP(hipMemcpyAsync(t->d_v + m0 * P * 3, d[cv], nm * P * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
            return MSH_OK;
        }, &vplan);
        if (st != MSH_OK) break;
        if ((st = upload(dF, f, 3 * T, s)) != MSH_OK) break;
        if ((st = dLo.reserve(3 * B * T * sizeof(double))) != MSH_OK) break;
        if ((st = dHi.reserve(3 * B * T * sizeof(double))) != MSH_OK) break;
        if ((st = dOrder.reserve(B * T * sizeof(uint32_t))) != MSH_OK) break;
        (void)hipEventRecord(e0, s);
        if ((st = tri_bounds_batch(t->d_v, P, dF.as<uint32_t>(), B, T, dLo.as<double>(), dHi.as<double>(), s)) != MSH_OK)
            break;
        if ((st = build_lbvh_batch(t, dLo.as<double>(), dHi.as<double>(), T, dOrder.as<uint32_t>())) != MSH_OK) break;
        if ((st = pack_tri_leaves_batch(t->d_v, P, dF.as<uint32_t>(), dOrder.as<uint32_t>(), B, T,
                                        static_cast<TriRec*>(t->d_leaves), s)) != MSH_OK)
            break;
        if ((st = build_obb(t, true, true)) != MSH_OK) break;
        (void)hipEventRecord(e1, s);
        if (t->ws_done) (void)hipEventRecord(t->ws_done, s);  // *_device calls on other streams wait for the build
    } while (0);
    if (st == MSH_OK) {
        // The tail of the build (leaf packing, oriented boxes) is still running on the handle's stream: return now, so
        // the caller's next call overlaps it (C4 through numpy: the queries' uploads run on the copy stream while the
        // boxes are built; the query kernels follow the build on the handle's stream).  Its temporaries and workspace
        // are freed by finish_pending once it has passed.
        t->pending = true;
        t->pend_e0 = e0;
        t->pend_done = e1;
        e0 = e1 = nullptr;
        for (DevBuf* b : {&dF, &dLo, &dHi, &dOrder}) {
            t->pend_free.push_back(b->ptr);
            b->ptr = nullptr;
            b->bytes = 0;
        }
        t->pend_ws = std::move(t->ws);
        ws_pool_take(t->device, t->ws);  // a freed tree's query workspace, if one is idle
    } else {
        (void)hipStreamSynchronize(s);
        dF.release(); dLo.release(); dHi.release(); dOrder.release();
        t->ws.release();
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return return_tree(t, st, out);
}

// meshes [mesh0, mesh0 + nmesh) of a batched tree; d_q and the outputs hold those meshes' rows only
static int batch_query_range(msh_tree* t, const double* d_q, size_t S, size_t mesh0, size_t nmesh, const SlotOut& o,
                             hipStream_t s) {
    const size_t n = nmesh * S;
    if (n == 0) return MSH_OK;
    WsOrder order(t, s);
    QueryOrder ord;
    MSH_TRY(sort_batch_queries(t, d_q, n, S, s, &ord, mesh0));
    return launch_nearest_batch(t, ord, n, S, o, s, mesh0);
}

static int batch_query(msh_tree* t, const double* d_q, size_t S, const SlotOut& o, void* stream, const char* fn) {
    MSH_TRY(check_batch(t, fn));
    const size_t n = t->B * S;
    if (n == 0) return MSH_OK;
    MSH_TRY(check_count(n, fn));
    // a build still running is waited for on the device (ws_done); its temporaries go once it has passed
    if (t->pending) {
        const hipError_t q = hipEventQuery(t->pend_done);
        // done, or failed: finish_pending reports a failed build's error instead of answering from it
        if (q != hipErrorNotReady) {
            (void)hipGetLastError();
            MSH_TRY(finish_pending(t));
        }
    }
    return batch_query_range(t, d_q, S, 0, t->B, o, pick(t, stream));
}

int msh_batch_nearest_device(msh_tree* t, const double* d_q, size_t S, uint32_t* d_face, uint32_t* d_part, double* d_pt,
                             void* stream) {
    return batch_query(t, d_q, S, SlotOut{d_face, d_part, d_pt, nullptr, nullptr}, stream, "msh_batch_nearest_device");
}

int msh_batch_nearest_bary_device(msh_tree* t, const double* d_q, size_t S, uint32_t* d_face, double* d_pt, double* d_w,
                                  void* stream) {
    if (!d_w) { set_error("msh_batch_nearest_bary_device: null weights"); return MSH_EINVAL; }
    return batch_query(t, d_q, S, SlotOut{d_face, nullptr, d_pt, nullptr, d_w}, stream, "msh_batch_nearest_bary_device");
}

// Host arrays of a batched tree, pipelined over meshes (hostpipe.cpp pipelined(): a chunk is a range of whole meshes, so
// its queries sort and run as the meshes' own launch): uploads, kernels and downloads of consecutive chunks overlap,
// and results go straight into page-locked pool arrays (msh_host_alloc) when the caller's arrays are carved from it.
// C4 (4096 meshes x 10k queries): one pageable upload of 983 MB and downloads of 1.3 GB had made the call 4x slower
// than its host-link bound.
static int batch_host(msh_tree* t, const double* q, size_t S, uint32_t* face, uint32_t* part, double* pt, double* w,
                      const char* fn) {
    MSH_TRY(check_batch(t, fn));
    const size_t n = t->B * S;
    if (n == 0) return MSH_OK;
    MSH_TRY(check_count(n, fn));
    if (!q || !face || !pt) { set_error("%s: null argument", fn); return MSH_EINVAL; }
    if (w) part = nullptr;
    // rows = meshes: q (24 S B in) | face (4 S out) | [part (4 S out)] | point (24 S out) | [weights (24 S out)]
    HostCols c;
    const auto cq = c.in(q, 3 * S);
    const auto cface = c.out(face, S);
    const Col<uint32_t> cpart = part ? c.out(part, S) : Col<uint32_t>{};  // an undeclared column reads as nullptr
    const auto cpt = c.out(pt, 3 * S);
    const Col<double> cw = w ? c.out(w, 3 * S) : Col<double>{};
    // chunks of ~2M then ~6M queries (whole meshes)
    const std::vector<size_t> plan = {std::max<size_t>(1, ((size_t)2 << 20) / S), std::max<size_t>(1, ((size_t)6 << 20) / S)};
    // the uploads of the first chunks overlap the tail of an asynchronous build; its kernels follow it on t->stream
    const int st = pipelined(t, t->B, c, [&](size_t m0, size_t nm, const Slabs& d) {
        return batch_query_range(t, d[cq], S, m0, nm, SlotOut{d[cface], d[cpart], d[cpt], nullptr, d[cw]}, t->stream);
    }, &plan);
    const int sb = finish_pending(t);
    return st != MSH_OK ? st : sb;
}

int msh_batch_nearest(msh_tree* t, const double* q, size_t S, uint32_t* face, uint32_t* part, double* pt) {
    return batch_host(t, q, S, face, part, pt, nullptr, "msh_batch_nearest");
}

int msh_batch_nearest_bary(msh_tree* t, const double* q, size_t S, uint32_t* face, double* pt, double* w) {
    if (!w) { set_error("msh_batch_nearest_bary: null weights"); return MSH_EINVAL; }
    return batch_host(t, q, S, face, nullptr, pt, w, "msh_batch_nearest_bary");
}

}  // extern "C"
