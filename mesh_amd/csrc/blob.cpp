// The tree blob: a built tree as one flat device buffer (header, vertices, nodes, leaves) that another device or
// process unpacks into a handle of its own -- the msh_blob_* / msh_tree_blob_* entry points (RCCL replication) and
// replicate_tree, which copies a fresh tree onto the other devices of the thread's device list through it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "internal.h"

using namespace msh;

extern "C" {

struct BlobHeader {
    uint64_t magic;
    int32_t kind, max_depth;
    uint64_t P, T, T_main, v_rows;
    double eps;
    float scene_lo[3], scene_hi[3];
    uint64_t off_v, off_nodes, off_leaves, total;
    double origin[3];
    uint32_t node_bytes, leaf_bytes;
};
static const uint64_t kBlobMagic = 0x4d53484c42564835ull;  // "MSHLBVH5" (interleaved node frame, bf16 scales)

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static void blob_layout_sizes(int kind, uint64_t P, uint64_t T, BlobHeader& h) {
    std::memset(&h, 0, sizeof(h));
    h.magic = kBlobMagic;
    h.kind = kind;
    h.P = P;
    h.T = T;
    // visibility trees keep the extra-mesh vertices after the main rows; only the main rows are needed
    h.v_rows = P;
    h.node_bytes = (uint32_t)sizeof(BNode);
    h.leaf_bytes = (uint32_t)(kind == kPoints ? sizeof(PtRec) : sizeof(TriRec));
    h.off_v = align256(sizeof(BlobHeader));
    h.off_nodes = align256(h.off_v + h.v_rows * 3 * sizeof(double));
    h.off_leaves = align256(h.off_nodes + (T > 1 ? (T - 1) * sizeof(BNode) : 0));
    h.total = align256(h.off_leaves + T * h.leaf_bytes);
}

static void blob_layout(const msh_tree* t, BlobHeader& h) {
    blob_layout_sizes(t->kind, t->P, t->T, h);
    h.max_depth = t->max_depth;
    h.T_main = t->T_main;
    h.eps = t->eps;
    for (int k = 0; k < 3; ++k) {
        h.scene_lo[k] = t->scene_lo[k];
        h.scene_hi[k] = t->scene_hi[k];
        h.origin[k] = t->origin[k];
    }
}

static int blob_check(const BlobHeader& h, size_t bytes) {
    BlobHeader want;
    if (h.magic != kBlobMagic) {
        set_error("not a meshsearch tree blob (magic %llx)", (unsigned long long)h.magic);
        return MSH_EINVAL;
    }
    if (h.kind < 0 || h.kind > 2 || h.T == 0 || h.T > 0x7FFFFFFFull || h.P > 0xFFFFFFFFull) {
        set_error("corrupt tree blob header (kind %d, P %llu, T %llu)", h.kind, (unsigned long long)h.P,
                  (unsigned long long)h.T);
        return MSH_EINVAL;
    }
    blob_layout_sizes(h.kind, h.P, h.T, want);
    if (h.node_bytes != want.node_bytes || h.leaf_bytes != want.leaf_bytes || h.off_v != want.off_v ||
        h.off_nodes != want.off_nodes || h.off_leaves != want.off_leaves || h.total != want.total) {
        set_error("tree blob layout mismatch (built by a different library version?)");
        return MSH_EINVAL;
    }
    if (h.total > bytes) {
        set_error("tree blob truncated: header says %llu bytes, %zu given", (unsigned long long)h.total, bytes);
        return MSH_EINVAL;
    }
    return MSH_OK;
}

static void blob_info_of(const BlobHeader& h, msh_blob_info* out) {
    out->kind = h.kind;
    out->max_depth = h.max_depth;
    out->n_points = h.P;
    out->n_faces = h.T;
    out->n_main_faces = h.T_main;
    out->off_vertices = h.off_v;
    out->off_nodes = h.off_nodes;
    out->off_leaves = h.off_leaves;
    out->total = h.total;
    out->node_bytes = h.node_bytes;
    out->leaf_bytes = h.leaf_bytes;
    for (int k = 0; k < 3; ++k) out->origin[k] = h.origin[k];
}

int msh_blob_header_write(int kind, uint64_t P, uint64_t T, uint64_t T_main, void* dst, size_t cap, msh_blob_info* info) {
    if (!dst || kind < 0 || kind > 2 || T == 0) { set_error("msh_blob_header_write: bad argument"); return MSH_EINVAL; }
    BlobHeader h;
    blob_layout_sizes(kind, P, T, h);
    h.T_main = T_main;
    if (cap < sizeof(h)) { set_error("msh_blob_header_write: %zu bytes < header", cap); return MSH_EINVAL; }
    std::memcpy(dst, &h, sizeof(h));
    if (info) blob_info_of(h, info);
    return MSH_OK;
}

int msh_blob_header_parse(const void* src, size_t bytes, msh_blob_info* info) {
    if (!src || !info) { set_error("msh_blob_header_parse: null argument"); return MSH_EINVAL; }
    BlobHeader h;
    if (bytes < sizeof(h)) { set_error("tree blob shorter than its header (%zu bytes)", bytes); return MSH_EINVAL; }
    std::memcpy(&h, src, sizeof(h));
    MSH_TRY(blob_check(h, bytes));
    blob_info_of(h, info);
    return MSH_OK;
}

int msh_tree_blob_size(const msh_tree* t, size_t* bytes) {
    if (!t || !bytes) { set_error("null argument"); return MSH_EINVAL; }
    if (t->B != 1 || t->d_boxes) { set_error("msh_tree_blob_size: batched trees are not serialisable"); return MSH_EINVAL; }
    BlobHeader h;
    blob_layout(t, h);
    *bytes = h.total;
    return MSH_OK;
}

int msh_tree_blob_pack(const msh_tree* t, void* d_dst, void* stream) {
    if (!t || !d_dst) { set_error("null argument"); return MSH_EINVAL; }
    if (t->B != 1 || t->d_boxes) { set_error("msh_tree_blob_pack: batched trees are not serialisable"); return MSH_EINVAL; }
    MSH_TRY(use_device(t->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : t->stream;
    BlobHeader h;
    blob_layout(t, h);
    char* dst = static_cast<char*>(d_dst);
    MSH_HIP(hipMemcpyAsync(dst, &h, sizeof(h), hipMemcpyHostToDevice, s));
    if (h.v_rows) MSH_HIP(hipMemcpyAsync(dst + h.off_v, t->d_v, h.v_rows * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (t->T > 1)
        MSH_HIP(hipMemcpyAsync(dst + h.off_nodes, t->d_nodes, (t->T - 1) * sizeof(BNode), hipMemcpyDeviceToDevice, s));
    MSH_HIP(hipMemcpyAsync(dst + h.off_leaves, t->d_leaves, t->T * h.leaf_bytes, hipMemcpyDeviceToDevice, s));
    MSH_HIP(hipStreamSynchronize(s));
    return MSH_OK;
}

int msh_tree_blob_unpack(const void* d_src, size_t bytes, int device, void* stream, msh_tree** out) {
    if (!d_src || !out) { set_error("null argument"); return MSH_EINVAL; }
    *out = nullptr;
    MSH_TRY(use_device(device));
    BlobHeader h;
    if (bytes < sizeof(h)) { set_error("tree blob shorter than its header (%zu bytes)", bytes); return MSH_EINVAL; }
    hipStream_t us = static_cast<hipStream_t>(stream);
    MSH_HIP(hipMemcpyAsync(&h, d_src, sizeof(h), hipMemcpyDeviceToHost, us));
    MSH_HIP(hipStreamSynchronize(us));
    MSH_TRY(blob_check(h, bytes));
    const int prev = g_device;
    g_device = device;
    msh_tree* t = nullptr;
    int st = new_tree(h.kind, &t);
    g_device = prev;
    MSH_TRY(st);
    t->max_depth = h.max_depth;
    t->P = h.P;
    t->T = h.T;
    t->T_main = h.T_main;
    t->eps = h.eps;
    for (int k = 0; k < 3; ++k) {
        t->scene_lo[k] = h.scene_lo[k];
        t->scene_hi[k] = h.scene_hi[k];
        t->origin[k] = h.origin[k];
    }
    {
        // from the fp32-rounded scene box: widened by far more than its rounding (2^-24 relative)
        const double box[6] = {h.scene_lo[0], h.scene_lo[1], h.scene_lo[2], h.scene_hi[0], h.scene_hi[1], h.scene_hi[2]};
        t->half_diag = half_diagonal(box, t->origin) * (1.0 + 1e-6);
    }
    const char* src = static_cast<const char*>(d_src);
    const size_t leaf = h.leaf_bytes;
    hipStream_t s = us ? us : t->stream;
    do {
        hipError_t e = dmalloc(&t->d_v, std::max<uint64_t>(h.v_rows, 1) * 3 * sizeof(double));
        if (e == hipSuccess && h.v_rows)
            e = hipMemcpyAsync(t->d_v, src + h.off_v, h.v_rows * 3 * sizeof(double), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && h.T > 1) e = dmalloc(&t->d_nodes, (h.T - 1) * sizeof(BNode));
        if (e == hipSuccess && h.T > 1)
            e = hipMemcpyAsync(t->d_nodes, src + h.off_nodes, (h.T - 1) * sizeof(BNode), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = dmalloc(&t->d_leaves, h.T * leaf);
        if (e == hipSuccess) e = hipMemcpyAsync(t->d_leaves, src + h.off_leaves, h.T * leaf, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error("blob unpack: %s", hipGetErrorString(e));
            st = MSH_EDEVICE;
            break;
        }
        if ((st = upload_origin(t, t->stream)) != MSH_OK) break;
        if (hipStreamSynchronize(t->stream) != hipSuccess) {
            set_error("blob unpack: origin upload failed");
            st = MSH_EDEVICE;
            break;
        }
        // the entry cut is derived from the tree: not shipped, built by the first closest-point query here
        t->ws.release();
    } while (0);
    return return_tree(t, st, out);
}

}  // extern "C"

// Copies of a freshly built tree on the other devices of the calling thread's device list (msh_set_devices): the
// tree is packed into one device blob (msh_tree_blob_pack), copied peer to peer to each device and unpacked there
// (msh_tree_blob_unpack) — the in-process form of bench.py's RCCL broadcast.  A replica on the handle's own device
// (a repeated entry of the list) unpacks from the blob in place.
int msh::replicate_tree(msh_tree* t) {
    // the list replicates trees built on its first device only (msh_set_device drops it; this is the backstop)
    if (g_devices.size() <= 1 || t->device != g_devices[0]) return MSH_OK;
    size_t bytes = 0;
    MSH_TRY(msh_tree_blob_size(t, &bytes));
    MSH_TRY(use_device(t->device));
    void* blob = nullptr;
    MSH_HIP(dmalloc(&blob, bytes));
    int st = msh_tree_blob_pack(t, blob, nullptr);
    const std::vector<int> devs = g_devices;
    for (size_t g = 1; g < devs.size() && st == MSH_OK; ++g) {
        const int d = devs[g];
        void* src = blob;
        void* copy = nullptr;
        if (d != t->device) {
            (void)hipSetDevice(d);
            hipError_t e = dmalloc(&copy, bytes);
            if (e == hipSuccess) e = hipMemcpyPeer(copy, d, blob, t->device, bytes);
            if (e != hipSuccess) {
                set_error("replicating the tree to device %d: %s", d, hipGetErrorString(e));
                st = e == hipErrorOutOfMemory ? MSH_ENOMEM : MSH_EDEVICE;
                if (copy) (void)dfree(copy);
                break;
            }
            src = copy;
        }
        msh_tree* r = nullptr;
        st = msh_tree_blob_unpack(src, bytes, d, nullptr, &r);
        if (copy) {
            (void)hipSetDevice(d);
            (void)dfree(copy);
        }
        if (st == MSH_OK) {
            r->cut_req = t->cut_req;
            r->cut_force = t->cut_force;
            r->build_ms = t->build_ms;
            t->replicas.push_back(r);
        }
    }
    (void)use_device(t->device);
    (void)dfree(blob);
    return st;
}
