// Device state of libmeshsearch: the calling thread's error text and device selection, the device-memory cache
// (DevCache) with DevBuf / Workspace on top of it, the pool of idle query workspaces (WsPool), kernel timing, and the
// life of a handle (new_tree / free_tree / finish_pending).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>

#include "hostpipe.h"
#include "internal.h"

namespace msh {

thread_local std::string g_err;
thread_local int g_device = -1;
// devices of the trees built next on this thread (msh_set_devices / msh_set_device_list); empty: one device
thread_local std::vector<int> g_devices;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

static void release_idle_device(int dev);  // idle pooled workspaces / staging slabs of a device (below)

// Device allocations of the library (tree buffers, build temporaries, scratch) go through one process-wide cache: a
// freed block is kept for the next request of a similar size on its device instead of being unmapped, so a caller
// that builds a tree per call (Mesh.closest_faces_and_points; C4's batched build + query: ~11 GB of buffers per
// call) does not pay hipMalloc / hipFree of gigabytes every time.  A free waits for the device as hipFree does (a
// block still read by queued launches is never handed out again), the cache holds at most MESH_AMD_DEVICE_CACHE_MB
// (default 16384; 0 turns it off) and msh_device_pool_trim empties it.
class DevCache {
  public:
    hipError_t alloc(void** p, size_t bytes) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const size_t want = grain(bytes);
        if (cap() > 0) {
            std::lock_guard<std::mutex> g(mu_);
            auto& fl = free_[dev];
            auto it = fl.lower_bound(want);
            if (it != fl.end() && it->first <= want + want / 4) {
                *p = it->second;
                cached_ -= it->first;
                fl.erase(it);
                return hipSuccess;
            }
        }
        e = hipMalloc(p, want);
        if (e == hipErrorOutOfMemory) {
            // everything the library holds idle on this device goes first: the idle query workspace and staging
            // slabs (their blocks come back into this cache), then the cached blocks themselves.  No lock of
            // this cache is held here, so the pools' lock -> cache lock order is kept.
            (void)hipGetLastError();
            release_idle_device(dev);
            trim_device(dev);
            e = hipMalloc(p, want);
        }
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> g(mu_);
        blocks_[*p] = Blk{want, dev};
        return hipSuccess;
    }
    hipError_t free(void* p) {
        if (!p) return hipSuccess;
        Blk b;
        {
            std::lock_guard<std::mutex> g(mu_);
            auto it = blocks_.find(p);
            if (it == blocks_.end()) return hipFree(p);  // not ours
            b = it->second;
            if (cap() == 0) {
                blocks_.erase(it);
                return hipFree(p);
            }
        }
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (cur != b.dev) (void)hipSetDevice(b.dev);
        const hipError_t e = hipDeviceSynchronize();  // the wait hipFree would make
        if (cur != b.dev && cur >= 0) (void)hipSetDevice(cur);
        std::vector<std::pair<void*, int>> drop;
        {
            std::lock_guard<std::mutex> g(mu_);
            free_[b.dev].emplace(b.bytes, p);
            cached_ += b.bytes;
            while (cached_ > cap()) {  // over the cap: unmap the largest cached blocks
                std::multimap<size_t, void*>* big = nullptr;
                int bd = 0;
                for (auto& kv : free_)
                    if (!kv.second.empty() && (!big || std::prev(kv.second.end())->first > std::prev(big->end())->first)) {
                        big = &kv.second;
                        bd = kv.first;
                    }
                if (!big) break;
                auto last = std::prev(big->end());
                cached_ -= last->first;
                blocks_.erase(last->second);
                drop.emplace_back(last->second, bd);
                big->erase(last);
            }
        }
        for (auto& d : drop) unmap(d.first, d.second);
        return e;
    }
    size_t trim() {
        std::vector<int> devs;
        {
            std::lock_guard<std::mutex> g(mu_);
            for (auto& kv : free_) devs.push_back(kv.first);
        }
        size_t n = 0;
        for (int dev : devs) n += trim_device(dev);
        return n;
    }
    size_t cached() {
        std::lock_guard<std::mutex> g(mu_);
        return cached_;
    }

  private:
    struct Blk {
        size_t bytes = 0;
        int dev = 0;
    };
    static size_t grain(size_t n) {
        if (n == 0) n = 16;
        const size_t g = n >= ((size_t)1 << 20) ? ((size_t)2 << 20) : 4096;
        return (n + g - 1) / g * g;
    }
    static size_t cap() {
        static const size_t c = [] {
            const char* e = getenv("MESH_AMD_DEVICE_CACHE_MB");
            const long long mb = e ? atoll(e) : 16384;
            return mb > 0 ? (size_t)mb << 20 : (size_t)0;
        }();
        return c;
    }
    static void unmap(void* p, int dev) {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);
        (void)hipFree(p);
        if (cur != dev && cur >= 0) (void)hipSetDevice(cur);
    }
    // unmaps the cached blocks of one device; returns their bytes
    size_t trim_device(int dev) {
        std::vector<void*> drop;
        size_t n = 0;
        {
            std::lock_guard<std::mutex> g(mu_);
            for (auto& x : free_[dev]) {
                n += x.first;
                blocks_.erase(x.second);
                drop.push_back(x.second);
            }
            free_[dev].clear();
            cached_ -= n;
        }
        for (void* p : drop) unmap(p, dev);
        return n;
    }
    std::mutex mu_;
    std::map<void*, Blk> blocks_;                     // every block this cache allocated (handed out or cached)
    std::map<int, std::multimap<size_t, void*>> free_;  // cached blocks per device, by size
    size_t cached_ = 0;
};
static DevCache& dev_cache() {
    static DevCache* c = new DevCache;  // never destroyed: the runtime may be gone at static destruction
    return *c;
}
hipError_t dmalloc_raw(void** p, size_t bytes) { return dev_cache().alloc(p, bytes); }
hipError_t dfree(void* p) { return dev_cache().free(p); }
size_t dcache_trim() { return dev_cache().trim(); }
size_t dcache_bytes() { return dev_cache().cached(); }

int DevBuf::reserve(size_t need) {
    if (need <= bytes && ptr) return MSH_OK;
    if (ptr) {
        hipError_t e = dfree(ptr);
        ptr = nullptr;
        bytes = 0;
        MSH_HIP(e);
    }
    if (need == 0) need = 16;
    MSH_HIP(dmalloc(&ptr, need));
    bytes = need;
    return MSH_OK;
}

void DevBuf::release() {
    if (ptr) (void)dfree(ptr);
    ptr = nullptr;
    bytes = 0;
}

void Workspace::release() {
    DevBuf* all[] = {&keys, &vals, &keys_alt, &vals_alt, &hist, &scan, &q, &n, &out_a, &out_b, &out_c, &out_d,
                     &flags, &counters, &spill, &stats, &ranges, &qs, &ns, &inv, &res, &res_w, &resume, &p2cand, &sgn};
    for (DevBuf* b : all) b->release();
}

size_t Workspace::bytes() const {
    const DevBuf* all[] = {&keys, &vals, &keys_alt, &vals_alt, &hist, &scan, &q, &n, &out_a, &out_b, &out_c, &out_d,
                           &flags, &counters, &spill, &stats, &ranges, &qs, &ns, &inv, &res, &res_w, &resume, &p2cand, &sgn};
    size_t t = 0;
    for (const DevBuf* b : all) t += b->bytes;
    return t;
}

// Query workspaces handed from a freed triangle tree to the next one built on the device.  A caller that builds a
// tree per query batch — the reference's Mesh.closest_faces_and_points (mesh.py:454-455) — otherwise allocated and
// freed the whole query workspace per call (~8 GB of device buffers at 100M queries).  free_tree gives the
// workspace back only after the tree's work has finished; one idle workspace is kept per device, others are freed.
class WsPool {
  public:
    void give(int dev, Workspace& ws) {
        std::lock_guard<std::mutex> g(mu_);
        idle_[dev] = std::move(ws);  // keep the newest (move-assignment frees the one it replaces)
    }
    void take(int dev, Workspace& ws) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = idle_.find(dev);
        if (it == idle_.end()) return;
        ws = std::move(it->second);
        idle_.erase(it);
    }
    // frees every idle workspace; returns the bytes released
    size_t trim() {
        std::lock_guard<std::mutex> g(mu_);
        size_t n = 0;
        int cur = 0;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        for (auto& kv : idle_) {
            n += kv.second.bytes();
            (void)hipSetDevice(kv.first);
            kv.second.release();
        }
        if (have) (void)hipSetDevice(cur);
        idle_.clear();
        return n;
    }
    size_t bytes() {
        std::lock_guard<std::mutex> g(mu_);
        size_t n = 0;
        for (auto& kv : idle_) n += kv.second.bytes();
        return n;
    }
    // the idle workspace of one device (the caller is on that device)
    void trim_device(int dev) {
        Workspace ws;
        take(dev, ws);
        ws.release();
    }

  private:
    std::mutex mu_;
    std::map<int, Workspace> idle_;
};
static WsPool& ws_pool() {
    static WsPool* p = new WsPool;  // never destroyed: the runtime may be gone at static destruction
    return *p;
}
void ws_pool_take(int dev, Workspace& ws) { ws_pool().take(dev, ws); }
size_t ws_pool_trim() { return ws_pool().trim(); }
size_t ws_pool_bytes() { return ws_pool().bytes(); }

static void release_idle_device(int dev) {
    ws_pool().trim_device(dev);
    stage_pool_trim_device(dev);
}

// ---- kernel timing ----
struct Pending {
    std::string name;
    hipEvent_t a, b;
};
static std::mutex g_tmu;
static bool g_timing = false;
static std::vector<Pending> g_pending;
static std::map<std::string, std::pair<double, int64_t>> g_times;

TimedLaunch::TimedLaunch(const char* n, hipStream_t st) : name(n), s(st) {
    std::lock_guard<std::mutex> g(g_tmu);
    if (!g_timing) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        a = b = nullptr;
        return;
    }
    (void)hipEventRecord(a, s);
}

TimedLaunch::~TimedLaunch() {
    if (!a) return;
    (void)hipEventRecord(b, s);
    std::lock_guard<std::mutex> g(g_tmu);
    g_pending.push_back(Pending{name, a, b});
}

void host_time(const char* name, std::chrono::steady_clock::time_point t0) {
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::lock_guard<std::mutex> g(g_tmu);
    if (!g_timing) return;
    auto& t = g_times[name];
    t.first += ms;
    t.second += 1;
}

static void resolve_pending() {
    std::vector<Pending> p;
    {
        std::lock_guard<std::mutex> g(g_tmu);
        p.swap(g_pending);
    }
    for (auto& e : p) {
        float ms = 0.f;
        if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            std::lock_guard<std::mutex> g(g_tmu);
            auto& t = g_times[e.name];
            t.first += ms;
            t.second += 1;
        }
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
}

extern "C" int msh_timing_enable(int on) {
    std::lock_guard<std::mutex> g(g_tmu);
    g_timing = on != 0;
    return MSH_OK;
}

extern "C" int msh_timing_get(const char* name, double* ms, int64_t* count) {
    resolve_pending();
    std::lock_guard<std::mutex> g(g_tmu);
    auto it = g_times.find(name ? name : "");
    *ms = it == g_times.end() ? 0.0 : it->second.first;
    *count = it == g_times.end() ? 0 : it->second.second;
    return MSH_OK;
}

extern "C" int msh_timing_reset(void) {
    resolve_pending();
    std::lock_guard<std::mutex> g(g_tmu);
    g_times.clear();
    return MSH_OK;
}

int use_device(int dev) {
    MSH_HIP(hipSetDevice(dev));
    return MSH_OK;
}

int current_device(int* dev) {
    if (g_device >= 0) {
        *dev = g_device;
        return MSH_OK;
    }
    int d = 0;
    MSH_HIP(hipGetDevice(&d));
    *dev = d;
    return MSH_OK;
}

// compute units of a device, looked up once per device (the persistent grids of the query launches are sized by it);
// 256 where the runtime does not say
int device_cus(int dev) {
    static std::mutex mu;
    static int cache[64] = {0};
    std::lock_guard<std::mutex> g(mu);
    if (dev < 0 || dev >= 64) return 256;
    if (!cache[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cache[dev] = n;
    }
    return cache[dev];
}

int plan_spill(Workspace& ws, int need, int lds_depth, unsigned nblk, uint2** spill, int* depth) {
    *spill = nullptr;
    *depth = 0;
    if (need <= lds_depth) return MSH_OK;
    *depth = need - lds_depth + 1;
    MSH_TRY(ws.spill.reserve((size_t)nblk * kBlock * (size_t)*depth * sizeof(uint2)));
    *spill = ws.spill.as<uint2>();
    return MSH_OK;
}

// End of an asynchronous batched build: wait for its last kernel, free its temporaries, read its GPU time.  A kernel
// failure of the build surfaces here (MSH_EDEVICE), at the first call that needs the tree.
int finish_pending(msh_tree* t) {
    if (!t->pending) return MSH_OK;
    (void)hipSetDevice(t->device);
    const hipError_t e = hipEventSynchronize(t->pend_done);
    float ms = 0.f;
    if (e == hipSuccess && hipEventElapsedTime(&ms, t->pend_e0, t->pend_done) == hipSuccess) t->build_ms += ms;
    for (void* p : t->pend_free)
        if (p) (void)dfree(p);
    t->pend_free.clear();
    t->pend_ws.release();
    (void)hipEventDestroy(t->pend_e0);
    (void)hipEventDestroy(t->pend_done);
    t->pend_e0 = t->pend_done = nullptr;
    t->pending = false;
    if (e != hipSuccess) {
        set_error("batched LBVH build failed: %s", hipGetErrorString(e));
        return MSH_EDEVICE;
    }
    return MSH_OK;
}

void free_tree(msh_tree* t) {
    if (!t) return;
    if (t->pending) {
        const std::string keep = g_err;
        (void)finish_pending(t);
        g_err = keep;
    }
    for (msh_tree* r : t->replicas) free_tree(r);
    t->replicas.clear();
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    if (t->ws_done) (void)hipEventSynchronize(t->ws_done);
    // triangle trees (single, batched, normals metric) took one when they were built, if one was idle
    if (t->kind != kPoints) ws_pool().give(t->device, t->ws);
    t->ws.release();
    void* owned[] = {t->d_v,   t->d_nodes,     t->d_orgs, t->d_boxes, t->d_leaves, t->d_vorder, t->d_vorder_shard,
                     t->d_cut, t->d_face_leaf, t->d_sign, t->d_wind};
    for (void* p : owned) (void)dfree(p);  // a null pointer is skipped
    t->stage.free_host();
    t->stage.free_device();
    for (int b = 0; b < 3; ++b) {
        if (t->e_up[b]) (void)hipEventDestroy(t->e_up[b]);
        if (t->e_run[b]) (void)hipEventDestroy(t->e_run[b]);
        if (t->e_down[b]) (void)hipEventDestroy(t->e_down[b]);
    }
    if (t->s_up) (void)hipStreamDestroy(t->s_up);
    if (t->s_down) (void)hipStreamDestroy(t->s_down);
    if (t->ws_done) (void)hipEventDestroy(t->ws_done);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
}

int return_tree(msh_tree* t, int st, msh_tree** out) {
    if (st != MSH_OK) {
        const std::string keep = g_err;
        free_tree(t);
        g_err = keep;
        return st;
    }
    *out = t;
    return MSH_OK;
}

int new_tree(int kind, msh_tree** out) {
    int dev = 0;
    MSH_TRY(current_device(&dev));
    MSH_TRY(use_device(dev));
    msh_tree* t = new msh_tree();
    t->device = dev;
    t->kind = kind;
    // A blocking stream: it orders with the legacy default stream, so a caller that queues its inputs there (torch's
    // default stream is handle 0, which the *_device entry points read as "the handle's own stream") and then
    // passes NULL sees its writes before the handle's kernels read them, and its later default-stream work after
    // them.  (A non-blocking stream here let the C3 query order read rows torch's generator was still writing.)
    hipError_t e = hipStreamCreateWithFlags(&t->stream, hipStreamDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->ws_done, hipEventDisableTiming);
    if (e != hipSuccess) {
        set_error("hipStreamCreate / hipEventCreate failed on device %d: %s", dev, hipGetErrorString(e));
        free_tree(t);
        return MSH_EDEVICE;
    }
    *out = t;
    return MSH_OK;
}

}  // namespace msh
