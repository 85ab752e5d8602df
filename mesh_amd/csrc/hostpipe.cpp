// The host-buffer pipeline (hostpipe.h): the copy workers, the staging-slab pool and the pinned result pool, the
// chunk pipeline that executes hostplan.h's plans (pipelined, and pipelined_registered for arrays page-locked in
// place), and the fan-out of one call over a handle's devices.
#include "hostpipe.h"

#include <atomic>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <thread>

namespace msh {

static int host_threads() {
    const char* e = getenv("MESH_AMD_COPY_THREADS");
    int n = e ? atoi(e) : 0;
    if (n <= 0) {
        const char* o = getenv("OMP_NUM_THREADS");
        n = o ? atoi(o) : 8;
    }
    return std::max(1, std::min(n, 32));
}

// Persistent host copy workers (created on first use, one pool per process): run(tasks) splits a list of
// memcpys into ~2 MB pieces and executes them on all workers plus the caller, so the pageable <-> pinned
// staging copies of one pipeline step (inputs of chunk k and outputs of chunk k - 2) move together at the
// host's memory bandwidth instead of one after the other, without creating threads per copy.
struct CopyTask {
    void* dst;
    const void* src;
    size_t bytes;
};
class CopyPool {
  public:
    explicit CopyPool(int n) {
        for (int i = 0; i < n; ++i) th_.emplace_back([this] { loop(); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void run(const std::vector<CopyTask>& tasks) {
        constexpr size_t kPiece = (size_t)2 << 20;
        std::vector<CopyTask> pieces;
        for (const CopyTask& t : tasks)
            for (size_t o = 0; o < t.bytes; o += kPiece)
                pieces.push_back({static_cast<char*>(t.dst) + o, static_cast<const char*>(t.src) + o,
                                  std::min(kPiece, t.bytes - o)});
        if (pieces.empty()) return;
        std::lock_guard<std::mutex> job(job_mu_);  // one job at a time
        {
            std::lock_guard<std::mutex> g(mu_);
            pieces_ = &pieces;
            next_.store(0);
            ++gen_;
        }
        cv_.notify_all();
        work(&pieces);
        // every worker that took this job has left it before `pieces` goes away
        std::unique_lock<std::mutex> g(mu_);
        done_cv_.wait(g, [&] { return busy_ == 0; });
        pieces_ = nullptr;
    }

  private:
    void work(std::vector<CopyTask>* p) {
        for (;;) {
            const size_t i = next_.fetch_add(1);
            if (i >= p->size()) return;
            std::memcpy((*p)[i].dst, (*p)[i].src, (*p)[i].bytes);
        }
    }
    void loop() {
        size_t seen = 0;
        for (;;) {
            std::vector<CopyTask>* p = nullptr;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                p = pieces_;
                if (p) ++busy_;
            }
            if (!p) continue;
            work(p);
            std::lock_guard<std::mutex> g(mu_);
            if (--busy_ == 0) done_cv_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_, job_mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<CopyTask>* pieces_ = nullptr;
    std::atomic<size_t> next_{0};
    int busy_ = 0;
    size_t gen_ = 0;
    bool stop_ = false;
};
static CopyPool& copy_pool() {
    static CopyPool pool(host_threads() - 1);
    return pool;
}

void StageSet::free_host() {
    for (void*& p : h) {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
    hbytes = 0;
}
void StageSet::free_device() {
    for (void*& p : d) {
        if (p) (void)dfree(p);
        p = nullptr;
    }
    dbytes = 0;
}

// Staging slabs shared by the handles of a device: a pipelined call leases one set (two pinned host slabs and three
// device slabs) into its handle and hands it back when it returns, so a caller that builds a tree per call (the
// reference's Mesh.closest_faces_and_points, mesh.py:454-455) pays the page-locking of ~1.5 GB of host slabs
// once per process instead of once per tree.  At most kStageKeep idle sets are kept per device.
class StagePool {
  public:
    StageSet take(int dev) {
        std::lock_guard<std::mutex> g(mu_);
        std::vector<StageSet>& v = idle_[dev];
        if (v.empty()) return StageSet{};
        StageSet s = v.back();
        v.pop_back();
        return s;
    }
    void give(int dev, StageSet s) {
        constexpr size_t kStageKeep = 2;
        std::lock_guard<std::mutex> g(mu_);
        std::vector<StageSet>& v = idle_[dev];
        if (v.size() < kStageKeep) {
            v.push_back(s);
            return;
        }
        s.free_host();  // an extra set (concurrent calls): freed
        s.free_device();
    }

    size_t device_bytes() {
        std::lock_guard<std::mutex> g(mu_);
        size_t n = 0;
        for (auto& kv : idle_)
            for (const StageSet& s : kv.second) n += 3 * s.dbytes;
        return n;
    }
    void trim() {
        std::lock_guard<std::mutex> g(mu_);
        for (auto& kv : idle_) {
            for (StageSet& s : kv.second) {
                s.free_host();
                s.free_device();
            }
            kv.second.clear();
        }
    }
    // the idle sets' device slabs of one device (the caller is on that device); their pinned host slabs stay
    void trim_device(int dev) {
        std::vector<StageSet> drop;  // the device halves, freed once the lock is dropped
        {
            std::lock_guard<std::mutex> g(mu_);
            for (StageSet& s : idle_[dev]) {
                drop.emplace_back();
                std::swap_ranges(s.d, s.d + 3, drop.back().d);
                s.dbytes = 0;
            }
        }
        for (StageSet& s : drop) s.free_device();
    }

  private:
    std::mutex mu_;
    std::map<int, std::vector<StageSet>> idle_;
};
static StagePool& stage_pool() {
    static StagePool* p = new StagePool;  // never destroyed: the runtime may be gone at static destruction
    return *p;
}

void stage_pool_trim() { stage_pool().trim(); }
void stage_pool_trim_device(int dev) { stage_pool().trim_device(dev); }
size_t stage_pool_device_bytes() { return stage_pool().device_bytes(); }

// the handle holds the leased set for one call (stage_setup grows it in place)
struct StageLease {
    msh_tree* t;
    explicit StageLease(msh_tree* tree) : t(tree) { t->stage = stage_pool().take(t->device); }
    ~StageLease() {
        stage_pool().give(t->device, t->stage);
        t->stage = StageSet{};
    }
};

// copy streams, events, and two host slabs of >= host_bytes and three device slabs of >= dev_bytes (grow-only)
static int stage_setup(msh_tree* t, size_t host_bytes, size_t dev_bytes) {
    StageSet& g = t->stage;
    if (!t->s_up) MSH_HIP(hipStreamCreateWithFlags(&t->s_up, hipStreamNonBlocking));
    if (!t->s_down) MSH_HIP(hipStreamCreateWithFlags(&t->s_down, hipStreamNonBlocking));
    for (int b = 0; b < 3; ++b) {
        if (!t->e_up[b]) MSH_HIP(hipEventCreateWithFlags(&t->e_up[b], hipEventDisableTiming));
        if (!t->e_run[b]) MSH_HIP(hipEventCreateWithFlags(&t->e_run[b], hipEventDisableTiming));
        if (!t->e_down[b]) MSH_HIP(hipEventCreateWithFlags(&t->e_down[b], hipEventDisableTiming));
    }
    if (g.hbytes < host_bytes) {
        g.free_host();
        for (void*& p : g.h) MSH_HIP(hipHostMalloc(&p, host_bytes, hipHostMallocDefault));
        g.hbytes = host_bytes;
    }
    if (g.dbytes < dev_bytes) {
        g.free_device();
        for (void*& p : g.d) MSH_HIP(dmalloc(&p, dev_bytes));
        g.dbytes = dev_bytes;
    }
    return MSH_OK;
}

// MESH_AMD_HOST_REGISTER=1: page-lock the caller's arrays in place instead of staging.  Off by default:
// registering C3's 5.6 GB of rows per call cost more than the staging copies (C3 numpy path 395 vs 280 ms).
static bool host_register_enabled() {
    const char* e = getenv("MESH_AMD_HOST_REGISTER");
    return e && atoi(e) != 0;
}

// Page-locked result pool (msh_host_alloc / msh_host_free, meshsearch.h).  Blocks are hipHostMalloc'd in 2-MB
// granules and kept after release for the next call of similar size, up to a cap; the host-buffer entry points
// download results straight into output arrays that lie inside a live block (pinned_range).
class PinnedPool {
  public:
    int alloc(size_t bytes, void** out) {
        constexpr size_t kGran = (size_t)2 << 20;
        const size_t want = (std::max<size_t>(bytes, 1) + kGran - 1) / kGran * kGran;
        std::lock_guard<std::mutex> g(mu_);
        auto it = free_.lower_bound(want);  // best fit, at most 5/4 of the request
        if (it != free_.end() && it->first <= want + want / 4) {
            *out = it->second;
            live_.insert(it->second);
            free_.erase(it);
            return MSH_OK;
        }
        const size_t cap = cap_bytes();
        // make room: release free blocks, largest first, until the new block fits under the cap
        while (total_ + want > cap && !free_.empty()) release_locked(std::prev(free_.end()));
        if (total_ + want > cap) {
            set_error("msh_host_alloc: pinned pool cap %zu MB reached", cap >> 20);
            return MSH_ENOMEM;
        }
        void* p = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            while (!free_.empty()) release_locked(std::prev(free_.end()));
            if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                set_error("msh_host_alloc: hipHostMalloc of %zu bytes failed", want);
                return MSH_ENOMEM;
            }
        }
        blocks_[p] = want;
        live_.insert(p);
        total_ += want;
        *out = p;
        return MSH_OK;
    }
    void release(void* p) {
        std::lock_guard<std::mutex> g(mu_);
        auto b = blocks_.find(p);
        if (b == blocks_.end() || !live_.erase(p)) return;
        free_.emplace(b->second, p);
    }
    int trim() {
        std::lock_guard<std::mutex> g(mu_);
        while (!free_.empty()) release_locked(std::prev(free_.end()));
        return MSH_OK;
    }
    size_t bytes() {
        std::lock_guard<std::mutex> g(mu_);
        return total_;
    }
    // [p, p + n) lies inside one live block
    bool contains(const void* p, size_t n) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = blocks_.upper_bound(const_cast<void*>(p));
        if (it == blocks_.begin()) return false;
        --it;
        const char* b = static_cast<const char*>(it->first);
        const char* c = static_cast<const char*>(p);
        return live_.count(it->first) && c >= b && c + n <= b + it->second;
    }

  private:
    static size_t cap_bytes() {
        const char* e = getenv("MESH_AMD_PINNED_POOL_MB");
        const long long mb = e ? atoll(e) : 16384;
        return mb > 0 ? (size_t)mb << 20 : 0;
    }
    void release_locked(std::multimap<size_t, void*>::iterator it) {
        void* p = it->second;
        (void)hipHostFree(p);
        total_ -= it->first;
        blocks_.erase(p);
        free_.erase(it);
    }
    std::mutex mu_;
    std::map<void*, size_t> blocks_;       // every block: base -> bytes
    std::set<void*> live_;                 // blocks handed out
    std::multimap<size_t, void*> free_;    // released blocks by size
    size_t total_ = 0;
};
static PinnedPool& pinned_pool() {
    static PinnedPool* p = new PinnedPool;  // never destroyed: live arrays may outlive static destructors
    return *p;
}

extern "C" int msh_host_alloc(size_t bytes, void** out) {
    if (!out) { set_error("msh_host_alloc: null argument"); return MSH_EINVAL; }
    *out = nullptr;
    return pinned_pool().alloc(bytes, out);
}

extern "C" void msh_host_free(void* p) {
    if (p) pinned_pool().release(p);
}

extern "C" int msh_host_pool_trim(void) {
    stage_pool().trim();
    return pinned_pool().trim();
}

extern "C" size_t msh_host_pool_bytes(void) { return pinned_pool().bytes(); }

// Enqueues on s the copies of n rows of every input (in) or output (!in) column between the device slab and the
// host: the same layout in a host slab, or (host == nullptr) the caller's own rows from row r0 on.
static hipError_t copy_cols(const HostCols& c, bool in, const Slabs& dev, const Slabs* host, size_t r0, size_t n,
                            hipStream_t s) {
    hipError_t e = hipSuccess;
    for (size_t j = 0; j < c.cols.size() && e == hipSuccess; ++j) {
        const HostCol& a = c.cols[j];
        if (in ? !a.in : !a.out) continue;
        char* rows = (in ? static_cast<char*>(const_cast<void*>(a.in)) : static_cast<char*>(a.out)) + r0 * a.row_bytes;
        char* h = host ? host->at(j) : rows;
        e = in ? hipMemcpyAsync(dev.at(j), h, n * a.row_bytes, hipMemcpyHostToDevice, s)
               : hipMemcpyAsync(h, dev.at(j), n * a.row_bytes, hipMemcpyDeviceToHost, s);
    }
    return e;
}

// pipelined() over caller arrays that are page-locked in place: per chunk an H2D copy of the input rows into a
// device slab (copy stream `up`), the kernels (handle stream), a D2H copy of the output rows straight into
// the caller's arrays (stream `down`); two device slabs alternate, so chunk k uploads while k - 1 computes and
// k - 2 downloads.
static int pipelined_registered(msh_tree* t, size_t S, const HostCols& c, size_t chunk, const ChunkRun& run) {
    MSH_TRY(stage_setup(t, 0, chunk * c.row()));
    hipStream_t sc = t->stream, up = t->s_up, down = t->s_down;
    int st = MSH_OK;
    hipError_t e = hipSuccess;
    const size_t nch = (S + chunk - 1) / chunk;
    for (size_t k = 0; k < nch && st == MSH_OK && e == hipSuccess; ++k) {
        const int b = (int)(k & 1);
        const size_t r0 = k * chunk, n = std::min(chunk, S - r0);
        const Slabs dev{static_cast<char*>(t->stage.d[b]), chunk, c.off.data()};
        // the slab's previous chunk (k - 2) must have been downloaded before it is overwritten
        if (k >= 2 && (e = hipStreamWaitEvent(up, t->e_down[b], 0)) != hipSuccess) break;
        if ((e = copy_cols(c, true, dev, nullptr, r0, n, up)) != hipSuccess || (e = hipEventRecord(t->e_up[b], up)) != hipSuccess ||
            (e = hipStreamWaitEvent(sc, t->e_up[b], 0)) != hipSuccess)
            break;
        if ((st = run(r0, n, dev)) != MSH_OK) break;
        if ((e = hipEventRecord(t->e_run[b], sc)) != hipSuccess || (e = hipStreamWaitEvent(down, t->e_run[b], 0)) != hipSuccess)
            break;
        if ((e = copy_cols(c, false, dev, nullptr, r0, n, down)) == hipSuccess) e = hipEventRecord(t->e_down[b], down);
    }
    const hipError_t e1 = hipStreamSynchronize(up), e2 = hipStreamSynchronize(sc), e3 = hipStreamSynchronize(down);
    if (e == hipSuccess) e = e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3);
    if (st == MSH_OK && e != hipSuccess) {
        set_error("host call (registered): %s", hipGetErrorString(e));
        st = e == hipErrorOutOfMemory ? MSH_ENOMEM : MSH_EDEVICE;
    }
    return st;
}

int pipelined(msh_tree* t, size_t S, const HostCols& c, const ChunkRun& run, const std::vector<size_t>* plan_rows) {
    const size_t row = c.row(), ncol = c.cols.size();
    // outputs inside the pinned result pool (msh_host_alloc) are downloaded straight into place: no staging
    // copy, and the host only waits for a slab's previous upload before refilling it
    bool direct_out = true;
    for (const HostCol& a : c.cols)
        if (a.out && !pinned_pool().contains(a.out, S * a.row_bytes)) direct_out = false;
    hipStream_t sc = t->stream;
    int st = MSH_OK;
    if (S * row <= ((size_t)16 << 20)) {  // small call: one pageable round trip through device scratch
        DevBuf tmp;
        MSH_TRY(tmp.reserve(S * row));
        const Slabs dev{static_cast<char*>(tmp.ptr), S, c.off.data()};
        hipError_t e = copy_cols(c, true, dev, nullptr, 0, S, sc);
        if (e == hipSuccess) st = run(0, S, dev);
        if (e == hipSuccess && st == MSH_OK) e = copy_cols(c, false, dev, nullptr, 0, S, sc);
        const hipError_t e2 = hipStreamSynchronize(sc);
        if (e == hipSuccess) e = e2;
        tmp.release();
        if (st == MSH_OK && e != hipSuccess) {
            set_error("host call: %s", hipGetErrorString(e));
            st = MSH_EDEVICE;
        }
        return st;
    }
    const HostChunks ch = host_chunks(host_plan(direct_out, plan_rows), S);
    const size_t chunk = ch.largest, nch = ch.n.size();
    StageLease lease(t);  // every stream is synchronised before pipelined returns, so the slabs are idle then
    // Optionally (host_register_enabled) page-lock the caller's arrays in place (hipHostRegister): the copy
    // engines then move the rows straight between the caller's memory and HBM, with no pageable <-> pinned
    // staging copies on the host.  Any registration failure falls back to staging.
    if (host_register_enabled()) {
        std::vector<std::pair<void*, size_t>> reg;
        bool ok = true;
        for (const HostCol& a : c.cols) {
            void* p = a.in ? const_cast<void*>(a.in) : a.out;
            if (!p) continue;
            if (hipHostRegister(p, S * a.row_bytes, hipHostRegisterDefault) != hipSuccess) {
                (void)hipGetLastError();
                ok = false;
                break;
            }
            reg.emplace_back(p, S * a.row_bytes);
        }
        if (ok) st = pipelined_registered(t, S, c, chunk, run);
        for (auto& r : reg) (void)hipHostUnregister(r.first);
        if (ok) return st;
    }
    MSH_TRY(stage_setup(t, chunk * (direct_out ? c.in_end : row), chunk * row));
    hipStream_t up = t->s_up, down = t->s_down;
    hipEvent_t *e_up = t->e_up, *e_run = t->e_run, *e_down = t->e_down;
    auto host = [&](int b) { return Slabs{static_cast<char*>(t->stage.h[b]), chunk, c.off.data()}; };
    auto dev = [&](int db) { return Slabs{static_cast<char*>(t->stage.d[db]), chunk, c.off.data()}; };
    auto fail = [&](hipError_t e, const char* what) {
        set_error("%s: %s", what, hipGetErrorString(e));
        st = e == hipErrorOutOfMemory ? MSH_ENOMEM : MSH_EDEVICE;
    };
    // Step k (host slab b = k & 1, device slab db = k % 3; a slab holds one chunk's input rows and, after them,
    // its output rows; events are per device slab):
    //   wait for chunk k - 2's upload (direct_out) or download (staged outputs, copied out of host slab b here),
    //   then copy chunk k's inputs into host slab b, on all copy workers at once, while the GPU works on earlier
    //   chunks; then enqueue chunk k's upload (copy stream; into device slab db once chunk k - 3's download has
    //   left it), kernels (handle stream) and download (second copy stream).  Three device slabs let chunk k's
    //   upload run while chunk k - 2 is still downloading (with two, each upload waited for the download of the
    //   chunk before: C3 numpy API 112 ms per 100M queries).
    do {
        hipError_t e = hipSuccess;
        for (size_t k = 0; k < nch + 2 && st == MSH_OK; ++k) {
            const int b = (int)(k & 1), db = (int)(k % 3), pb = (int)((k + 1) % 3);  // pb: chunk k - 2's slab
            const Slabs hs = host(b), ds = dev(db);
            std::vector<CopyTask> tasks;
            if (k >= 2) {
                const auto tw = std::chrono::steady_clock::now();
                if (direct_out) {
                    if ((e = hipEventSynchronize(e_up[pb])) != hipSuccess) { fail(e, "upload"); break; }
                } else {
                    if ((e = hipEventSynchronize(e_down[pb])) != hipSuccess) { fail(e, "kernels / download"); break; }
                    for (size_t j = 0; j < ncol; ++j)  // chunk k - 2's outputs, out of host slab b
                        if (const HostCol& a = c.cols[j]; a.out)
                            tasks.push_back({static_cast<char*>(a.out) + ch.r0[k - 2] * a.row_bytes, hs.at(j),
                                             ch.n[k - 2] * a.row_bytes});
                }
                host_time("host_wait", tw);
            }
            const bool have = k < nch;
            const size_t r0 = have ? ch.r0[k] : S, n = have ? ch.n[k] : 0;
            if (have)
                for (size_t j = 0; j < ncol; ++j)
                    if (const HostCol& a = c.cols[j]; a.in)
                        tasks.push_back({hs.at(j), static_cast<const char*>(a.in) + r0 * a.row_bytes, n * a.row_bytes});
            const auto tc = std::chrono::steady_clock::now();
            copy_pool().run(tasks);
            host_time("host_copy", tc);
            if (!have) continue;
            // the device slab's previous chunk (k - 3) must have been downloaded before it is overwritten (staged
            // outputs: the host waited for chunk k - 2's download above, which the in-order download stream implies)
            if (direct_out && k >= 3 && (e = hipStreamWaitEvent(up, e_down[db], 0)) != hipSuccess) { fail(e, "upload"); break; }
            e = copy_cols(c, true, ds, &hs, 0, n, up);
            if (e == hipSuccess) e = hipEventRecord(e_up[db], up);
            if (e == hipSuccess) e = hipStreamWaitEvent(sc, e_up[db], 0);
            if (e != hipSuccess) { fail(e, "upload"); break; }
            if ((st = run(r0, n, ds)) != MSH_OK) break;
            if ((e = hipEventRecord(e_run[db], sc)) != hipSuccess || (e = hipStreamWaitEvent(down, e_run[db], 0)) != hipSuccess) {
                fail(e, "launch");
                break;
            }
            e = copy_cols(c, false, ds, direct_out ? nullptr : &hs, r0, n, down);
            if (e == hipSuccess) e = hipEventRecord(e_down[db], down);
            if (e != hipSuccess) { fail(e, "download"); break; }
        }
    } while (0);
    // every chunk's kernels and copies end here: in direct_out mode no earlier wait saw their status (the loop
    // only waits for uploads), so an asynchronous kernel or copy failure surfaces through these syncs
    const hipError_t e1 = hipStreamSynchronize(up), e2 = hipStreamSynchronize(down), e3 = hipStreamSynchronize(sc);
    const hipError_t ef = e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3);
    if (st == MSH_OK && ef != hipSuccess) fail(ef, "host call (kernels / download)");
    return st;
}

// ---- one handle on several devices (msh_set_devices) ----
// Host-buffer calls below this many bytes of rows stay on the handle's own device (a fan-out costs a thread per
// replica and a chunk pipeline per device).
constexpr size_t kFanMinBytes = (size_t)32 << 20;

int fan_out(msh_tree* t, size_t S, size_t row_bytes, const std::function<int(msh_tree* h, size_t r0, size_t n)>& call) {
    const size_t G = 1 + t->replicas.size();
    if (G == 1 || S * row_bytes < kFanMinBytes || S < G) return call(t, (size_t)0, S);
    std::vector<int> st(G, MSH_OK);
    std::vector<std::string> err(G);
    std::vector<std::thread> th;
    th.reserve(G - 1);
    for (size_t g = 1; g < G; ++g)
        th.emplace_back([&, g] {
            size_t r0, n;
            shard_rows(S, G, g, &r0, &n);
            if (n) st[g] = call(t->replicas[g - 1], r0, n);
            if (st[g] != MSH_OK) err[g] = g_err;
        });
    size_t r0, n;
    shard_rows(S, G, 0, &r0, &n);
    st[0] = call(t, r0, n);
    if (st[0] != MSH_OK) err[0] = g_err;
    for (auto& x : th) x.join();
    (void)use_device(t->device);  // the caller's thread stays on the handle's device
    for (size_t g = 0; g < G; ++g)
        if (st[g] != MSH_OK) {
            g_err = err[g];
            return st[g];
        }
    return MSH_OK;
}

int host_call(msh_tree* t, size_t S, const HostCols& cols, bool settle_cut, const HandleRun& run) {
    return fan_out(t, S, cols.row(), [&](msh_tree* h, size_t r0, size_t S_h) {
        MSH_TRY(use_device(h->device));
        if (settle_cut) ensure_entry_cut(h, S);
        return pipelined(h, S_h, cols.shard(r0), [&](size_t, size_t n, const Slabs& d) { return run(h, n, d); });
    });
}

}  // namespace msh
