// Planning of a host-buffer call, with no HIP call in it: the columns an entry point declares and the slab layout,
// row width and shard offsets derived from them; the chunk list of a pipelined call; the row shards of a handle on
// several devices.  hostpipe.cpp executes these plans; tests/csrc/hostplan_check.cpp checks them on the CPU.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace msh {

// One column of a call's rows: caller memory it reads (in) or writes (out), row_bytes per row.  Neither: a device
// slab only (an output the caller did not ask for; nothing is downloaded from it).
struct HostCol {
    const void* in;
    void* out;
    size_t row_bytes;
};

// a declared column, by position and element type (k < 0: not declared)
template <class T>
struct Col {
    int k = -1;
};

// The columns of a call, declared once from the caller's typed pointers, inputs first.  A device slab of `chunk` rows
// holds column k at byte off[k] * chunk (off: the prefix sums of the row widths), so off.back() is the width of a
// row and in_end the inputs' share of it.
struct HostCols {
    std::vector<HostCol> cols;
    std::vector<size_t> off = {0};
    size_t in_end = 0;
    template <class T>
    Col<const T> in(const T* p, size_t per_row) {
        add({p, nullptr, per_row * sizeof(T)});
        in_end = row();
        return {(int)cols.size() - 1};
    }
    template <class T>
    Col<T> out(T* p, size_t per_row) {
        add({nullptr, p, per_row * sizeof(T)});
        return {(int)cols.size() - 1};
    }
    size_t row() const { return off.back(); }
    // the same columns from row r0 on (a replica's shard)
    HostCols shard(size_t r0) const {
        HostCols c = *this;
        for (HostCol& a : c.cols) {
            if (a.in) a.in = static_cast<const char*>(a.in) + r0 * a.row_bytes;
            if (a.out) a.out = static_cast<char*>(a.out) + r0 * a.row_bytes;
        }
        return c;
    }

  private:
    void add(const HostCol& a) {
        cols.push_back(a);
        off.push_back(off.back() + a.row_bytes);
    }
};

// one slab of `chunk` rows laid out by a HostCols' offsets: what a chunk's run callback gets
struct Slabs {
    char* base;
    size_t chunk;
    const size_t* off;
    char* at(size_t k) const { return base + off[k] * chunk; }
    template <class T>
    T* operator[](Col<T> c) const {
        return c.k < 0 ? nullptr : reinterpret_cast<T*>(at((size_t)c.k));
    }
};

// Chunk plan of a pipelined call: the rows of each chunk, the last entry repeated.  Larger chunks keep the sorted
// traversal coherent and cut per-chunk launch tails; a small first chunk lets the first download start early.
// The host link moves both directions at ~57 GB/s combined (scripts/pcie_probe.py), and a C3 call moves 2.4 GB
// up and 3.2 GB down per 100M queries, so a call is bound by its copies once they overlap the kernels.
// Measured on C3 (100M queries, results in pinned pool arrays, three device slabs; profiles/r04_c3np_plan_ab.json):
// 32M chunks 98 ms, 24M 94-96, 16M 120, 6M + 30M 96, 4M + 12M + 28M 94-96, 8M + 16M + 32M 92-94, 12M + 28M 91,
// 8M + 24M 89-91, 8M + 20M 86-89.  Staged outputs (caller arrays outside the pool): 16M chunks (4M 155 ms, 8M 137,
// 16M 134, 32M 150).  Test hook: MESH_AMD_HOST_CHUNK = rows (uniform chunks, so small calls run several chunks; it
// also overrides the plans of callers whose rows are meshes or cameras).
inline size_t host_chunk_env() {
    const char* e = getenv("MESH_AMD_HOST_CHUNK");
    const long long c = e ? atoll(e) : 0;
    return c > 0 ? (size_t)c : 0;
}
// plan_rows (optional): the caller's own plan, for rows that are whole meshes (batched trees) or cameras (visibility)
inline std::vector<size_t> host_plan(bool direct_out, const std::vector<size_t>* plan_rows = nullptr) {
    if (const size_t c = host_chunk_env()) return {c};
    if (plan_rows && !plan_rows->empty()) return *plan_rows;
    if (direct_out) return {(size_t)8 << 20, (size_t)20 << 20};
    return {(size_t)16 << 20};
}

// the chunks of rows [0, S) under a plan: first rows r0[k], rows n[k] >= 1; slabs are sized for the largest
struct HostChunks {
    std::vector<size_t> r0, n;
    size_t largest = 0;
};
inline HostChunks host_chunks(const std::vector<size_t>& plan, size_t S) {
    HostChunks c;
    for (size_t r = 0, j = 0; r < S; ++j) {
        const size_t n = std::min(std::max<size_t>(1, plan[std::min(j, plan.size() - 1)]), S - r);
        c.r0.push_back(r);
        c.n.push_back(n);
        c.largest = std::max(c.largest, n);
        r += n;
    }
    return c;
}

// Contiguous shards of n rows over G parts, the first n % G one row larger (mesh_amd/distributed.py shard_range).
inline void shard_rows(size_t n, size_t G, size_t g, size_t* r0, size_t* cnt) {
    const size_t base = n / G, rem = n % G;
    *r0 = g * base + std::min(g, rem);
    *cnt = base + (g < rem ? 1 : 0);
}

}  // namespace msh
