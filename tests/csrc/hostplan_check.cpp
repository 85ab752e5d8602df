// Host-only check of mesh_amd/csrc/hostplan.h, the planning of a host-buffer call: the chunk list, the column
// layout and the row shards.  No GPU and no HIP: a plain C++ program (tests/test_abi.py compiles and runs it, once
// more under AddressSanitizer + UBSan).
//
//   c++ -O1 -std=c++17 hostplan_check.cpp -I<csrc> -o hostplan_check && ./hostplan_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "hostplan.h"

using namespace msh;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

// 1. the chunks of a plan tile [0, S) in order, none empty, each the plan's entry (the last repeated) except a ragged
// last one, and the slab is sized for the largest
static void chunk_cover(const std::vector<size_t>& plan) {
    size_t sum = 0;
    for (size_t p : plan) sum += p;
    const size_t at[] = {0, 1, plan[0] - 1, plan[0], plan[0] + 1, sum - 1, sum, sum + 1, 3 * sum + 7};
    for (size_t S : at) {
        const HostChunks c = host_chunks(plan, S);
        CHECK(c.r0.size() == c.n.size());
        CHECK((S == 0) == c.n.empty());
        size_t next = 0, largest = 0;
        for (size_t k = 0; k < c.n.size(); ++k) {
            CHECK(c.r0[k] == next);
            CHECK(c.n[k] >= 1);
            const size_t want = std::max<size_t>(1, plan[std::min(k, plan.size() - 1)]);
            CHECK(k + 1 == c.n.size() ? c.n[k] <= want : c.n[k] == want);
            next += c.n[k];
            largest = std::max(largest, c.n[k]);
        }
        CHECK(next == S);
        CHECK(c.largest == largest);
    }
}

// 2. a column set: the offsets are the prefix sums of the declared widths, inputs first; row and in_end as given
static void layout(const HostCols& c, const std::vector<size_t>& widths, size_t n_in, size_t row, size_t in_end) {
    CHECK(c.cols.size() == widths.size() && c.off.size() == widths.size() + 1);
    size_t sum = 0, ins = 0;
    for (size_t k = 0; k < c.cols.size(); ++k) {
        CHECK(c.off[k] == sum);
        CHECK(c.cols[k].row_bytes == widths[k]);
        CHECK((c.cols[k].in != nullptr) == (k < n_in));  // inputs first
        CHECK(!(c.cols[k].in && c.cols[k].out));
        sum += widths[k];
        if (k < n_in) ins = sum;
    }
    CHECK(c.off.back() == sum && c.row() == row && sum == row);
    CHECK(c.in_end == in_end && ins == in_end);
    // a slab of 1000 rows: column k at off[k] * 1000, and a shard moves every caller pointer by its own row width
    char* base = reinterpret_cast<char*>(uintptr_t(1) << 20);
    const Slabs s{base, 1000, c.off.data()};
    const HostCols sh = c.shard(37);
    for (size_t k = 0; k < c.cols.size(); ++k) {
        CHECK(s.at(k) == base + c.off[k] * 1000);
        const HostCol &a = c.cols[k], &b = sh.cols[k];
        CHECK(b.row_bytes == a.row_bytes && sh.off[k] == c.off[k]);
        if (a.in) CHECK(static_cast<const char*>(b.in) == static_cast<const char*>(a.in) + 37 * a.row_bytes);
        if (a.out) CHECK(static_cast<char*>(b.out) == static_cast<char*>(a.out) + 37 * a.row_bytes);
        CHECK((a.in == nullptr) == (b.in == nullptr) && (a.out == nullptr) == (b.out == nullptr));
    }
}

int main() {
    const size_t M = (size_t)1 << 20;
    unsetenv("MESH_AMD_HOST_CHUNK");
    CHECK(host_plan(true) == (std::vector<size_t>{8 * M, 20 * M}));
    CHECK(host_plan(false) == (std::vector<size_t>{16 * M}));
    const std::vector<size_t> own = {3, 5};
    CHECK(host_plan(true, &own) == own);
    setenv("MESH_AMD_HOST_CHUNK", "131072", 1);  // the test hook overrides every plan
    CHECK(host_plan(true) == (std::vector<size_t>{131072}) && host_plan(false, &own) == (std::vector<size_t>{131072}));
    unsetenv("MESH_AMD_HOST_CHUNK");
    chunk_cover({8 * M, 20 * M});
    chunk_cover({16 * M});
    chunk_cover({1});
    chunk_cover({2, 3, 5, 7, 11, 13, 17, 19});  // longer than most of its calls
    {
        const HostChunks c = host_chunks({8 * M, 20 * M}, 100 * 1000 * 1000);  // C3: 8M, then 20M chunks, a ragged last
        CHECK(c.n.size() == 6 && c.n[0] == 8 * M && c.n[1] == 20 * M && c.n[4] == 20 * M && c.largest == 20 * M);
        CHECK(host_chunks({0}, 3).n.size() == 3);  // a zero entry still makes chunks of one row
    }

    // the column sets of the host-buffer entry points, declared from typed caller pointers as api.cpp declares them;
    // their row widths are the literals the fan-out threshold was given by hand before the columns carried them
    double dbuf[16] = {0};
    uint32_t ubuf[16] = {0};
    const double* q = dbuf;
    double* d = dbuf;
    uint32_t* u = ubuf;
    uint32_t* none = nullptr;
    {  // msh_tree_nearest: q | face | part | point, with and without part
        HostCols c;
        const auto cq = c.in(q, 3);
        const auto cf = c.out(u, 1), cp = c.out(none, 1);
        const auto cpt = c.out(d, 3);
        layout(c, {24, 4, 4, 24}, 1, 56, 24);
        CHECK(cq.k == 0 && cf.k == 1 && cp.k == 2 && cpt.k == 3);
        CHECK(!c.cols[2].in && !c.cols[2].out);  // no caller array: a slab that nothing is downloaded from
        char* base = reinterpret_cast<char*>(uintptr_t(1) << 20);
        const Slabs s{base, 10, c.off.data()};
        CHECK(reinterpret_cast<const char*>(s[cq]) == base && reinterpret_cast<char*>(s[cp]) == base + 280 &&
              reinterpret_cast<char*>(s[cpt]) == base + 320);
        CHECK(s[Col<double>{}] == nullptr);  // an undeclared column
    }
    {  // msh_tree_nearest_bary: q | face | point | weights
        HostCols c;
        c.in(q, 3), c.out(u, 1), c.out(d, 3), c.out(d, 3);
        layout(c, {24, 4, 24, 24}, 1, 76, 24);
    }
    {  // msh_tree_signed_distance: q | sdist | face | part | point
        HostCols c;
        c.in(q, 3), c.out(d, 1), c.out(u, 1), c.out(none, 1), c.out(d, 3);
        layout(c, {24, 8, 4, 4, 24}, 1, 64, 24);
    }
    {  // msh_tree_winding_number: q | w
        HostCols c;
        c.in(q, 3), c.out(d, 1);
        layout(c, {24, 8}, 1, 32, 24);
    }
    {  // msh_tree_nearest_alongnormal: p | n | dist | face | point
        HostCols c;
        c.in(q, 3), c.in(q, 3), c.out(d, 1), c.out(u, 1), c.out(d, 3);
        layout(c, {24, 24, 8, 4, 24}, 2, 84, 48);
    }
    {  // msh_ntree_nearest: q | n | face | point
        HostCols c;
        c.in(q, 3), c.in(q, 3), c.out(u, 1), c.out(d, 3);
        layout(c, {24, 24, 4, 24}, 2, 76, 48);
    }
    {  // msh_points_nearest: q | index | distance
        HostCols c;
        c.in(q, 3), c.out(u, 1), c.out(d, 1);
        layout(c, {24, 4, 8}, 1, 36, 24);
    }
    {  // msh_visibility: rows are cameras of P = 7 vertices: vis | ndc
        const size_t P = 7;
        HostCols c;
        c.out(u, P), c.out(d, P);
        layout(c, {4 * P, 8 * P}, 0, 12 * P, 0);
    }
    {  // msh_batch_nearest(_bary): rows are meshes of S = 5 queries; part and weights only when asked for
        const size_t S = 5;
        HostCols c;
        c.in(q, 3 * S), c.out(u, S), c.out(d, 3 * S), c.out(d, 3 * S);
        layout(c, {24 * S, 4 * S, 24 * S, 24 * S}, 1, 76 * S, 24 * S);
    }

    // 3. shards: contiguous, covering, balanced
    const size_t rows[] = {0, 1, 5, 7, 100, 100000000, 4294967295ull};
    for (size_t n : rows)
        for (size_t G = 1; G <= 8; ++G) {
            size_t next = 0, lo = SIZE_MAX, hi = 0;
            for (size_t g = 0; g < G; ++g) {
                size_t r0, cnt;
                shard_rows(n, G, g, &r0, &cnt);
                CHECK(r0 == next);
                next += cnt;
                lo = std::min(lo, cnt);
                hi = std::max(hi, cnt);
            }
            CHECK(next == n && hi - lo <= 1);
        }
    std::printf("hostplan_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
