// The entry cut's host side: which trees take one (cut_applies), the grid sizes of the automatic policy, the build
// of one grid (build_entry_cut) and the policy that settles a handle's cut before a call (ensure_entry_cut).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "internal.h"

namespace msh {

// Entry cut of a single triangle tree (the walks' start: knn.h cut_start; the records: cutbuild.hip k_cut_level): a G^3 grid over the scene box
// widened by 1/4 on every side (each axis at least 1/20 of the largest, so flat meshes get cells of a sane
// shape), MSH_CUT_PER_LEAF cells per leaf up to 2^MSH_CUT_MAX_LOG2 cells (below; round 3 with leader phases:
// G = 64 / 126 / 160: 1718 / 1742-1765 / 1782 M q/s against 1789-1800 at G = 200); the cell centres are answered
// by the tree itself, then every cell's start entries are cut from the root.  Trees under kCutMinLeaves
// leaves start at the root (their top levels are few).  Built lazily (ensure_entry_cut): the automatic grid once the
// handle's closest-point and alongnormal calls have brought enough rows (ensure_entry_cut), so visibility and
// normals-metric trees and a few small calls never pay its memory or build time; msh_tree_set_entry_cut chooses the
// grid (built by the next closest-point or alongnormal call) or turns it off.
constexpr size_t kCutMinLeaves = 4096;

bool cut_applies(const msh_tree* t) {
    return t->kind == kTriangles && t->B == 1 && !t->d_boxes && t->T >= kCutMinLeaves && t->d_nodes && t->cut_req != 0;
}

void free_entry_cut(msh_tree* t) {
    free_after_use(t, t->d_cut);
    t->cut_G = 0;
    t->cut_ms = 0.0;
}

// The automatic grid comes in two sizes (round 6).  A coarse grid, 8 cells per leaf (at most 2^23 cells; C3: G = 200,
// 256 MB), is built by the call that brings the handle's rows to 1/16 of its cells (C3: 500k rows); it costs a
// one-shot caller ~10 ms.  The fine grid, 64 cells per leaf (at most 2^26; C3: G = 400, 2.05 GB), replaces it once the
// handle has answered kFineRowsPerCell rows per fine cell (C3: ~1G rows): its build (round 6: ~46 ms; ~113 ms with
// round 8's directional drop) pays back after that many queries (C3 100M-query batches: ~3 ms faster each than with
// the coarse grid, ~6 with the drop).  msh_tree_set_entry_cut(t, -1) asks for the fine grid at the next call (a caller
// that keeps the tree for many batches, as bench.py does).  The volume threshold is sized for that build, so the
// upgrade the policy makes on its own keeps the directional drop on whole cells (depth 0); the sub-cell depths of round
// 12, whose build is 6 / 27 times longer (C3: 0.66 / 3.05 s for 1.5 / 2.6 ms more per batch), go to the grids a caller
// asked for (build_entry_cut).
// Round-5 figures (68-B cells of 8 entries and a separate hint), C3 in M q/s: 8 per leaf, 2^23 cells: G = 200, 46.9
// node visits per query, 2156-2213; 16, 2^25: G = 252, 45.2 visits, 2238; 32, 2^25: G = 318, 43.6 visits, 2247-2290
// (profiles/r05_ab_noleaders_cut.jsonl); in another session 32: 2261-2286, 64, 2^26: G = 400, 42.2 visits,
// 2293-2321, 128, 2^27: G = 505, 41.0 visits, 2297-2333 (profiles/r05_ab_cut_size.jsonl).  Round 6's 32-B records of
// 7 entries at G = 400: 42.5 visits, 2322-2363 against 2301-2351 for the 68-B cells in one session
// (profiles/r06_c3_cut_levels_ab.jsonl).
#ifndef MSH_CUT_PER_LEAF
#define MSH_CUT_PER_LEAF 64
#endif
#ifndef MSH_CUT_MAX_LOG2
#define MSH_CUT_MAX_LOG2 26
#endif
constexpr size_t kCutCoarsePerLeaf = 8;
constexpr int kCutCoarseMaxLog2 = 23;
constexpr size_t kFineRowsPerCell = 16;
static size_t auto_cut_cells(const msh_tree* t, bool fine) {
    return fine ? std::min<size_t>((size_t)MSH_CUT_PER_LEAF * t->T, (size_t)1 << MSH_CUT_MAX_LOG2)
                : std::min<size_t>(kCutCoarsePerLeaf * t->T, (size_t)1 << kCutCoarseMaxLog2);
}
// record bytes per cell: 32 (4-B entries) for trees of <= 2^20 leaves, else 64
static size_t cut_rec_bytes(const msh_tree* t) { return t->T <= kEnt4MaxLeaves ? 32 : 64; }

// cells per axis of the grid to build: the caller's G, else the automatic coarse grid or the fine one at twice its
// resolution (8 x its cells: the fine grid's cells nest in the coarse one's, whose records then start them)
static int cut_grid(const msh_tree* t, bool fine) {
    if (t->cut_req > 0) return t->cut_req;
    const int Gc = std::max(16, (int)std::lround(std::cbrt((double)auto_cut_cells(t, false))));
    return fine ? 2 * Gc : Gc;
}

// The grid's cell centres are answered exactly by the tree (walks from the installed coarse grid when the fine one is
// built, else from the root), then every cell is cut (cutbuild.hip k_cut_level): from the enclosing coarse cell's start
// list when the coarse grid is installed and this grid is twice its resolution, else from the root.  C3 (round 6):
// coarse grid 11 ms; fine grid from it 46 ms (centre walks 26, cut 18), 67 ms from the root
// (profiles/r06_c3_cut_staged_ab.jsonl).  Round 6 also tried a pyramid -- the
// coarsest grid answered exactly, each finer level cut from the coarser one's records with hints taken from the 8
// coarse cells around it -- which built C3's grid in 41 ms instead of ~70 but started queries from worse hints:
// 49.4 node visits per query against 42.5, 2.02-2.06 G q/s against 2.32-2.36 (profiles/r06_c3_cut_levels_ab.jsonl).
// subdiv: the sub-cell depth of the directional drop, where the grid takes the drop at all (cutbuild.hip cut_dir_drop).
static int build_entry_cut(msh_tree* t, bool fine, int subdiv) {
    const int G = cut_grid(t, fine);
    double half[3], H = 0.0, lo[3], w[3];
    for (int k = 0; k < 3; ++k) {
        half[k] = 0.5 * ((double)t->scene_hi[k] - (double)t->scene_lo[k]);
        H = std::max(H, half[k]);
    }
    if (!(H > 0.0) || !std::isfinite(H)) {
        set_error("entry cut: degenerate scene box");
        return MSH_EINVAL;
    }
    for (int k = 0; k < 3; ++k) {
        const double m = 0.5 * ((double)t->scene_hi[k] + (double)t->scene_lo[k]);
        const double e = 1.25 * std::max(half[k], 0.05 * H);
        lo[k] = m - e;
        w[k] = 2.0 * e / G;
    }
    const size_t n = (size_t)G * G * G;
    if (n > 0xFFFFFFFFull) {
        set_error("entry cut: %d^3 cells exceed one query call", G);
        return MSH_ENOMEM;
    }
    const bool e4 = t->T <= kEnt4MaxLeaves;
    const size_t rb = cut_rec_bytes(t);
    // the directional drop on whole cells triples the cut launch (fp64 work per kept child: C3 coarse 3.7 -> 11.2 ms,
    // fine 22 -> 81 ms; 76 ms at round 12's parent), which a kept tree's batches repay within ~20 (C3 G = 400: 42.4 ->
    // 34.0 node visits per query) and a one-shot caller's single batch on the automatic coarse grid does not (G = 200:
    // 47.0 -> 41.6 visits, ~2 ms of 100M rows for +8 ms of build): the fine grid and a grid the caller asked for take it,
    // the automatic coarse grid keeps the ball rule alone.  Proved on sub-cells (subdiv 1 / 2) the fine launch takes
    // 0.6 / 3.0 s on C3 for 29.6 / 26.6 visits, repaid after ~355 / ~1120 batches of 100M rows: the caller's choice
    // (ensure_entry_cut), never the automatic upgrade's
    const bool directional = fine || t->cut_req > 0;
    hipStream_t s = t->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    MSH_HIP(hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    if (e != hipSuccess) {
        (void)hipEventDestroy(e0);
        MSH_HIP(e);
    }
    (void)hipEventRecord(e0, s);
    uint32_t* cut = nullptr;
    uint64_t flagged = 0;
    int st = MSH_OK;
    {
        DevBuf dq, df, dp, dinv, dhint, dflag;
        do {
            if ((st = dflag.reserve(sizeof(unsigned long long))) != MSH_OK) break;
            if ((e = hipMemsetAsync(dflag.ptr, 0, sizeof(unsigned long long), s)) != hipSuccess) {
                set_error("entry cut: %s", hipGetErrorString(e));
                st = MSH_EDEVICE;
                break;
            }
            if ((st = dq.reserve(n * 3 * sizeof(double))) != MSH_OK) break;
            if ((st = df.reserve(n * sizeof(uint32_t))) != MSH_OK) break;
            if ((st = dp.reserve(n * 3 * sizeof(double))) != MSH_OK) break;
            if ((st = dhint.reserve(n * sizeof(int))) != MSH_OK) break;
            if ((st = dinv.reserve(t->T * sizeof(uint32_t))) != MSH_OK) break;
            if ((st = cut_centres(G, lo, w, dq.as<double>(), s)) != MSH_OK) break;
            // (capping the centres' walks at 64 / 128 node steps, their best face so far an upper bound of d(c): the
            // walks 32 -> 27 / 29.5 ms on C3, the queries from the grid 42.46 -> 43.45 / 42.61 node visits,
            // profiles/r06_c3_cut_build_probe.jsonl; not kept)
            if ((st = msh_tree_nearest_device(t, dq.as<double>(), n, df.as<uint32_t>(), nullptr, dp.as<double>(), s)) !=
                MSH_OK)
                break;
            if ((st = cut_hints(t, df.as<uint32_t>(), n, dinv.as<uint32_t>(), dhint.as<int>(), s)) != MSH_OK) break;
            dq.release();  // the centres' rows are not needed by the cut itself
            e = dmalloc(&cut, n * rb);
            if (e != hipSuccess) {
                set_error("hipMalloc entry cut (%zu cells): %s", n, hipGetErrorString(e));
                st = MSH_ENOMEM;
                break;
            }
            // the installed grid, when it is this one at half resolution over the same box (the automatic coarse grid
            // under the fine one), gives every cell its start list (k_cut_level)
            const uint32_t* half = nullptr;
            if (t->d_cut && 2 * t->cut_G == G && t->cut_wide == (e4 ? 0 : 1) &&
                t->cut_lo[0] == lo[0] && t->cut_lo[1] == lo[1] && t->cut_lo[2] == lo[2])
                half = t->d_cut;
            if ((st = cut_level(t, G, lo, w, dp.as<double>(), dhint.as<int>(), cut, e4, s, half,
                                dflag.as<unsigned long long>(), directional ? subdiv : -1)) != MSH_OK)
                break;
            (void)hipEventRecord(e1, s);
            unsigned long long nflag = 0;
            if ((e = hipMemcpyAsync(&nflag, dflag.ptr, sizeof(nflag), hipMemcpyDeviceToHost, s)) != hipSuccess ||
                (e = hipStreamSynchronize(s)) != hipSuccess) {
                set_error("entry cut build: %s", hipGetErrorString(e));
                st = MSH_EDEVICE;
            }
            flagged = nflag;
        } while (0);
        (void)hipStreamSynchronize(s);  // the temporaries are freed (DevBuf destructors) as this scope ends
    }
    if (st == MSH_OK) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        t->cut_ms = ms;
        t->cut_flagged = flagged;
        t->d_cut = cut;
        t->cut_wide = e4 ? 0 : 1;
        t->cut_G = G;
        for (int k = 0; k < 3; ++k) {
            t->cut_lo[k] = lo[k];
            t->cut_iw[k] = 1.0 / w[k];
        }
    } else if (cut) {
        (void)dfree(cut);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return st;
}

// Closest-point call of S rows: settle the handle's cut first.  The automatic policy (above auto_cut_cells): the
// coarse grid once the handle has answered one row per kCutAutoCellsPerRow of its cells (C3: 500k rows; a few small
// calls on a large mesh walk from the root instead of paying for it), the fine grid once it has answered
// kFineRowsPerCell rows per fine cell; after msh_tree_set_entry_cut, the grid asked for at the next call.  The cut is
// an optimisation, so a failure (device memory, most likely) is not the query's: the partial buffers are freed, the
// error is cleared and queries start at the root (or from the coarse grid, if the fine one failed).
constexpr size_t kCutAutoCellsPerRow = 16;
void ensure_entry_cut(msh_tree* t, size_t S) {
    if (t->cut_state == kCutOff || t->cut_state == kCutFailed) return;
    if (!cut_applies(t)) {
        if (t->cut_state == kCutPending) t->cut_state = kCutOff;
        return;
    }
    const bool automatic = !t->cut_force && t->cut_req < 0;
    bool fine = t->cut_req < 0;  // an automatic request: the fine grid (explicit -1, or the volume reached)
    if (automatic) {
        t->cut_rows += S;
        const size_t coarse_rows = auto_cut_cells(t, false) / kCutAutoCellsPerRow;
        const size_t fine_rows = auto_cut_cells(t, true) * kFineRowsPerCell;
        if (t->cut_state == kCutBuilt) {  // a coarse grid: upgrade once the volume pays for the fine one
            if (t->cut_fine || t->cut_rows < fine_rows) return;
        } else if (t->cut_rows < coarse_rows) {
            return;
        }
        fine = t->cut_rows >= fine_rows;
    } else if (t->cut_state == kCutBuilt) {
        return;
    }
    const std::string keep = g_err;
    // a fine grid asked for with no grid installed (msh_tree_set_entry_cut(t, -1) before the first call) is built in
    // two stages: the coarse grid first (its own centre walks from the root), then the fine one, whose centre walks and
    // start lists begin from it (build_entry_cut); the coarse grid is then freed like an upgrade's
    double staged_ms = 0.0;
    if (fine && !t->d_cut && t->cut_req < 0) {
        t->cut_state = kCutOff;
        if (build_entry_cut(t, false, 0) == MSH_OK) {
            staged_ms = t->cut_ms;
        } else {
            (void)hipGetLastError();  // the fine grid is then built from the root
            t->d_cut = nullptr;
        }
    }
    // while a grid is built its cell-centre queries start from the coarse grid, when one is installed (an upgrade),
    // else from the root; the state is off meanwhile, so the build's own queries do not build again
    uint32_t* old = t->d_cut;
    const int old_G = t->cut_G, old_wide = t->cut_wide;
    const double old_ms = t->cut_ms;
    const uint64_t old_flagged = t->cut_flagged;
    double old_lo[3], old_iw[3];
    for (int k = 0; k < 3; ++k) {
        old_lo[k] = t->cut_lo[k];
        old_iw[k] = t->cut_iw[k];
    }
    t->cut_state = kCutOff;
    // a grid the caller asked for (msh_tree_set_entry_cut) takes the sub-cell depth; the policy's own upgrade does not
    const int st = build_entry_cut(t, fine, automatic ? 0 : kCutSubdivDefault);
    if (st == MSH_OK) {
        t->cut_ms += staged_ms;
        if (old) {
            if (t->ws_done) (void)hipEventSynchronize(t->ws_done);
            (void)dfree(old);
        }
        t->cut_state = kCutBuilt;
        t->cut_fine = fine;
    } else {
        (void)hipGetLastError();  // clear a sticky launch / allocation error of the failed build
        if (old) {  // a failed upgrade keeps the coarse grid
            t->d_cut = old;
            t->cut_G = old_G;
            t->cut_wide = old_wide;
            t->cut_ms = old_ms;
            t->cut_flagged = old_flagged;
            for (int k = 0; k < 3; ++k) {
                t->cut_lo[k] = old_lo[k];
                t->cut_iw[k] = old_iw[k];
            }
            t->cut_state = kCutBuilt;
            t->cut_fine = true;  // no second try
        } else {
            // an automatic grid is tried again after another threshold of rows (memory may have been freed by then),
            // at most twice; a grid the caller asked for fails at once (msh_tree_set_entry_cut re-arms it)
            t->cut_state = automatic && ++t->cut_fails <= 2 ? kCutPending : kCutFailed;
            t->cut_rows = 0;
        }
    }
    g_err = keep;
}

}  // namespace msh
