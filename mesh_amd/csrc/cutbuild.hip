// Build-time half of the entry cut (entrycut.cpp build_entry_cut is its only caller; the walks that start from the
// records are in nearest.hip and rays.hip): the cell centres, the per-cell start lists with the ball rule and the
// directional drop, the hint leaves, and the closest points of given faces.
#include <algorithm>
#include <cstdlib>

#include "knn.h"

namespace msh {

// ---- entry cut (build time) ----
// cell (ix, iy, iz) = row (iz G + iy) G + ix; centre lo + (i + 1/2) w per axis
__global__ __launch_bounds__(kBlock) void k_cut_centres(int G, double lx, double ly, double lz, double wx, double wy,
                                                        double wz, double* __restrict__ q) {
    const size_t n = (size_t)G * G * G;
    const size_t cell = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= n) return;
    const size_t ix = cell % (size_t)G, iy = (cell / (size_t)G) % (size_t)G, iz = cell / ((size_t)G * G);
    q[3 * cell] = lx + ((double)ix + 0.5) * wx;
    q[3 * cell + 1] = ly + ((double)iy + 0.5) * wy;
    q[3 * cell + 2] = lz + ((double)iz + 0.5) * wz;
}

// The entry cut, one thread per cell of a G^3 grid (cell (ix, iy, iz) = row (iz G + iy) G + ix), from the root (or from
// the records of the installed half-resolution grid, d_half below), with
// U(c) = the exact distance from the centre c to its closest point (pts[cell], the centre's own query; its face's leaf
// is hint[cell]).
// R = (U(c) + 2r) (1 + 1e-6), r the cell's half-diagonal + 0.1 %.  For q in the cell, d(q) <= U(c) + r, so a subtree
// farther than R from c holds neither q's answer nor a tie.  Entries (internal nodes or ~leaves) are replaced by their
// children whose bound from c is within R, in passes over the list, while it keeps at most kCutK entries; a child
// outside R is dropped (the cull is the traversal's own: bound > fp32(R^2 (1 + 2^-40)) rounded up).  An entry's bound
// from c: its box bound when its parent node was expanded, raised to the smaller of its children's bounds when its own
// node is loaded -- each a lower bound of the squared distance from c to what it holds.  (Exact leaf distances as the
// leaves' bounds, dropping leaves beyond R: 0.4 % fewer leaf tests per query for 10 ms more of build on C3,
// profiles/r06_c3_cut_build_probe.jsonl.)  An entry that cannot be expanded is retried only once the list shrank.
// Out (E4: 32-B records of 4-B entries, trees of <= 2^20 leaves; else 64-B records: word 1 the radius R around c the
// list covers, then (ref, bound bits) pairs): word 0 the hint leaf, then the entries nearest-first with max(s, 0)^2
// rounded down to fp32, s = sqrt(bound) (1 - 1e-5) - r (1 + 1e-5): a lower bound of the squared distance from any q
// of the cell.
//
// The directional drop (cut_dir_drop; DIR launches: the fine grid and grids a caller asked for).  A child the ball
// rule kept is tried on the whole cell and, when that fails, piece by piece on the cell's octants and their octants
// (round 12, "Sub-cells" below; the depth is a launch argument, MESH_AMD_CUT_SUBDIV in cut_level).
// The ball rule is the triangle inequality on two distances from c; it ignores
// that, as q moves in the cell, the distance to a box B and the distance to c's closest point pc move almost together.
// Let a_k (k = 0, 1, 2) be the node's fp32 frame rows (n, t, b = n x t as frame_b rounds it) taken as exact reals, A
// the matrix of these rows, o the tree origin, and B = {x : lo_k <= a_k . (x - o) <= hi_k} the child's decoded box: a
// convex set that contains every vertex below the child (build.hip projects the fp64 vertices on these same widened
// axes and rounds every bound outward by at least an fp32 ulp, which covers its own fp64 roundings; looser is safe).
// With y = A (x - o) the box is axis-aligned, and since lambda_max(A A^T) <= 1 + 1e-6 (node_child_bounds; this is all
// the rule asks of the frame: neither unit rows nor right angles), |A v| <= (1 + 1e-6)^(1/2) |v|, hence
//   dist(x, B) >= k D(x),  D(x) = the distance from A (x - o) to the axis-aligned box [lo, hi],  k = 1 - 1e-6.
// Take F(x) = k D(x) - |x - pc| <= dist(x, B) - |x - pc|.  Where D > 0 and x != pc it is differentiable with
//   grad F(x) = k A^T u(x) - v(x),  u = g / |g| (g the signed slab-gap vector of A (x - o)),  v = (x - pc) / |x - pc|.
// g is 1-Lipschitz in y (y minus its projection on a convex set) and normalising costs at most a factor 2 / length
// (|a/|a| - b/|b|| <= 2 |a - b| / max(|a|, |b|)), so along the segment from c to any x with |x - c| = s <= r
//   |grad F(x) - grad F(c)| <= 2 k lambda_max s / D(c) + 2 s / |c - pc| <= 4 s / d_B + 2 s / d_p,
// d_B = D(c), d_p = |c - pc|, provided D > 0 and x != pc on the segment: D(x) >= d_B - (1 + 1e-6) r and
// |x - pc| >= d_p - r, so the rule is tried only when d_B > r (1 + 1e-5) and d_p > r (1 + 1e-5).  Integrating,
//   F(q) >= F(c) - r (|grad F(c)| + 4 r / d_B + 2 r / d_p)   for every q within r of c
// (every q of the cell: r is its half-diagonal + 0.1 %, which also covers the rounding of cut_cell's cell index).
// When the right side exceeds the margin m > 0, every q of the cell has
//   dist(q, any face below the child) >= dist(q, B) >= F(q) + |q - pc| > |q - pc| + m >= d(q) + m:
// the subtree holds neither q's answer nor a tie, and the walk's result is unchanged bit for bit.
// The margin m = 2^-40 (|c - o|_1 + |pc - o|_1 + d_B + d_p) stands for everything computed rather than exact: the
// left side is ~40 fp64 operations on operands no larger than those four magnitudes, each rounding <= 2^-53 of
// them (no cancellation is relied on: the differences are bounded by the operands), so its error is < 2^-46 of the
// sum; pc is the centre walk's fp64 construction, within a few 2^-53 |pc - o| of a true mesh point; and the walks
// compare squared distances computed to a few 2^-53 relative, so a face farther by m > 2^-41 d(q) can neither win
// nor tie in their arithmetic.  The inequality is strict.  The test is OR-ed with the ball rule (it only drops
// children the ball rule kept), the stored entry bounds keep their formula, and a fine cell may still start from
// its coarse cell's record: a drop proved for every q of the coarse cell holds for the fine cell's.
// The alongnormal walks (rays.hip k_rays<0>) read a record as "every face within R of c is below the list", which a
// directional drop breaks: such a record is flagged -- kCutDirFlag in word 0 of a 32-B record, word 1 (the radius) 0
// in a 64-B one -- and inherits the flag of the coarse record it starts from; a ray in a flagged cell starts at the
// root.  The closest-point walks mask the flag (cut_hint_leaf).  nflag: the number of flagged cells.
//
// Sub-cells (round 12).  Nothing above uses that the expansion point is the cell's centre, nor that pc is that point's
// own closest point.  For any point x0 and radius rho, with d_B = D(x0) > rho (1 + 1e-5) and
// d_p = |x0 - pc| > rho (1 + 1e-5), the same integration along the segments from x0 gives
//   F(q) >= F(x0) - rho (|grad F(x0)| + 4 rho / d_B + 2 rho / d_p)   for every q within rho of x0,
// and the last step needs of pc only that it is a point of the mesh: |q - pc| >= d(q), so F(q) > m still gives
// dist(q, any face below the child) > d(q) + m.  The first-order term halves with rho and the other two quarter, so a
// child the whole cell cannot drop may still be dropped piece by piece: when the test fails on (c, r) it is tried on
// the cell's 8 octants -- centres c +- w / 4 per axis, radius r / 2 -- and an octant that fails on its own 8 octants
// (radius r / 4), down to depth kCutSubdiv; the child is dropped only if every piece proves it.  The pieces' balls
// cover what the cell's ball had to: an octant's half-diagonal is |w| / 4 and its ball's radius |w| / 4 + 0.1 %, so
// the balls of a level cover the cell widened by 0.1 % of the piece's size, ~2.5e-4 of a cell width at depth 2.  The
// centres are formed in fp64 (c, then +- w / 4, +- w / 8: each within 2^-51 of the grid's extent of its exact
// place), and cut_cell assigns q to a cell from (q - lo) (1 / w) in fp64, wrong by at most a few 2^-52 of G cell
// widths: both are below 1e-12 of a cell width for any G this library builds (G^3 < 2^32), against the 2.5e-4 to
// spare.  Each piece takes its own guards and its own margin m = 2^-40 (|x0 - o|_1 + |pc - o|_1 + d_B + d_p) with its
// own d_B and d_p: the same ~40 operations on operands no larger than these.  A child whose fp32 bound from c is
// within d_p(c)^2 is tried on no piece (the caller's s0 / s1): c lies in the ball of every octant, so F(c) <= 0
// fails the first octant it meets, at either depth.  A drop proved piece by piece is a drop proved for every q of
// the cell, so what is said above of coarse records, flags and the alongnormal walks holds unchanged.
//
// The ball of one test: the expansion point relative to the tree origin, v = (x0 - pc) / d_p, d_p, the radius,
// r2p = 2 rho^2 / d_p, and mag = |x0 - o|_1 + |pc - o|_1 + d_p.
struct CutBall {
    D3 xo, vp;
    double dp, rho, r2p, mag;
};
// k_cut_level<*, true>'s grid argument: G below this bit (a grid has at most 2^32 cells, entrycut.cpp build_entry_cut, so
// G < 1626), the depth above
constexpr int kCutSubShift = 24;
// whether the rule proves on ball b that the child with frame ax and box [e[0..2], e[3..5]] can be dropped
__device__ inline bool cut_ball_drops(const float (&ax)[3][3], const float (&e)[6], const CutBall& b) {
    const double kf = 1.0 - 1e-6;
    double g[3], d2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double p = (double)ax[k][0] * b.xo.x + (double)ax[k][1] * b.xo.y + (double)ax[k][2] * b.xo.z;
        const double lo = (double)e[k], hi = (double)e[3 + k];
        g[k] = p < lo ? p - lo : (p > hi ? p - hi : 0.0);
        d2 += g[k] * g[k];
    }
    const double dB = sqrt(d2);
    if (!(dB > b.rho * (1.0 + 1e-5))) return false;       // also NaN / a non-finite box
    if (!(kf * dB - b.dp - b.r2p > 0.0)) return false;    // the common case near the foot point: no gradient needed
    const double inv = 1.0 / dB, ks = kf * inv;
    const D3 w = D3{ks * ((double)ax[0][0] * g[0] + (double)ax[1][0] * g[1] + (double)ax[2][0] * g[2]) - b.vp.x,
                    ks * ((double)ax[0][1] * g[0] + (double)ax[1][1] * g[1] + (double)ax[2][1] * g[2]) - b.vp.y,
                    ks * ((double)ax[0][2] * g[0] + (double)ax[1][2] * g[1] + (double)ax[2][2] * g[2]) - b.vp.z};
    const double lhs = kf * dB - b.dp - b.rho * (sqrt(vdot(w, w)) + 4.0 * b.rho * inv) - b.r2p;
    return lhs > 9.094947017729282e-13 * (b.mag + dB);  // 2^-40
}
// Both children at once (they share the frame); h0 / h1: in, the child passed the ball rule; out, it also survives
// this one.  cell: the whole cell's ball (c, r).  s0 / s1: the child may be tried on sub-cells, down to depth subdiv
// (0: the whole cell only); pco = pc - o, pmag = |pc - o|_1, qw = w / 4.  Returns whether a child was dropped.
__device__ inline bool cut_dir_drop(const NodeV& nd, bool& h0, bool& h1, bool s0, bool s1, const CutBall& cell,
                                    const D3& pco, double pmag, const D3& qw, int subdiv) {
    float ax[3][3], e0[6], e1[6];
    nd.frame(ax[0], ax[1], ax[2]);
    nd.extents(e0, e1);
    bool dropped = false;
    if (h0 && cut_ball_drops(ax, e0, cell)) {
        h0 = false;
        dropped = true;
    }
    if (h1 && cut_ball_drops(ax, e1, cell)) {
        h1 = false;
        dropped = true;
    }
    if (subdiv < 1) return dropped;
    // (this kernel runs once per kept tree: one copy of the test in a loop over sides and pieces, not 2 x 16 copies)
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
        if (!(side ? h1 && s1 : h0 && s0)) continue;
        float e[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) e[k] = side ? e1[k] : e0[k];
        // octant o of the cell, then (sub >= 0) octant sub of that octant; the child survives at the first piece
        // that fails at full depth
        int o = 0, sub = -1;
        while (o < 8) {
            const double f1 = sub < 0 ? 0.0 : 0.5;
            CutBall b;
            b.xo = D3{cell.xo.x + ((o & 1) ? qw.x : -qw.x) + f1 * ((sub & 1) ? qw.x : -qw.x),
                      cell.xo.y + ((o & 2) ? qw.y : -qw.y) + f1 * ((sub & 2) ? qw.y : -qw.y),
                      cell.xo.z + ((o & 4) ? qw.z : -qw.z) + f1 * ((sub & 4) ? qw.z : -qw.z)};
            b.rho = cell.rho * (sub < 0 ? 0.5 : 0.25);
            const D3 d = vsub(b.xo, pco);
            b.dp = sqrt(vdot(d, d));
            bool ok = b.dp > b.rho * (1.0 + 1e-5) && b.dp < INFINITY;
            if (ok) {
                b.vp = D3{d.x / b.dp, d.y / b.dp, d.z / b.dp};
                b.r2p = 2.0 * b.rho * b.rho / b.dp;
                b.mag = fabs(b.xo.x) + fabs(b.xo.y) + fabs(b.xo.z) + pmag + b.dp;
                ok = cut_ball_drops(ax, e, b);
            }
            if (sub < 0) {
                if (ok)
                    ++o;
                else if (subdiv < 2)
                    break;
                else
                    sub = 0;
            } else {
                if (!ok) break;
                if (++sub == 8) {
                    sub = -1;
                    ++o;
                }
            }
        }
        if (o == 8) {
            (side ? h1 : h0) = false;
            dropped = true;
        }
    }
    return dropped;
}
// DIR: with the directional drop (its fp64 work doubles the kernel's registers, so the ball-rule-only launches of the
// automatic coarse grid keep their own instantiation: C3 3.7 ms against 5.0 ms as a launch argument), proved on
// sub-cells down to the depth that rides in the grid argument: Gs = G + (depth << kCutSubShift) for DIR, plain G
// otherwise.  (An argument of its own would rename the ball-rule instantiations too, and a shared body inlined into
// two kernels compiles them differently: packed, the ball-rule kernels' code is the previous round's, instruction
// for instruction, scripts/isa_check.py --diff.)
template <bool E4, bool DIR>
__global__ __launch_bounds__(kBlock) void k_cut_level(const BNode* __restrict__ nodes, const TriRec* __restrict__ tris,
                                                      double ox, double oy, double oz, double tm, int Gs, double lx,
                                                      double ly, double lz, double wx, double wy, double wz,
                                                      const double* __restrict__ pts, const int* __restrict__ hint,
                                                      uint32_t* __restrict__ rec, const uint32_t* __restrict__ crec,
                                                      unsigned long long* __restrict__ nflag) {
    const int G = DIR ? Gs & ((1 << kCutSubShift) - 1) : Gs;
    const int subdiv = DIR ? Gs >> kCutSubShift : 0;
    constexpr int kw = E4 ? 8 : 16;  // record words
    // a wave takes a 4 x 4 x 4 brick of cells (bricks in row order): its cells' start lists share their nodes, and
    // under a half-resolution grid it reads 8 records
    const size_t gid = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t GB = ((size_t)G + 3) / 4, brick = gid >> 6;
    const unsigned ln = (unsigned)(gid & 63);
    if (brick >= GB * GB * GB) return;
    const size_t ix = (brick % GB) * 4 + (ln & 3), iy = ((brick / GB) % GB) * 4 + ((ln >> 2) & 3),
                 iz = (brick / (GB * GB)) * 4 + (ln >> 4);
    if (ix >= (size_t)G || iy >= (size_t)G || iz >= (size_t)G) return;
    const size_t cell = (iz * G + iy) * G + ix;
    const D3 c = D3{lx + ((double)ix + 0.5) * wx, ly + ((double)iy + 0.5) * wy, lz + ((double)iz + 0.5) * wz};
    const double r = 0.5 * sqrt(wx * wx + wy * wy + wz * wz) * 1.001;
    int ref[kCutK];
    float bd[kCutK];  // bound from c; -1: not formed yet (the root)
    int stuck[kCutK];  // list size at which the entry could not be expanded (0: not stuck): retried only once smaller
    const int best_leaf = hint[cell];
    ref[0] = 0;
    bd[0] = -1.f;
    stuck[0] = 0;
    int m = 1;
    // U(c): the distance from c to its answer's point (pts: the centre walks' closest points; NaN without an answer)
    const D3 pc = D3{pts[3 * cell], pts[3 * cell + 1], pts[3 * cell + 2]};
    float limf = INFINITY;
    const double dp = sqrt(sqdist(c, pc));
    {
        const double R = (dp + 2.0 * r) * (1.0 + 1e-6);
        if (R < INFINITY) limf = __double2float_ru(R * R * kSlack);  // NaN / inf (no answer): the root only
    }
    // the directional drop's constants (cut_dir_drop): c and pc relative to the origin, v = (c - pc) / d_p
    const D3 co = D3{c.x - ox, c.y - oy, c.z - oz};
    const bool dir = DIR && dp > r * (1.0 + 1e-5) && dp < INFINITY;
    const float dp2f = __double2float_rd(dp * dp);
    const D3 pco = D3{pc.x - ox, pc.y - oy, pc.z - oz};
    const double pmag = fabs(pco.x) + fabs(pco.y) + fabs(pco.z);
    const CutBall ball = CutBall{co, D3{(c.x - pc.x) / dp, (c.y - pc.y) / dp, (c.z - pc.z) / dp}, dp, r, 2.0 * r * r / dp,
                                 fabs(co.x) + fabs(co.y) + fabs(co.z) + pmag + dp};
    const D3 qw = D3{0.25 * wx, 0.25 * wy, 0.25 * wz};  // the octants' centres: c +- w / 4
    bool flagged = false;  // a directional drop removed what the ball rule kept (here or in the coarse record)
    if (crec) {
        // start from the enclosing cell of the half-resolution grid (G = 2 Gc, the same box): a subtree its record left
        // out lies farther than d(q) from every q of that cell, this one's included.  Its entries keep their records'
        // bounds -- already lower bounds for every q of the larger cell -- as (sqrt(b) + r)^2, which the store below
        // maps back to <= sqrt(b); a node's bound is raised when it is loaded
        const size_t Gc = (size_t)G / 2;
        const uint32_t* cr = crec + (((iz >> 1) * Gc + (iy >> 1)) * Gc + (ix >> 1)) * kw;
        flagged = E4 ? ((int)cr[0] >= 0 && (cr[0] & kCutDirFlag)) : cr[1] == 0u;
        m = 0;
        for (int k = 0; k < kCutK; ++k) {
            uint32_t rv, bb;
            if (E4) {
                const uint32_t e = cr[1 + k];
                if (e & 0x80000000u) break;  // empty: the list ends
                rv = (uint32_t)Ent4::ref(e);
                bb = __float_as_uint(Ent4::bound(e));
            } else {
                rv = cr[2 + 2 * k];
                if (rv == kCutEmpty) break;
                bb = cr[3 + 2 * k];
            }
            if (__uint_as_float(bb) > limf) continue;  // farther than R from c (its bound holds from c too)
            const float sb = sqrtf(__uint_as_float(bb)) + (float)r;
            ref[m] = (int)rv;
            bd[m] = sb * sb;  // its rounding is far inside the store's 1e-5 shrink
            stuck[m] = 0;
            ++m;
        }
        if (m == 0) {
            ref[0] = 0;
            bd[0] = -1.f;
            m = 1;
        }
    }
    const double o3[3] = {ox, oy, oz};
    const QF qf = make_qf(c, o3, tm);
    if (m > 0 && limf < INFINITY) {
        for (int pass = 0; pass < 256; ++pass) {
            bool changed = false;
            const int m0 = m;
            for (int k = 0; k < m0 && k < m; ++k) {
                if (ref[k] < 0) continue;  // a leaf: final, with its box bound
                if (stuck[k] && m >= stuck[k]) continue;  // no room has been freed since it was stuck: no reload
                const NodeV nd = load_node(nodes, ref[k]);
                float d0, d1;
                node_child_bounds(nd, qf, d0, d1);
                bd[k] = fmaxf(bd[k], fminf(d0, d1));
                bool h0 = d0 <= limf, h1 = d1 <= limf;
                // (a child whose fp32 bound is within d_p^2 is not tried: the rule needs d_B > d_p; skipping is safe)
                const bool s0 = h0 && d0 > dp2f, s1 = h1 && d1 > dp2f;
                if (dir && (s0 || s1) && cut_dir_drop(nd, h0, h1, s0, s1, ball, pco, pmag, qw, subdiv)) flagged = true;
                const int cnt = (int)h0 + (int)h1;
                if (m - 1 + cnt > kCutK) {
                    stuck[k] = m;
                    continue;
                }
                changed = true;
                if (cnt == 0) {  // nothing within R below this entry
                    ref[k] = ref[m - 1];
                    bd[k] = bd[m - 1];
                    stuck[k] = stuck[m - 1];
                    --m;
                    continue;
                }
                const int c0 = nd.child(0), c1 = nd.child(1);
                stuck[k] = 0;
                if (h0) {
                    ref[k] = c0;
                    bd[k] = d0;
                    if (h1) {
                        ref[m] = c1;
                        bd[m] = d1;
                        stuck[m] = 0;
                        ++m;
                    }
                } else {
                    ref[k] = c1;
                    bd[k] = d1;
                }
            }
            if (!changed || m == 0) break;
        }
    }
    if (m == 0) {  // no answer for c, or (cannot happen for a consistent tree) nothing within R: the root
        ref[0] = 0;
        bd[0] = 0.f;
        m = 1;
    }
    for (int k = 1; k < m; ++k)  // nearest first
        for (int j = k; j > 0 && bd[j] < bd[j - 1]; --j) {
            const int tr = ref[j];
            ref[j] = ref[j - 1];
            ref[j - 1] = tr;
            const float tb = bd[j];
            bd[j] = bd[j - 1];
            bd[j - 1] = tb;
        }
    uint32_t* out = rec + cell * kw;
    out[0] = (uint32_t)best_leaf | (E4 && flagged && best_leaf >= 0 ? kCutDirFlag : 0u);
    // 64-B records: word 1 the radius R around c the list covers (every subtree left out lies farther from c), fp32
    // rounded down (0: none, or a flagged record) -- the alongnormal walks' first phase reads it (rays.hip)
    if (!E4)
        out[1] = limf < INFINITY && !flagged
                     ? __float_as_uint(__double2float_rd(sqrt((double)limf / kSlack) * (1.0 - 1e-7)))
                     : 0u;
    if (nflag) {
        const unsigned long long fl = __ballot(flagged);
        if (flagged && (unsigned)__ffsll((long long)fl) - 1u == ln) atomicAdd(nflag, (unsigned long long)__popcll(fl));
    }
    for (int k = 0; k < kCutK; ++k) {
        uint32_t ev = 0xFFFFFFFFu, rv = kCutEmpty, bb = 0u;
        if (k < m) {
            const double b = bd[k] > 0.f ? (double)bd[k] : 0.0;
            const double sv = sqrt(b) * (1.0 - 1e-5) - r * (1.0 + 1e-5);
            bb = __float_as_uint(sv > 0.0 ? __double2float_rd(sv * sv) : 0.f);
            ev = Ent4::make((uint32_t)ref[k], bb);
            rv = (uint32_t)ref[k];
        }
        if (E4) {
            out[1 + k] = ev;
        } else {
            out[2 + 2 * k] = rv;
            out[3 + 2 * k] = bb;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_face_leaf(const TriRec* __restrict__ tris, size_t T, uint32_t* __restrict__ inv) {
    const size_t l = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= T) return;
    D3 x, y, z;
    uint32_t face;
    load_tri(tris, (int)l, x, y, z, face);
    if (face < T) inv[face] = (uint32_t)l;
}
__global__ __launch_bounds__(kBlock) void k_cut_hint(const uint32_t* __restrict__ face, size_t n, size_t T,
                                                     const uint32_t* __restrict__ inv, int* __restrict__ hint) {
    const size_t c = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n) return;
    const uint32_t f = face[c];
    hint[c] = f < T ? (int)inv[f] : -1;
}

// The closest point and part code of each row on a GIVEN face: the fp64 construction the traversal's answer store
// runs for its winning face (write_result), so for a row the traversal answered with face f this gives the
// traversal's point and part bit for bit.  Rows with face MSH_NO_FACE (or >= T) get NaN and part 0, as the
// traversal's non-finite rows do.  The narrow result exchange (mesh_amd/distributed.py NarrowRing) all-gathers
// faces only and rebuilds the other ranks' points with it.  inv: face -> leaf (k_face_leaf).
__global__ __launch_bounds__(kBlock) void k_points_from_faces(const TriRec* __restrict__ tris, const uint32_t* __restrict__ inv,
                                                              size_t T, const double* __restrict__ q, size_t S,
                                                              const uint32_t* __restrict__ face, uint32_t* __restrict__ part,
                                                              double* __restrict__ pt) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= S) return;
    const uint32_t f = face[i];
    D3 o = D3{NAN, NAN, NAN};
    int pc = 0;
    if (f < T) {
        D3 ta, tb, tc;
        uint32_t ff;
        load_tri(tris, (int)inv[f], ta, tb, tc, ff);
        closest_on_triangle(D3{q[3 * i], q[3 * i + 1], q[3 * i + 2]}, ta, tb, tc, o, pc);
    }
    if (part) part[i] = (uint32_t)pc;
    pt[3 * i] = o.x;
    pt[3 * i + 1] = o.y;
    pt[3 * i + 2] = o.z;
}

int face_leaf_map(const msh_tree* tree, uint32_t* d_inv, hipStream_t s) {
    const size_t T = tree->T;
    k_face_leaf<<<blocks_for(T), kBlock, 0, s>>>(static_cast<const TriRec*>(tree->d_leaves), T,
                                                                          d_inv);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int points_from_faces(const msh_tree* tree, const uint32_t* d_inv, const double* d_q, size_t S, const uint32_t* d_face,
                      uint32_t* d_part, double* d_pt, hipStream_t s) {
    if (S == 0) return MSH_OK;
    TimedLaunch tl("points_from_faces", s);
    k_points_from_faces<<<blocks_for(S), kBlock, 0, s>>>(
        static_cast<const TriRec*>(tree->d_leaves), d_inv, tree->T, d_q, S, d_face, d_part, d_pt);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int cut_hints(const msh_tree* tree, const uint32_t* d_face, size_t n, uint32_t* d_inv, int* d_hint, hipStream_t s) {
    const size_t T = tree->T;
    k_face_leaf<<<blocks_for(T), kBlock, 0, s>>>(static_cast<const TriRec*>(tree->d_leaves), T,
                                                                          d_inv);
    MSH_HIP(hipGetLastError());
    k_cut_hint<<<blocks_for(n), kBlock, 0, s>>>(d_face, n, T, d_inv, d_hint);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int cut_centres(int G, const double* lo, const double* w, double* d_q, hipStream_t s) {
    const size_t n = (size_t)G * G * G;
    k_cut_centres<<<blocks_for(n), kBlock, 0, s>>>(G, lo[0], lo[1], lo[2], w[0], w[1], w[2], d_q);
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

int cut_level(const msh_tree* tree, int G, const double* lo, const double* w, const double* d_pts, const int* d_hint,
              uint32_t* d_rec, bool e4, hipStream_t s, const uint32_t* d_half, unsigned long long* d_nflag,
              int subdiv) {
    const size_t GB = ((size_t)G + 3) / 4;  // 4^3-cell bricks, one per wave
    const unsigned nb = blocks_for(GB * GB * GB * 64);
    const TriRec* tris = static_cast<const TriRec*>(tree->d_leaves);
    const double tm = tree_margin(tree->half_diag);
    TimedLaunch tl("cut_level", s);
    auto launch = [&](auto kern, int Gs) {
        kern<<<nb, kBlock, 0, s>>>(tree->d_nodes, tris, tree->origin[0], tree->origin[1], tree->origin[2], tm, Gs, lo[0],
                                   lo[1], lo[2], w[0], w[1], w[2], d_pts, d_hint, d_rec, d_half, d_nflag);
    };
    if (subdiv >= 0) {
        // test hook: the sub-cell depth of the directional drop, 0 (the whole cell only) to kCutSubdiv
        const char* e = getenv("MESH_AMD_CUT_SUBDIV");
        const int depth = std::max(0, std::min(e ? atoi(e) : subdiv, kCutSubdiv));
        const int Gs = G + (depth << kCutSubShift);
        e4 ? launch(k_cut_level<true, true>, Gs) : launch(k_cut_level<false, true>, Gs);
    } else {
        e4 ? launch(k_cut_level<true, false>, G) : launch(k_cut_level<false, false>, G);
    }
    MSH_HIP(hipGetLastError());
    return MSH_OK;
}

}  // namespace msh
