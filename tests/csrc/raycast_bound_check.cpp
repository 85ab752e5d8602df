// Host property test of the ray-casting node test (mesh_amd/csrc/common.h make_rayf_range + ray_child_first_key, and
// ray_child_slabs on the same ranged model): for nodes whose decoded oriented boxes contain their points (the build's
// contract; the node generator is bound_check.cpp's), a ray o + t d through a point x = o + t* d of a child, with a
// parameter range [t0, t1] that holds t*, must take that child -- also with t* exactly at t0, at t1, or both -- and the
// child's first-hit key must be <= t* L, L = |d| (the model's parameter of the point).  Random frames, point clouds
// and rays at every scale and offset, directions of any length, along a frame axis or grazing a face.  Prints
// "violations=N" (and the worst cases) and exits 1 when N > 0.  -DMUTATE_RAYCAST_KEY takes the key from the far end
// of the child's interval: that build must fail (the test's sensitivity check, tests/test_raycast_host.py).
//   hipcc -O2 -std=c++17 -ffp-contract=off -x hip raycast_bound_check.cpp -I<csrc> -o rbc && ./rbc 300000
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "common.h"

using namespace msh;

namespace {

// tightest valid 8-bit code for a bound v against base / scale: dequant(lo code) <= v <= dequant(hi code)
uint32_t code_lo(double v, float base, float sc) {
    double c = std::floor((v - (double)base) / (double)sc);
    uint32_t u = (uint32_t)std::fmin(std::fmax(c, 0.0), 255.0);
    while (u > 0u && (double)dequant(u, sc, base) > v) --u;
    while (u < 255u && (double)dequant(u + 1, sc, base) <= v) ++u;
    return u;
}
uint32_t code_hi(double v, float base, float sc) {
    double c = std::ceil((v - (double)base) / (double)sc);
    uint32_t u = (uint32_t)std::fmin(std::fmax(c, 0.0), 255.0);
    while (u < 255u && (double)dequant(u, sc, base) < v) ++u;
    while (u > 0u && (double)dequant(u - 1, sc, base) >= v) --u;
    return u;
}

}  // namespace

int main(int argc, char** argv) {
    const long trials = argc > 1 ? std::atol(argv[1]) : 100000;
    std::mt19937_64 rng(54321);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    auto unit = [&]() {
        for (;;) {
            double x = U(rng), y = U(rng), z = U(rng);
            double l = std::sqrt(x * x + y * y + z * z);
            if (l > 0.1 && l <= 1.0) return D3{x / l, y / l, z / l};
        }
    };
    long viol = 0, skipped = 0, checks = 0, ray_skipped = 0, take_viol = 0, key_viol = 0, tight = 0, at_end = 0;
    for (long tr = 0; tr < trials; ++tr) {
        // scene scale, node size relative to it, offset of the tree origin
        const double S = std::pow(10.0, (int)(rng() % 7) - 3);         // 1e-3 .. 1e3
        const double node = S * std::pow(10.0, -(double)(rng() % 7));  // node size S .. 1e-6 S
        const double off = (rng() % 3 == 0) ? 0.0 : S * std::pow(10.0, (double)(rng() % 6));
        const double origin[3] = {off * U(rng), off * U(rng), off * U(rng)};
        const bool at_origin = tr % 4 == 0;  // the node centred on the tree origin, child 0 below and child 1 above t = 0
        const D3 c = at_origin ? D3{0, 0, 0} : D3{S * U(rng), S * U(rng), S * U(rng)};
        // frame as the build makes it: unit n, t = e - (e.n) n normalised, b = n x t in fp32
        const D3 n = unit();
        const D3 e = std::fabs(n.x) < 0.9 ? D3{1, 0, 0} : D3{0, 1, 0};
        D3 t = vsub(e, vscale(vdot(e, n), n));
        const double tl = std::sqrt(vdot(t, t));
        t = D3{t.x / tl, t.y / tl, t.z / tl};
        float nf[3] = {(float)n.x, (float)n.y, (float)n.z}, tf[3] = {(float)t.x, (float)t.y, (float)t.z}, bf[3];
        frame_b(nf, tf, bf);
        const double A[3][3] = {{nf[0], nf[1], nf[2]}, {tf[0], tf[1], tf[2]}, {bf[0], bf[1], bf[2]}};
        // two children: 6 points each, flattened along n like surface patches (absolute fp64 coordinates)
        D3 pts[2][6];
        double mn[2][3], mx[2][3];
        double half_diag = 0.0;
        for (int ch = 0; ch < 2; ++ch) {
            for (int k = 0; k < 3; ++k) { mn[ch][k] = INFINITY; mx[ch][k] = -INFINITY; }
            for (int i = 0; i < 6; ++i) {
                double a = node * U(rng);
                const double b = node * U(rng), h = node * 1e-3 * U(rng);
                if (at_origin) a = ch == 0 ? -std::fabs(a) : std::fabs(a);
                const D3 r = D3{c.x + a * t.x + b * (n.y * t.z - n.z * t.y) + h * n.x,
                                c.y + a * t.y + b * (n.z * t.x - n.x * t.z) + h * n.y,
                                c.z + a * t.z + b * (n.x * t.y - n.y * t.x) + h * n.z};
                pts[ch][i] = D3{origin[0] + r.x, origin[1] + r.y, origin[2] + r.z};
                const double rx = pts[ch][i].x - origin[0], ry = pts[ch][i].y - origin[1], rz = pts[ch][i].z - origin[2];
                half_diag = std::fmax(half_diag, std::sqrt(rx * rx + ry * ry + rz * rz));
                for (int k = 0; k < 3; ++k) {
                    const double pr = A[k][0] * rx + A[k][1] * ry + A[k][2] * rz;
                    mn[ch][k] = std::fmin(mn[ch][k], pr);
                    mx[ch][k] = std::fmax(mx[ch][k], pr);
                }
            }
        }
        // the build first rounds each bound outward to fp32 (build.hip out_lo / out_hi)
        for (int ch = 0; ch < 2; ++ch)
            for (int k = 0; k < 3; ++k) {
                float lo = (float)mn[ch][k], hi = (float)mx[ch][k];
                if ((double)lo > mn[ch][k]) lo = nextafterf(lo, -INFINITY);
                if ((double)hi < mx[ch][k]) hi = nextafterf(hi, INFINITY);
                mn[ch][k] = lo;
                mx[ch][k] = hi;
            }
        // node encoding: fp32 base below both children, bf16 scale (build.hip encode_node), tightest codes
        BNode bn;
        std::memset(&bn, 0, sizeof(bn));
        float* f = bn.f;
        encode_frame(f, nf, tf);
        f[6] = u2f(~0u);
        f[7] = u2f(~1u);
        uint32_t u[12];
        float scs[3];
        for (int k = 0; k < 3; ++k) {
            float base = (float)std::fmin(mn[0][k], mn[1][k]);
            if ((double)base > std::fmin(mn[0][k], mn[1][k])) base = nextafterf(base, -INFINITY);
            const double range = std::fmax(mx[0][k], mx[1][k]) - (double)base;
            const float sc = bf16_scale_up(range);
            f[kBase + k] = base;
            scs[k] = sc;
            for (int ch = 0; ch < 2; ++ch) {
                u[6 * ch + k] = code_lo(mn[ch][k], base, sc);
                u[6 * ch + 3 + k] = code_hi(mx[ch][k], base, sc);
            }
        }
        for (int j = 0; j < 3; ++j) f[11 + j] = u2f(u[4 * j] | (u[4 * j + 1] << 8) | (u[4 * j + 2] << 16) | (u[4 * j + 3] << 24));
        encode_scales(f, scs);
        NodeV nd;
        std::memcpy(&nd, &bn, sizeof(bn));
        // the decoded boxes must contain the points (what the build guarantees)
        float e0[6], e1[6];
        nd.extents(e0, e1);
        bool ok = true;
        for (int k = 0; k < 3; ++k)
            ok = ok && (double)e0[k] <= mn[0][k] && (double)e0[3 + k] >= mx[0][k] && (double)e1[k] <= mn[1][k] &&
                 (double)e1[3 + k] >= mx[1][k];
        if (!ok) {
            ++skipped;
            continue;
        }
        const double M = half_diag * (1.0 + 1e-9);
        for (int ri = 0; ri < 8; ++ri) {
            const int ch = (int)(rng() % 2);
            const D3 x = pts[ch][rng() % 6];
            // direction: random, along a frame axis (parallel to two slab pairs), grazing the n = const faces; any length
            const int dk = (int)(rng() % 3);
            D3 d = unit();
            if (dk == 1) {
                const int ax = (int)(rng() % 3);
                d = D3{A[ax][0], A[ax][1], A[ax][2]};
            } else if (dk == 2) {
                const double g = std::pow(10.0, -(double)(3 + rng() % 8)) * U(rng);
                d = D3{A[1][0] + g * A[0][0], A[1][1] + g * A[0][1], A[1][2] + g * A[0][2]};
            }
            if (rng() % 2 == 0) d = vscale(std::pow(10.0, (double)((int)(rng() % 13) - 6)), d);
            // the point's distance from the origin of the ray: 0, within the node, up to 1e3 scene sizes
            const int sk = (int)(rng() % 4);
            const double dist = sk == 0 ? 0.0 : (sk == 1 ? node * std::pow(10.0, -(double)(rng() % 8))
                                                         : S * std::pow(10.0, (double)(rng() % 4)));
            const double ts = dist / std::sqrt(vdot(d, d));  // t*
            const D3 o = D3{x.x - ts * d.x, x.y - ts * d.y, x.z - ts * d.z};
            // the rounded origin moves the ray off x by ~1 ulp of |o|: keep the rays whose point x' = o + t* d (long
            // double) still lies in the decoded box
            {
                const long double xr[3] = {(long double)o.x + (long double)ts * d.x - origin[0],
                                           (long double)o.y + (long double)ts * d.y - origin[1],
                                           (long double)o.z + (long double)ts * d.z - origin[2]};
                const float* ex = ch == 0 ? e0 : e1;
                bool in = true;
                for (int k = 0; k < 3; ++k) {
                    const long double pr = A[k][0] * xr[0] + A[k][1] * xr[1] + A[k][2] * xr[2];
                    in = in && pr >= (long double)ex[k] && pr <= (long double)ex[3 + k];
                }
                if (!in || sqrtl(xr[0] * xr[0] + xr[1] * xr[1] + xr[2] * xr[2]) > (long double)M) {
                    ++ray_skipped;
                    continue;
                }
            }
            // the row's range: the whole ray, t* at its start, at its end, both, strictly inside, a negative start
            const int rk = (int)(rng() % 6);
            const double w = ts * std::pow(10.0, -(double)(rng() % 16)) + (rng() % 2 ? 0.0 : std::pow(10.0, (double)((int)(rng() % 13) - 6)));
            double t0 = 0.0, t1 = INFINITY;
            if (rk == 1) { t0 = ts; t1 = ts + w; }
            else if (rk == 2) { t0 = std::fmax(ts - w, 0.0); t1 = ts; }
            else if (rk == 3) { t0 = ts; t1 = ts; }
            else if (rk == 4) { t0 = std::fmax(ts - w, 0.0); t1 = ts + w; }
            else if (rk == 5) { t0 = -w; t1 = rng() % 2 ? ts : INFINITY; }
            if (t0 == ts || t1 == ts) ++at_end;
            double L = 0.0;
            const RayF rf = make_rayf_range(D3{o.x - origin[0], o.y - origin[1], o.z - origin[2]}, d, M,
                                            std::fmax(t0, 0.0), t1, &L);
            bool h[2], hs[2];
            float k[2], s[2];
            ray_child_first_key(nd, rf, h[0], h[1], k[0], k[1]);
            ray_child_slabs(nd, rf, hs[0], hs[1], s[0], s[1]);
            const long double sstar = (long double)ts *
                sqrtl((long double)d.x * d.x + (long double)d.y * d.y + (long double)d.z * d.z);
            ++checks;
            if (h[ch] && sstar > 0 && (long double)k[ch] > 0.5L * sstar) ++tight;
            if (!h[ch] || !hs[ch]) {
                ++viol;
                ++take_viol;
                if (take_viol <= 5)
                    std::fprintf(stderr, "child not taken: dk=%d sk=%d rk=%d S=%g node=%g off=%g t*=%g t0=%g t1=%g\n", dk,
                                 sk, rk, S, node, off, ts, t0, t1);
            } else if (!((long double)k[ch] <= sstar)) {
                ++viol;
                ++key_viol;
                if (key_viol <= 5)
                    std::fprintf(stderr, "key violation: dk=%d sk=%d rk=%d key=%.9g s*=%.17Lg L=%g\n", dk, sk, rk, k[ch],
                                 sstar, L);
            }
        }
    }
    std::printf("at_range_end=%ld tight=%ld take_violations=%ld key_violations=%ld\n", at_end, tight, take_viol, key_viol);
    std::printf("trials=%ld skipped=%ld checks=%ld ray_skipped=%ld violations=%ld\n", trials, skipped, checks, ray_skipped,
                viol);
    return viol == 0 && skipped == 0 && checks > trials ? 0 : 1;
}
