// The shared device pieces of the ray kernels (rays.hip: nearest_alongnormal and visibility; raycast.hip: first-hit
// and occlusion queries for arbitrary rays): the closed ray-triangle predicate and CGAL's plane/line construction, the
// direction of a CGAL Ray_3, the policy-driven walk and the any-hit policy.  The ray semantics are described at the
// head of rays.hip.
#pragma once
#include "internal.h"

namespace msh {

__device__ inline double det3(const D3& a, const D3& b, const D3& c) { return vdot(vcross(a, b), c); }

// the ray's overlap with the triangle in its own plane, clipped starting from the parameter range [t0, t1]
__device__ inline bool coplanar_ray_tri(const D3& p, const D3& d, const D3& a, const D3& b, const D3& c, double& tout,
                                        double t0 = 0.0, double t1 = INFINITY) {
    const D3 n = vcross(vsub(b, a), vsub(c, a));
    if (n.x == 0.0 && n.y == 0.0 && n.z == 0.0) return false;
    double tlo = t0, thi = t1;
    const D3 v[3] = {a, b, c};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const D3& s = v[e];
        const D3& t = v[(e + 1) % 3];
        const D3 et = vsub(t, s);
        const double f0 = vdot(n, vcross(et, vsub(p, s)));
        const double f1 = vdot(n, vcross(et, d));
        if (f1 == 0.0) {
            if (f0 < 0.0) return false;
        } else {
            const double tt = -f0 / f1;
            if (f1 > 0.0) tlo = fmax(tlo, tt);
            else thi = fmin(thi, tt);
        }
    }
    if (tlo > thi) return false;
    tout = tlo;
    return true;
}

// 0: miss; 1: proper hit at parameter t; 2: coplanar hit entering at parameter t.  [t0, t1]: the closed parameter
// range of the ray (the whole ray by default)
__device__ inline int ray_tri(const D3& p, const D3& d, const D3& a, const D3& b, const D3& c, double& tout,
                              double t0 = 0.0, double t1 = INFINITY) {
    const D3 u = vsub(a, p), v = vsub(b, p), w = vsub(c, p);
    const double s0 = det3(u, v, d), s1 = det3(v, w, d), s2 = det3(w, u, d);
    const bool pos = s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0;
    const bool neg = s0 <= 0.0 && s1 <= 0.0 && s2 <= 0.0;
    if (!pos && !neg) return 0;
    const D3 n = vcross(vsub(b, a), vsub(c, a));
    const double num = vdot(n, u);
    const double den = vdot(n, d);
    if (den == 0.0 || (s0 == 0.0 && s1 == 0.0 && s2 == 0.0)) {
        if (num != 0.0) return 0;
        return coplanar_ray_tri(p, d, a, b, c, tout, t0, t1) ? 2 : 0;
    }
    const double t = num / den;
    if (t < t0 || t > t1) return 0;
    tout = t;
    return 1;
}

// CGAL intersection(Plane_3(a, b, c), Line_3(p, p + v)) with direction d = (p + v) - p; false if the
// line is parallel to the plane in this arithmetic
__device__ inline bool cgal_plane_line(const D3& p, const D3& d, const D3& a, const D3& b, const D3& c, D3& out) {
    double A, B, C, D;
    plane_of(a, b, c, A, B, C, D);
    const double num = A * p.x + B * p.y + C * p.z + D;
    const double den = A * d.x + B * d.y + C * d.z;
    if (den == 0.0) return false;
    out = D3{(den * p.x - num * d.x) / den, (den * p.y - num * d.y) / den, (den * p.z - num * d.z) / den};
    return true;
}

__device__ inline D3 ray_dir(const D3& p, const D3& v) { return vsub(vadd(p, v), p); }

// ---- generic traversal: the policy decides box hits (and ordering key) and leaf tests ----
template <class Pol, bool STATS>
__device__ inline void traverse_rays(const BNode* __restrict__ nodes, size_t T, Pol& pol, uint2* __restrict__ lds,
                                     uint2* __restrict__ spill, unsigned& n_nodes, unsigned& n_leaves) {
    if (T == 1) {
        pol.test(0);
        if (STATS) ++n_leaves;
        return;
    }
    int node = 0, sp = 0;
    for (size_t guard = 0; guard < T; ++guard) {
        const NodeV nd = load_node(nodes, node);
        if (STATS) ++n_nodes;
        bool h0, h1;
        float k0, k1;
        pol.children(nd, h0, h1, k0, k1);
        const int c0 = nd.child(0), c1 = nd.child(1);
        if (h0 && c0 < 0) {
            pol.test(~c0);
            if (STATS) ++n_leaves;
            h0 = false;
            if (pol.done()) return;
        }
        if (h1 && c1 < 0) {
            pol.test(~c1);
            if (STATS) ++n_leaves;
            h1 = false;
            if (pol.done()) return;
        }
        h0 = h0 && pol.keep(k0);
        h1 = h1 && pol.keep(k1);
        if (h0 && h1) {
            int nearc = c0, farc = c1;
            float kf = k1;
            if (k1 < k0) { nearc = c1; farc = c0; kf = k0; }
            const uint2 e = make_uint2((unsigned)farc, __float_as_uint(kf));
            stack_put(lds, spill, sp, e);
            ++sp;
            node = nearc;
            continue;
        }
        if (h0 || h1) {
            node = h0 ? c0 : c1;
            continue;
        }
        bool found = false;
        while (sp > 0) {
            --sp;
            const uint2 e = stack_get(lds, spill, sp);
            if (pol.keep(__uint_as_float(e.y))) {
                node = (int)e.x;
                found = true;
                break;
            }
        }
        if (!found) break;
    }
}

// any hit of the closed ray src + t d, t >= 0; key = entry parameter
struct AnyPol {
    const TriRec* __restrict__ tris;
    D3 src, d;
    RayF rf;
    bool hit;
    __device__ void children(const NodeV& nd, bool& h0, bool& h1, float& k0, float& k1) const {
        ray_child_slabs(nd, rf, h0, h1, k0, k1);
    }
    __device__ bool keep(float) const { return !hit; }
    __device__ bool done() const { return hit; }
    __device__ void test(int leaf) {
        D3 a, b, c;
        uint32_t face;
        load_tri(tris, leaf, a, b, c, face);
        double t;
        if (ray_tri(src, d, a, b, c, t)) hit = true;
    }
};

}  // namespace msh
