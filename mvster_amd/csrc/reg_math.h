// The Tanks and Temples evaluation protocol: the definition, shared by geo_reg.hip and the host build
// used only by the tests (tests/hostmath/reg_hostmath.cpp).  Like eval_math.h: IEEE fp64, one correctly rounded operation per
// step in the order written, contraction switched off for both compilers, so the kernels and the host build give the same bits.
//
// 1. Transform.  T [12] = the first three rows of a 4 x 4 matrix, row-major (the fourth row is 0 0 0 1: the caller checks it).
//    q_a = ((T[4a] * x + T[4a + 1] * y) + T[4a + 2] * z) + T[4a + 3] with x, y, z the float32 coordinates widened to fp64;
//    without a transform q = (double)p.  The moved point is (float)q, rounded to nearest.
//
// 2. Crop volume.  A prism: a polygon of P vertices (3 <= P <= 1024) in the plane of the axes (u, v), extruded along w from
//    axis_min to axis_max; (u, v, w) = (1, 2, 0) for the orthogonal axis X (0), (0, 2, 1) for Y (1), (0, 1, 2) for Z (2).  The
//    polygon comes as `poly` [P][2] = (u, v) of every vertex.  A point q (fp64) is inside iff every coordinate is finite,
//    axis_min <= q_w <= axis_max (both ends included) and an odd number of edges (j, k = (j + 1) mod P) both cross and have
//    node < q_u (strictly): an edge crosses iff (v_j < q_v && v_k >= q_v) || (v_k < q_v && v_j >= q_v), and
//    node = u_j + (q_v - v_j) / (v_k - v_j) * (u_k - u_j), evaluated left to right and only where the edge crosses (there
//    v_k != v_j, so the quotient is finite for a finite polygon).  The rule's values on vertices and edges are part of the
//    definition (the even-odd ray to -u; a vertex or edge belongs to the polygon only where that ray says so).
//
// 3. Correspondence sums.  For a moved source point s (float32, widened) with nearest target t (float32, widened) and squared
//    distance d2 (nn::dist2), the 18 terms of a pair, in the order of the output:
//      1, d2, s_0, s_1, s_2, t_0, t_1, t_2, (s_0 * s_0 + s_1 * s_1) + s_2 * s_2, t_a * s_b (a the row, b the column).
//    Products of two widened float32 are exact in fp64.  A pair counts iff the search gave it a target (index >= 0).  The sums
//    themselves are fp64 additions in an order the kernel fixes (lane, wave, workgroup, row): not part of this header.
//
// 4. Histogram.  edges [B + 1] fp64, non-decreasing; bin(d) = the largest k with edges[k] <= d, B - 1 for d == edges[B], and
//    none for d < edges[0], d > edges[B] or NaN: np.histogram(d, edges).
#pragma once
#include "nn_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace reg {

constexpr int kMinPolygon = 3, kMaxPolygon = 1024;
constexpr int kMaxBins = 4096;
constexpr int kSums = 18;

// q = T p (T [12]: three rows of four)
MV_HD void transform(const double* T, const float* p, double* q) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
}

MV_HD void widen(const float* p, double* q) {
    q[0] = (double)p[0];
    q[1] = (double)p[1];
    q[2] = (double)p[2];
}

// the axes of the polygon's plane and the one it is extruded along: 0 = X, 1 = Y, 2 = Z
MV_HD int axis_u(int axis) { return axis == 0 ? 1 : 0; }
MV_HD int axis_v(int axis) { return axis == 2 ? 1 : 2; }

MV_HD bool finite(double x) { return x - x == 0.0; }                        // false for NaN and +-inf

MV_HD bool edge_crosses(double vj, double vk, double qv) { return (vj < qv && vk >= qv) || (vk < qv && vj >= qv); }

MV_HD double edge_node(double uj, double vj, double uk, double vk, double qv) {
    return uj + (qv - vj) / (vk - vj) * (uk - uj);
}

// poly [P][2] = (u, v)
MV_HD bool inside(const double* q, int axis, double axis_min, double axis_max, const double* poly, int P) {
    if (!(finite(q[0]) && finite(q[1]) && finite(q[2]))) return false;
    const double qu = q[axis_u(axis)], qv = q[axis_v(axis)], qw = q[axis];
    if (!(qw >= axis_min && qw <= axis_max)) return false;
    bool odd = false;
    double uj = poly[2 * (P - 1)], vj = poly[2 * (P - 1) + 1];              // edge (P - 1, 0) first: the parity has no order
    for (int k = 0; k < P; ++k) {
        const double uk = poly[2 * k], vk = poly[2 * k + 1];
        if (edge_crosses(vj, vk, qv) && edge_node(uj, vj, uk, vk, qv) < qu) odd = !odd;
        uj = uk;
        vj = vk;
    }
    return odd;
}

// the 18 terms of one pair into term[]
MV_HD void pair_terms(const float* s, const float* t, double d2, double* term) {
    double a[3], b[3];
    widen(s, a);
    widen(t, b);
    term[0] = 1.0;
    term[1] = d2;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        term[2 + j] = a[j];
        term[5 + j] = b[j];
    }
    term[8] = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) term[9 + 3 * r + c] = b[r] * a[c];
    }
}

// -> the bin of d, -1 for none.  edges [B + 1] non-decreasing.  At most 13 steps for B <= 4096.
MV_HD int hist_bin(double d, const double* edges, int B) {
    if (!(d >= edges[0] && d <= edges[B])) return -1;                       // also NaN
    int lo = 0, hi = B;                                                     // edges[lo] <= d; the answer is in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (edges[mid] <= d) lo = mid;
        else hi = mid - 1;
    }
    return lo == B ? B - 1 : lo;
}

}  // namespace reg
