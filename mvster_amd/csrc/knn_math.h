// Cleaning a fused cloud: the k nearest points, the radius and the statistical outlier filter and the
// normals -- the definition, shared by geo_knn.hip and the host build used only by the tests (tests/hostmath/knn_hostmath.cpp).
// Like nn_math.h: IEEE fp64, one correctly rounded operation per step, only + - * / sqrt, contraction switched off for both
// compilers, so the kernels and the host build give the same bits.
//
// k nearest (k = 1 .. 32; max_dist, cell, validity and d2 as in nn_math.h).  The candidates of a valid query are the valid
// targets with d2 <= max_dist^2; with exclude_self (Q == M) the target whose index equals the query's own position is left out --
// only that one: a duplicate at the same coordinates with another index stays a candidate.  The result is the first
// min(k, candidates) candidates in ascending lexicographic (d2, index) order: dist2 [Q,k], index [Q,k], count [Q]; unfilled
// places hold +inf / -1; an invalid query gets NaN / -1 and count 0.  That is a brute force over all pairs: the result depends
// neither on cell, nor on the table, nor on the run.
//
// Grid: as in nn_math.h, own cell, then the shells r = 1 .. R, R = nn::rings(max_dist, cell).  A query may stop after shell
// r >= 1 once its list is full and its k-th d2 <= (r * cell)^2 * (1 - 2^-20).
//   Why: nn_math.h proves that the computed d2 of any target in a shell beyond r is strictly above (r * cell)^2 * (1 - 2^-20),
//   hence strictly above the k-th d2 of the full list: such a target is behind all k entries in the (d2, index) order whatever
//   its index, so it enters neither the list nor a tie at its end.  The bound R concerns candidates only and holds unchanged.
//
// Radius filter: neighbours(i) = the candidates of point i within `radius` with exclude_self, uncapped; keep iff the point is
// valid and neighbours(i) >= nb_points (Open3D counts the point itself and asks for > nb_points: the same rule).
//
// Statistical filter (PCL's rule with a search cap): a valid point takes part iff it has k candidates within max_dist
// (exclude_self); mean_i = (sum_j sqrt(d2_ij)) / k summed in the list's order; isolated points have mean +inf, invalid ones NaN.
// Over the n participants mu = (sum mean_i) / n, var = (sum (mean_i - mu)^2) / (n - 1), sigma = sqrt(var) (0 for n < 2),
// threshold = mu + std_ratio * sigma; keep iff the point takes part and mean_i <= threshold.  Both sums in this fixed order:
// rows = stat_rows(M) workgroups of 256 lanes; row c covers the points [c * len, (c + 1) * len), len = ceil(M / rows); lane l
// adds its points l, l + 256, ... in that order; the 64 lanes of a wave fold as v[i] += v[i + o] for o = 32, 16 .. 1; the four
// waves as (w0 + w1) + (w2 + w3); the rows are added in row order.  n is an integer, exact.
//
// Normals: the neighbourhood of point i is the point itself plus its k nearest others within max_dist (exclude_self), `count`
// of them.  count < 2: the normal is (0, 0, 0) and not valid.  Otherwise e_j = (double)p_j - (double)p_i per axis, S1 = sum e_j
// and S2 = sum e_j e_j^T (xx, xy, xz, yy, yz, zz) in list order, m = count + 1, C = S2 / m - (S1 / m)(S1 / m)^T; the normal is
// the unit eigenvector of C's smallest eigenvalue by kSweeps cyclic Jacobi sweeps over the pivots (0,1), (0,2), (1,2) --
// `normal` below IS the definition.  Raw sign: the component of largest magnitude is positive, the first one on ties.  With
// `toward`: flipped so that n . (toward_i - p_i) >= 0 in fp64; an exact 0 keeps the raw sign.
#pragma once
#include "nn_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace knn {

constexpr int kMaxK = 32;
constexpr int kSweeps = 8;
constexpr int kStatRows = 256;            // workgroups of a statistics pass at most
constexpr int kStatChunk = 4096;          // points a workgroup covers at least
constexpr int kStatWG = 256;

MV_HD bool k_ok(int k) { return k >= 1 && k <= kMaxK; }

MV_HD double inf() { return __builtin_huge_val(); }

// after shell r >= 1: nothing in a later shell can enter the list
MV_HD bool ring_done(int r, float cell, bool full, double kth_d2) { return full && nn::ring_done(r, cell, kth_d2); }

MV_HD int stat_rows(long M) {
    const long s = (M + kStatChunk - 1) / kStatChunk;
    return (int)(s < kStatRows ? s : kStatRows);
}
MV_HD long stat_len(long M, int rows) { return (M + rows - 1) / rows; }

// a mean of the statistical filter that takes part: not +inf (isolated), not NaN (invalid)
MV_HD bool takes_part(double mean) { return mean < inf(); }

MV_HD double mean_of(double sum, int k) { return sum / (double)k; }
MV_HD double mu_of(double sum, double n) { return sum / n; }                     // n = 0: NaN
MV_HD double sq_dev(double mean, double mu) { const double d = mean - mu; return d * d; }
MV_HD double sigma_of(double ss, double n) { return n < 2.0 ? 0.0 : sqrt(ss / (n - 1.0)); }
MV_HD double threshold_of(double mu, double sigma, double std_ratio) { return mu + std_ratio * sigma; }
MV_HD bool stat_keep(double mean, double threshold) { return takes_part(mean) && mean <= threshold; }

// The sums of a neighbourhood: add() once per list entry, in list order.
struct Moments {
    double x, y, z, xx, xy, xz, yy, yz, zz;
};

MV_HD Moments no_moments() {
    Moments s;
    s.x = s.y = s.z = s.xx = s.xy = s.xz = s.yy = s.yz = s.zz = 0.0;
    return s;
}

MV_HD void add(Moments& s, const float* pi, const float* pj) {
    const double ex = (double)pj[0] - (double)pi[0], ey = (double)pj[1] - (double)pi[1], ez = (double)pj[2] - (double)pi[2];
    s.x = s.x + ex;
    s.y = s.y + ey;
    s.z = s.z + ez;
    s.xx = s.xx + ex * ex;
    s.xy = s.xy + ex * ey;
    s.xz = s.xz + ex * ez;
    s.yy = s.yy + ey * ey;
    s.yz = s.yz + ey * ez;
    s.zz = s.zz + ez * ez;
}

struct Sym3 {
    double xx, xy, xz, yy, yz, zz;
};
struct Vec3 {
    double x, y, z;
};

MV_HD Sym3 covariance(const Moments& s, int count) {
    const double m = (double)(count + 1);
    const double mx = s.x / m, my = s.y / m, mz = s.z / m;
    Sym3 C;
    C.xx = s.xx / m - mx * mx;
    C.xy = s.xy / m - mx * my;
    C.xz = s.xz / m - mx * mz;
    C.yy = s.yy / m - my * my;
    C.yz = s.yz / m - my * mz;
    C.zz = s.zz / m - mz * mz;
    return C;
}

// One Jacobi rotation on the pivot (p, q), r the third index: a_pq becomes 0; the columns p and q of V turn with it.
MV_HD void rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p,
                  double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = theta < 0.0 ? -theta : theta;
    double t = 1.0 / (at + sqrt(theta * theta + 1.0));                           // |theta| huge: t = 0, nothing turns
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double tp = t * apq;
    app = app - tp;
    aqq = aqq + tp;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0; v0q = b0;
    v1p = a1; v1q = b1;
    v2p = a2; v2q = b2;
}

// C -> the unit eigenvector of the smallest eigenvalue (the first of equal ones), raw sign
MV_HD Vec3 smallest_eigenvector(const Sym3& C) {
    double a00 = C.xx, a01 = C.xy, a02 = C.xz, a11 = C.yy, a12 = C.yz, a22 = C.zz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);           // (0, 1), r = 2
        rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);           // (0, 2), r = 1
        rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);           // (1, 2), r = 0
    }
    const bool one = a11 < a00;                                                  // selects on values, never on addresses
    const double b01 = one ? a11 : a00;
    const double x01 = one ? v01 : v00, y01 = one ? v11 : v10, z01 = one ? v21 : v20;
    const bool two = a22 < b01;
    double x = two ? v02 : x01, y = two ? v12 : y01, z = two ? v22 : z01;
    const double len = sqrt((x * x + y * y) + z * z);
    x = x / len;
    y = y / len;
    z = z / len;
    const double ax = x < 0.0 ? -x : x, ay = y < 0.0 ? -y : y, az = z < 0.0 ? -z : z;
    const double lead = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
    const bool flip = lead < 0.0;
    Vec3 n;
    n.x = flip ? -x : x;
    n.y = flip ? -y : y;
    n.z = flip ? -z : z;
    return n;
}

// The normal of the point (px, py, pz) from its neighbourhood's sums; face: turn it to the position (tx, ty, tz), which is
// not looked at otherwise.  count < 2 -> false and zeros.
MV_HD bool normal(const Moments& s, int count, float px, float py, float pz, bool face, float tx, float ty, float tz, float& nx,
                  float& ny, float& nz) {
    nx = ny = nz = 0.0f;
    if (count < 2) return false;
    Vec3 n = smallest_eigenvector(covariance(s, count));
    if (face) {
        const double dx = (double)tx - (double)px, dy = (double)ty - (double)py, dz = (double)tz - (double)pz;
        const double dot = (n.x * dx + n.y * dy) + n.z * dz;
        if (dot < 0.0) {
            n.x = -n.x;
            n.y = -n.y;
            n.z = -n.z;
        }
    }
    nx = (float)n.x;
    ny = (float)n.y;
    nz = (float)n.z;
    return true;
}

}  // namespace knn
