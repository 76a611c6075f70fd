// A scan from a structure-from-motion model: the score of a pair of views over the sparse points both
// see, a view's source list and its depth range -- the definition, shared by geo_sfm.hip and the host build used only by the
// tests (tests/hostmath/sfm_hostmath.cpp).  Like knn_math.h: IEEE fp64, one correctly rounded operation per step in the order
// written, only + - * / sqrt, contraction switched off for both compilers, and no call into libm: `angle_deg` and `exp_neg` below
// ARE the definition, so the kernels and the host build give the same bits.
//
// Inputs.  V views with world-to-camera rotation R_v, translation t_v and centre C_v = -R_v^T t_v (fp64, the centre formed once
// on the host); P sparse points X_p (fp64); per view the sorted DISTINCT indices of the points it observes (view_ptr [V+1],
// view_pts) and the transpose, per point the sorted distinct views that observe it (pt_ptr [P+1], pt_views).  A point observed
// twice in one image counts once.
//
// Term of the views i < j that both see p: a = C_i - X_p, b = C_j - X_p; a.a == 0 or b.b == 0 (or not a number): 0.  Otherwise
// theta = angle_deg(a, b) and term = exp_neg(-(theta - theta0)^2 / (2 sigma^2)), sigma = sigma1 if theta <= theta0 else sigma2.
// q_term = (uint64)(term * 2^32 + 0.5); q[i][j] = q[j][i] = the integer sum of q_term over the common points: independent of
// the order, and score = q / 2^32 is exact in fp64.
//
// Sources of view i: the first num_src views j != i with q[i][j] > 0 in (q descending, j ascending) order (`before`).
//
// Depth range of view v: z = ((r20 x + r21 y) + r22 z_p) + t2 per distinct point; only finite z > 0 is kept; of the n kept
// values in ascending order depth_min = z[n / 100] and depth_max = z[(99 n) / 100] (integer division); n = 0: no range (NaN).
// The bit pattern of a positive finite double orders as the double does, so an exact radix selection over the patterns is
// the selection over the values.
//
// Accuracy of `term` (theta0 in [0, 180], sigma1, sigma2 >= kSigmaMin = 0.05; u = 2^-53):
//   angle_deg.  na, nb carry at most 2.5 u relative error each (three products, two sums, a square root); the components of
//     nb a and na b at most 3.5 u; y = |nb a - na b| and x = |nb a + na b| therefore carry an ABSOLUTE error of at most
//     about 12 u na nb (the cancelling one) and a relative one of at most 6 u (the other), and since y^2 + x^2 = 4 na^2 nb^2
//     the angle atan2(y, x) moves by at most 12 u rad whatever theta is: the form is as well conditioned at 0 and 180 as in
//     between.  atan_unit halves the angle twice (each t / (1 + sqrt(1 + t^2)): at most 4 u relative) down to w <= tan(pi / 16)
//     < 0.19892 and sums the alternating series through w^25 / 25; its terms fall in magnitude, so the remainder is below the
//     first one left out, w^27 / 27 < 4.4e-21, and the Horner evaluation adds at most 3 u relative.  With the quotient, the two
//     doublings, pi / 2 - . and the factor 180 / pi the computed theta is within 64 u * 180 < 1.3e-12 degrees of the true angle.
//   exp_neg(x), -kExpCut <= x <= 0.  k = trunc(x / ln 2 - 1/2) has |k - x / ln 2| <= 1/2 + 2^-40, so r = (x - k ln2_hi) - k ln2_lo
//     has |r| <= 0.34658 (k ln2_hi is exact: ln2_hi ends in 20 zero bits and |k| < 2^8; |k ln2_lo - k (ln 2 - ln2_hi)| < 2^-90).
//     The polynomial is the Taylor sum through r^13 / 13!: remainder <= |r|^14 / 14! * e^|r| < 6e-18; Horner adds at most 4 u.
//     The scale by 2^k is exact.  The result is within 2^-51 relative of exp(x).  x < -kExpCut gives 0, off by e^-100 < 4e-44.
//   term.  The argument's own rounding (four operations on |x| <= 100) moves exp by at most 100 * 4 u relative = 4.5e-14, and
//     d term / d theta is at most 1 / (sigma sqrt(e)) <= 12.2 per degree, so the error in theta moves it by at most 1.6e-11.
//     Together below 1.7e-11 < 2^-33 = 1.16e-10: two implementations that each meet this bound differ by at most one unit of
//     2^-32 in q_term.  Measured on the host build against long double libm: DESIGN.md section 4.21.
#pragma once
#include "mvster_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace sfm {

constexpr int kMaxSources = 64;           // num_src at most
constexpr int kMaxViews = 16384;          // V at most: q [V,V] is 2 GiB there
constexpr double kSigmaMin = 0.05;        // degrees
constexpr double kExpCut = 100.0;
constexpr double kRadToDeg = 57.29577951308232;        // 180 / pi
constexpr double kHalfPi = 1.5707963267948966;
constexpr double kInvLn2 = 1.4426950408889634;
constexpr double kLn2Hi = 6.93147180369123816490e-01;   // 0x3fe62e42fee00000
constexpr double kLn2Lo = 1.90821492927058770002e-10;   // ln 2 - kLn2Hi
constexpr double kTwo32 = 4294967296.0;

MV_HD double nan64() { return __builtin_nan(""); }

MV_HD bool params_ok(double theta0, double sigma1, double sigma2) {
    return theta0 >= 0.0 && theta0 <= 180.0 && sigma1 >= kSigmaMin && sigma2 >= kSigmaMin && sigma1 < __builtin_huge_val() &&
           sigma2 < __builtin_huge_val();
}

// atan(t) for 0 <= t <= 1
MV_HD double atan_unit(double t) {
    const double h = t / (1.0 + sqrt(1.0 + t * t));                             // tan(atan(t) / 2)
    const double w = h / (1.0 + sqrt(1.0 + h * h));                             // tan(atan(t) / 4) <= tan(pi / 16)
    const double s = w * w;
    double p = 1.0 / 25.0;
    p = 1.0 / 23.0 - s * p;
    p = 1.0 / 21.0 - s * p;
    p = 1.0 / 19.0 - s * p;
    p = 1.0 / 17.0 - s * p;
    p = 1.0 / 15.0 - s * p;
    p = 1.0 / 13.0 - s * p;
    p = 1.0 / 11.0 - s * p;
    p = 1.0 / 9.0 - s * p;
    p = 1.0 / 7.0 - s * p;
    p = 1.0 / 5.0 - s * p;
    p = 1.0 / 3.0 - s * p;
    p = 1.0 - s * p;
    return 4.0 * (w * p);
}

// The angle between a and b in degrees, 0 .. 180, from |nb a - na b| and |nb a + na b| (na = |a|, nb = |b|); aa = a.a and
// bb = b.b, both > 0.
MV_HD double angle_deg(const double a[3], const double b[3], double aa, double bb) {
    const double na = sqrt(aa), nb = sqrt(bb);
    const double ux = nb * a[0], uy = nb * a[1], uz = nb * a[2];
    const double vx = na * b[0], vy = na * b[1], vz = na * b[2];
    const double dx = ux - vx, dy = uy - vy, dz = uz - vz;
    const double sx = ux + vx, sy = uy + vy, sz = uz + vz;
    const double y = sqrt((dx * dx + dy * dy) + dz * dz);
    const double x = sqrt((sx * sx + sy * sy) + sz * sz);
    double half;                                                                // atan2(y, x), both >= 0
    if (y <= x) half = x > 0.0 ? atan_unit(y / x) : 0.0;
    else half = kHalfPi - atan_unit(x / y);
    return (2.0 * half) * kRadToDeg;
}

// exp(x) for x <= 0; 0 below -kExpCut
MV_HD double exp_neg(double x) {
    if (!(x >= -kExpCut)) return 0.0;
    const long long k = (long long)(x * kInvLn2 - 0.5);                         // truncation: the nearest integer, halves up
    const double kd = (double)k;
    const double r = (x - kd * kLn2Hi) - kd * kLn2Lo;
    double p = 1.0 / 6227020800.0;                                              // 1 / 13!
    p = 1.0 / 479001600.0 + r * p;
    p = 1.0 / 39916800.0 + r * p;
    p = 1.0 / 3628800.0 + r * p;
    p = 1.0 / 362880.0 + r * p;
    p = 1.0 / 40320.0 + r * p;
    p = 1.0 / 5040.0 + r * p;
    p = 1.0 / 720.0 + r * p;
    p = 1.0 / 120.0 + r * p;
    p = 1.0 / 24.0 + r * p;
    p = 1.0 / 6.0 + r * p;
    p = 0.5 + r * p;
    p = 1.0 + r * p;
    p = 1.0 + r * p;
    const unsigned long long bits = (unsigned long long)(k + 1023) << 52;       // 2^k, k >= -145: a normal number
    double scale;
    __builtin_memcpy(&scale, &bits, sizeof scale);
    return p * scale;
}

// theta is handed back for the tests
MV_HD double term(const double ci[3], const double cj[3], const double x[3], double theta0, double sigma1, double sigma2,
                  double& theta) {
    const double a[3] = {ci[0] - x[0], ci[1] - x[1], ci[2] - x[2]};
    const double b[3] = {cj[0] - x[0], cj[1] - x[1], cj[2] - x[2]};
    const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const double bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    theta = nan64();
    if (!(aa > 0.0) || !(bb > 0.0)) return 0.0;
    theta = angle_deg(a, b, aa, bb);
    const double sigma = theta <= theta0 ? sigma1 : sigma2;
    const double d = theta - theta0;
    return exp_neg(-(d * d) / (2.0 * (sigma * sigma)));
}

MV_HD unsigned long long quantise(double t) { return t > 0.0 ? (unsigned long long)(t * kTwo32 + 0.5) : 0ull; }

// Pair e = 0 .. L (L - 1) / 2 - 1 of a track of L views -> positions a < b, rows first: (0,1) (0,2) .. (0,L-1) (1,2) ..., so
// that consecutive e share a and walk b.  In integers: the square root only proposes, the two loops settle it (at most a
// step each for L <= 2^20).
MV_HD void pair_of(long long e, long long L, long long& a, long long& b) {
    const long long m = L * (L - 1) / 2 - 1 - e;                                // the same pair counted from the end
    long long c = (long long)((1.0 + sqrt((double)(8 * m + 1))) / 2.0);         // c (c - 1) / 2 <= m < (c + 1) c / 2
    while (c * (c - 1) / 2 > m) --c;
    while ((c + 1) * c / 2 <= m) ++c;
    const long long r = m - c * (c - 1) / 2;                                    // 0 <= r < c
    a = L - 1 - c;
    b = L - 1 - r;
}

MV_HD long long pairs_of(long long L) { return L * (L - 1) / 2; }

// depth of x in the view whose row is rt = (r20, r21, r22, t2)
MV_HD double depth(const double rt[4], const double x[3]) { return ((rt[0] * x[0] + rt[1] * x[1]) + rt[2] * x[2]) + rt[3]; }

MV_HD bool depth_kept(double z) { return z > 0.0 && z < __builtin_huge_val(); }

MV_HD unsigned long long depth_bits(double z) {
    unsigned long long b;
    __builtin_memcpy(&b, &z, sizeof b);
    return b;
}

MV_HD long long rank_min(long long n) { return n / 100; }
MV_HD long long rank_max(long long n) { return (99 * n) / 100; }

// (q, j) comes before (p, i) in a source list
MV_HD bool before(unsigned long long q, int j, unsigned long long p, int i) { return q > p || (q == p && j < i); }

}  // namespace sfm
