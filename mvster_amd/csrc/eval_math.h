// The DTU evaluation protocol: the definition, shared by geo_eval.hip and the host build used only by
// the tests (tests/hostmath/eval_hostmath.cpp).  Like voxel_math.h and nn_math.h: IEEE fp64 on the float32 coordinates, one
// correctly rounded operation per step in the order written, contraction switched off for both compilers, so the kernels and
// the host build give the same bits.
//
// 1. Point reduction (reducePts_haa.m).  dst float32, finite, > 0.  A point is valid iff vox::point_key(p, dst, ...) accepts it.
//    Point i has the priority (key_i, i), compared lexicographically (`before`); key_i = splitmix64(i, seed), or the caller's
//    int64 priority[i] with its sign bit flipped (`key_of_int64`), so that the unsigned order of the keys is the signed order
//    of the priorities.  Two points are close iff nn::dist2(p_i, p_j) <= (double)dst * (double)dst (`close`, inclusive).  A
//    point is kept iff it is valid and no kept point of smaller priority is close to it.  By induction over the priority order
//    that set is unique and is what the serial loop of the .m file leaves set.
//
//    Search bound.  The cloud is binned into cells of edge c = f * dst (the CloudGrid of nn_math.h) and a point looks at the
//    cells within the Chebyshev radius R of its own: f = 2 and R = 1 (27 cells), or f = 1 and R = 2 (125 cells) -- `reduce_cell`,
//    `reduce_shells`; the first is the one used wherever 2 * dst is a finite float32 (exact: a power of two), because it probes
//    a fifth of the cells.  Why R is enough: a cell index is floor of the fp64 quotient p / c, of magnitude < 2^20, so a point of
//    cell i has its real quotient in [i - 2^-33, i + 1 + 2^-33] (nn_math.h).  A close pair has a computed d2 <= dst^2; the
//    computed d2 is within 2^-50 relative of the real one, so on every axis the real |a - b| <= dst * (1 + 2^-49) and the real
//    quotients differ by at most (1 + 2^-49) / f: with a in cell i, b's quotient is below i + 1 + 1 / f + 2^-32, so b's cell is at
//    most i + 1 for f = 2 and i + 2 for f = 1 (and at least as much below).  With f = 1, shell 2 does occur: a = -1e-30 lies in
//    cell -1 (its quotient is a tiny negative) and b = dst in cell 1, and they are close; 27 cells of edge dst would miss that
//    pair.  The grid at f = 2 accepts more points than are valid (validity is at dst): those start dropped, like every invalid
//    point, and a dropped point suppresses nobody.
//
//    Rounds.  state[i] is 0 (undecided), 1 (kept) or 2 (dropped); invalid points start dropped.  In a round every undecided
//    point looks at the points that are close to it and before it: one of them kept -> dropped (`kDropped`); none kept and none
//    undecided -> kept; otherwise it stays undecided.  A state is written once and a written state is the final answer, so a
//    round may read the states of this round (in place) or of the one before (double-buffered): either way every decision made
//    is the definition's, and the first undecided point in priority order decides in every round.
//
// 2. Masks (PointCompareMain.m, MaxDistCP.m).  BB [2,3], Res and P [4] are the doubles of the .mat files.
//    in_obs_mask: v_a = mround(((double)p_a - BB1_a) / Res + 1.0), mround = MATLAB's round (halves away from zero); inside iff
//    1 <= v_a <= S_a on all axes and mask[((v_1 - 1) * S_2 + (v_2 - 1)) * S_3 + (v_3 - 1)] != 0 (C-contiguous [S1,S2,S3]).  A NaN
//    or infinite coordinate fails the range test by itself.
//    above_plane: ((P1 * x + P2 * y) + P3 * z) + P4 > 0.
//    covered: on every axis p_a >= BB1_a and p_a < BB1_a + (floor((BB2_a - BB1_a) / B) + 1.0) * B, B = max_block = 60: the union
//    of MaxDistCP's blocks; a point outside keeps the distance 60 there, which the < 20 filter discards.  Deviation: the .m
//    file's neighbouring blocks meet at (BB1 + x * B) + B against BB1 + (x + 1) * B, which can differ by one ulp, so a point
//    exactly in such a gap would fall between two blocks there; the interval here has no gaps.
//
// 3. Statistics (ComputeStat_func.m) of one direction.  d = sqrt(dist2); a point is selected iff its selection byte is set,
//    dist2 is finite and d < (double)max_dist (strict).  n; mean = sum(d) / n; var = sum((d - mean)^2) / (n - 1), 0 for n = 1;
//    median = (sqrt(a) + sqrt(b)) / 2 with a, b the dist2 of ranks (n - 1) / 2 and n / 2 among the selected (for odd n they are
//    one value and (x + x) / 2 = x exactly).  A non-negative double orders as its bit pattern, so the two ranks are an exact
//    radix selection over the uint64 patterns.  n = 0: mean, var and median are NaN.
#pragma once
#include "nn_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace ev {

// the two grids of the reduction: cell factor f (2 or 1) -> the cell edge and the Chebyshev radius searched
MV_HD float reduce_cell(float dst, int factor) { return factor == 2 ? 2.0f * dst : dst; }
MV_HD int reduce_shells(int factor) { return factor == 2 ? 1 : 2; }
constexpr int kUndecided = 0, kKept = 1, kDropped = 2;

MV_HD unsigned long long splitmix64(unsigned long long i, unsigned long long seed) {
    unsigned long long z = i + (seed + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

MV_HD unsigned long long key_of_int64(long long priority) { return (unsigned long long)priority ^ (1ull << 63); }

// priority (ka, ia) before (kb, ib)
MV_HD bool before(unsigned long long ka, long long ia, unsigned long long kb, long long ib) {
    return ka < kb || (ka == kb && ia < ib);
}

MV_HD double reach2(float dst) { return (double)dst * (double)dst; }

MV_HD bool close(const float* a, const float* b, double reach) {
    return nn::dist2(a[0], a[1], a[2], b[0], b[1], b[2]) <= reach;
}

// MATLAB's round: halves away from zero.  For 0.5 <= |x| < 2^52 the sum |x| + 0.5 is exact unless it crosses a power of two,
// where it rounds to a value with the same floor; below 0.5 the answer is 0 (the double just below 0.5 would sum to 1).
MV_HD double mround(double x) {
    const double a = fabs(x);
    if (!(a < 0x1p52)) return x;                          // an integer already, or NaN / inf
    const double r = a < 0.5 ? 0.0 : floor(a + 0.5);
    return x < 0.0 ? -r : r;
}

// bb = BB1 (3), BB2 (3); S = the mask's shape
MV_HD bool in_obs_mask(const float* p, const double* bb, double res, const long* S, const unsigned char* mask) {
    long v[3];
    for (int a = 0; a < 3; ++a) {
        const double r = mround(((double)p[a] - bb[a]) / res + 1.0);
        if (!(r >= 1.0 && r <= (double)S[a])) return false;
        v[a] = (long)r - 1;
    }
    return mask[(v[0] * S[1] + v[1]) * S[2] + v[2]] != 0;
}

MV_HD bool above_plane(const float* p, const double* P) {
    return ((P[0] * (double)p[0] + P[1] * (double)p[1]) + P[2] * (double)p[2]) + P[3] > 0.0;
}

MV_HD bool covered(const float* p, const double* bb, double max_block) {
    for (int a = 0; a < 3; ++a) {
        const double hi = bb[a] + (floor((bb[3 + a] - bb[a]) / max_block) + 1.0) * max_block;
        if (!((double)p[a] >= bb[a] && (double)p[a] < hi)) return false;
    }
    return true;
}

// One direction's selection and distance: -> selected; d = sqrt(dist2).  The selection byte is set iff it has every bit of
// `need` (the flag bytes of mvster_eval_flags carry three predicates; a plain 0 / 1 byte goes with need = 1).
MV_HD bool stat_selected(double dist2, unsigned char sel, int need, float max_dist, double& d) {
    d = sqrt(dist2);
    return (sel & need) == need && dist2 >= 0.0 && dist2 < __builtin_inf() && d < (double)max_dist;
}

// The pattern a selected dist2 is ordered by (-0.0 + 0.0 = +0.0: the one non-negative value whose pattern is not).
MV_HD unsigned long long order_bits(double dist2) { return __builtin_bit_cast(unsigned long long, dist2 + 0.0); }

MV_HD double stat_mean(double sum, long long n) { return n > 0 ? sum / (double)n : __builtin_nan(""); }

MV_HD double stat_var(double sq, long long n) { return n > 1 ? sq / (double)(n - 1) : (n == 1 ? 0.0 : __builtin_nan("")); }

// a, b: the dist2 of the two middle ranks
MV_HD double stat_median(double a, double b) { return (sqrt(a) + sqrt(b)) / 2.0; }

}  // namespace ev
