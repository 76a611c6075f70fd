// Cloud-to-cloud nearest distances: the definition, shared by geo_nn.hip and the host build used only by
// the tests (tests/hostmath/nn_hostmath.cpp).  Like voxel_math.h: IEEE fp64, one correctly rounded operation per step,
// contraction switched off for both compilers, so the kernels and the host build give the same bits.
//
// Definition (max_dist and cell float32, finite, > 0).  A point is valid iff vox::point_key(p, cell, ...) accepts it: all
// coordinates finite and within 2^20 cells of the origin.  For a valid query a and a valid target b, dx = (double)a.x -
// (double)b.x (likewise dy, dz) and d2 = (dx * dx + dy * dy) + dz * dz in that order.  The candidates of a query are the valid
// targets with d2 <= (double)max_dist * (double)max_dist; its result is the candidate with the lexicographically smallest
// (d2, target index): dist2 = d2, dist = (float)sqrt(d2), index.  No candidate: +inf, +inf, -1.  Invalid query: NaN, NaN, -1.
// That is a brute force over all pairs; the grid is only a way to reach it.
//
// Grid: the targets hashed by their cell (edge `cell`).  A query searches its own cell, then the shells of Chebyshev radius
// r = 1 .. R around it, R = ceil(max_dist / cell) + 1, and may stop after shell r >= 1 once best_d2 <= (r * cell)^2 * (1 - 2^-20).
//
// Why both bounds hold.  A cell index is floor of the fp64 quotient p / cell, of magnitude < 2^20, so the quotient carries an
// absolute rounding error <= 2^-33: a point of cell i has its real quotient in [i - 2^-33, i + 1 + 2^-33].  A target in a shell
// beyond r lies r + 1 cells or more from the query's cell on some axis, so the two real quotients differ by more than
// r - 2^-32 on that axis and the real distance exceeds (r - 2^-32) * cell.
//   * Stop: the computed d2 of such a target (four products and sums, each within 2^-53 relative) is above
//     (r * cell)^2 * (1 - 2^-30), and the computed (r * cell)^2 is within 2^-52 of the real one: with the factor 1 - 2^-20 the
//     target's d2 is strictly above best_d2, so it wins neither on distance nor on an index tie.
//   * R: ceil(max_dist / cell) + 1 >= max_dist / cell + 1 - 2^-50, so a target beyond shell R is further than
//     (max_dist / cell + 1 - 2^-31) * cell > max_dist * (1 + 2^-50): its computed d2 exceeds max_dist^2, it is no candidate.
#pragma once
#include "voxel_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace nn {

constexpr int kMaxRings = 17;                            // R for the smallest cell allowed, max_dist / 15, rounded either way

MV_HD double dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by, dz = (double)az - (double)bz;
    return (dx * dx + dy * dy) + dz * dz;
}

MV_HD double max_dist2(float max_dist) { return (double)max_dist * (double)max_dist; }

// (d2, index) before (best_d2, best_index) in the lexicographic order
MV_HD bool better(double d2, long long index, double best_d2, long long best_index) {
    return d2 < best_d2 || (d2 == best_d2 && index < best_index);
}

MV_HD float dist_of(double d2) { return (float)sqrt(d2); }

// the smallest cell a caller may pass: cell >= max_dist / 15 (in fp64 on the float32 values)
MV_HD bool cell_ok(float max_dist, float cell) { return (double)cell >= (double)max_dist / 15.0; }

// R: shells a query searches at most
MV_HD int rings(float max_dist, float cell) { return (int)ceil((double)max_dist / (double)cell) + 1; }

// after shell r >= 1: nothing in a later shell can replace the best
MV_HD bool ring_done(int r, float cell, double best_d2) {
    const double e = (double)r * (double)cell;
    return best_d2 <= (e * e) * (1.0 - 0x1p-20);
}

// Neighbour cell (ix + dx, iy + dy, iz + dz) of a key's cell -> whether it exists (inside +-2^20), and its key.
MV_HD bool neighbour_key(long long ix, long long iy, long long iz, int dx, int dy, int dz, unsigned long long& key) {
    const long long x = ix + dx + vox::kHalf, y = iy + dy + vox::kHalf, z = iz + dz + vox::kHalf;
    if ((unsigned long long)x >= 2ull * vox::kHalf || (unsigned long long)y >= 2ull * vox::kHalf ||
        (unsigned long long)z >= 2ull * vox::kHalf)
        return false;
    key = ((unsigned long long)x << 42) | ((unsigned long long)y << 21) | (unsigned long long)z;
    return true;
}

}  // namespace nn
