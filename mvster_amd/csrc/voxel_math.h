// Per-point arithmetic of the voxel-grid thinning of a fused cloud, shared by geo_thin.hip and the
// host build used only by the tests (tests/hostmath/voxel_hostmath.cpp).  Everything is IEEE fp64, one correctly rounded
// operation per step: a division (never a reciprocal), floor, a subtraction, a product by a power of two.  No expression
// below has a product feeding a sum whose fused form would round differently, and contraction is switched off for both
// compilers all the same, so the kernels and the host build give the same bits.
//
// Definition (voxel edge v, float32, finite, > 0; per point and axis): q = (double)p / (double)v, i = floor(q); the point is
// valid iff -2^20 <= i < 2^20 on all three axes (NaN and +-inf fail that by themselves); key = ((ix + 2^20) << 42) |
// ((iy + 2^20) << 21) | (iz + 2^20), 63 bits; the offset inside the voxel in 16-bit fixed point is
// t = min((int64)floor((q - i) * 65536), 65535) -- the clamp is real: for p = -1e-30, q - i rounds to 1.0.
#pragma once
#include "mvster_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace vox {

constexpr long long kHalf = 1ll << 20;                   // voxel indices lie in [-2^20, 2^20) per axis
constexpr unsigned long long kEmpty = ~0ull;             // never a key: keys use 63 bits

// One axis: -> valid; i = floor(p / v), t = the fixed-point offset inside voxel i.
MV_HD bool axis(float p, float v, long long& i, int& t) {
    const double q = (double)p / (double)v;
    const double fi = floor(q);
    if (!(fi >= -(double)kHalf && fi < (double)kHalf)) return false;      // also NaN and +-inf
    i = (long long)fi;
    const long long f = (long long)floor((q - fi) * 65536.0);
    t = (int)(f < 65535 ? f : 65535);
    return true;
}

// A point: -> valid; key and the three offsets.
MV_HD bool point_key(const float* p, float v, unsigned long long& key, int t[3]) {
    long long ix, iy, iz;
    const bool okx = axis(p[0], v, ix, t[0]), oky = axis(p[1], v, iy, t[1]), okz = axis(p[2], v, iz, t[2]);
    if (!(okx && oky && okz)) return false;
    key = ((unsigned long long)(ix + kHalf) << 42) | ((unsigned long long)(iy + kHalf) << 21) | (unsigned long long)(iz + kHalf);
    return true;
}

MV_HD long long key_axis(unsigned long long key, int ax) { return (long long)((key >> (42 - 21 * ax)) & 0x1fffffull) - kHalf; }

// Home slot of a key before the mask (the splitmix64 finaliser: neighbouring voxels differ in few low bits of one field).
MV_HD unsigned long long hash(unsigned long long k) {
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k;
}

// reduce "mean": voxel i with n points whose offsets sum to S -> the mean of the offsets' cell centres, rounded once
MV_HD float mean_coord(long long i, unsigned long long S, unsigned n, float v) {
    return (float)(((double)i + ((double)S + 0.5 * (double)n) / ((double)n * 65536.0)) * (double)v);
}

// colour channel sum C over n points -> C / n rounded half up, in integers
MV_HD unsigned char mean_color(unsigned long long C, unsigned n) {
    return (unsigned char)((2ull * C + n) / (2ull * n));
}

}  // namespace vox
