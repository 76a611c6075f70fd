// Per-pixel arithmetic of the depth-map fusion step, shared by geo_filter.hip (one
// reference view per launch), geo_scene.hip (a whole scan per launch, fixed or dynamic thresholds) and the host builds
// used only by the tests (tests/hostmath/geo_hostmath.cpp, geo_dyn_hostmath.cpp).  Every kernel that inlines one of these functions executes the same expression
// tree: products that feed a sum are explicit fma, fp32 steps go through mv::*_rn, everything else is a single
// correctly rounded operation, so neither hipcc's contraction nor the host build (-ffp-contract=off) changes a bit.
//
// The dtype flow is the reference's (test_mvs4.py:273-328, :352-407): camera matrices are float32 values widened to
// double, the geometry runs in fp64 (NumPy: float32 matrix x float64 points), the maps and the two consistency tests
// are fp32 exactly where the reference casts.
#pragma once
#include "mvster_math.h"

namespace geo {

constexpr int kViewDoubles = 42;   // per source view: A[3x4] = E_src inv(E_ref), K_src[3x3], inv(K_src)[3x3], B[3x4] = E_ref inv(E_src)
constexpr int kRefDoubles = 30;    // per reference view: inv(K_ref)[3x3], K_ref[3x3], inv(E_ref)[3x4]

MV_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

MV_HD void mat3(const double* m, double x, double y, double z, double& ox, double& oy, double& oz) {
    ox = fma(m[2], z, fma(m[1], y, m[0] * x));
    oy = fma(m[5], z, fma(m[4], y, m[3] * x));
    oz = fma(m[8], z, fma(m[7], y, m[6] * x));
}

MV_HD void mat34(const double* m, double x, double y, double z, double& ox, double& oy, double& oz) {
    ox = fma(m[2], z, fma(m[1], y, m[0] * x)) + m[3];
    oy = fma(m[6], z, fma(m[5], y, m[4] * x)) + m[7];
    oz = fma(m[10], z, fma(m[9], y, m[8] * x)) + m[11];
}

// cv2.remap(src, x, y, INTER_LINEAR), BORDER_CONSTANT 0: fixed-point coordinates with 5 fractional bits
MV_HD float remap_linear(const float* __restrict__ src, int H, int W, float x, float y) {
    if (!(fabsf(x) < 1e6f) || !(fabsf(y) < 1e6f)) return 0.0f;        // also NaN: every tap is outside
    const int sx = (int)rintf(mv::mul_rn(x, 32.0f)), sy = (int)rintf(mv::mul_rn(y, 32.0f));  // cvRound (half to even)
    const int ix = sx >> 5, iy = sy >> 5;
    const float fx = (float)(sx & 31) * (1.0f / 32.0f), fy = (float)(sy & 31) * (1.0f / 32.0f);
    const bool x0 = (unsigned)ix < (unsigned)W, x1 = (unsigned)(ix + 1) < (unsigned)W;
    const bool y0 = (unsigned)iy < (unsigned)H, y1 = (unsigned)(iy + 1) < (unsigned)H;
    const int cx0 = clampi(ix, 0, W - 1), cx1 = clampi(ix + 1, 0, W - 1);
    const int cy0 = clampi(iy, 0, H - 1), cy1 = clampi(iy + 1, 0, H - 1);
    const float v00 = src[(long)cy0 * W + cx0], v01 = src[(long)cy0 * W + cx1];
    const float v10 = src[(long)cy1 * W + cx0], v11 = src[(long)cy1 * W + cx1];
    const float s00 = (y0 && x0) ? v00 : 0.0f, s01 = (y0 && x1) ? v01 : 0.0f;
    const float s10 = (y1 && x0) ? v10 : 0.0f, s11 = (y1 && x1) ? v11 : 0.0f;
    const float w00 = mv::mul_rn(1.0f - fy, 1.0f - fx), w01 = mv::mul_rn(1.0f - fy, fx);
    const float w10 = mv::mul_rn(fy, 1.0f - fx), w11 = mv::mul_rn(fy, fx);
    return mv::add_rn(mv::add_rn(mv::add_rn(mv::mul_rn(s00, w00), mv::mul_rn(s01, w01)), mv::mul_rn(s10, w10)),
                      mv::mul_rn(s11, w11));
}

// inv(K_ref) @ ((x, y, 1) * depth): the reference pixel in its own camera space (test_mvs4.py:280-281); the same
// for every source view, so callers compute it once per pixel
MV_HD void lift_ref(const double* ref_mats, int x, int y, float dref, double& rx, double& ry, double& rz) {
    const double d = (double)dref;
    mat3(ref_mats, (double)x * d, (double)y * d, d, rx, ry, rz);
}

struct Vote {
    bool ok;        // within pix_thres pixels and rel_thres relative depth (test_mvs4.py:319-324)
    float depth;    // reprojected depth, 0 where !ok (:326)
    float x_src;    // where the pixel lands in the source view (:286-289)
    float y_src;
};

struct ViewError {
    double dist;    // reprojection error in pixels (test_mvs4.py:319), fp64
    float rel;      // relative depth error (:322-323), fp32
    float drep;     // reprojected depth (:326), not yet thresholded
    float x_src;    // where the pixel lands in the source view (:286-289)
    float y_src;
};

// One (reference pixel, source view) round trip: project the lifted pixel into the source view, sample the source depth
// map, lift with the sampled depth, project back, measure the two errors (test_mvs4.py:283-323).  `m` = this view's 42
// doubles.  No threshold is applied: view_vote (fixed thresholds) and level_passes (dynamic consistency) do that.
MV_HD ViewError view_error(const float* __restrict__ depth_src, int H, int W, const double* ref_mats, const double* m, int x,
                           int y, float dref, double rx, double ry, double rz) {
    ViewError r;
    double qx, qy, qz, kx, ky, kz;
    mat34(m, rx, ry, rz, qx, qy, qz);                              // source camera space
    mat3(m + 12, qx, qy, qz, kx, ky, kz);                          // K_src @ .
    const double xs = kx / kz, ys = ky / kz;
    r.x_src = (float)xs;
    r.y_src = (float)ys;
    const float sampled = remap_linear(depth_src, H, W, r.x_src, r.y_src);
    const double sd = (double)sampled;
    double sx3, sy3, sz3, bx, by, bz, ux, uy, uz;
    mat3(m + 21, xs * sd, ys * sd, sd, sx3, sy3, sz3);             // inv(K_src) @ ((xs, ys, 1) * sampled)
    mat34(m + 30, sx3, sy3, sz3, bx, by, bz);                      // back in the reference camera space
    r.drep = (float)bz;
    mat3(ref_mats + 9, bx, by, bz, ux, uy, uz);                    // K_ref @ .
    const float xr = (float)(ux / uz), yr = (float)(uy / uz);
    const double ex = (double)xr - (double)x, ey = (double)yr - (double)y;
    r.dist = sqrt(fma(ex, ex, ey * ey));
    r.rel = mv::div_rn(fabsf(mv::sub_rn(r.drep, dref)), dref);
    return r;
}

// The fixed-threshold vote of check_geometric_consistency (test_mvs4.py:319-328) on the round trip above.
MV_HD Vote view_vote(const float* __restrict__ depth_src, int H, int W, const double* ref_mats, const double* m, int x, int y,
                     float dref, double rx, double ry, double rz, float pix_thres, float rel_thres) {
    const ViewError e = view_error(depth_src, H, W, ref_mats, m, x, y, dref, rx, ry, rz);
    Vote r;
    r.x_src = e.x_src;
    r.y_src = e.y_src;
    r.ok = e.dist < (double)pix_thres && e.rel < rel_thres;
    r.depth = r.ok ? e.drep : 0.0f;
    return r;
}

// votes and the float32 depth sum of filter_depth (test_mvs4.py:380-383), in source-view order
MV_HD void accumulate(const Vote& v, int& count, float& dsum) {
    count += v.ok ? 1 : 0;
    dsum = mv::add_rn(dsum, v.depth);
}

// (sum(reprojected depths) + depth_ref) / (votes + 1) (test_mvs4.py:385): float32 sum, float64 quotient
MV_HD double average(float dsum, float dref, int count) {
    return (double)mv::add_rn(dsum, dref) / (double)(count + 1);
}

// ---- dynamic consistency checking: level n asks for n sources within n times the base errors ----

constexpr int kMaxLevelSources = 32;   // sources per reference view the level counts below hold

// source passes level n: both errors below n times their base, thresholds rounded once in fp32; NaN fails
MV_HD bool level_passes(const ViewError& e, int n, float pix_base, float rel_base) {
    return e.dist < (double)mv::mul_rn((float)n, pix_base) && e.rel < mv::mul_rn((float)n, rel_base);
}

// Histogram of the sources' smallest passing level: 32 bins of 8 bits (a bin holds at most 32) in four 64-bit registers,
// bin b = level n0 + b.  Selected with compares, never indexed, so it stays in registers on the GPU.
struct LevelCounts {
    unsigned long long w0, w1, w2, w3;
};

MV_HD void level_bump(LevelCounts& c, int bin) {
    const unsigned long long one = 1ull << ((bin & 7) * 8);
    const int w = bin >> 3;
    c.w0 += w == 0 ? one : 0ull;
    c.w1 += w == 1 ? one : 0ull;
    c.w2 += w == 2 ? one : 0ull;
    c.w3 += w == 3 ? one : 0ull;
}

MV_HD int level_bin(const LevelCounts& c, int bin) {
    const int w = bin >> 3;
    const unsigned long long v = w == 0 ? c.w0 : (w == 1 ? c.w1 : (w == 2 ? c.w2 : c.w3));
    return (int)((v >> ((bin & 7) * 8)) & 0xffull);
}

struct DynamicVotes {
    int count;      // sources passing the loosest level La = max(L, n0): geo_mask_sum
    int level;      // smallest n in n0..L with at least n sources passing level n, 0 if none: geo_level
    float dsum;     // fp32 sum of their reprojected depths, pair-file order (failing sources add 0)
};

// One reference pixel against its row of the pair table (`pairs_row` [Smax], `vm_row` [Smax, 42]; the row ends at the
// first index outside [0, V)).  Each source walks n upward from n0 to its smallest passing level -- the thresholds grow
// with n, so it passes every level above -- and bumps that bin; the prefix of the bins is count_n.
MV_HD DynamicVotes dynamic_votes(const float* __restrict__ depth, long hw, int H, int W, const int* __restrict__ pairs_row,
                                 int Smax, int V, const double* ref_mats, const double* vm_row, int x, int y, float dref,
                                 double rx, double ry, double rz, int n0, float pix_base, float rel_base) {
    int L = 0;
    while (L < Smax && (unsigned)pairs_row[L] < (unsigned)V) ++L;
    const int bins = L > n0 ? L - n0 + 1 : 1;                      // levels n0 .. La, La = max(L, n0) the averaging level
    LevelCounts c = {0ull, 0ull, 0ull, 0ull};
    DynamicVotes r = {0, 0, 0.0f};
    for (int s = 0; s < L; ++s) {
        const ViewError e = view_error(depth + (long)pairs_row[s] * hw, H, W, ref_mats, vm_row + (long)s * kViewDoubles, x, y,
                                       dref, rx, ry, rz);
        int b = 0;
        while (b < bins && !level_passes(e, n0 + b, pix_base, rel_base)) ++b;
        Vote v;
        v.ok = b < bins;
        v.depth = v.ok ? e.drep : 0.0f;
        v.x_src = e.x_src;
        v.y_src = e.y_src;
        if (v.ok) level_bump(c, b);
        accumulate(v, r.count, r.dsum);
    }
    int cum = 0;
    for (int b = 0; b <= L - n0; ++b) {                            // empty when L < n0: no level, nothing survives
        cum += level_bin(c, b);
        if (r.level == 0 && cum >= n0 + b) r.level = n0 + b;
    }
    return r;
}

// inv(E_ref)[:3] @ (inv(K_ref) @ ((x, y, 1) * depth), 1): a surviving pixel in world space (test_mvs4.py:399-405)
MV_HD void backproject(const double* kinv, const double* einv34, int x, int y, double depth, double& wx, double& wy,
                       double& wz) {
    double cx, cy, cz;
    mat3(kinv, (double)x * depth, (double)y * depth, depth, cx, cy, cz);
    mat34(einv34, cx, cy, cz, wx, wy, wz);
}

// (color * 255).astype(np.uint8) of a float32 image in 0..1 (test_mvs4.py:395-396, :407): one fp32 product, truncated
MV_HD unsigned char color_u8(float c) { return (unsigned char)(int)mv::mul_rn(c, 255.0f); }

}  // namespace geo
