// Undistortion of a structure-from-motion scan: the radial / tangential distortion of COLMAP's
// SIMPLE_RADIAL, RADIAL and OPENCV cameras, its inverse, the pinhole camera an undistorted image gets and the resampling of
// one output pixel -- the definition, shared by geo_undistort.hip and the host build used only by the tests
// (tests/hostmath/undistort_hostmath.cpp).  Like sfm_math.h: IEEE fp64, one correctly rounded operation per step in the order
// written, only + - * /, contraction switched off for both compilers, and no call into libm, so the kernels and the host build
// give the same bits.  It is this project's own definition, modelled on COLMAP's undistortion; DESIGN.md lists the deviations.
//
// Camera record, 12 doubles: model id (2 SIMPLE_RADIAL, 3 RADIAL, 4 OPENCV), W, H, fx, fy (fx = fy = f for 2 and 3), cx, cy,
// k1, k2, p1, p2 (0 where the model has none), one pad.  The arithmetic is the same for the three models: the terms a model
// lacks are multiplied by its zeros.
//
// Undistorted camera, 8 doubles: W', H', fx, fy, cx', cy' (a PINHOLE camera with the same focal lengths), the worst residual of
// the inversion over the border points, and the number of border points whose residual exceeds kResidualBound.
//
// distort (u, v) -> (ud, vd) on normalised coordinates: r2 = u u + v v, rad = k1 r2 + k2 r2^2,
//   ud = ((u + u rad) + (2 p1) (u v)) + p2 (r2 + 2 u u),  vd = ((v + v rad) + (2 p2) (u v)) + p1 (r2 + 2 v v).
// undistort (ud, vd) -> (u, v): Newton with the analytic 2x2 Jacobian from (ud, vd), kNewtonSteps steps and no early exit; a
//   non-finite iterate or a determinant <= 0 ends the updates of that point, whose residual is then +inf; otherwise the residual
//   is max(|distort(u, v) - (ud, vd)|) of the final iterate.
// sample: output pixel (x, y) looks at u = (x + 0.5 - cx') / fx, v likewise, (ud, vd) = distort(u, v), sx = fx ud + cx - 0.5, sy
//   likewise; it is valid iff 0 <= sx <= W-1 and 0 <= sy <= H-1; then x0 = floor(sx), x1 = min(x0 + 1, W-1), the same in y, and
//   per channel (top = a (1 - wx) + b wx, bottom likewise, value = top (1 - wy) + bottom wy) -> (unsigned char)(value + 0.5)
//   clamped to 0 .. 255.  An invalid pixel is (0, 0, 0).
#pragma once
#include "mvster_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace und {

constexpr int kNewtonSteps = 10;
constexpr int kCam = 12;                  // doubles per camera record
constexpr int kOut = 8;                   // doubles per undistorted camera
constexpr double kResidualBound = 1e-9;   // normalised units
constexpr long kMaxSide = 1l << 20;       // W, H at most

MV_HD double inf64() { return __builtin_huge_val(); }
MV_HD double abs64(double x) { return x < 0.0 ? -x : x; }
MV_HD bool finite64(double x) { return x - x == 0.0; }
MV_HD double min64(double a, double b) { return b < a ? b : a; }               // a NaN in b is dropped
MV_HD double max64(double a, double b) { return b > a ? b : a; }

// a record the other functions can work on: a known model, a size within 1 .. kMaxSide, focal lengths > 0
MV_HD bool camera_ok(const double* c) {
    return (c[0] == 2.0 || c[0] == 3.0 || c[0] == 4.0) && c[1] >= 1.0 && c[1] <= (double)kMaxSide && c[2] >= 1.0 &&
           c[2] <= (double)kMaxSide && c[3] > 0.0 && c[3] < inf64() && c[4] > 0.0 && c[4] < inf64() && finite64(c[5]) &&
           finite64(c[6]);
}

MV_HD void distort(const double* c, double u, double v, double& ud, double& vd) {
    const double k1 = c[7], k2 = c[8], p1 = c[9], p2 = c[10];
    const double uu = u * u, vv = v * v, uv = u * v;
    const double r2 = uu + vv;
    const double rad = k1 * r2 + k2 * (r2 * r2);
    ud = ((u + u * rad) + (2.0 * p1) * uv) + p2 * (r2 + 2.0 * uu);
    vd = ((v + v * rad) + (2.0 * p2) * uv) + p1 * (r2 + 2.0 * vv);
}

// the Jacobian of distort at (u, v): a = d ud / du, b = d ud / dv, cc = d vd / du, d = d vd / dv
MV_HD void jacobian(const double* c, double u, double v, double& a, double& b, double& cc, double& d) {
    const double k1 = c[7], k2 = c[8], p1 = c[9], p2 = c[10];
    const double uu = u * u, vv = v * v, uv = u * v;
    const double r2 = uu + vv;
    const double rad = k1 * r2 + k2 * (r2 * r2);
    const double g = 2.0 * (k1 + (2.0 * k2) * r2);                              // d rad / d r2, doubled
    a = (((1.0 + rad) + g * uu) + (2.0 * p1) * v) + (6.0 * p2) * u;
    d = (((1.0 + rad) + g * vv) + (2.0 * p2) * u) + (6.0 * p1) * v;
    b = (g * uv + (2.0 * p1) * u) + (2.0 * p2) * v;
    cc = b;
}

// -> the residual
MV_HD double undistort(const double* c, double ud, double vd, double& u, double& v) {
    u = ud;
    v = vd;
    bool ok = finite64(ud) && finite64(vd);
    for (int s = 0; s < kNewtonSteps; ++s) {
        double fu, fv, a, b, cc, d;
        distort(c, u, v, fu, fv);
        jacobian(c, u, v, a, b, cc, d);
        const double eu = fu - ud, ev = fv - vd;
        const double det = a * d - b * cc;
        ok = ok && det > 0.0 && finite64(det);
        const double nu = u - (d * eu - b * ev) / det;
        const double nv = v - (a * ev - cc * eu) / det;
        ok = ok && finite64(nu) && finite64(nv);
        if (ok) {
            u = nu;
            v = nv;
        }
    }
    double fu, fv;
    distort(c, u, v, fu, fv);
    const double r = max64(abs64(fu - ud), abs64(fv - vd));
    return ok && finite64(r) ? r : inf64();
}

// ---- the undistorted camera ----------------------------------------------------------------------------------------------------

// what the border points are folded into: min and max only (and an integer count), so the order does not matter
struct Border {
    double left_min, left_max, right_min, right_max, top_min, top_max, bottom_min, bottom_max, worst;
    long over;
};

MV_HD Border border_empty() {
    Border e;
    e.left_min = e.right_max = e.top_min = e.bottom_max = -inf64();             // (these four are maxima)
    e.left_max = e.right_min = e.top_max = e.bottom_min = inf64();
    e.worst = 0.0;
    e.over = 0;
    return e;
}

MV_HD long border_points(const double* c) { return 2 * ((long)c[1] + (long)c[2]); }

// border point i = 0 .. 2 (W + H) - 1: the left column top down, the right column, the top row, the bottom row
MV_HD void border_add(const double* c, long i, Border& e) {
    const long W = (long)c[1], H = (long)c[2];
    const double fx = c[3], fy = c[4], cx = c[5], cy = c[6];
    int side;
    double px, py;
    if (i < H) { side = 0; px = 0.5; py = (double)i + 0.5; }
    else if (i < 2 * H) { side = 1; px = (double)W - 0.5; py = (double)(i - H) + 0.5; }
    else if (i < 2 * H + W) { side = 2; px = (double)(i - 2 * H) + 0.5; py = 0.5; }
    else { side = 3; px = (double)(i - 2 * H - W) + 0.5; py = (double)H - 0.5; }
    double u, v;
    const double r = undistort(c, (px - cx) / fx, (py - cy) / fy, u, v);
    const double x = u * fx + cx, y = v * fy + cy;
    if (side == 0) { e.left_min = max64(e.left_min, x); e.left_max = min64(e.left_max, x); }
    else if (side == 1) { e.right_min = min64(e.right_min, x); e.right_max = max64(e.right_max, x); }
    else if (side == 2) { e.top_min = max64(e.top_min, y); e.top_max = min64(e.top_max, y); }
    else { e.bottom_min = min64(e.bottom_min, y); e.bottom_max = max64(e.bottom_max, y); }
    e.worst = max64(e.worst, r);
    if (!(r <= kResidualBound)) e.over += 1;
}

MV_HD void border_merge(Border& e, const Border& o) {
    e.left_min = max64(e.left_min, o.left_min);
    e.left_max = min64(e.left_max, o.left_max);
    e.right_min = min64(e.right_min, o.right_min);
    e.right_max = max64(e.right_max, o.right_max);
    e.top_min = max64(e.top_min, o.top_min);
    e.top_max = min64(e.top_max, o.top_max);
    e.bottom_min = min64(e.bottom_min, o.bottom_min);
    e.bottom_max = max64(e.bottom_max, o.bottom_max);
    e.worst = max64(e.worst, o.worst);
    e.over += o.over;
}

// a scale within [lo, hi]; anything that is not a number becomes lo
MV_HD double clamp_scale(double s, double lo, double hi) {
    if (!(s >= lo)) s = lo;
    if (s > hi) s = hi;
    return s;
}

MV_HD void scales_of(const double* c, const Border& e, double blank, double min_scale, double max_scale, double& sx, double& sy) {
    const double W = c[1], H = c[2], cx = c[5], cy = c[6];
    const double min_x = min64(cx / (cx - e.left_min), ((W - 0.5) - cx) / (e.right_max - cx));
    const double max_x = max64(cx / (cx - e.left_max), ((W - 0.5) - cx) / (e.right_min - cx));
    const double min_y = min64(cy / (cy - e.top_min), ((H - 0.5) - cy) / (e.bottom_max - cy));
    const double max_y = max64(cy / (cy - e.top_max), ((H - 0.5) - cy) / (e.bottom_min - cy));
    sx = clamp_scale(1.0 / (min_x * blank + max_x * (1.0 - blank)), min_scale, max_scale);
    sy = clamp_scale(1.0 / (min_y * blank + max_y * (1.0 - blank)), min_scale, max_scale);
}

// out [kOut] from the scales (within (0, 2^10]: the sizes stay below 2^31)
MV_HD void camera_of(const double* c, double sx, double sy, double worst, long over, double* out) {
    const double W = c[1], H = c[2];
    long w = (long)(clamp_scale(sx, 0.0, 1024.0) * W), h = (long)(clamp_scale(sy, 0.0, 1024.0) * H);
    if (w < 1) w = 1;
    if (h < 1) h = 1;
    out[0] = (double)w;
    out[1] = (double)h;
    out[2] = c[3];
    out[3] = c[4];
    out[4] = (c[5] * (double)w) / W;
    out[5] = (c[6] * (double)h) / H;
    out[6] = worst;
    out[7] = (double)over;
}

// a record that is not camera_ok: nothing can be said
MV_HD void camera_none(double* out) {
    for (int k = 0; k < kOut; ++k) out[k] = 0.0;
    out[6] = inf64();
}

// ---- points in pixel coordinates ----------------------------------------------------------------------------------------------------

// direction 0: distort, 1: undistort; both sides in the pixels of the camera's own fx, fy, cx, cy.  -> the residual (0 for 0)
MV_HD double point(const double* c, int direction, double x, double y, double& ox, double& oy) {
    const double fx = c[3], fy = c[4], cx = c[5], cy = c[6];
    const double a = (x - cx) / fx, b = (y - cy) / fy;
    double u, v, r = 0.0;
    if (direction) r = undistort(c, a, b, u, v);
    else distort(c, a, b, u, v);
    ox = u * fx + cx;
    oy = v * fy + cy;
    return r;
}

// ---- one output pixel ---------------------------------------------------------------------------------------------------------------

MV_HD unsigned char to_byte(double v) {
    const double r = v + 0.5;
    return r >= 255.0 ? (unsigned char)255 : (r > 0.0 ? (unsigned char)r : (unsigned char)0);
}

// the source location of output pixel (x, y) of the undistorted camera o (kOut) of camera c (kCam)
MV_HD double source_u(const double* o, long x) { return (((double)x + 0.5) - o[4]) / o[2]; }     // a column's u
MV_HD double source_v(const double* o, long y) { return (((double)y + 0.5) - o[5]) / o[3]; }     // a row's v

MV_HD void source_at(const double* c, double u, double v, double& sx, double& sy) {
    double ud, vd;
    distort(c, u, v, ud, vd);
    sx = (c[3] * ud + c[5]) - 0.5;
    sy = (c[4] * vd + c[6]) - 0.5;
}

MV_HD void source_of(const double* c, const double* o, long x, long y, double& sx, double& sy) {
    source_at(c, source_u(o, x), source_v(o, y), sx, sy);
}

MV_HD double blend(double a, double b, double cc, double d, double wx, double wy) {
    const double top = a * (1.0 - wx) + b * wx;
    const double bottom = cc * (1.0 - wx) + d * wx;
    return top * (1.0 - wy) + bottom * wy;
}

// src [Hs,Ws,3] uint8 -> rgb of the output pixel that looks along (u, v); false (and black) where that is outside the source
MV_HD bool pixel_at(const double* c, const unsigned char* src, long Hs, long Ws, double u, double v, unsigned char* rgb) {
    double sx, sy;
    source_at(c, u, v, sx, sy);
    rgb[0] = rgb[1] = rgb[2] = 0;
    if (!(sx >= 0.0 && sx <= (double)(Ws - 1) && sy >= 0.0 && sy <= (double)(Hs - 1))) return false;
    const long x0 = (long)sx, y0 = (long)sy;                                    // >= 0: truncation is the floor
    const long x1 = x0 + 1 < Ws ? x0 + 1 : Ws - 1, y1 = y0 + 1 < Hs ? y0 + 1 : Hs - 1;
    const double wx = sx - (double)x0, wy = sy - (double)y0;
    const unsigned char* pa = src + (y0 * Ws + x0) * 3;
    const unsigned char* pb = src + (y0 * Ws + x1) * 3;
    const unsigned char* pc = src + (y1 * Ws + x0) * 3;
    const unsigned char* pd = src + (y1 * Ws + x1) * 3;
    for (int k = 0; k < 3; ++k) rgb[k] = to_byte(blend((double)pa[k], (double)pb[k], (double)pc[k], (double)pd[k], wx, wy));
    return true;
}

MV_HD bool pixel(const double* c, const double* o, const unsigned char* src, long Hs, long Ws, long x, long y, unsigned char* rgb) {
    return pixel_at(c, src, Hs, Ws, source_u(o, x), source_v(o, y), rgb);
}

}  // namespace und
