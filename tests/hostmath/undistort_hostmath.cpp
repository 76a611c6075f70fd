// Host build of mvster_amd/csrc/undistort_math.h -- TEST INFRASTRUCTURE ONLY.
// The distortion, its inverse, the undistorted camera and the resampling of an image with the very functions the kernels of
// geo_undistort.hip inline, as serial loops that follow the definition.  Never loaded by the product.
// Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/undistort_cases.py).
#include "../../mvster_amd/csrc/undistort_math.h"

extern "C" {

// n points in normalised coordinates through the distortion of one camera (cam [12])
void hm_und_distort(const double* cam, long n, const double* uv, double* out) {
    for (long k = 0; k < n; ++k) und::distort(cam, uv[2 * k], uv[2 * k + 1], out[2 * k], out[2 * k + 1]);
}

// and back, with the residual
void hm_und_undistort(const double* cam, long n, const double* uv, double* out, double* residual) {
    for (long k = 0; k < n; ++k) residual[k] = und::undistort(cam, uv[2 * k], uv[2 * k + 1], out[2 * k], out[2 * k + 1]);
}

// cams [C,12] -> out [C,8]: the border walked point by point in its order
void hm_und_cameras(const double* cams, int C, double blank, double min_scale, double max_scale, int given, double sx, double sy,
                    double* out) {
    for (int r = 0; r < C; ++r) {
        const double* c = cams + (long)r * und::kCam;
        double* o = out + (long)r * und::kOut;
        if (!und::camera_ok(c)) {
            und::camera_none(o);
            continue;
        }
        if (given) {
            und::camera_of(c, sx, sy, 0.0, 0, o);
            continue;
        }
        und::Border e = und::border_empty();
        const long n = und::border_points(c);
        for (long i = 0; i < n; ++i) und::border_add(c, i, e);
        double ax, ay;
        und::scales_of(c, e, blank, min_scale, max_scale, ax, ay);
        und::camera_of(c, ax, ay, e.worst, e.over, o);
    }
}

// N points in pixel coordinates, a camera row each
void hm_und_points(const double* cams, int C, const int* row, long N, int direction, const double* xy, double* out, double* residual) {
    for (long i = 0; i < N; ++i) {
        double ox = und::inf64(), oy = und::inf64(), res = und::inf64();
        if (row[i] >= 0 && row[i] < C && und::camera_ok(cams + (long)row[i] * und::kCam))
            res = und::point(cams + (long)row[i] * und::kCam, direction, xy[2 * i], xy[2 * i + 1], ox, oy);
        out[2 * i] = ox;
        out[2 * i + 1] = oy;
        residual[i] = res;
    }
}

// one image: src [Hs,Ws,3] through camera cam [12] into the undistorted camera ucam [8] -> dst [Hd,Wd,3], valid [Hd,Wd]
void hm_und_image(const unsigned char* src, long Hs, long Ws, const double* cam, const double* ucam, long Hd, long Wd,
                  unsigned char* dst, unsigned char* valid) {
    for (long y = 0; y < Hd; ++y)
        for (long x = 0; x < Wd; ++x) valid[y * Wd + x] = und::pixel(cam, ucam, src, Hs, Ws, x, y, dst + (y * Wd + x) * 3) ? 1 : 0;
}

// the source location of every output pixel: sxy [Hd,Wd,2]
void hm_und_sources(const double* cam, const double* ucam, long Hd, long Wd, double* sxy) {
    for (long y = 0; y < Hd; ++y)
        for (long x = 0; x < Wd; ++x) und::source_of(cam, ucam, x, y, sxy[(y * Wd + x) * 2], sxy[(y * Wd + x) * 2 + 1]);
}

int hm_und_newton_steps() { return und::kNewtonSteps; }

}  // extern "C"
