// Undistortion of a structure-from-motion scan on the GPU (the definition is undistort_math.h): the
// pinhole cameras of the undistorted images, points through the distortion and back, and the images themselves.
//
//   mvster_undistort_cameras   undistort_camera_kernel   one workgroup per camera, lanes strided over the 2 (W + H) border points;
//                                                         the extremes fold with min / max only (and an integer count), through
//                                                         LDS, so the result is the host loop's whatever the order; lane 0
//                                                         finishes the scalar arithmetic
//   mvster_undistort_points    undistort_points_kernel   one lane per point, a camera row each
//   mvster_undistort_images    undistort_images_kernel   all views of a chunk: one lane per group of 4 consecutive output pixels
//                                                         of a view's flat [Hd Wd] order; group_ptr [V+1] is the prefix sum of the
//                                                         views' groups.  A workgroup owns 256 consecutive groups, searches
//                                                         group_ptr once for the views they span and walks them, so a view's
//                                                         record and cameras are the same in every lane (scalar registers).
//                                                         12 output bytes leave as three dwords and 4 mask bytes
//                                                         as one; the last group of a view may be partial and stores bytes.
//                                                         Source taps are byte loads: neighbouring lanes read neighbouring
//                                                         source pixels.  No atomics, no LDS: two runs give the same bytes.
#include "common.hpp"
#include "undistort_math.h"

namespace {

constexpr int kWG = 256;
constexpr int kFold = 9;                  // the doubles of und::Border

typedef long long i64;

struct CameraArgs {
    const double* cams;               // [C,12]
    double* out;                      // [C,8]
    double blank, min_scale, max_scale, sx, sy;
    int given;                        // the caller's (sx, sy): no border walk
};

__global__ void __launch_bounds__(kWG) undistort_camera_kernel(CameraArgs a) {
    __shared__ double fold[kFold][kWG];
    __shared__ long over[kWG];
    const int t = threadIdx.x;
    double c[und::kCam];
    for (int k = 0; k < und::kCam; ++k) c[k] = a.cams[(i64)blockIdx.x * und::kCam + k];
    double* out = a.out + (i64)blockIdx.x * und::kOut;
    if (!und::camera_ok(c)) {                                                   // the same in every lane
        if (t == 0) und::camera_none(out);
        return;
    }
    if (a.given) {
        if (t == 0) und::camera_of(c, a.sx, a.sy, 0.0, 0, out);
        return;
    }
    und::Border e = und::border_empty();
    const long n = und::border_points(c);
    for (long i = t; i < n; i += kWG) und::border_add(c, i, e);
    fold[0][t] = e.left_min;
    fold[1][t] = e.left_max;
    fold[2][t] = e.right_min;
    fold[3][t] = e.right_max;
    fold[4][t] = e.top_min;
    fold[5][t] = e.top_max;
    fold[6][t] = e.bottom_min;
    fold[7][t] = e.bottom_max;
    fold[8][t] = e.worst;
    over[t] = e.over;
    __syncthreads();
    for (int s = kWG / 2; s > 0; s >>= 1) {
        if (t < s) {
            und::Border x, y;
            x.left_min = fold[0][t], y.left_min = fold[0][t + s];
            x.left_max = fold[1][t], y.left_max = fold[1][t + s];
            x.right_min = fold[2][t], y.right_min = fold[2][t + s];
            x.right_max = fold[3][t], y.right_max = fold[3][t + s];
            x.top_min = fold[4][t], y.top_min = fold[4][t + s];
            x.top_max = fold[5][t], y.top_max = fold[5][t + s];
            x.bottom_min = fold[6][t], y.bottom_min = fold[6][t + s];
            x.bottom_max = fold[7][t], y.bottom_max = fold[7][t + s];
            x.worst = fold[8][t], y.worst = fold[8][t + s];
            x.over = over[t], y.over = over[t + s];
            und::border_merge(x, y);
            fold[0][t] = x.left_min;
            fold[1][t] = x.left_max;
            fold[2][t] = x.right_min;
            fold[3][t] = x.right_max;
            fold[4][t] = x.top_min;
            fold[5][t] = x.top_max;
            fold[6][t] = x.bottom_min;
            fold[7][t] = x.bottom_max;
            fold[8][t] = x.worst;
            over[t] = x.over;
        }
        __syncthreads();
    }
    if (t == 0) {
        e.left_min = fold[0][0];
        e.left_max = fold[1][0];
        e.right_min = fold[2][0];
        e.right_max = fold[3][0];
        e.top_min = fold[4][0];
        e.top_max = fold[5][0];
        e.bottom_min = fold[6][0];
        e.bottom_max = fold[7][0];
        double sx, sy;
        und::scales_of(c, e, a.blank, a.min_scale, a.max_scale, sx, sy);
        und::camera_of(c, sx, sy, fold[8][0], over[0], out);
    }
}

__global__ void __launch_bounds__(kWG) undistort_points_kernel(const double* __restrict__ cams, int C, const int* __restrict__ row,
                                                               i64 N, int direction, const double* __restrict__ xy,
                                                               double* __restrict__ out, double* __restrict__ residual) {
    const i64 i = (i64)blockIdx.x * kWG + threadIdx.x;
    if (i >= N) return;
    const int r = row[i];
    double ox = und::inf64(), oy = und::inf64(), res = und::inf64();            // a row outside the table: nothing can be said
    if (r >= 0 && r < C) {
        double c[und::kCam];
        for (int k = 0; k < und::kCam; ++k) c[k] = cams[(i64)r * und::kCam + k];
        if (und::camera_ok(c)) res = und::point(c, direction, xy[2 * i], xy[2 * i + 1], ox, oy);
    }
    out[2 * i] = ox;
    out[2 * i + 1] = oy;
    residual[i] = res;
}

// a view of mvster_undistort_images: 8 int64
struct View {
    i64 src, dst, valid;              // byte offsets into the three buffers; dst and valid multiples of 16
    i64 Hs, Ws, Hd, Wd;
    i64 cam;                          // its row in both camera tables
};

// the last v in [0, V-1] with ptr[v] <= g
__device__ __forceinline__ int find_view(const i64* __restrict__ ptr, int V, i64 g) {
    int lo = 0, hi = V - 1;
    while (lo < hi) {                                                           // at most 31 halvings
        const int mid = lo + (hi - lo + 1) / 2;
        if (ptr[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Group `group` (4 consecutive pixels from pixel 4 group on) of view w, which is the same in every lane of the workgroup: its
// record and its two cameras sit in scalar registers.  v = the row's normalised coordinate is formed once per row, not per pixel.
__device__ __forceinline__ void undistort_group(const View& w, i64 group, const unsigned char* __restrict__ src_all,
                                                unsigned char* __restrict__ dst_all, unsigned char* __restrict__ valid_all,
                                                const double* __restrict__ cams, const double* __restrict__ ucams) {
    const i64 npix = w.Hd * w.Wd, first = group * 4;
    if (first >= npix) return;
    double c[und::kCam], o[und::kOut];
    for (int k = 0; k < und::kCam; ++k) c[k] = cams[w.cam * und::kCam + k];
    for (int k = 0; k < und::kOut; ++k) o[k] = ucams[w.cam * und::kOut + k];
    const unsigned char* src = src_all + w.src;
    const int count = npix - first < 4 ? (int)(npix - first) : 4;
    i64 y, x;
    if (npix < (1ll << 31)) {                                                   // (the same in every lane: 32-bit division)
        const unsigned q = (unsigned)first / (unsigned)w.Wd;
        y = q;
        x = (unsigned)first - q * (unsigned)w.Wd;
    } else {
        y = first / w.Wd;
        x = first - y * w.Wd;
    }
    unsigned char rgb[12], ok[4];
    double v = und::source_v(o, y);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        rgb[3 * k] = rgb[3 * k + 1] = rgb[3 * k + 2] = 0;
        ok[k] = 0;
        if (k < count) ok[k] = und::pixel_at(c, src, w.Hs, w.Ws, und::source_u(o, x), v, rgb + 3 * k) ? 1 : 0;
        if (++x == w.Wd) {                                                      // a group may straddle a row end
            x = 0;
            ++y;
            v = und::source_v(o, y);
        }
    }
    unsigned char* dst = dst_all + w.dst + 3 * first;
    unsigned char* valid = valid_all + w.valid + first;
    if (count == 4) {
        unsigned* d32 = reinterpret_cast<unsigned*>(dst);                       // 12 (first / 4) past a multiple of 16
#pragma unroll
        for (int k = 0; k < 3; ++k)
            d32[k] = (unsigned)rgb[4 * k] | ((unsigned)rgb[4 * k + 1] << 8) | ((unsigned)rgb[4 * k + 2] << 16) |
                     ((unsigned)rgb[4 * k + 3] << 24);
        *reinterpret_cast<unsigned*>(valid) = (unsigned)ok[0] | ((unsigned)ok[1] << 8) | ((unsigned)ok[2] << 16) | ((unsigned)ok[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                           // (unrolled: rgb stays in registers)
            if (k < count) {
                dst[3 * k] = rgb[3 * k];
                dst[3 * k + 1] = rgb[3 * k + 1];
                dst[3 * k + 2] = rgb[3 * k + 2];
                valid[k] = ok[k];
            }
        }
    }
}

// A workgroup owns kWG consecutive groups.  It searches group_ptr once for the views its groups span (mostly one) and walks
// them; per view every lane whose group lies in it works.  Nothing read from the device tables is trusted as an address: a
// view whose extents leave its buffers, whose offsets are not aligned or whose camera row is outside the tables writes nothing.
__global__ void __launch_bounds__(kWG) undistort_images_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                               unsigned char* __restrict__ valid, i64 src_bytes, i64 dst_bytes,
                                                               i64 valid_bytes, const View* __restrict__ views,
                                                               const i64* __restrict__ group_ptr, const double* __restrict__ cams,
                                                               const double* __restrict__ ucams, int V, int C, i64 groups) {
    const i64 g0 = (i64)blockIdx.x * kWG;
    if (g0 >= groups) return;
    const i64 g1 = (g0 + kWG < groups ? g0 + kWG : groups) - 1;
    const int v0 = find_view(group_ptr, V, g0), v1 = find_view(group_ptr, V, g1);       // the same in every lane
    const i64 g = g0 + threadIdx.x;
    for (int vi = v0; vi <= v1; ++vi) {
        const i64 lo = group_ptr[vi], hi = group_ptr[vi + 1];
        const View w = views[vi];
        if (w.Hs < 1 || w.Ws < 1 || w.Hd < 1 || w.Wd < 1 || w.Hs > und::kMaxSide || w.Ws > und::kMaxSide || w.Hd > und::kMaxSide ||
            w.Wd > und::kMaxSide || w.cam < 0 || w.cam >= C)
            continue;
        const i64 npix = w.Hd * w.Wd;
        if (w.src < 0 || w.src + 3 * w.Hs * w.Ws > src_bytes || w.dst < 0 || (w.dst & 15) || w.dst + 3 * npix > dst_bytes ||
            w.valid < 0 || (w.valid & 15) || w.valid + npix > valid_bytes)
            continue;
        if (g < lo || g >= hi || g > g1) continue;
        undistort_group(w, g - lo, src, dst, valid, cams, ucams);
    }
}

}  // namespace

extern "C" int mvster_undistort_cameras(const double* cams, int C, double blank_pixels, double min_scale, double max_scale,
                                        int scale_given, double scale_x, double scale_y, double* out, void* stream) {
    if (!cams || !out) return MVSTER_ERR_NULL;
    if (C < 1 || C > (1 << 20)) return MVSTER_ERR_SHAPE;
    if (!(blank_pixels >= 0.0 && blank_pixels <= 1.0) || !(min_scale > 0.0) || !(max_scale >= min_scale) || !(max_scale <= 1024.0))
        return MVSTER_ERR_SHAPE;
    if (scale_given && !(scale_x > 0.0 && scale_x <= 1024.0 && scale_y > 0.0 && scale_y <= 1024.0)) return MVSTER_ERR_SHAPE;
    CameraArgs a;
    a.cams = cams;
    a.out = out;
    a.blank = blank_pixels;
    a.min_scale = min_scale;
    a.max_scale = max_scale;
    a.sx = scale_x;
    a.sy = scale_y;
    a.given = scale_given ? 1 : 0;
    MV_NOTE_KERNEL("undistort_camera_kernel");
    hipLaunchKernelGGL(undistort_camera_kernel, dim3((unsigned)C), dim3(kWG), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}

extern "C" int mvster_undistort_points(const double* cams, int C, const int* camera_row, long N, int direction, const double* xy,
                                       double* out, double* residual, void* stream) {
    if (!cams) return MVSTER_ERR_NULL;
    if (N > 0 && (!camera_row || !xy || !out || !residual)) return MVSTER_ERR_NULL;
    if (C < 1 || C > (1 << 20) || N < 0 || N >= (1l << 31) * kWG || (direction != 0 && direction != 1)) return MVSTER_ERR_SHAPE;
    if (N == 0) return MVSTER_OK;
    MV_NOTE_KERNEL("undistort_points_kernel");
    hipLaunchKernelGGL(undistort_points_kernel, dim3((unsigned)((N + kWG - 1) / kWG)), dim3(kWG), 0, (hipStream_t)stream, cams, C,
                       camera_row, (i64)N, direction, xy, out, residual);
    return mv_check_launch();
}

extern "C" int mvster_undistort_images(const unsigned char* src, long src_bytes, unsigned char* dst, long dst_bytes,
                                       unsigned char* valid, long valid_bytes, const long* views, const long* group_ptr, int V,
                                       long groups, const double* cams, const double* ucams, int C, void* stream) {
    if (!src || !dst || !valid || !views || !group_ptr || !cams || !ucams) return MVSTER_ERR_NULL;
    if (V < 1 || C < 1 || C > (1 << 20) || src_bytes < 1 || dst_bytes < 1 || valid_bytes < 1 || groups < 1 ||
        groups >= (1l << 31) * kWG)
        return MVSTER_ERR_SHAPE;
    if (((uintptr_t)dst & 15) || ((uintptr_t)valid & 15)) return MVSTER_ERR_SHAPE;
    MV_NOTE_KERNEL("undistort_images_kernel");
    hipLaunchKernelGGL(undistort_images_kernel, dim3((unsigned)((groups + kWG - 1) / kWG)), dim3(kWG), 0, (hipStream_t)stream, src, dst,
                       valid, (i64)src_bytes, (i64)dst_bytes, (i64)valid_bytes, reinterpret_cast<const View*>(views),
                       reinterpret_cast<const i64*>(group_ptr), cams, ucams, V, C, (i64)groups);
    return mv_check_launch();
}
