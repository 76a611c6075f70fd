// Geometric-consistency filter of the depth-map fusion step: what the reference does per
// (reference view, source view) pair with NumPy + cv2.remap on the CPU (test_mvs4.py:273-328) and then sums over
// the source views (:362-385), as ONE launch per reference view.  One thread per reference pixel walks all source
// views: lift the pixel with the reference depth, project into the source view, sample the source depth map
// (cv2.remap INTER_LINEAR semantics: coordinates quantised to 1/32 pixel, constant-0 border), lift with the
// sampled depth, project back, and keep the view if the pixel lands within 1 px and 1 % relative depth.  The per-pixel
// arithmetic lives in geo_math.h (shared with geo_scene.hip and the host build of the CPU tests).
// HBM-bound and tiny: per pixel and view 4 gathered floats; the geometry runs in fp64 like NumPy's
// (float32 matrices x float64 points), the maps and the comparisons in fp32 exactly where the reference casts.
#include "common.hpp"
#include "geo_math.h"

namespace {

struct GeoArgs {
    const float* depth_ref;    // [H, W]
    const float* depth_src;    // [NS, H, W]
    const double* ref_mats;    // inv(K_ref)[9], K_ref[9]
    const double* view_mats;   // [NS, 42]
    int* mask_sum;             // [H, W]
    float* depth_sum;          // [H, W]  sum over views of the masked reprojected depth (view order)
    unsigned char* view_mask;  // optional [NS, H, W]
    float* view_depth;         // optional [NS, H, W]
    float* x_src;              // optional [NS, H, W]
    float* y_src;              // optional [NS, H, W]
    int NS, H, W;
    float pix_thres, rel_thres;
};

__global__ void __launch_bounds__(256) geo_filter_kernel(GeoArgs a) {
    const long hw = (long)a.H * a.W;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
    const float dref = a.depth_ref[p];
    double rx, ry, rz;
    geo::lift_ref(a.ref_mats, x, y, dref, rx, ry, rz);
    int count = 0;
    float dsum = 0.0f;
    for (int v = 0; v < a.NS; ++v) {
        const geo::Vote r = geo::view_vote(a.depth_src + (long)v * hw, a.H, a.W, a.ref_mats,
                                           a.view_mats + (long)v * geo::kViewDoubles, x, y, dref, rx, ry, rz, a.pix_thres,
                                           a.rel_thres);
        geo::accumulate(r, count, dsum);
        if (a.view_mask) a.view_mask[(long)v * hw + p] = r.ok ? 1 : 0;
        if (a.view_depth) a.view_depth[(long)v * hw + p] = r.depth;
        if (a.x_src) a.x_src[(long)v * hw + p] = r.x_src;
        if (a.y_src) a.y_src[(long)v * hw + p] = r.y_src;
    }
    a.mask_sum[p] = count;
    a.depth_sum[p] = dsum;
}

}  // namespace

extern "C" int mvster_geo_filter(const float* depth_ref, const float* depth_src, const double* ref_mats,
                                 const double* view_mats, int* mask_sum, float* depth_sum, unsigned char* view_mask,
                                 float* view_depth, float* x_src, float* y_src, int NS, int H, int W, float pix_thres,
                                 float rel_thres, void* stream) {
    if (!depth_ref || !depth_src || !ref_mats || !view_mats || !mask_sum || !depth_sum) return MVSTER_ERR_NULL;
    if (NS <= 0 || H <= 0 || W <= 0) return MVSTER_ERR_SHAPE;
    GeoArgs a;
    a.depth_ref = depth_ref; a.depth_src = depth_src; a.ref_mats = ref_mats; a.view_mats = view_mats;
    a.mask_sum = mask_sum; a.depth_sum = depth_sum; a.view_mask = view_mask; a.view_depth = view_depth;
    a.x_src = x_src; a.y_src = y_src; a.NS = NS; a.H = H; a.W = W; a.pix_thres = pix_thres; a.rel_thres = rel_thres;
    const long hw = (long)H * W;
    hipLaunchKernelGGL(geo_filter_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}
