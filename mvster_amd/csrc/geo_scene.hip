// Depth-map fusion of a whole scan: the reference's filter_depth (test_mvs4.py:331-421) loops
// over the reference views of pair.txt on the CPU, and for each one over its source views (:362-385), builds the
// three masks (:361, :387-388), lifts the surviving pixels to world space (:397-407) and concatenates the per-view
// pieces (:409-418).  Here every map of the scan sits on the GPU once and three launches do all of it:
//
//   geo_scene_filter_kernel  one thread per (reference view, pixel): walks that view's row of the pair table in
//                            pair-file order with the arithmetic of geo_math.h, writes votes, averaged depth, the three
//                            masks, and the survivor count of its workgroup (a workgroup never straddles two views);
//   geo_scene_scan_kernel    exclusive scan of the workgroup counts into 64-bit offsets, one workgroup, 16 counts per
//                            thread and pass; offsets[n] is the number of points, the one value the host reads back;
//   geo_scene_emit_kernel    the same grid again: every survivor ranks itself inside its workgroup (ballot + popcount),
//                            adds the workgroup's offset and writes its point and colour there.
//
// The output order is the reference's (reference views in pair-file order, pixels row-major) and comes from the scan
// alone: no atomics, two runs give the same bytes.
#include "common.hpp"
#include "geo_math.h"

namespace {

constexpr int kWG = 256;              // threads (= pixels) per workgroup of the filter and emit passes
constexpr int kScanThreads = 1024;
constexpr int kScanItems = 16;        // counts per thread and pass of the scan

struct SceneFilterArgs {
    const float* depth;          // [V, H, W]
    const float* conf;           // [V, H, W]
    const int* pairs;            // [R, Smax] source-view indices, -1 = padding
    const int* ref_view;         // [R]
    const double* ref_mats;      // [R, 30]
    const double* view_mats;     // [R, Smax, 42]
    int* mask_sum;               // [R, H, W]
    double* depth_avg;           // [R, H, W]
    unsigned char* photo_mask;   // [R, H, W] 0 / 1
    unsigned char* geo_mask;
    unsigned char* final_mask;
    int* wg_counts;              // [R * nblk]
    int R, Smax, V, H, W, nblk, thres_view;
    float conf_thres, pix_thres, rel_thres;
};

__global__ void __launch_bounds__(kWG) geo_scene_filter_kernel(SceneFilterArgs a) {
    __shared__ int wave_count[kWG / 64];
    const long hw = (long)a.H * a.W;
    const int r = (int)(blockIdx.x / (unsigned)a.nblk), blk = (int)(blockIdx.x - (unsigned)r * (unsigned)a.nblk);
    const long p = (long)blk * kWG + threadIdx.x;
    const int rv = a.ref_view[r];
    const bool inside = p < hw;
    const bool valid = inside && (unsigned)rv < (unsigned)a.V;
    bool fin = false;
    if (valid) {
        const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
        const double* rm = a.ref_mats + (long)r * geo::kRefDoubles;
        const float dref = a.depth[(long)rv * hw + p];
        double rx, ry, rz;
        geo::lift_ref(rm, x, y, dref, rx, ry, rz);
        int count = 0;
        float dsum = 0.0f;
        for (int s = 0; s < a.Smax; ++s) {
            const int sv = a.pairs[(long)r * a.Smax + s];
            if ((unsigned)sv >= (unsigned)a.V) break;                       // -1: end of this view's source list
            const geo::Vote vt = geo::view_vote(a.depth + (long)sv * hw, a.H, a.W, rm,
                                                a.view_mats + ((long)r * a.Smax + s) * geo::kViewDoubles, x, y, dref, rx, ry,
                                                rz, a.pix_thres, a.rel_thres);
            geo::accumulate(vt, count, dsum);
        }
        const bool photo = a.conf[(long)rv * hw + p] > a.conf_thres;
        const bool g = count >= a.thres_view;
        fin = photo && g;
        const long o = (long)r * hw + p;
        a.mask_sum[o] = count;
        a.depth_avg[o] = geo::average(dsum, dref, count);
        a.photo_mask[o] = photo ? 1 : 0;
        a.geo_mask[o] = g ? 1 : 0;
        a.final_mask[o] = fin ? 1 : 0;
    } else if (inside) {                                                    // a view index outside the stack: nothing survives
        const long o = (long)r * hw + p;
        a.mask_sum[o] = 0;
        a.depth_avg[o] = 0.0;
        a.photo_mask[o] = 0;
        a.geo_mask[o] = 0;
        a.final_mask[o] = 0;
    }
    const unsigned long long b = __ballot(fin);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < kWG / 64; ++w) c += wave_count[w];
        a.wg_counts[blockIdx.x] = c;
    }
}

struct SceneDynamicArgs {
    SceneFilterArgs f;           // pix_thres / rel_thres unused
    unsigned char* geo_level;    // [R, H, W] the level that kept the pixel, 0 = none
    float pix_base, rel_base;
};

// The filter pass under dynamic consistency checking (geo::dynamic_votes): same grid, same outputs and the same workgroup
// count as geo_scene_filter_kernel, plus geo_level; the level counts are a packed histogram in registers.
__global__ void __launch_bounds__(kWG) geo_scene_dynamic_filter_kernel(SceneDynamicArgs d) {
    __shared__ int wave_count[kWG / 64];
    const SceneFilterArgs& a = d.f;
    const long hw = (long)a.H * a.W;
    const int r = (int)(blockIdx.x / (unsigned)a.nblk), blk = (int)(blockIdx.x - (unsigned)r * (unsigned)a.nblk);
    const long p = (long)blk * kWG + threadIdx.x;
    const int rv = a.ref_view[r];
    const bool inside = p < hw;
    const bool valid = inside && (unsigned)rv < (unsigned)a.V;
    bool fin = false;
    if (valid) {
        const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
        const double* rm = a.ref_mats + (long)r * geo::kRefDoubles;
        const float dref = a.depth[(long)rv * hw + p];
        double rx, ry, rz;
        geo::lift_ref(rm, x, y, dref, rx, ry, rz);
        const geo::DynamicVotes v = geo::dynamic_votes(a.depth, hw, a.H, a.W, a.pairs + (long)r * a.Smax, a.Smax, a.V, rm,
                                                       a.view_mats + (long)r * a.Smax * geo::kViewDoubles, x, y, dref, rx,
                                                       ry, rz, a.thres_view, d.pix_base, d.rel_base);
        const bool photo = a.conf[(long)rv * hw + p] > a.conf_thres;
        const bool g = v.level != 0;
        fin = photo && g;
        const long o = (long)r * hw + p;
        a.mask_sum[o] = v.count;
        a.depth_avg[o] = geo::average(v.dsum, dref, v.count);
        a.photo_mask[o] = photo ? 1 : 0;
        a.geo_mask[o] = g ? 1 : 0;
        a.final_mask[o] = fin ? 1 : 0;
        d.geo_level[o] = (unsigned char)v.level;
    } else if (inside) {                                                    // a view index outside the stack: nothing survives
        const long o = (long)r * hw + p;
        a.mask_sum[o] = 0;
        a.depth_avg[o] = 0.0;
        a.photo_mask[o] = 0;
        a.geo_mask[o] = 0;
        a.final_mask[o] = 0;
        d.geo_level[o] = 0;
    }
    const unsigned long long b = __ballot(fin);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < kWG / 64; ++w) c += wave_count[w];
        a.wg_counts[blockIdx.x] = c;
    }
}

// offsets[i] = sum(counts[0..i)), i = 0..n
__global__ void __launch_bounds__(kScanThreads) geo_scene_scan_kernel(const int* __restrict__ counts, long* __restrict__ offsets,
                                                                      long n) {
    __shared__ long wave_sum[kScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long carry = 0;
    for (long base = 0; base < n; base += (long)kScanThreads * kScanItems) {
        const long first = base + (long)tid * kScanItems;
        int v[kScanItems];
        long mine = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            v[k] = first + k < n ? counts[first + k] : 0;
            mine += v[k];
        }
        long incl = mine;                                                   // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        long before = 0, total = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) {
            const long ws = wave_sum[w];
            if (w < wave) before += ws;
            total += ws;
        }
        long run = carry + before + incl - mine;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            if (first + k < n) offsets[first + k] = run;
            run += v[k];
        }
        carry += total;
        __syncthreads();                                                    // wave_sum is rewritten by the next pass
    }
    if (tid == 0) offsets[n] = carry;
}

struct SceneEmitArgs {
    const double* depth_avg;          // [R, H, W]
    const unsigned char* final_mask;  // [R, H, W]
    const int* ref_view;              // [R]
    const double* ref_mats;           // [R, 30]
    const void* images;               // [V, H, W, 3] u8 or f32 (0..1)
    const long* offsets;              // [R * nblk + 1]
    float* points;                    // [M, 3]
    unsigned char* colors;            // [M, 3]
    long M;
    int R, V, H, W, nblk, image_f32;
};

__global__ void __launch_bounds__(kWG) geo_scene_emit_kernel(SceneEmitArgs a) {
    __shared__ int wave_count[kWG / 64];
    const long hw = (long)a.H * a.W;
    const int r = (int)(blockIdx.x / (unsigned)a.nblk), blk = (int)(blockIdx.x - (unsigned)r * (unsigned)a.nblk);
    const long p = (long)blk * kWG + threadIdx.x;
    const int rv = a.ref_view[r];
    const bool valid = p < hw && (unsigned)rv < (unsigned)a.V;
    const bool fin = valid && a.final_mask[(long)r * hw + p] != 0;
    const unsigned long long b = __ballot(fin);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = __popcll(b);
    __syncthreads();
    if (!fin) return;
    long dst = a.offsets[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) dst += wave_count[w];
    if (dst >= a.M) return;                                                 // capacity of the caller's buffers
    const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
    const double* rm = a.ref_mats + (long)r * geo::kRefDoubles;
    double wx, wy, wz;
    geo::backproject(rm, rm + 18, x, y, a.depth_avg[(long)r * hw + p], wx, wy, wz);
    a.points[dst * 3 + 0] = (float)wx;                                      // fp64 world point rounded once
    a.points[dst * 3 + 1] = (float)wy;
    a.points[dst * 3 + 2] = (float)wz;
    const long src = ((long)rv * hw + p) * 3;
    unsigned char c0, c1, c2;
    if (a.image_f32) {
        const float* im = static_cast<const float*>(a.images) + src;
        c0 = geo::color_u8(im[0]); c1 = geo::color_u8(im[1]); c2 = geo::color_u8(im[2]);
    } else {                                                                // (v / 255f * 255f) truncated is v for all 256 values
        const unsigned char* im = static_cast<const unsigned char*>(a.images) + src;
        c0 = im[0]; c1 = im[1]; c2 = im[2];
    }
    a.colors[dst * 3 + 0] = c0;
    a.colors[dst * 3 + 1] = c1;
    a.colors[dst * 3 + 2] = c2;
}

long scene_blocks(int R, int H, int W) { return (long)R * (((long)H * W + kWG - 1) / kWG); }

}  // namespace

int mv_scan_counts(const int* counts, long* offsets, long n, hipStream_t stream) {
    hipLaunchKernelGGL(geo_scene_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, counts, offsets, n);
    return mv_check_launch();
}

extern "C" int mvster_geo_scene_blocks(int R, int H, int W) {
    if (R <= 0 || H <= 0 || W <= 0) return MVSTER_ERR_SHAPE;
    const long n = scene_blocks(R, H, W);
    return n > 0x7fffffffL - 1 ? MVSTER_ERR_SHAPE : (int)n;
}

extern "C" int mvster_geo_scene_filter(const float* depth, const float* confidence, const int* pairs, const int* ref_view,
                                       const double* ref_mats, const double* view_mats, int* mask_sum, double* depth_avg,
                                       unsigned char* photo_mask, unsigned char* geo_mask, unsigned char* final_mask,
                                       int* wg_counts, long* wg_offsets, int R, int Smax, int V, int H, int W,
                                       float conf_thres, int thres_view, float pix_thres, float rel_thres, void* stream) {
    if (!depth || !confidence || !pairs || !ref_view || !ref_mats || !view_mats || !mask_sum || !depth_avg || !photo_mask ||
        !geo_mask || !final_mask || !wg_counts || !wg_offsets)
        return MVSTER_ERR_NULL;
    if (R <= 0 || Smax <= 0 || V <= 0 || H <= 0 || W <= 0) return MVSTER_ERR_SHAPE;
    const int nwg = mvster_geo_scene_blocks(R, H, W);
    if (nwg < 0) return MVSTER_ERR_SHAPE;
    SceneFilterArgs a;
    a.depth = depth; a.conf = confidence; a.pairs = pairs; a.ref_view = ref_view; a.ref_mats = ref_mats;
    a.view_mats = view_mats; a.mask_sum = mask_sum; a.depth_avg = depth_avg; a.photo_mask = photo_mask;
    a.geo_mask = geo_mask; a.final_mask = final_mask; a.wg_counts = wg_counts;
    a.R = R; a.Smax = Smax; a.V = V; a.H = H; a.W = W; a.nblk = nwg / R; a.thres_view = thres_view;
    a.conf_thres = conf_thres; a.pix_thres = pix_thres; a.rel_thres = rel_thres;
    hipLaunchKernelGGL(geo_scene_filter_kernel, dim3((unsigned)nwg), dim3(kWG), 0, (hipStream_t)stream, a);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    return mv_scan_counts(wg_counts, wg_offsets, (long)nwg, (hipStream_t)stream);
}

extern "C" int mvster_geo_scene_filter_dynamic(const float* depth, const float* confidence, const int* pairs,
                                               const int* ref_view, const double* ref_mats, const double* view_mats,
                                               int* mask_sum, double* depth_avg, unsigned char* photo_mask,
                                               unsigned char* geo_mask, unsigned char* final_mask, unsigned char* geo_level,
                                               int* wg_counts, long* wg_offsets, int R, int Smax, int V, int H, int W,
                                               float conf_thres, int thres_view, float pix_base, float rel_base,
                                               void* stream) {
    if (!depth || !confidence || !pairs || !ref_view || !ref_mats || !view_mats || !mask_sum || !depth_avg || !photo_mask ||
        !geo_mask || !final_mask || !geo_level || !wg_counts || !wg_offsets)
        return MVSTER_ERR_NULL;
    if (R <= 0 || Smax <= 0 || V <= 0 || H <= 0 || W <= 0) return MVSTER_ERR_SHAPE;
    const int nwg = mvster_geo_scene_blocks(R, H, W);
    if (nwg < 0) return MVSTER_ERR_SHAPE;
    if (Smax > geo::kMaxLevelSources) return MVSTER_ERR_UNSUPPORTED;       // the level counts hold 32 sources
    if (thres_view < 1) return MVSTER_ERR_SHAPE;
    if (!(pix_base > 0.0f) || !(rel_base > 0.0f) || std::isinf(pix_base) || std::isinf(rel_base)) return MVSTER_ERR_SHAPE;
    SceneDynamicArgs d;
    SceneFilterArgs& a = d.f;
    a.depth = depth; a.conf = confidence; a.pairs = pairs; a.ref_view = ref_view; a.ref_mats = ref_mats;
    a.view_mats = view_mats; a.mask_sum = mask_sum; a.depth_avg = depth_avg; a.photo_mask = photo_mask;
    a.geo_mask = geo_mask; a.final_mask = final_mask; a.wg_counts = wg_counts;
    a.R = R; a.Smax = Smax; a.V = V; a.H = H; a.W = W; a.nblk = nwg / R; a.thres_view = thres_view;
    a.conf_thres = conf_thres; a.pix_thres = 0.0f; a.rel_thres = 0.0f;
    d.geo_level = geo_level; d.pix_base = pix_base; d.rel_base = rel_base;
    hipLaunchKernelGGL(geo_scene_dynamic_filter_kernel, dim3((unsigned)nwg), dim3(kWG), 0, (hipStream_t)stream, d);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    return mv_scan_counts(wg_counts, wg_offsets, (long)nwg, (hipStream_t)stream);
}

extern "C" int mvster_geo_scene_emit(const double* depth_avg, const unsigned char* final_mask, const int* ref_view,
                                     const double* ref_mats, const void* images, int image_kind, const long* wg_offsets,
                                     float* points, unsigned char* colors, long M, int R, int V, int H, int W,
                                     void* stream) {
    if (!depth_avg || !final_mask || !ref_view || !ref_mats || !images || !wg_offsets) return MVSTER_ERR_NULL;
    if (M > 0 && (!points || !colors)) return MVSTER_ERR_NULL;
    if (M < 0 || R <= 0 || V <= 0 || H <= 0 || W <= 0) return MVSTER_ERR_SHAPE;
    if (image_kind != 0 && image_kind != 1) return MVSTER_ERR_UNSUPPORTED;
    const int nwg = mvster_geo_scene_blocks(R, H, W);
    if (nwg < 0) return MVSTER_ERR_SHAPE;
    if (M == 0) return MVSTER_OK;                                           // nothing survived: nothing to write
    SceneEmitArgs a;
    a.depth_avg = depth_avg; a.final_mask = final_mask; a.ref_view = ref_view; a.ref_mats = ref_mats; a.images = images;
    a.offsets = wg_offsets; a.points = points; a.colors = colors; a.M = M;
    a.R = R; a.V = V; a.H = H; a.W = W; a.nblk = nwg / R; a.image_f32 = image_kind;
    hipLaunchKernelGGL(geo_scene_emit_kernel, dim3((unsigned)nwg), dim3(kWG), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}
