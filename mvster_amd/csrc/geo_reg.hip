// The Tanks and Temples evaluation protocol on the GPU (the definition is reg_math.h): the similarity
// transform and the crop to the scene's polygon volume in one pass, the correspondence sums of an ICP iteration, and the
// distance histogram of the cumulative curves.  The nearest neighbours themselves are geo_nn.hip's, the thinning geo_thin.hip's.
//
//   mvster_reg_transform    reg_transform_kernel   one lane per point, grid-stride: out = (float)(T p)
//   mvster_reg_crop_flags   reg_crop_flags_kernel  one lane per point, a workgroup per tile of 256 points, grid-stride over the
//                                                  tiles: q = T p, flags[k] = inside(q); the polygon's edges are read at
//                                                  wave-uniform addresses and the fp64 division runs only for a crossing edge;
//                                                  wg_counts[tile] = the tile's kept points (ballot + popcount, no atomics)
//                           (mv_scan_counts)       wg_offsets [tiles + 1]: the exclusive scan; its last word is the kept count,
//                                                  the caller's one read-back
//   mvster_reg_crop_emit    reg_crop_emit_kernel   every kept point ranks itself (ballot + popcount + the tile's offset) and
//                                                  writes (float)q, its index and its colour: the input's order is kept
//   mvster_reg_sums         reg_sums_kernel        one row of 18 fp64 partial sums per workgroup over a contiguous run of
//                                                  source points: 18 accumulators in registers, wave shuffles, the four waves
//                                                  through LDS in wave order
//                           reg_sums_finish_kernel the rows in row order (staged through LDS 64 rows at a time)
//   mvster_reg_histogram    reg_hist_zero_kernel + reg_hist_kernel: an LDS sub-histogram per workgroup (integer atomics),
//                                                  flushed with one 64-bit integer atomic per non-empty bin
// No floating-point atomics anywhere: two runs give the same bytes.
#include "common.hpp"
#include "reg_math.h"

namespace {

constexpr int kWG = 256;
constexpr int kMaxGrid = 2048;            // workgroups of a grid-stride launch at most (8 per CU)
constexpr int kSumRows = 1024;            // rows of partial sums at most
constexpr int kSumChunk = 4096;           // source points a row covers at least
constexpr int kFinishRows = 64;           // rows the finish kernel stages at a time
constexpr int kHistChunk = 16 * kWG;      // distances a workgroup of the histogram covers at least

typedef unsigned long long u64;

struct Affine {
    double T[12];
    int use;                              // 0: q = (double)p
};

__device__ __forceinline__ void moved(const Affine& a, const float* __restrict__ points, long k, double* q, float* out) {
    const float p[3] = {points[k * 3 + 0], points[k * 3 + 1], points[k * 3 + 2]};
    if (a.use) {
        reg::transform(a.T, p, q);
#pragma unroll
        for (int j = 0; j < 3; ++j) out[j] = (float)q[j];
    } else {
        reg::widen(p, q);
#pragma unroll
        for (int j = 0; j < 3; ++j) out[j] = p[j];                          // bits unchanged
    }
}

long tiles_of(long n) { return (n + kWG - 1) / kWG; }

unsigned grid_of(long tiles, int cap) { return (unsigned)(tiles < cap ? tiles : cap); }

__global__ void __launch_bounds__(kWG) reg_transform_kernel(Affine a, const float* __restrict__ points, long N,
                                                            float* __restrict__ out) {
    for (long k = (long)blockIdx.x * kWG + threadIdx.x; k < N; k += (long)gridDim.x * kWG) {
        double q[3];
        float o[3];
        moved(a, points, k, q, o);
#pragma unroll
        for (int j = 0; j < 3; ++j) out[k * 3 + j] = o[j];
    }
}

// volume [2 + 2 P] doubles: axis_min, axis_max, then (u, v) of the P vertices
__global__ void __launch_bounds__(kWG) reg_crop_flags_kernel(Affine a, const float* __restrict__ points, long N,
                                                             const double* __restrict__ volume, int P, int axis, long tiles,
                                                             unsigned char* __restrict__ flags, int* __restrict__ wg_counts) {
    __shared__ int wave_count[kWG / 64];
    const double axis_min = volume[0], axis_max = volume[1];
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {         // uniform per workgroup: the barriers are met by all
        const long k = tile * kWG + threadIdx.x;
        bool in = false;
        if (k < N) {
            double q[3];
            float o[3];
            moved(a, points, k, q, o);
            in = reg::inside(q, axis, axis_min, axis_max, volume + 2, P);
            flags[k] = in ? 1 : 0;
        }
        const u64 b = __ballot(in);
        if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(b);
        __syncthreads();
        if (threadIdx.x == 0) wg_counts[tile] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
        __syncthreads();                                                    // wave_count is written again in the next tile
    }
}

__global__ void __launch_bounds__(kWG) reg_crop_emit_kernel(Affine a, const float* __restrict__ points,
                                                            const unsigned char* __restrict__ colors, long N,
                                                            const unsigned char* __restrict__ flags,
                                                            const long* __restrict__ offsets, long tiles, long K,
                                                            float* __restrict__ out_points, unsigned char* __restrict__ out_colors,
                                                            long* __restrict__ out_index) {
    __shared__ int wave_count[kWG / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long k = tile * kWG + threadIdx.x;
        const bool in = k < N && flags[k] != 0;
        const u64 b = __ballot(in);
        if (lane == 0) wave_count[wave] = __popcll(b);
        __syncthreads();
        if (in) {
            long r = offsets[tile] + __popcll(b & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) r += wave_count[w];
            if ((unsigned long)r < (unsigned long)K) {                      // capacity of the caller's buffers
                double q[3];
                float o[3];
                moved(a, points, k, q, o);
#pragma unroll
                for (int j = 0; j < 3; ++j) out_points[r * 3 + j] = o[j];
                out_index[r] = k;
                if (colors) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) out_colors[r * 3 + j] = colors[k * 3 + j];
                }
            }
        }
        __syncthreads();
    }
}

__host__ __device__ inline long row_len(long Q, int rows) { return (Q + rows - 1) / rows; }

// partial [rows][18].  Fixed order: a lane's points in index order, the wave's lanes by the shuffle tree, the four waves in
// wave order.  The count travels as a double (exact below 2^53).
__global__ void __launch_bounds__(kWG) reg_sums_kernel(const float* __restrict__ source, const long* __restrict__ index,
                                                       const double* __restrict__ dist2, long Q, const float* __restrict__ target,
                                                       long M, int rows, double* __restrict__ partial) {
    __shared__ double red[kWG / 64][reg::kSums];
    const long len = row_len(Q, rows);
    const long lo = (long)blockIdx.x * len, hi = lo + len < Q ? lo + len : Q;
    double acc[reg::kSums];
#pragma unroll
    for (int j = 0; j < reg::kSums; ++j) acc[j] = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += kWG) {
        const long t = index[i];
        if ((unsigned long)t >= (unsigned long)M) continue;                 // -1: no candidate, or an invalid query
        const float s[3] = {source[i * 3 + 0], source[i * 3 + 1], source[i * 3 + 2]};
        const float g[3] = {target[t * 3 + 0], target[t * 3 + 1], target[t * 3 + 2]};
        double term[reg::kSums];
        reg::pair_terms(s, g, dist2[i], term);
#pragma unroll
        for (int j = 0; j < reg::kSums; ++j) acc[j] += term[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < reg::kSums; ++j) acc[j] += __shfl_down(acc[j], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < reg::kSums; ++j) red[threadIdx.x >> 6][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < reg::kSums) {
        const int j = threadIdx.x;
        partial[(long)blockIdx.x * reg::kSums + j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
    }
}

__global__ void __launch_bounds__(kWG) reg_sums_finish_kernel(const double* __restrict__ partial, int rows, double* __restrict__ out) {
    __shared__ double stage[kFinishRows * reg::kSums];
    double s = 0.0;
    for (int base = 0; base < rows; base += kFinishRows) {
        const int n = rows - base < kFinishRows ? rows - base : kFinishRows;
        for (int i = threadIdx.x; i < n * reg::kSums; i += kWG) stage[i] = partial[(long)base * reg::kSums + i];
        __syncthreads();
        if (threadIdx.x < reg::kSums) {
            for (int r = 0; r < n; ++r) s += stage[r * reg::kSums + threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x < reg::kSums) out[threadIdx.x] = s;
}

__global__ void __launch_bounds__(kWG) reg_hist_zero_kernel(u64* __restrict__ hist, int bins) {
    const int i = blockIdx.x * kWG + threadIdx.x;
    if (i < bins) hist[i] = 0;
}

__global__ void __launch_bounds__(kWG) reg_hist_kernel(const float* __restrict__ dist, long N, const double* __restrict__ edges,
                                                       int bins, u64* hist) {
    __shared__ unsigned h[reg::kMaxBins];
    for (int i = threadIdx.x; i < bins; i += kWG) h[i] = 0u;
    __syncthreads();
    for (long k = (long)blockIdx.x * kWG + threadIdx.x; k < N; k += (long)gridDim.x * kWG) {
        const int b = reg::hist_bin((double)dist[k], edges, bins);
        if (b >= 0) atomicAdd(&h[b], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += kWG) {
        const unsigned c = h[i];
        if (c) atomicAdd(&hist[i], (u64)c);
    }
}

bool cloud_ok(long N) { return N > 0 && N <= (1l << 29); }

Affine affine_of(const double* T) {
    Affine a;
    a.use = T ? 1 : 0;
    for (int j = 0; j < 12; ++j) a.T[j] = T ? T[j] : 0.0;
    return a;
}

int sum_rows(long Q) {
    const long s = (Q + kSumChunk - 1) / kSumChunk;
    return (int)(s < kSumRows ? s : kSumRows);
}

}  // namespace

extern "C" int mvster_reg_blocks(long N) {
    if (!cloud_ok(N)) return MVSTER_ERR_SHAPE;
    return (int)tiles_of(N);
}

extern "C" int mvster_reg_transform(const float* points, long N, const double* T, float* out, void* stream) {
    if (!points || !T || !out) return MVSTER_ERR_NULL;
    if (!cloud_ok(N)) return MVSTER_ERR_SHAPE;
    hipLaunchKernelGGL(reg_transform_kernel, dim3(grid_of(tiles_of(N), kMaxGrid)), dim3(kWG), 0, (hipStream_t)stream, affine_of(T),
                       points, N, out);
    return mv_check_launch();
}

extern "C" int mvster_reg_crop_flags(const float* points, long N, const double* T, const double* volume, int P, int axis,
                                     int max_grid, unsigned char* flags, int* wg_counts, long* wg_offsets, void* stream) {
    if (!points || !volume || !flags || !wg_counts || !wg_offsets) return MVSTER_ERR_NULL;
    if (!cloud_ok(N) || P < reg::kMinPolygon || P > reg::kMaxPolygon || axis < 0 || axis > 2) return MVSTER_ERR_SHAPE;
    if (max_grid < 0 || max_grid > kMaxGrid) return MVSTER_ERR_SHAPE;
    const long tiles = tiles_of(N);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(reg_crop_flags_kernel, dim3(grid_of(tiles, max_grid ? max_grid : kMaxGrid)), dim3(kWG), 0, st, affine_of(T),
                       points, N, volume, P, axis, tiles, flags, wg_counts);
    const int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    return mv_scan_counts(wg_counts, wg_offsets, tiles, st);
}

extern "C" int mvster_reg_crop_emit(const float* points, const unsigned char* colors, long N, const double* T,
                                    const unsigned char* flags, const long* wg_offsets, long K, int max_grid, float* out_points,
                                    unsigned char* out_colors, long* out_index, void* stream) {
    if (!points || !flags || !wg_offsets) return MVSTER_ERR_NULL;
    if (!cloud_ok(N) || K < 0 || K > N || max_grid < 0 || max_grid > kMaxGrid) return MVSTER_ERR_SHAPE;
    if (K == 0) return MVSTER_OK;                                           // nothing kept: nothing to write
    if (!out_points || !out_index || (colors && !out_colors)) return MVSTER_ERR_NULL;
    const long tiles = tiles_of(N);
    hipLaunchKernelGGL(reg_crop_emit_kernel, dim3(grid_of(tiles, max_grid ? max_grid : kMaxGrid)), dim3(kWG), 0, (hipStream_t)stream,
                       affine_of(T), points, colors, N, flags, wg_offsets, tiles, K, out_points, out_colors, out_index);
    return mv_check_launch();
}

extern "C" int mvster_reg_sum_rows(long Q) {
    if (!cloud_ok(Q)) return MVSTER_ERR_SHAPE;
    return sum_rows(Q);
}

extern "C" int mvster_reg_sums(const float* source, const long* index, const double* dist2, long Q, const float* target, long M,
                               double* partial, double* out, void* stream) {
    if (!source || !index || !dist2 || !partial || !out) return MVSTER_ERR_NULL;
    if (!cloud_ok(Q) || M < 0 || M > (1l << 29) || (M > 0 && !target)) return MVSTER_ERR_SHAPE;
    const int rows = sum_rows(Q);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(reg_sums_kernel, dim3((unsigned)rows), dim3(kWG), 0, st, source, index, dist2, Q, target, M, rows, partial);
    const int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(reg_sums_finish_kernel, dim3(1), dim3(kWG), 0, st, partial, rows, out);
    return mv_check_launch();
}

extern "C" int mvster_reg_histogram(const float* dist, long N, const double* edges, int bins, unsigned long long* hist,
                                    void* stream) {
    if (!dist || !edges || !hist) return MVSTER_ERR_NULL;
    if (!cloud_ok(N) || bins < 1 || bins > reg::kMaxBins) return MVSTER_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(reg_hist_zero_kernel, dim3((unsigned)((bins + kWG - 1) / kWG)), dim3(kWG), 0, st, hist, bins);
    const int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    const long chunks = (N + kHistChunk - 1) / kHistChunk;
    hipLaunchKernelGGL(reg_hist_kernel, dim3(grid_of(chunks, kMaxGrid)), dim3(kWG), 0, st, dist, N, edges, bins, hist);
    return mv_check_launch();
}
