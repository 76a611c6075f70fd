// Validation pass (train_mvs4.py:140-192, test_sample_depth :252-307) without a host synchronisation:
//   * the four depth metrics every sample reports (utils.py:125-159: AbsDepthError_metrics, Thres_metrics at 2 / 4 / 8 mm).
//     The reference forms them with boolean-mask gathers (depth_est[mask]: a device synchronisation, not capturable) per
//     image and per metric; here one pass over est / gt / mask gives every image's count of valid pixels, sum of errors
//     and count of errors above each threshold, and a one-workgroup finish turns them into the batch's metrics.
//   * DictAverageMeter.update (utils.py:103-122) on the device: the epoch's running sums of a sample's scalars.
// Both latency-bound: 12 bytes per pixel over a few MB, and 17 numbers.
#include "common.hpp"

namespace {

constexpr int kMaxThres = 8;
constexpr int kChunk = 2048;         // pixels a workgroup covers at least (two float4 rounds of 256 lanes)
constexpr int kMaxSlots = 256;       // workgroups per image at most (the finish sums an image's slots serially)

struct Thresholds { float t[kMaxThres]; };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// pixels of one image a slot covers: a multiple of 4, so that every slot of a float4-able image starts on a 16-byte boundary
__host__ __device__ inline long slot_len(long HW, int slots) { return ((HW + slots - 1) / slots + 3) & ~3L; }

// One workgroup = (image n, slot c): pixels [c * len, min((c + 1) * len, HW)) of image n, in rounds of 1024 with lane t on
// pixels 4t .. 4t + 3 of a round -- one float4 per plane when `vec` (HW % 4 == 0 and 16-byte aligned planes), four guarded
// scalar loads otherwise: the same pixels in the same order either way, so the sums do not depend on the alignment.
// partial [N][slots][2 + K] doubles: valid pixels, sum of e, #{e > t[k]} (LE: #{e <= t[k]} -- counted, not derived as valid
// minus above: a NaN error is neither); fixed order (lane, wave shuffles, the four waves through LDS), no atomics.  An empty
// slot (c * len >= HW) writes zeros.
template <bool LE>
__global__ void __launch_bounds__(256) depth_metrics_partial_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                                    const float* __restrict__ mask,
                                                                    const float* __restrict__ scale, Thresholds th, int K,
                                                                    long HW, int slots, int vec, double* __restrict__ partial) {
    __shared__ double red_sum[4];
    __shared__ unsigned red_cnt[4][1 + kMaxThres];
    const int n = blockIdx.x / slots, c = blockIdx.x - n * slots;
    const long len = slot_len(HW, slots);
    const long lo = (long)c * len, hi = lo + len < HW ? lo + len : HW;
    const float* e_ = est + (long)n * HW;
    const float* g_ = gt + (long)n * HW;
    const float* m_ = mask + (long)n * HW;
    const bool scaled = scale != nullptr;
    const float s = scaled ? scale[n] : 1.0f;
    double sum = 0.0;
    unsigned cnt[1 + kMaxThres];
#pragma unroll
    for (int k = 0; k <= kMaxThres; ++k) cnt[k] = 0u;
    for (long p = lo + 4 * (long)threadIdx.x; p < hi; p += 1024) {
        float ev[4], gv[4], mv[4];
        if (vec) {                                   // (hi - p is a multiple of 4 here)
            const f32x4 a = ld4(e_ + p), b = ld4(g_ + p), m = ld4(m_ + p);
#pragma unroll
            for (int j = 0; j < 4; ++j) { ev[j] = a[j]; gv[j] = b[j]; mv[j] = m[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = p + j < hi;
                ev[j] = in ? e_[p + j] : 0.0f;
                gv[j] = in ? g_[p + j] : 0.0f;
                mv[j] = in ? m_[p + j] : 0.0f;       // (past the end: not valid)
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(mv[j] > 0.5f)) continue;
            // every operation rounded on its own (no contraction into an FMA): the host restates it exactly
            const float e = scaled ? fabsf(__fsub_rn(__fmul_rn(ev[j], s), __fmul_rn(gv[j], s))) : fabsf(__fsub_rn(ev[j], gv[j]));
            cnt[0] += 1u;
            sum += (double)e;
#pragma unroll
            for (int k = 0; k < kMaxThres; ++k) cnt[1 + k] += (k < K && (LE ? e <= th.t[k] : e > th.t[k])) ? 1u : 0u;
        }
    }
    sum = wave_sum(sum);
#pragma unroll
    for (int k = 0; k <= kMaxThres; ++k) cnt[k] = wave_sum(cnt[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_sum[wave] = sum;
#pragma unroll
        for (int k = 0; k <= kMaxThres; ++k) red_cnt[wave][k] = cnt[k];
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < 2 + K) {
        double* out = partial + ((long)n * slots + c) * (2 + K);
        if (j == 1) {
            out[1] = (red_sum[0] + red_sum[1]) + (red_sum[2] + red_sum[3]);
        } else {
            const int k = j == 0 ? 0 : j - 1;
            out[j] = (double)((red_cnt[0][k] + red_cnt[1][k]) + (red_cnt[2][k] + red_cnt[3][k]));
        }
    }
}

// raw [N][2 + K] = an image's slots summed in index order (one thread per (image, column); the counts are integers below
// 2^53: exact); then, by thread j <= K, out [1 + K] = the metrics of the batch as compute_metrics_for_each_image forms them
// (utils.py:126-136): per image (float)(x / count) -- the quotient in double, rounded once -- and the fp32 mean over the
// images in image order.  An image without a valid pixel gives 0 / 0 = NaN, like torch.mean of an empty tensor.
__global__ void __launch_bounds__(256) depth_metrics_finish_kernel(const double* __restrict__ partial, int N, int K, int slots,
                                                                   double* __restrict__ raw, float* __restrict__ out) {
    const int cols = 2 + K;
    for (int i = threadIdx.x; i < N * cols; i += 256) {
        const int n = i / cols, j = i - n * cols;
        const double* p = partial + (long)n * slots * cols + j;
        double s = 0.0;
        for (int c = 0; c < slots; ++c) s += p[(long)c * cols];
        raw[i] = s;
    }
    __syncthreads();                 // (raw written above by this workgroup: visible to it after the barrier)
    if (threadIdx.x <= K) {
        const int j = threadIdx.x;
        float acc = 0.0f;
        for (int n = 0; n < N; ++n) acc = __fadd_rn(acc, (float)(raw[(long)n * cols + 1 + j] / raw[(long)n * cols]));
        out[j] = __fdiv_rn(acc, (float)N);
    }
}

// Blend_loss's error figures (MVS4Net.py:202-205), pooled over the batch: raw as above (its threshold columns hold
// #{e <= t[k]}); then, by thread j <= K, the columns summed over the images in image order (counts exact, the error sum
// fp64) and out [1 + K] = epe = (float)(sum_e / count) -- the quotient in double, rounded once -- and err_k =
// fl32(fl32(count_le_k / count) * 100): (err <= t).float().mean() * 100.  A batch without a valid pixel gives 0 / 0 = NaN.
__global__ void __launch_bounds__(256) pooled_metrics_finish_kernel(const double* __restrict__ partial, int N, int K, int slots,
                                                                    double* __restrict__ raw, float* __restrict__ out) {
    const int cols = 2 + K;
    for (int i = threadIdx.x; i < N * cols; i += 256) {
        const int n = i / cols, j = i - n * cols;
        const double* p = partial + (long)n * slots * cols + j;
        double s = 0.0;
        for (int c = 0; c < slots; ++c) s += p[(long)c * cols];
        raw[i] = s;
    }
    __syncthreads();                 // (raw written above by this workgroup: visible to it after the barrier)
    if (threadIdx.x <= K) {
        const int j = threadIdx.x;
        double count = 0.0, x = 0.0;
        for (int n = 0; n < N; ++n) {
            count += raw[(long)n * cols];
            x += raw[(long)n * cols + 1 + j];
        }
        const float q = (float)(x / count);
        out[j] = j == 0 ? q : __fmul_rn(q, 100.0f);
    }
}

constexpr int kMaxGather = 32;
struct ScalarPtrs { const float* p[kMaxGather]; };

// row[i] = *src.p[i], sums[i] += row[i] in double, count += 1: a step's scalars, scattered over as many device tensors,
// into one row and into the running sums in one launch
__global__ void __launch_bounds__(64) scalar_gather_accumulate_kernel(ScalarPtrs src, int n, float* __restrict__ row,
                                                                      double* __restrict__ sums, long* __restrict__ count) {
    const int i = threadIdx.x;
    if (i < n) {
        const float v = *src.p[i];
        row[i] = v;
        sums[i] += (double)v;
    }
    if (i == 0) count[0] += 1L;
}

// sums[i] += row[i] in double, count += 1; `reset`: both to zero instead (row is not read)
__global__ void __launch_bounds__(64) scalar_accumulate_kernel(const float* __restrict__ row, int n, double* __restrict__ sums,
                                                               long* __restrict__ count, int reset) {
    if (reset) {
        for (int i = threadIdx.x; i < n; i += 64) sums[i] = 0.0;
        if (threadIdx.x == 0) count[0] = 0L;
        return;
    }
    for (int i = threadIdx.x; i < n; i += 64) sums[i] += (double)row[i];
    if (threadIdx.x == 0) count[0] += 1L;
}

}  // namespace

// Workgroups per image of mvster_depth_metrics for planes of hw pixels (partial holds N * slots * (2 + K) doubles).
extern "C" int mvster_depth_metrics_slots(long hw) {
    const long b = (hw + kChunk - 1) / kChunk;
    return (int)(b < 1 ? 1 : (b > kMaxSlots ? kMaxSlots : b));
}

// est, gt, mask [N,HW] (mask > 0.5 = valid), scale [N] or null, thres [K] on the HOST (1 <= K <= 8) ->
//   partial [N][mvster_depth_metrics_slots(HW)][2 + K] doubles    (scratch)
//   raw     [N][2 + K] doubles: valid pixels, sum of e = |est*s - gt*s| over them, #{e > thres[k]}
//   out     [1 + K] floats: abs_depth_error, thres_k error of the batch (see the finish kernel)
// Two launches, no atomics: bit-reproducible.
extern "C" int mvster_depth_metrics(const float* est, const float* gt, const float* mask, const float* scale, const float* thres,
                                    int K, int N, long HW, double* partial, double* raw, float* out, void* stream) {
    if (!est || !gt || !mask || !thres || !partial || !raw || !out) return MVSTER_ERR_NULL;
    if (K < 1 || K > kMaxThres || N <= 0 || HW <= 0) return MVSTER_ERR_SHAPE;
    const int slots = mvster_depth_metrics_slots(HW);
    if ((long)N * slots >= (1L << 31) || (long)N * (2 + kMaxThres) >= (1L << 31)) return MVSTER_ERR_SHAPE;
    Thresholds th;
    for (int k = 0; k < kMaxThres; ++k) th.t[k] = k < K ? thres[k] : 0.0f;
    const int vec = (HW % 4 == 0) && ((((uintptr_t)est | (uintptr_t)gt | (uintptr_t)mask) & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_metrics_partial_kernel<false>, dim3((unsigned)(N * slots)), dim3(256), 0, s, est, gt, mask, scale, th,
                       K, HW, slots, vec, partial);
    hipLaunchKernelGGL(depth_metrics_finish_kernel, dim3(1), dim3(256), 0, s, partial, N, K, slots, raw, out);
    return mv_check_launch();
}

// Blend_loss's epe / err<t> (MVS4Net.py:202-205), pooled over all valid pixels of the batch: arguments as
// mvster_depth_metrics, the thresholds BY VALUE (thres [K] on the host is read before the call returns) ->
//   raw [N][2 + K] doubles: valid pixels, sum of e = |est*s - gt*s| over them, #{e <= thres[k]}
//   out [1 + K] floats: epe, err_k in per cent (see the finish kernel)
// Two launches, no atomics: bit-reproducible.
extern "C" int mvster_pooled_metrics(const float* est, const float* gt, const float* mask, const float* scale, const float* thres,
                                     int K, int N, long HW, double* partial, double* raw, float* out, void* stream) {
    if (!est || !gt || !mask || !thres || !partial || !raw || !out) return MVSTER_ERR_NULL;
    if (K < 1 || K > kMaxThres || N <= 0 || HW <= 0) return MVSTER_ERR_SHAPE;
    const int slots = mvster_depth_metrics_slots(HW);
    if ((long)N * slots >= (1L << 31) || (long)N * (2 + kMaxThres) >= (1L << 31)) return MVSTER_ERR_SHAPE;
    Thresholds th;
    for (int k = 0; k < kMaxThres; ++k) th.t[k] = k < K ? thres[k] : 0.0f;
    const int vec = (HW % 4 == 0) && ((((uintptr_t)est | (uintptr_t)gt | (uintptr_t)mask) & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_metrics_partial_kernel<true>, dim3((unsigned)(N * slots)), dim3(256), 0, s, est, gt, mask, scale, th,
                       K, HW, slots, vec, partial);
    hipLaunchKernelGGL(pooled_metrics_finish_kernel, dim3(1), dim3(256), 0, s, partial, N, K, slots, raw, out);
    return mv_check_launch();
}

// DictAverageMeter.update on the device: sums [n] doubles += row [n] floats, count [1] += 1.  One launch of one workgroup;
// reads and writes only through its arguments (capturable).
extern "C" int mvster_scalar_accumulate(const float* row, int n, double* sums, long* count, void* stream) {
    if (!row || !sums || !count) return MVSTER_ERR_NULL;
    if (n <= 0) return MVSTER_ERR_SHAPE;
    hipLaunchKernelGGL(scalar_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, row, n, sums, count, 0);
    return mv_check_launch();
}

// A training step's scalars into one row and into the running sums, one launch: ptrs [n] on the HOST = the device address of
// every scalar (1 <= n <= 32; read before the call returns) -> row [n] floats = the scalars, sums [n] doubles += them,
// count [1] += 1: torch.stack + mvster_scalar_accumulate, the same sums.  Reads and writes only through its arguments.
extern "C" int mvster_scalar_gather_accumulate(const void* const* ptrs, int n, float* row, double* sums, long* count,
                                               void* stream) {
    if (!ptrs || !row || !sums || !count) return MVSTER_ERR_NULL;
    if (n <= 0 || n > kMaxGather) return MVSTER_ERR_SHAPE;
    ScalarPtrs src;
    for (int i = 0; i < kMaxGather; ++i) {
        src.p[i] = i < n ? (const float*)ptrs[i] : nullptr;
        if (i < n && !src.p[i]) return MVSTER_ERR_NULL;
    }
    hipLaunchKernelGGL(scalar_gather_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, src, n, row, sums, count);
    return mv_check_launch();
}

// sums [n] = 0, count [1] = 0: a kernel, not a memset node (a captured sequence stays kernels only)
extern "C" int mvster_scalar_reset(double* sums, int n, long* count, void* stream) {
    if (!sums || !count) return MVSTER_ERR_NULL;
    if (n <= 0) return MVSTER_ERR_SHAPE;
    hipLaunchKernelGGL(scalar_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)nullptr, n, sums, count, 1);
    return mv_check_launch();
}
