// The DTU evaluation protocol on the GPU (the definition is eval_math.h): the point reduction of
// reducePts_haa.m, the observability mask, ground plane and block cover of PointCompareMain.m / MaxDistCP.m, and the statistics
// of ComputeStat_func.m.  The nearest distances themselves are geo_nn.hip's.
//
//   mvster_eval_reduce_init    eval_zero_kernel + reduce_init_kernel: state[i] = undecided for a valid point, dropped for an
//                                                    invalid one; the invalid points counted with one integer atomic per wave
//   mvster_eval_reduce_rounds  eval_zero_kernel      counts [nrounds] = 0
//                              reduce_round_kernel   x nrounds: one lane per record of the cloud's grid (cell = 2 dst or dst) in cell
//                                                    order; a lane whose point is undecided walks the 27 (or 125) cells around it
//                                                    and decides from the states of the close points before it; the points left
//                                                    undecided are counted with one integer atomic per wave into counts[round]
//   mvster_eval_flags          eval_zero_kernel + eval_flags_kernel: one byte per point = in_obs_mask | above_plane << 1 |
//                                                    covered << 2, and how many points have each bit
//   mvster_eval_stats          stats_sum_kernel<0> + stats_finish_kernel<0>   n, mean (per-workgroup partials in slot order)
//                              stats_sum_kernel<1> + stats_finish_kernel<1>   var from the second pass
//                              (stats_hist_kernel + stats_pick_kernel) x 8    radix selection of the two middle dist2, 8 bits a
//                                                    pass from the top: integer histograms, then the bin that holds the rank
#include "common.hpp"
#include "eval_math.h"

namespace {

constexpr int kWG = 256;
constexpr int kStatSlots = 256;           // workgroups of a statistics pass at most
constexpr int kStatChunk = 4096;          // distances a workgroup covers at least
constexpr int kMaxRounds = 64;            // rounds per call of mvster_eval_reduce_rounds at most
constexpr int kDigits = 8;                // radix passes: 8 bits each over the 64-bit pattern
constexpr int kBins = 256;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

unsigned blocks_of(long n) { return (unsigned)((n + kWG - 1) / kWG); }

__global__ void __launch_bounds__(kWG) eval_zero_kernel(u64* __restrict__ p, int n) {
    const int i = blockIdx.x * kWG + threadIdx.x;
    if (i < n) p[i] = 0;
}

__global__ void __launch_bounds__(kWG) reduce_init_kernel(const float* __restrict__ points, long M, float dst,
                                                          int* __restrict__ state, u64* invalid) {
    const long k = (long)blockIdx.x * kWG + threadIdx.x;
    bool bad = false;
    if (k < M) {
        const float p[3] = {points[k * 3 + 0], points[k * 3 + 1], points[k * 3 + 2]};
        u64 key = 0;
        int t[3];
        bad = !vox::point_key(p, dst, key, t);
        state[k] = bad ? ev::kDropped : ev::kUndecided;
    }
    const u64 b = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(invalid, (u64)__popcll(b));
}

struct ReduceArgs {
    const i32x4* records;             // [nrecords] the valid points in cell order
    long nrecords;
    const u64* keys;                  // the grid's table [mask + 1]
    const int* cell_of_slot;          // [mask + 1]
    const long* starts;               // [ncells + 1]
    long ncells;
    unsigned mask;
    float dst, cell;                  // the grid's cell: ev::reduce_cell(dst, factor)
    int R;                            // ev::reduce_shells(factor)
    const long long* priority;        // [M] or null: splitmix64(i, seed)
    u64 seed;
    long M;
    int* state;                       // [M]
};

__device__ __forceinline__ u64 priority_key(const ReduceArgs& a, long long i) {
    return a.priority ? ev::key_of_int64(a.priority[i]) : ev::splitmix64((u64)i, a.seed);
}

// States are read and written in place with relaxed atomics: a state leaves kUndecided once, so whatever a lane sees of
// another point is either final or "not yet", and "not yet" only costs a round.
__global__ void __launch_bounds__(kWG) reduce_round_kernel(ReduceArgs a, u64* undecided) {
    const long t = (long)blockIdx.x * kWG + threadIdx.x;
    bool left = false;
    if (t < a.nrecords) {
        const i32x4 q = a.records[t];
        const long long i = q[3];
        if ((unsigned long)i < (unsigned long)a.M &&
            __hip_atomic_load(&a.state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ev::kUndecided) {
            const float p[3] = {__int_as_float(q[0]), __int_as_float(q[1]), __int_as_float(q[2])};
            u64 key = 0;
            int off[3];
            vox::point_key(p, a.cell, key, off);
            const long long ix = vox::key_axis(key, 0), iy = vox::key_axis(key, 1), iz = vox::key_axis(key, 2);
            const double reach = ev::reach2(a.dst);
            const u64 ki = priority_key(a, i);
            int verdict = ev::kKept;
            const int R = a.R, W = 2 * R + 1;                               // 27 or 125 cells: bounded
            for (int c = 0; c < W * W * W && verdict != ev::kDropped; ++c) {
                const int dx = c % W - R, dy = c / W % W - R, dz = c / (W * W) - R;
                u64 nk;
                if (!nn::neighbour_key(ix, iy, iz, dx, dy, dz, nk)) continue;
                unsigned s = (unsigned)vox::hash(nk) & a.mask;
                int id = -1;
                for (unsigned it = 0; it <= a.mask; ++it) {                 // at most `slots` probes: never spins
                    const u64 cur = a.keys[s];
                    if (cur == nk) id = a.cell_of_slot[s];
                    if (cur == nk || cur == vox::kEmpty) break;
                    s = (s + 1) & a.mask;
                }
                if ((unsigned long)id >= (unsigned long)a.ncells) continue;
                long lo = a.starts[id], hi = a.starts[id + 1];
                if (lo < 0) lo = 0;
                if (hi > a.nrecords) hi = a.nrecords;
                for (long j = lo; j < hi; ++j) {
                    const i32x4 b = a.records[j];
                    const long long jj = b[3];
                    if (jj == i || (unsigned long)jj >= (unsigned long)a.M) continue;
                    const float o[3] = {__int_as_float(b[0]), __int_as_float(b[1]), __int_as_float(b[2])};
                    if (!ev::close(p, o, reach) || !ev::before(priority_key(a, jj), jj, ki, i)) continue;
                    const int sj = __hip_atomic_load(&a.state[jj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (sj == ev::kKept) {
                        verdict = ev::kDropped;
                        break;
                    }
                    if (sj == ev::kUndecided) verdict = ev::kUndecided;
                }
            }
            if (verdict != ev::kUndecided) __hip_atomic_store(&a.state[i], verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else left = true;
        }
    }
    const u64 b = __ballot(left);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(undecided, (u64)__popcll(b));
}

// params [12] doubles: BB1 (3), BB2 (3), Res, max_block, P (4)
__global__ void __launch_bounds__(kWG) eval_flags_kernel(const float* __restrict__ points, long N,
                                                         const unsigned char* __restrict__ mask, long S1, long S2, long S3,
                                                         const double* __restrict__ params, int which,
                                                         unsigned char* __restrict__ flags, u64* counts) {
    const long k = (long)blockIdx.x * kWG + threadIdx.x;
    int f = 0;
    if (k < N) {
        const float p[3] = {points[k * 3 + 0], points[k * 3 + 1], points[k * 3 + 2]};
        double bb[6], P[4];
#pragma unroll
        for (int j = 0; j < 6; ++j) bb[j] = params[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) P[j] = params[8 + j];
        const long S[3] = {S1, S2, S3};
        if ((which & 1) && ev::in_obs_mask(p, bb, params[6], S, mask)) f |= 1;
        if ((which & 2) && ev::above_plane(p, P)) f |= 2;
        if ((which & 4) && ev::covered(p, bb, params[7])) f |= 4;
        flags[k] = (unsigned char)f;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const u64 b = __ballot((f >> j) & 1);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&counts[j], (u64)__popcll(b));
    }
}

__host__ __device__ inline long stat_len(long N, int slots) { return (N + slots - 1) / slots; }

// work [6] u64: n, the bits of mean, the two prefixes of the selection, the two ranks left inside the prefix
// PASS 0: partial [slots][2] = the selected count (exact in a double) and the fp64 sum of d; PASS 1: [slot][1] = the sum of
// (d - mean)^2.  Fixed order: lane, wave shuffles, the four waves through LDS.  No atomics.
template <int PASS>
__global__ void __launch_bounds__(kWG) stats_sum_kernel(const double* __restrict__ dist2, const unsigned char* __restrict__ flags,
                                                        long N, int need, float max_dist, int slots,
                                                        const u64* __restrict__ work, double* __restrict__ partial) {
    __shared__ double red_sum[kWG / 64];
    __shared__ unsigned red_cnt[kWG / 64];
    const long len = stat_len(N, slots);
    const long lo = (long)blockIdx.x * len, hi = lo + len < N ? lo + len : N;
    const double mean = PASS ? __longlong_as_double((long long)work[1]) : 0.0;
    double sum = 0.0;
    unsigned cnt = 0;
    for (long i = lo + threadIdx.x; i < hi; i += kWG) {
        double d;
        if (ev::stat_selected(dist2[i], flags[i], need, max_dist, d)) {
            cnt += 1u;
            if (PASS) {
                const double e = d - mean;
                sum += e * e;
            } else {
                sum += d;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_down(sum, o, 64);
        cnt += __shfl_down(cnt, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_sum[wave] = sum;
        red_cnt[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[(long)blockIdx.x * 2 + 0] = (double)((red_cnt[0] + red_cnt[1]) + (red_cnt[2] + red_cnt[3]));
        partial[(long)blockIdx.x * 2 + 1] = (red_sum[0] + red_sum[1]) + (red_sum[2] + red_sum[3]);
    }
}

// the slots in slot order; PASS 0 also clears the histograms and sets up the selection
template <int PASS>
__global__ void __launch_bounds__(kWG) stats_finish_kernel(const double* __restrict__ partial, int slots, u64* __restrict__ work,
                                                           unsigned* __restrict__ hist, double* __restrict__ out) {
    if (PASS == 0) {
        for (int i = threadIdx.x; i < kDigits * 2 * kBins; i += kWG) hist[i] = 0u;
    }
    if (threadIdx.x != 0) return;
    double c = 0.0, s = 0.0;
    for (int k = 0; k < slots; ++k) {
        c += partial[(long)k * 2 + 0];
        s += partial[(long)k * 2 + 1];
    }
    const long long n = (long long)c;
    if (PASS == 0) {
        const double mean = ev::stat_mean(s, n);
        work[0] = (u64)n;
        work[1] = (u64)__double_as_longlong(mean);
        work[2] = work[3] = 0;
        work[4] = n > 0 ? (u64)((n - 1) / 2) : 0;
        work[5] = n > 0 ? (u64)(n / 2) : 0;
        out[0] = (double)n;
        out[1] = mean;
    } else {
        out[2] = ev::stat_var(s, n);
    }
}

// pass p looks at bits [56 - 8 p, 64 - 8 p) of the patterns that agree with a prefix above them
__global__ void __launch_bounds__(kWG) stats_hist_kernel(const double* __restrict__ dist2, const unsigned char* __restrict__ flags,
                                                         long N, int need, float max_dist, int slots, int pass,
                                                         const u64* __restrict__ work, unsigned* hist) {
    __shared__ unsigned h[2][kBins];
    h[0][threadIdx.x] = 0u;
    h[1][threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const u64 pre0 = work[2], pre1 = work[3];
    const long len = stat_len(N, slots);
    const long lo = (long)blockIdx.x * len, hi = lo + len < N ? lo + len : N;
    for (long i = lo + threadIdx.x; i < hi; i += kWG) {
        const double v = dist2[i];
        double d;
        if (!ev::stat_selected(v, flags[i], need, max_dist, d)) continue;
        const u64 bits = ev::order_bits(v);
        const unsigned digit = (unsigned)(bits >> shift) & 255u;
        const u64 above = pass ? bits >> (shift + 8) : 0;
        if (above == (pass ? pre0 >> (shift + 8) : 0)) atomicAdd(&h[0][digit], 1u);
        if (above == (pass ? pre1 >> (shift + 8) : 0)) atomicAdd(&h[1][digit], 1u);
    }
    __syncthreads();
    unsigned* g = hist + (long)pass * 2 * kBins;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const unsigned c = h[t][threadIdx.x];
        if (c) atomicAdd(&g[t * kBins + threadIdx.x], c);
    }
}

// the bin of pass p that holds each rank; after the last pass the prefixes are the two middle dist2
__global__ void __launch_bounds__(64) stats_pick_kernel(const unsigned* __restrict__ hist, int pass, u64* __restrict__ work,
                                                        double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const u64 n = work[0];
    if (n > 0) {
        const unsigned* g = hist + (long)pass * 2 * kBins;
        for (int t = 0; t < 2; ++t) {
            u64 rank = work[4 + t], cum = 0;
            int digit = kBins - 1;
            for (int b = 0; b < kBins; ++b) {                               // 256 bins: bounded
                const u64 c = g[t * kBins + b];
                if (rank < cum + c) {
                    digit = b;
                    break;
                }
                cum += c;
            }
            work[4 + t] = rank - cum;
            work[2 + t] |= (u64)digit << (56 - 8 * pass);
        }
    }
    if (pass == kDigits - 1)
        out[3] = n > 0 ? ev::stat_median(__longlong_as_double((long long)work[2]), __longlong_as_double((long long)work[3]))
                       : __longlong_as_double(0x7ff8000000000000ll);
}

bool length_ok(float v) { return v > 0.0f && !std::isinf(v); }

int stat_slots(long N) {
    const long s = (N + kStatChunk - 1) / kStatChunk;
    return (int)(s < kStatSlots ? s : kStatSlots);
}

}  // namespace

extern "C" int mvster_eval_reduce_init(const float* points, long M, float dst, int* state, unsigned long long* invalid,
                                       void* stream) {
    if (!points || !state || !invalid) return MVSTER_ERR_NULL;
    if (M <= 0 || M > (1l << 29) || !length_ok(dst)) return MVSTER_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_zero_kernel, dim3(1), dim3(kWG), 0, st, invalid, 1);
    const int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(reduce_init_kernel, dim3(blocks_of(M)), dim3(kWG), 0, st, points, M, dst, state, invalid);
    return mv_check_launch();
}

extern "C" int mvster_eval_reduce_rounds(const void* records, long nrecords, const unsigned long long* keys, const int* cell_of_slot,
                                         long table_slots, const long* starts, long ncells, float dst, int cell_factor,
                                         const long* priority, long seed, long M, int* state, unsigned long long* counts,
                                         int nrounds, void* stream) {
    if (!records || !keys || !cell_of_slot || !starts || !state || !counts) return MVSTER_ERR_NULL;
    if (M <= 0 || M > (1l << 29) || nrecords <= 0 || nrecords > M || ncells <= 0 || ncells > nrecords) return MVSTER_ERR_SHAPE;
    if (table_slots < 64 || table_slots > (1l << 30) || (table_slots & (table_slots - 1))) return MVSTER_ERR_SHAPE;
    if (!length_ok(dst) || seed < 0 || nrounds < 1 || nrounds > kMaxRounds) return MVSTER_ERR_SHAPE;
    if ((cell_factor != 1 && cell_factor != 2) || !length_ok(ev::reduce_cell(dst, cell_factor))) return MVSTER_ERR_SHAPE;
    ReduceArgs a;
    a.records = static_cast<const i32x4*>(records);
    a.nrecords = nrecords;
    a.keys = keys;
    a.cell_of_slot = cell_of_slot;
    a.starts = starts;
    a.ncells = ncells;
    a.mask = (unsigned)(table_slots - 1);
    a.dst = dst;
    a.cell = ev::reduce_cell(dst, cell_factor);
    a.R = ev::reduce_shells(cell_factor);
    a.priority = reinterpret_cast<const long long*>(priority);
    a.seed = (u64)seed;
    a.M = M;
    a.state = state;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_zero_kernel, dim3(1), dim3(kWG), 0, st, counts, nrounds);
    int rc = mv_check_launch();
    for (int r = 0; r < nrounds && rc == MVSTER_OK; ++r) {
        hipLaunchKernelGGL(reduce_round_kernel, dim3(blocks_of(nrecords)), dim3(kWG), 0, st, a, counts + r);
        rc = mv_check_launch();
    }
    return rc;
}

extern "C" int mvster_eval_flags(const float* points, long N, const unsigned char* mask, long S1, long S2, long S3,
                                 const double* params, int which, unsigned char* flags, unsigned long long* counts, void* stream) {
    if (!points || !params || !flags || !counts || ((which & 1) && !mask)) return MVSTER_ERR_NULL;
    if (N <= 0 || N > (1l << 29) || which < 1 || which > 7) return MVSTER_ERR_SHAPE;
    if ((which & 1) && (S1 <= 0 || S2 <= 0 || S3 <= 0 || S1 > (1l << 20) || S2 > (1l << 20) || S3 > (1l << 20))) return MVSTER_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_zero_kernel, dim3(1), dim3(kWG), 0, st, counts, 3);
    const int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(eval_flags_kernel, dim3(blocks_of(N)), dim3(kWG), 0, st, points, N, mask, S1, S2, S3, params, which, flags,
                       counts);
    return mv_check_launch();
}

extern "C" int mvster_eval_stats_slots(long N) {
    if (N <= 0 || N > (1l << 29)) return MVSTER_ERR_SHAPE;
    return stat_slots(N);
}

extern "C" int mvster_eval_stats(const double* dist2, const unsigned char* flags, long N, int need, float max_dist, double* partial,
                                 unsigned* hist, unsigned long long* work, double* out, void* stream) {
    if (!dist2 || !flags || !partial || !hist || !work || !out) return MVSTER_ERR_NULL;
    if (N <= 0 || N > (1l << 29) || need < 1 || need > 255 || !length_ok(max_dist)) return MVSTER_ERR_SHAPE;
    const int slots = stat_slots(N);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(stats_sum_kernel<0>, dim3((unsigned)slots), dim3(kWG), 0, st, dist2, flags, N, need, max_dist, slots, work, partial);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(stats_finish_kernel<0>, dim3(1), dim3(kWG), 0, st, partial, slots, work, hist, out);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(stats_sum_kernel<1>, dim3((unsigned)slots), dim3(kWG), 0, st, dist2, flags, N, need, max_dist, slots, work, partial);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(stats_finish_kernel<1>, dim3(1), dim3(kWG), 0, st, partial, slots, work, hist, out);
    rc = mv_check_launch();
    for (int p = 0; p < kDigits && rc == MVSTER_OK; ++p) {
        hipLaunchKernelGGL(stats_hist_kernel, dim3((unsigned)slots), dim3(kWG), 0, st, dist2, flags, N, need, max_dist, slots, p, work, hist);
        rc = mv_check_launch();
        if (rc != MVSTER_OK) return rc;
        hipLaunchKernelGGL(stats_pick_kernel, dim3(1), dim3(64), 0, st, hist, p, work, out);
        rc = mv_check_launch();
    }
    return rc;
}
