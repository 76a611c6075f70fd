// Voxel-grid thinning of a fused point cloud: one output point per occupied voxel of edge v, either
// the first input point of the voxel or the mean of its points, in the order of each voxel's first point -- so the thinned
// cloud keeps the order of the cloud it came from.  The arithmetic per point is voxel_math.h; every sum is an integer sum,
// so the result does not depend on the order in which the atomics arrive: two runs give the same bytes.
//
//   mvster_voxel_thin_insert
//     thin_fill_kernel      keys = empty, first = INT_MAX, the dropped count and the status word = 0 (a kernel, no memset node)
//     thin_insert_kernel    one thread per point: key, claim-or-find its slot in the open-addressing table (64-bit
//                           compare-and-swap, linear probing that wraps, at most `slots` probes), atomicMin of the point's
//                           index on first[slot]; slot[k] = the slot, -1 for an invalid point; invalid points are counted
//                           with one atomic per wave
//     thin_leaders_kernel   point k leads its voxel iff first[slot[k]] == k; a leader's slot[k] becomes -2 - slot; leaders
//                           per workgroup
//     (mv_scan_counts)      exclusive scan of the workgroup counts; the three values behind it -- U, dropped, status -- are
//                           the one read-back of the host
//   mvster_voxel_thin_emit
//     thin_zero_kernel      counts [U] and, for the mean, the sums [U,6] = 0
//     thin_rank_kernel      every leader ranks itself (ballot + popcount + the workgroup's offset), writes out_first[rank]
//                           and puts the rank where first[slot] was; nobody reads first[] in this launch
//     thin_accumulate_kernel every valid point adds 1 (and for the mean its three offsets and three colour bytes) to row
//                           first[slot] with integer atomics, runs of lanes with the same row combined in the wave first
//     thin_emit_kernel      one thread per output voxel
#include <limits.h>

#include "common.hpp"
#include "voxel_math.h"

namespace {

constexpr int kWG = 256;
constexpr long kMaxSlots = 1l << 30;      // slot[k] holds a slot or -2 - slot in 32 bits

__global__ void __launch_bounds__(kWG) thin_fill_kernel(unsigned long long* __restrict__ keys, int* __restrict__ first, long slots,
                                                        long* __restrict__ tail) {
    const long s = (long)blockIdx.x * kWG + threadIdx.x;
    if (s < slots) {
        keys[s] = vox::kEmpty;
        first[s] = INT_MAX;
    }
    if (s < 2) tail[s] = 0;                                                 // dropped, status
}

__global__ void __launch_bounds__(kWG) thin_insert_kernel(const float* __restrict__ points, long M, float v,
                                                          unsigned long long* keys, int* first, unsigned mask,
                                                          int* __restrict__ slot, long* tail) {
    const long k = (long)blockIdx.x * kWG + threadIdx.x;
    const bool inside = k < M;
    bool ok = false;
    if (inside) {
        const float p[3] = {points[k * 3 + 0], points[k * 3 + 1], points[k * 3 + 2]};
        unsigned long long key = 0;
        int t[3];
        ok = vox::point_key(p, v, key, t);
        int found = -1;
        if (ok) {
            unsigned s = (unsigned)vox::hash(key) & mask;
            for (unsigned it = 0; it <= mask; ++it) {                       // at most `slots` probes: never spins
                unsigned long long cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == vox::kEmpty) {
                    cur = atomicCAS(&keys[s], vox::kEmpty, key);
                    if (cur == vox::kEmpty) cur = key;                      // claimed
                }
                if (cur == key) {
                    found = (int)s;
                    break;
                }
                s = (s + 1) & mask;
            }
            if (found >= 0) atomicMin(&first[found], (int)k);
            else tail[1] = 1;                                               // table full: the host turns this into an error
        }
        slot[k] = found;
    }
    const unsigned long long b = __ballot(inside && !ok);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(reinterpret_cast<unsigned long long*>(tail), (unsigned long long)__popcll(b));
}

// lanes of the workgroup with `flag` -> their number (thread 0 only needs it) through wave_count
__device__ __forceinline__ void wave_counts(bool flag, int* wave_count, unsigned long long& b) {
    b = __ballot(flag);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
}

__global__ void __launch_bounds__(kWG) thin_leaders_kernel(int* __restrict__ slot, const int* __restrict__ first, long M,
                                                           int* __restrict__ wg_counts) {
    __shared__ int wave_count[kWG / 64];
    const long k = (long)blockIdx.x * kWG + threadIdx.x;
    bool lead = false;
    if (k < M) {
        const int s = slot[k];
        if (s >= 0 && first[s] == (int)k) {
            lead = true;
            slot[k] = -2 - s;
        }
    }
    unsigned long long b;
    wave_counts(lead, wave_count, b);
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < kWG / 64; ++w) c += wave_count[w];
        wg_counts[blockIdx.x] = c;
    }
}

__global__ void __launch_bounds__(kWG) thin_zero_kernel(int* __restrict__ counts, unsigned long long* __restrict__ sums, long U) {
    const long r = (long)blockIdx.x * kWG + threadIdx.x;
    if (r >= U) return;
    counts[r] = 0;
    if (sums) {
#pragma unroll
        for (int j = 0; j < 6; ++j) sums[r * 6 + j] = 0;
    }
}

__global__ void __launch_bounds__(kWG) thin_rank_kernel(const int* __restrict__ slot, int* __restrict__ first,
                                                        const long* __restrict__ offsets, long* __restrict__ out_first, long M,
                                                        long U) {
    __shared__ int wave_count[kWG / 64];
    const long k = (long)blockIdx.x * kWG + threadIdx.x;
    const int sv = k < M ? slot[k] : -1;
    const bool lead = sv <= -2;
    unsigned long long b;
    wave_counts(lead, wave_count, b);
    if (!lead) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long r = offsets[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) r += wave_count[w];
    if (r >= U) return;                                                     // capacity of the caller's buffers
    out_first[r] = k;
    first[-2 - sv] = (int)r;
}

// Neighbouring points of one view often share a voxel, and the integer atomics are bound by the number of requests, not by
// their bytes: a run of consecutive lanes with the same row is summed with a shuffle-down tree and only the run's first lane
// issues atomics.  Integer sums: the same bits as one set of atomics per point (measured against that form: DESIGN.md
// section 4.16).
template <bool MEAN>
__global__ void __launch_bounds__(kWG) thin_accumulate_kernel(const float* __restrict__ points,
                                                              const unsigned char* __restrict__ colors, long M, float v,
                                                              const int* __restrict__ slot, const int* __restrict__ rank,
                                                              int* counts, unsigned long long* sums, long U) {
    constexpr int kVals = MEAN ? 7 : 1;                                     // n, then the three offsets and the three colours
    const long k = (long)blockIdx.x * kWG + threadIdx.x;
    long r = -1;                                                            // -1: this lane adds nothing
    if (k < M) {
        const int sv = slot[k];
        if (sv != -1) r = rank[sv <= -2 ? -2 - sv : sv];
        if ((unsigned long)r >= (unsigned long)U) r = -1;
    }
    int val[kVals];
    val[0] = 1;
    if (MEAN) {
#pragma unroll
        for (int j = 1; j < kVals; ++j) val[j] = 0;
        if (r >= 0) {
            const float p[3] = {points[k * 3 + 0], points[k * 3 + 1], points[k * 3 + 2]};
            unsigned long long key;
            int t[3];
            vox::point_key(p, v, key, t);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                val[1 + j] = t[j];
                val[4 + j] = colors[k * 3 + j];
            }
        }
    }
    const int lane = threadIdx.x & 63;
    const long prev = __shfl_up(r, 1, 64);
    const bool starts = lane == 0 || prev != r;                             // first lane of a run of equal rows
    const unsigned long long sb = __ballot(starts);
    if (sb != ~0ull) {                                                      // some run is longer than one lane
        const int run = 63 - __clzll(sb & (~0ull >> (63 - lane)));          // my run's first lane
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {                                  // a wave's sums stay below 2^22: 32-bit shuffles
            const bool take = __shfl_down(run, d, 64) == run && lane + d < 64;
#pragma unroll
            for (int j = 0; j < kVals; ++j) {
                const int o = __shfl_down(val[j], d, 64);
                if (take) val[j] += o;
            }
        }
    }
    if (r < 0 || !starts) return;
    atomicAdd(&counts[r], val[0]);
    if (MEAN) {
#pragma unroll
        for (int j = 0; j < 6; ++j) atomicAdd(&sums[r * 6 + j], (unsigned long long)val[1 + j]);
    }
}

template <bool MEAN>
__global__ void __launch_bounds__(kWG) thin_emit_kernel(const float* __restrict__ points, const unsigned char* __restrict__ colors,
                                                        long M, float v, const long* __restrict__ out_first,
                                                        const int* __restrict__ counts, const unsigned long long* __restrict__ sums,
                                                        float* __restrict__ out_points, unsigned char* __restrict__ out_colors,
                                                        long U) {
    const long r = (long)blockIdx.x * kWG + threadIdx.x;
    if (r >= U) return;
    const long f = out_first[r];
    if ((unsigned long)f >= (unsigned long)M) return;
    const float p[3] = {points[f * 3 + 0], points[f * 3 + 1], points[f * 3 + 2]};
    if (MEAN) {
        const unsigned n = (unsigned)counts[r];
        unsigned long long key = 0;
        int t[3];
        vox::point_key(p, v, key, t);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            out_points[r * 3 + j] = vox::mean_coord(vox::key_axis(key, j), sums[r * 6 + j], n, v);
            out_colors[r * 3 + j] = vox::mean_color(sums[r * 6 + 3 + j], n);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            out_points[r * 3 + j] = p[j];
            out_colors[r * 3 + j] = colors[f * 3 + j];
        }
    }
}

bool voxel_ok(float v) { return v > 0.0f && !std::isinf(v); }

unsigned blocks_of(long n) { return (unsigned)((n + kWG - 1) / kWG); }

}  // namespace

extern "C" int mvster_voxel_thin_blocks(long M) {
    if (M <= 0 || M > kMaxSlots / 2) return MVSTER_ERR_SHAPE;
    return (int)blocks_of(M);
}

extern "C" int mvster_voxel_thin_insert(const float* points, long M, float voxel, unsigned long long* keys, int* first,
                                        long table_slots, int* slot, int* wg_counts, long* wg_offsets, void* stream) {
    if (!points || !keys || !first || !slot || !wg_counts || !wg_offsets) return MVSTER_ERR_NULL;
    const int nblk = mvster_voxel_thin_blocks(M);
    if (nblk < 0 || !voxel_ok(voxel)) return MVSTER_ERR_SHAPE;
    if (table_slots < 64 || table_slots > kMaxSlots || (table_slots & (table_slots - 1)) || table_slots < 2 * M)
        return MVSTER_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    long* tail = wg_offsets + nblk + 1;                                     // dropped, status behind U
    hipLaunchKernelGGL(thin_fill_kernel, dim3(blocks_of(table_slots)), dim3(kWG), 0, st, keys, first, table_slots, tail);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(thin_insert_kernel, dim3((unsigned)nblk), dim3(kWG), 0, st, points, M, voxel, keys, first,
                       (unsigned)(table_slots - 1), slot, tail);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(thin_leaders_kernel, dim3((unsigned)nblk), dim3(kWG), 0, st, slot, first, M, wg_counts);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    return mv_scan_counts(wg_counts, wg_offsets, (long)nblk, st);
}

extern "C" int mvster_voxel_thin_emit(const float* points, const unsigned char* colors, long M, float voxel, int reduce,
                                      int* first, const int* slot, const long* wg_offsets, unsigned long long* sums,
                                      float* out_points, unsigned char* out_colors, int* out_counts, long* out_first, long U,
                                      void* stream) {
    if (!points || !colors || !first || !slot || !wg_offsets) return MVSTER_ERR_NULL;
    const int nblk = mvster_voxel_thin_blocks(M);
    if (nblk < 0 || !voxel_ok(voxel) || U < 0 || U > M) return MVSTER_ERR_SHAPE;
    if (reduce != 0 && reduce != 1) return MVSTER_ERR_UNSUPPORTED;
    if (U == 0) return MVSTER_OK;
    if (!out_points || !out_colors || !out_counts || !out_first || (reduce == 0 && !sums)) return MVSTER_ERR_NULL;
    hipStream_t st = (hipStream_t)stream;
    const bool mean = reduce == 0;
    hipLaunchKernelGGL(thin_zero_kernel, dim3(blocks_of(U)), dim3(kWG), 0, st, out_counts, mean ? sums : nullptr, U);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(thin_rank_kernel, dim3((unsigned)nblk), dim3(kWG), 0, st, slot, first, wg_offsets, out_first, M, U);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    if (mean) {
        hipLaunchKernelGGL(thin_accumulate_kernel<true>, dim3((unsigned)nblk), dim3(kWG), 0, st, points, colors, M, voxel, slot,
                           first, out_counts, sums, U);
        rc = mv_check_launch();
        if (rc != MVSTER_OK) return rc;
        hipLaunchKernelGGL(thin_emit_kernel<true>, dim3(blocks_of(U)), dim3(kWG), 0, st, points, colors, M, voxel, out_first,
                           out_counts, sums, out_points, out_colors, U);
    } else {
        hipLaunchKernelGGL(thin_accumulate_kernel<false>, dim3((unsigned)nblk), dim3(kWG), 0, st, points, colors, M, voxel, slot,
                           first, out_counts, sums, U);
        rc = mv_check_launch();
        if (rc != MVSTER_OK) return rc;
        hipLaunchKernelGGL(thin_emit_kernel<false>, dim3(blocks_of(U)), dim3(kWG), 0, st, points, colors, M, voxel, out_first,
                           out_counts, sums, out_points, out_colors, U);
    }
    return mv_check_launch();
}
