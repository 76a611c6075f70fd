// Cloud-to-cloud nearest distances and the scan scores built on them (the definition is nn_math.h):
// for every point of a query cloud the nearest point of a target cloud up to a maximum distance, as the lexicographic minimum of
// (d2, target index) -- so the answer depends neither on the grid nor on the order inside a cell nor on the run.
//
//   (mvster_voxel_thin_insert of geo_thin.hip, called by the caller first: the cells of a cloud = the voxels of edge `cell`,
//    claimed in the open-addressing table; slot[k], the leaders per workgroup and their scan; U, dropped, status)
//   mvster_cloud_grid_build
//     nn_zero_kernel        counts [ncells] = 0
//     nn_rank_kernel        every leader ranks itself like thin_rank_kernel: first[slot] = the cell's dense id
//     nn_count_kernel       every valid point: id = first[slot]; local[k] = atomicAdd(counts[id], 1); slot[k] = id
//     (mv_scan_counts)      starts [ncells + 1] = the exclusive scan of counts; starts[ncells] = the valid points
//     nn_scatter_kernel     records[starts[id] + local[k]] = (x, y, z, k): a cell is one contiguous run of 16-byte records
//   mvster_cloud_nn_query   one launch, one lane per query in the cell order of the query cloud's own records
//   mvster_cloud_score      nn_score_partial_kernel (one slot per workgroup) + nn_score_finish_kernel (slots in slot order)
#include "common.hpp"
#include "nn_math.h"

extern "C" int mvster_voxel_thin_blocks(long M);

namespace {

constexpr int kWG = 256;
constexpr int kScoreSlots = 256;          // workgroups of the score pass at most
constexpr int kScoreChunk = 4096;         // distances a workgroup covers at least

typedef int i32x4 __attribute__((ext_vector_type(4)));

unsigned blocks_of(long n) { return (unsigned)((n + kWG - 1) / kWG); }

__global__ void __launch_bounds__(kWG) nn_zero_kernel(int* __restrict__ counts, long n) {
    const long r = (long)blockIdx.x * kWG + threadIdx.x;
    if (r < n) counts[r] = 0;
}

__global__ void __launch_bounds__(kWG) nn_rank_kernel(const int* __restrict__ slot, int* __restrict__ first,
                                                      const long* __restrict__ offsets, long M, long ncells) {
    __shared__ int wave_count[kWG / 64];
    const long k = (long)blockIdx.x * kWG + threadIdx.x;
    const int sv = k < M ? slot[k] : -1;
    const bool lead = sv <= -2;
    const unsigned long long b = __ballot(lead);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = __popcll(b);
    __syncthreads();
    if (!lead) return;
    long r = offsets[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) r += wave_count[w];
    first[-2 - sv] = r < ncells ? (int)r : -1;                              // -1: beyond the caller's buffers, never counted
}

__global__ void __launch_bounds__(kWG) nn_count_kernel(int* __restrict__ slot, const int* __restrict__ first, long M,
                                                       int* counts, int* __restrict__ local) {
    const long k = (long)blockIdx.x * kWG + threadIdx.x;
    if (k >= M) return;
    const int sv = slot[k];
    if (sv == -1) return;
    const int id = first[sv <= -2 ? -2 - sv : sv];
    slot[k] = id;
    if (id >= 0) local[k] = atomicAdd(&counts[id], 1);
}

__global__ void __launch_bounds__(kWG) nn_scatter_kernel(const float* __restrict__ points, const int* __restrict__ cell_id,
                                                         const int* __restrict__ local, const long* __restrict__ starts, long M,
                                                         long ncells, i32x4* __restrict__ records) {
    const long k = (long)blockIdx.x * kWG + threadIdx.x;
    if (k >= M) return;
    const int id = cell_id[k];
    if (id < 0) return;
    const long dst = starts[id] + local[k];
    if (dst >= starts[ncells] || dst >= M) return;                          // capacity of the caller's buffer
    i32x4 rec;
    rec[0] = __float_as_int(points[k * 3 + 0]);
    rec[1] = __float_as_int(points[k * 3 + 1]);
    rec[2] = __float_as_int(points[k * 3 + 2]);
    rec[3] = (int)k;
    records[dst] = rec;
}

struct NnQueryArgs {
    const i32x4* qrecords;            // [qtotal] the valid queries in the cell order of their own grid
    const int* qcell;                 // [Q] a query's cell id, < 0 for an invalid query
    const long* qtotal;               // the valid queries (the last word of the query grid's starts)
    long Q;
    const unsigned long long* keys;   // the target's table [mask + 1]
    const int* cell_of_slot;          // [mask + 1]
    const long* starts;               // [cells + 1]
    const i32x4* records;             // [valid targets]
    long ncells, nrecords;
    unsigned mask;
    int R;
    float max_dist, cell;
    float* dist;
    double* dist2;
    long* index;
};

// One lane per query.  Lanes of a wave hold queries of the same or neighbouring cells, so they walk the same neighbour cells
// and the records of a cell come through the cache once per wave; (best_d2, best_index) live in registers.
__global__ void __launch_bounds__(kWG) nn_query_kernel(NnQueryArgs a) {
    const long t = (long)blockIdx.x * kWG + threadIdx.x;
    if (t >= a.Q) return;
    if (a.qcell[t] < 0) {                                                   // the query at position t is invalid
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        a.dist[t] = (float)nan;
        a.dist2[t] = nan;
        a.index[t] = -1;
    }
    if (t >= *a.qtotal) return;                                             // (qrecords may be null where this is 0)
    const i32x4 q = a.qrecords[t];
    const long at = q[3];
    if ((unsigned long)at >= (unsigned long)a.Q) return;
    const float p[3] = {__int_as_float(q[0]), __int_as_float(q[1]), __int_as_float(q[2])};
    unsigned long long key = 0;
    int off[3];
    vox::point_key(p, a.cell, key, off);
    const long long ix = vox::key_axis(key, 0), iy = vox::key_axis(key, 1), iz = vox::key_axis(key, 2);
    const double limit = nn::max_dist2(a.max_dist);
    double best = __longlong_as_double(0x7ff0000000000000ll);               // +inf
    long long best_index = -1;
    for (int r = 0; r <= a.R; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            for (int dy = -r; dy <= r; ++dy) {
                const bool face = dz == -r || dz == r || dy == -r || dy == r;
                const int step = face ? 1 : 2 * r;                          // inside the shell's faces only dx = -r and r
                for (int dx = -r; dx <= r; dx += step) {
                    unsigned long long nk;
                    if (!nn::neighbour_key(ix, iy, iz, dx, dy, dz, nk)) continue;
                    unsigned s = (unsigned)vox::hash(nk) & a.mask;
                    int id = -1;
                    for (unsigned it = 0; it <= a.mask; ++it) {             // at most `slots` probes: never spins
                        const unsigned long long cur = a.keys[s];
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
                        const double d2 = nn::dist2(p[0], p[1], p[2], __int_as_float(b[0]), __int_as_float(b[1]), __int_as_float(b[2]));
                        if (d2 <= limit && nn::better(d2, (long long)b[3], best, best_index)) {
                            best = d2;
                            best_index = b[3];
                        }
                    }
                }
            }
        }
        if (r >= 1 && nn::ring_done(r, a.cell, best)) break;
    }
    a.dist[at] = nn::dist_of(best);
    a.dist2[at] = best;
    a.index[at] = best_index;
}

__host__ __device__ inline long score_len(long Q, int slots) { return (Q + slots - 1) / slots; }

// partial [slots][4] doubles: valid (not NaN), dist <= max_dist, dist < tau, the fp64 sum of the dist <= max_dist; slot c covers
// dist[c * len, min((c + 1) * len, Q)).  Fixed order: lane, wave shuffles, the four waves through LDS.  No atomics.
__global__ void __launch_bounds__(kWG) nn_score_partial_kernel(const float* __restrict__ dist, long Q, float max_dist, float tau,
                                                               int slots, double* __restrict__ partial) {
    __shared__ double red_sum[kWG / 64];
    __shared__ unsigned red_cnt[kWG / 64][3];
    const long len = score_len(Q, slots);
    const long lo = (long)blockIdx.x * len, hi = lo + len < Q ? lo + len : Q;
    double sum = 0.0;
    unsigned cnt[3] = {0u, 0u, 0u};
    for (long i = lo + threadIdx.x; i < hi; i += kWG) {
        const float d = dist[i];
        cnt[0] += d == d ? 1u : 0u;
        cnt[2] += d < tau ? 1u : 0u;
        if (d <= max_dist) {
            cnt[1] += 1u;
            sum += (double)d;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_down(sum, o, 64);
#pragma unroll
        for (int k = 0; k < 3; ++k) cnt[k] += __shfl_down(cnt[k], o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_sum[wave] = sum;
#pragma unroll
        for (int k = 0; k < 3; ++k) red_cnt[wave][k] = cnt[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int j = threadIdx.x;
        double* out = partial + (long)blockIdx.x * 4;
        if (j == 3) out[3] = (red_sum[0] + red_sum[1]) + (red_sum[2] + red_sum[3]);
        else out[j] = (double)((red_cnt[0][j] + red_cnt[1][j]) + (red_cnt[2][j] + red_cnt[3][j]));
    }
}

// out [4] = the slots summed in slot order (the counts are integers below 2^53: exact)
__global__ void __launch_bounds__(64) nn_score_finish_kernel(const double* __restrict__ partial, int slots, double* __restrict__ out) {
    const int j = threadIdx.x;
    if (j >= 4) return;
    double s = 0.0;
    for (int c = 0; c < slots; ++c) s += partial[(long)c * 4 + j];
    out[j] = s;
}

bool dist_ok(float v) { return v > 0.0f && !std::isinf(v); }

}  // namespace

extern "C" int mvster_cloud_grid_build(const float* points, long M, int* first, int* slot, const long* wg_offsets, int* counts,
                                       int* local, long* starts, long ncells, void* records, void* stream) {
    if (!points || !first || !slot || !wg_offsets || !counts || !local || !starts || !records) return MVSTER_ERR_NULL;
    const int nblk = mvster_voxel_thin_blocks(M);
    if (nblk < 0 || ncells <= 0 || ncells > M) return MVSTER_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nn_zero_kernel, dim3(blocks_of(ncells)), dim3(kWG), 0, st, counts, ncells);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(nn_rank_kernel, dim3((unsigned)nblk), dim3(kWG), 0, st, slot, first, wg_offsets, M, ncells);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(nn_count_kernel, dim3((unsigned)nblk), dim3(kWG), 0, st, slot, first, M, counts, local);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    rc = mv_scan_counts(counts, starts, ncells, st);
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(nn_scatter_kernel, dim3((unsigned)nblk), dim3(kWG), 0, st, points, slot, local, starts, M, ncells,
                       static_cast<i32x4*>(records));
    return mv_check_launch();
}

extern "C" int mvster_cloud_nn_query(const void* qrecords, const int* qcell, const long* qtotal, long Q,
                                     const unsigned long long* keys, const int* cell_of_slot, long table_slots, const long* starts,
                                     const void* records, long ncells, long nrecords, float max_dist, float cell, float* dist,
                                     double* dist2, long* index, void* stream) {
    if (!qcell || !qtotal || !keys || !cell_of_slot || !starts || !dist || !dist2 || !index) return MVSTER_ERR_NULL;
    if (Q <= 0 || Q > (1l << 29) || ncells < 0 || nrecords < 0 || (nrecords > 0 && !records)) return MVSTER_ERR_SHAPE;
    if (table_slots < 64 || table_slots > (1l << 30) || (table_slots & (table_slots - 1))) return MVSTER_ERR_SHAPE;
    if (!dist_ok(max_dist) || !dist_ok(cell) || !nn::cell_ok(max_dist, cell)) return MVSTER_ERR_SHAPE;
    NnQueryArgs a;
    a.qrecords = static_cast<const i32x4*>(qrecords);
    a.qcell = qcell;
    a.qtotal = qtotal;
    a.Q = Q;
    a.keys = keys;
    a.cell_of_slot = cell_of_slot;
    a.starts = starts;
    a.records = static_cast<const i32x4*>(records);
    a.ncells = ncells;
    a.nrecords = nrecords;
    a.mask = (unsigned)(table_slots - 1);
    a.R = nn::rings(max_dist, cell);
    if (a.R < 2 || a.R > nn::kMaxRings) return MVSTER_ERR_SHAPE;
    a.max_dist = max_dist;
    a.cell = cell;
    a.dist = dist;
    a.dist2 = dist2;
    a.index = index;
    hipLaunchKernelGGL(nn_query_kernel, dim3(blocks_of(Q)), dim3(kWG), 0, (hipStream_t)stream, a);
    return mv_check_launch();
}

extern "C" int mvster_cloud_score_slots(long Q) {
    if (Q <= 0 || Q > (1l << 29)) return MVSTER_ERR_SHAPE;
    const long s = (Q + kScoreChunk - 1) / kScoreChunk;
    return (int)(s < kScoreSlots ? s : kScoreSlots);
}

extern "C" int mvster_cloud_score(const float* dist, long Q, float max_dist, float tau, double* partial, double* out,
                                  void* stream) {
    if (!dist || !partial || !out) return MVSTER_ERR_NULL;
    const int slots = mvster_cloud_score_slots(Q);
    if (slots < 0 || !dist_ok(max_dist) || !(tau >= 0.0f && tau <= max_dist)) return MVSTER_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nn_score_partial_kernel, dim3((unsigned)slots), dim3(kWG), 0, st, dist, Q, max_dist, tau, slots, partial);
    const int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(nn_score_finish_kernel, dim3(1), dim3(64), 0, st, partial, slots, out);
    return mv_check_launch();
}
