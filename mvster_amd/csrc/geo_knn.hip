// Cleaning a fused cloud (the definition is knn_math.h): the k nearest points of a cloud on the hash grid
// of geo_nn.hip, and what is built on them -- the radius and the statistical outlier filter and the normals.
//
//   mvster_cloud_knn_query      knn_kernel<CAP, WG, kLists>    the [Q,k] lists for a caller who wants them
//   mvster_cloud_knn_mean       knn_kernel<CAP, WG, kMean>     count [M], mean [M] of the statistical filter: no lists in memory
//   mvster_cloud_knn_normals    knn_kernel<CAP, WG, kNormals>  normals [M,3], valid [M]: sums, Jacobi solve and sign in the lane
//   mvster_cloud_radius_count   radius_count_kernel            the search without a list and without an early stop
//   mvster_cloud_knn_stats      two passes of stat_partial_kernel (one row per workgroup) + stat_finish_kernel (rows in row order)
//   mvster_cloud_keep_flags     keep_flags_kernel + (mv_scan_counts) + keep_tail_kernel: flags [M], the kept points per tile of 256
//                               and their exclusive scan, as mvster_reg_crop_flags leaves them: mvster_reg_crop_emit compacts
//
// One lane per query in the cell order of the query grid, as nn_query_kernel walks.  The candidate list of a lane is a column of
// LDS, [place][lane]: a wave's accesses to one place hit consecutive banks, and no register array is indexed at run time.  The
// kernels are instantiated per capacity CAP = 4 / 8 / 16 / 32 with WG = 256 / 256 / 128 / 64 lanes: 12 bytes per entry, at most
// 24 KB per workgroup, so six workgroups fit the 160 KB of a CU by LDS at every capacity.  A lane keeps the place and the value of
// its worst entry in registers: a candidate behind it costs one comparison, an accepted one a rescan of k places; the list is
// ordered once at the end.  No atomics at all, no scratch, every loop bounded.
#include "common.hpp"
#include "knn_math.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int kLists = 0, kMean = 1, kNormals = 2;
constexpr int kTile = 256;                // points per tile of the compaction (mvster_reg_blocks)

struct Grid {
    const i32x4* qrecords;            // [qtotal] the valid queries in the cell order of their own grid
    const int* qcell;                 // [Q] a query's cell id, < 0 for an invalid query
    const long* qtotal;
    long Q;
    const u64* keys;                  // the target's table [mask + 1]
    const int* cell_of_slot;
    const long* starts;               // [ncells + 1]
    const i32x4* records;             // [nrecords]
    long ncells, nrecords;
    unsigned mask;
    int R;
    float max_dist, cell;
};

struct KnnOut {
    int k, exclude_self;
    double* dist2;                    // kLists [Q,k]
    long* index;                      // kLists [Q,k]
    int* count;                       // kLists, kMean [Q]
    double* mean;                     // kMean [Q]
    const float* points;              // kNormals [M,3]: the cloud both grids were built from
    const float* toward;              // kNormals [M,3] or NULL
    float* normals;                   // kNormals [M,3]
    unsigned char* valid;             // kNormals [M]
    long M;
};

// The cells of shell r around (ix, iy, iz) in the order of nn_query_kernel; f(record) for every record of every cell.
template <class F>
__device__ __forceinline__ void walk_shell(const Grid& g, long long ix, long long iy, long long iz, int r, F&& f) {
    for (int dz = -r; dz <= r; ++dz) {
        for (int dy = -r; dy <= r; ++dy) {
            const bool face = dz == -r || dz == r || dy == -r || dy == r;
            const int step = (face || r == 0) ? 1 : 2 * r;                  // inside the shell's faces only dx = -r and r
            for (int dx = -r; dx <= r; dx += step) {
                u64 nk;
                if (!nn::neighbour_key(ix, iy, iz, dx, dy, dz, nk)) continue;
                unsigned s = (unsigned)vox::hash(nk) & g.mask;
                int id = -1;
                for (unsigned it = 0; it <= g.mask; ++it) {                 // at most `slots` probes: never spins
                    const u64 cur = g.keys[s];
                    if (cur == nk) id = g.cell_of_slot[s];
                    if (cur == nk || cur == vox::kEmpty) break;
                    s = (s + 1) & g.mask;
                }
                if ((unsigned long)id >= (unsigned long)g.ncells) continue;
                long lo = g.starts[id], hi = g.starts[id + 1];
                if (lo < 0) lo = 0;
                if (hi > g.nrecords) hi = g.nrecords;
                for (long j = lo; j < hi; ++j) f(g.records[j]);
            }
        }
    }
}

template <int CAP, int WG, int MODE>
__global__ void __launch_bounds__(WG) knn_kernel(Grid g, KnnOut o) {
    __shared__ double l_d2[CAP][WG];
    __shared__ int l_ix[CAP][WG];
    const long t = (long)blockIdx.x * WG + threadIdx.x;
    if (t >= g.Q) return;
    const int c = threadIdx.x, k = o.k < CAP ? o.k : CAP;
    const double inf = knn::inf();
    if (g.qcell[t] < 0) {                                                   // the query at position t is invalid
        if (MODE == kLists) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            for (int j = 0; j < k; ++j) {
                o.dist2[t * k + j] = nan;
                o.index[t * k + j] = -1;
            }
            o.count[t] = 0;
        } else if (MODE == kMean) {
            o.mean[t] = __longlong_as_double(0x7ff8000000000000ll);
            o.count[t] = 0;
        } else {
            o.normals[t * 3 + 0] = o.normals[t * 3 + 1] = o.normals[t * 3 + 2] = 0.0f;
            o.valid[t] = 0;
        }
    }
    if (t >= *g.qtotal) return;                                             // (qrecords may be null where this is 0)
    const i32x4 q = g.qrecords[t];
    const long at = q[3];
    if ((unsigned long)at >= (unsigned long)g.Q) return;
    const float p[3] = {__int_as_float(q[0]), __int_as_float(q[1]), __int_as_float(q[2])};
    u64 key = 0;
    int off[3];
    vox::point_key(p, g.cell, key, off);
    const long long ix = vox::key_axis(key, 0), iy = vox::key_axis(key, 1), iz = vox::key_axis(key, 2);
    const double limit = nn::max_dist2(g.max_dist);
    const long long self = o.exclude_self ? (long long)at : -1;
    int n = 0, wpos = 0;
    double wd2 = inf;                                                       // the worst entry once the list is full
    long long wix = -1;
    auto rescan = [&]() {
        wpos = 0;
        wd2 = l_d2[0][c];
        wix = l_ix[0][c];
        for (int j = 1; j < k; ++j) {
            const double d = l_d2[j][c];
            const long long i = l_ix[j][c];
            if (nn::better(wd2, wix, d, i)) {
                wpos = j;
                wd2 = d;
                wix = i;
            }
        }
    };
    for (int r = 0; r <= g.R; ++r) {
        walk_shell(g, ix, iy, iz, r, [&](const i32x4 b) {
            const double d2 = nn::dist2(p[0], p[1], p[2], __int_as_float(b[0]), __int_as_float(b[1]), __int_as_float(b[2]));
            const long long bi = b[3];
            if (!(d2 <= limit) || bi == self) return;
            if (n < k) {
                l_d2[n][c] = d2;
                l_ix[n][c] = (int)bi;
                ++n;
                if (n == k) rescan();
            } else if (nn::better(d2, bi, wd2, wix)) {
                l_d2[wpos][c] = d2;
                l_ix[wpos][c] = (int)bi;
                rescan();
            }
        });
        if (r >= 1 && knn::ring_done(r, g.cell, n == k, wd2)) break;
    }
    for (int j = 1; j < n; ++j) {                                           // the final order, once: insertion sort of the column
        const double d = l_d2[j][c];
        const int i = l_ix[j][c];
        int m = j;
        while (m > 0 && nn::better(d, i, l_d2[m - 1][c], l_ix[m - 1][c])) {
            l_d2[m][c] = l_d2[m - 1][c];
            l_ix[m][c] = l_ix[m - 1][c];
            --m;
        }
        l_d2[m][c] = d;
        l_ix[m][c] = i;
    }
    if (MODE == kLists) {
        for (int j = 0; j < k; ++j) {
            o.dist2[at * k + j] = j < n ? l_d2[j][c] : inf;
            o.index[at * k + j] = j < n ? (long)l_ix[j][c] : -1l;
        }
        o.count[at] = n;
    } else if (MODE == kMean) {
        double sum = 0.0;
        for (int j = 0; j < n; ++j) sum = sum + sqrt(l_d2[j][c]);
        o.mean[at] = n == k ? knn::mean_of(sum, k) : inf;
        o.count[at] = n;
    } else {
        knn::Moments s = knn::no_moments();
        for (int j = 0; j < n; ++j) {
            const long i = l_ix[j][c];
            if ((unsigned long)i >= (unsigned long)o.M) continue;           // (an index always comes from a record: below M)
            const float pj[3] = {o.points[i * 3 + 0], o.points[i * 3 + 1], o.points[i * 3 + 2]};
            knn::add(s, p, pj);
        }
        float tx = 0.0f, ty = 0.0f, tz = 0.0f, nx, ny, nz;
        if (o.toward) {
            tx = o.toward[at * 3 + 0];
            ty = o.toward[at * 3 + 1];
            tz = o.toward[at * 3 + 2];
        }
        const bool ok = knn::normal(s, n, p[0], p[1], p[2], o.toward != nullptr, tx, ty, tz, nx, ny, nz);
        o.normals[at * 3 + 0] = nx;
        o.normals[at * 3 + 1] = ny;
        o.normals[at * 3 + 2] = nz;
        o.valid[at] = ok ? 1 : 0;
    }
}

// neighbours [M]: the targets within max_dist of every point but the point itself; every shell up to R counts.
__global__ void __launch_bounds__(256) radius_count_kernel(Grid g, int* __restrict__ neighbours) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= g.Q) return;
    if (g.qcell[t] < 0) neighbours[t] = 0;
    if (t >= *g.qtotal) return;
    const i32x4 q = g.qrecords[t];
    const long at = q[3];
    if ((unsigned long)at >= (unsigned long)g.Q) return;
    const float p[3] = {__int_as_float(q[0]), __int_as_float(q[1]), __int_as_float(q[2])};
    u64 key = 0;
    int off[3];
    vox::point_key(p, g.cell, key, off);
    const long long ix = vox::key_axis(key, 0), iy = vox::key_axis(key, 1), iz = vox::key_axis(key, 2);
    const double limit = nn::max_dist2(g.max_dist);
    int n = 0;
    for (int r = 0; r <= g.R; ++r) {
        walk_shell(g, ix, iy, iz, r, [&](const i32x4 b) {
            const double d2 = nn::dist2(p[0], p[1], p[2], __int_as_float(b[0]), __int_as_float(b[1]), __int_as_float(b[2]));
            n += (d2 <= limit && (long)b[3] != at) ? 1 : 0;
        });
    }
    neighbours[at] = n;
}

// partial [rows][2]: the participants of the row and the sum of their means (pass 0) or of their squared deviations from
// stats[1] = mu (pass 1), in the fixed order of knn_math.h.
template <int PASS>
__global__ void __launch_bounds__(knn::kStatWG) stat_partial_kernel(const double* __restrict__ mean, long M, int rows,
                                                                    const double* __restrict__ stats, double* __restrict__ partial) {
    __shared__ double red_sum[knn::kStatWG / 64];
    __shared__ double red_cnt[knn::kStatWG / 64];
    const long len = knn::stat_len(M, rows);
    const long lo = (long)blockIdx.x * len, hi = lo + len < M ? lo + len : M;
    const double mu = PASS ? stats[1] : 0.0;
    double sum = 0.0, cnt = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += knn::kStatWG) {
        const double m = mean[i];
        if (knn::takes_part(m)) {
            cnt = cnt + 1.0;
            sum = sum + (PASS ? knn::sq_dev(m, mu) : m);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum = sum + __shfl_down(sum, o, 64);
        cnt = cnt + __shfl_down(cnt, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_sum[wave] = sum;
        red_cnt[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[(long)blockIdx.x * 2 + 0] = (red_cnt[0] + red_cnt[1]) + (red_cnt[2] + red_cnt[3]);
        partial[(long)blockIdx.x * 2 + 1] = (red_sum[0] + red_sum[1]) + (red_sum[2] + red_sum[3]);
    }
}

// stats [5] = n, mu, sigma, threshold, (the kept count, by keep_tail_kernel): pass 0 writes n and mu, pass 1 sigma and threshold
template <int PASS>
__global__ void __launch_bounds__(64) stat_finish_kernel(const double* __restrict__ partial, int rows, double std_ratio,
                                                         double* __restrict__ stats) {
    if (threadIdx.x != 0) return;
    double n = 0.0, s = 0.0;
    for (int c = 0; c < rows; ++c) {
        n = n + partial[(long)c * 2 + 0];
        s = s + partial[(long)c * 2 + 1];
    }
    if (PASS == 0) {
        stats[0] = n;
        stats[1] = knn::mu_of(s, n);
    } else {
        const double sigma = knn::sigma_of(s, n);
        stats[2] = sigma;
        stats[3] = knn::threshold_of(stats[1], sigma, std_ratio);
    }
}

// flags [M] and the kept points of every tile of 256.  mean != NULL: the statistical rule against stats[3]; else the radius rule.
__global__ void __launch_bounds__(kTile) keep_flags_kernel(const int* __restrict__ qcell, const int* __restrict__ neighbours,
                                                           int nb_points, const double* __restrict__ mean,
                                                           const double* __restrict__ stats, long M, unsigned char* __restrict__ flags,
                                                           int* __restrict__ wg_counts) {
    __shared__ int wave_count[kTile / 64];
    const long k = (long)blockIdx.x * kTile + threadIdx.x;
    bool keep = false;
    if (k < M) {
        keep = mean ? knn::stat_keep(mean[k], stats[3]) : (qcell[k] >= 0 && neighbours[k] >= nb_points);
        flags[k] = keep ? 1 : 0;
    }
    const u64 b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) wg_counts[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

__global__ void __launch_bounds__(64) keep_tail_kernel(const long* __restrict__ wg_offsets, long tiles, double* __restrict__ stats) {
    if (threadIdx.x == 0) stats[4] = (double)wg_offsets[tiles];
}

bool dist_ok(float v) { return v > 0.0f && !std::isinf(v); }
bool cloud_ok(long N) { return N > 0 && N <= (1l << 29); }

// The checks of mvster_cloud_nn_query, and the grid as the kernels take it.
int make_grid(const void* qrecords, const int* qcell, const long* qtotal, long Q, const u64* keys, const int* cell_of_slot,
              long table_slots, const long* starts, const void* records, long ncells, long nrecords, float max_dist, float cell,
              Grid& g) {
    if (!qcell || !qtotal || !keys || !cell_of_slot || !starts) return MVSTER_ERR_NULL;
    if (!cloud_ok(Q) || ncells < 0 || nrecords < 0 || (nrecords > 0 && !records)) return MVSTER_ERR_SHAPE;
    if (table_slots < 64 || table_slots > (1l << 30) || (table_slots & (table_slots - 1))) return MVSTER_ERR_SHAPE;
    if (!dist_ok(max_dist) || !dist_ok(cell) || !nn::cell_ok(max_dist, cell)) return MVSTER_ERR_SHAPE;
    g.qrecords = static_cast<const i32x4*>(qrecords);
    g.qcell = qcell;
    g.qtotal = qtotal;
    g.Q = Q;
    g.keys = keys;
    g.cell_of_slot = cell_of_slot;
    g.starts = starts;
    g.records = static_cast<const i32x4*>(records);
    g.ncells = ncells;
    g.nrecords = nrecords;
    g.mask = (unsigned)(table_slots - 1);
    g.R = nn::rings(max_dist, cell);
    if (g.R < 2 || g.R > nn::kMaxRings) return MVSTER_ERR_SHAPE;
    g.max_dist = max_dist;
    g.cell = cell;
    return MVSTER_OK;
}

template <int CAP, int WG, int MODE>
void launch_one(const Grid& g, const KnnOut& o, hipStream_t st) {
    hipLaunchKernelGGL((knn_kernel<CAP, WG, MODE>), dim3((unsigned)((g.Q + WG - 1) / WG)), dim3(WG), 0, st, g, o);
}

template <int MODE>
int launch_knn(const Grid& g, const KnnOut& o, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (o.k <= 4) launch_one<4, 256, MODE>(g, o, st);
    else if (o.k <= 8) launch_one<8, 256, MODE>(g, o, st);
    else if (o.k <= 16) launch_one<16, 128, MODE>(g, o, st);
    else launch_one<32, 64, MODE>(g, o, st);
    return mv_check_launch();
}

KnnOut no_out(int k, int exclude_self) {
    KnnOut o;
    o.k = k;
    o.exclude_self = exclude_self;
    o.dist2 = nullptr;
    o.index = nullptr;
    o.count = nullptr;
    o.mean = nullptr;
    o.points = nullptr;
    o.toward = nullptr;
    o.normals = nullptr;
    o.valid = nullptr;
    o.M = 0;
    return o;
}

}  // namespace

extern "C" int mvster_cloud_knn_query(const void* qrecords, const int* qcell, const long* qtotal, long Q,
                                      const unsigned long long* keys, const int* cell_of_slot, long table_slots, const long* starts,
                                      const void* records, long ncells, long nrecords, float max_dist, float cell, int k,
                                      int exclude_self, long M, double* dist2, long* index, int* count, void* stream) {
    if (!dist2 || !index || !count) return MVSTER_ERR_NULL;
    if (!knn::k_ok(k) || (exclude_self != 0 && exclude_self != 1) || (exclude_self && Q != M)) return MVSTER_ERR_SHAPE;
    Grid g;
    const int rc = make_grid(qrecords, qcell, qtotal, Q, keys, cell_of_slot, table_slots, starts, records, ncells, nrecords, max_dist,
                             cell, g);
    if (rc != MVSTER_OK) return rc;
    KnnOut o = no_out(k, exclude_self);
    o.dist2 = dist2;
    o.index = index;
    o.count = count;
    return launch_knn<kLists>(g, o, stream);
}

extern "C" int mvster_cloud_knn_mean(const void* records, const int* cell_of_point, long M, const unsigned long long* keys,
                                     const int* cell_of_slot, long table_slots, const long* starts, long ncells, long nrecords,
                                     float max_dist, float cell, int k, int* count, double* mean, void* stream) {
    if (!count || !mean || !starts) return MVSTER_ERR_NULL;
    if (!knn::k_ok(k) || ncells < 0) return MVSTER_ERR_SHAPE;
    Grid g;
    const int rc = make_grid(records, cell_of_point, starts + ncells, M, keys, cell_of_slot, table_slots, starts, records, ncells,
                             nrecords, max_dist, cell, g);
    if (rc != MVSTER_OK) return rc;
    KnnOut o = no_out(k, 1);
    o.count = count;
    o.mean = mean;
    return launch_knn<kMean>(g, o, stream);
}

extern "C" int mvster_cloud_knn_normals(const void* records, const int* cell_of_point, long M, const unsigned long long* keys,
                                        const int* cell_of_slot, long table_slots, const long* starts, long ncells, long nrecords,
                                        float max_dist, float cell, int k, const float* points, const float* toward, float* normals,
                                        unsigned char* valid, void* stream) {
    if (!points || !normals || !valid || !starts) return MVSTER_ERR_NULL;
    if (!knn::k_ok(k) || ncells < 0) return MVSTER_ERR_SHAPE;
    Grid g;
    const int rc = make_grid(records, cell_of_point, starts + ncells, M, keys, cell_of_slot, table_slots, starts, records, ncells,
                             nrecords, max_dist, cell, g);
    if (rc != MVSTER_OK) return rc;
    KnnOut o = no_out(k, 1);
    o.points = points;
    o.toward = toward;
    o.normals = normals;
    o.valid = valid;
    o.M = M;
    return launch_knn<kNormals>(g, o, stream);
}

extern "C" int mvster_cloud_radius_count(const void* records, const int* cell_of_point, long M, const unsigned long long* keys,
                                         const int* cell_of_slot, long table_slots, const long* starts, long ncells, long nrecords,
                                         float radius, float cell, int* neighbours, void* stream) {
    if (!neighbours || !starts) return MVSTER_ERR_NULL;
    if (ncells < 0) return MVSTER_ERR_SHAPE;
    Grid g;
    const int rc = make_grid(records, cell_of_point, starts + ncells, M, keys, cell_of_slot, table_slots, starts, records, ncells,
                             nrecords, radius, cell, g);
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(radius_count_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, neighbours);
    return mv_check_launch();
}

extern "C" int mvster_cloud_knn_stats_rows(long M) {
    if (!cloud_ok(M)) return MVSTER_ERR_SHAPE;
    return knn::stat_rows(M);
}

extern "C" int mvster_cloud_knn_stats(const double* mean, long M, double std_ratio, double* partial, double* stats, void* stream) {
    if (!mean || !partial || !stats) return MVSTER_ERR_NULL;
    if (!cloud_ok(M) || !(std_ratio == std_ratio) || std::isinf(std_ratio)) return MVSTER_ERR_SHAPE;
    const int rows = knn::stat_rows(M);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(stat_partial_kernel<0>, dim3((unsigned)rows), dim3(knn::kStatWG), 0, st, mean, M, rows, stats, partial);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(stat_finish_kernel<0>, dim3(1), dim3(64), 0, st, partial, rows, std_ratio, stats);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(stat_partial_kernel<1>, dim3((unsigned)rows), dim3(knn::kStatWG), 0, st, mean, M, rows, stats, partial);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(stat_finish_kernel<1>, dim3(1), dim3(64), 0, st, partial, rows, std_ratio, stats);
    return mv_check_launch();
}

extern "C" int mvster_cloud_keep_flags(const int* cell_of_point, const int* neighbours, int nb_points, const double* mean,
                                       double* stats, long M, unsigned char* flags, int* wg_counts, long* wg_offsets, void* stream) {
    if (!flags || !wg_counts || !wg_offsets) return MVSTER_ERR_NULL;
    if (mean ? !stats : (!cell_of_point || !neighbours)) return MVSTER_ERR_NULL;
    if (!cloud_ok(M) || (!mean && nb_points < 1)) return MVSTER_ERR_SHAPE;
    const long tiles = (M + kTile - 1) / kTile;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(keep_flags_kernel, dim3((unsigned)tiles), dim3(kTile), 0, st, cell_of_point, neighbours, nb_points, mean, stats,
                       M, flags, wg_counts);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    rc = mv_scan_counts(wg_counts, wg_offsets, tiles, st);
    if (rc != MVSTER_OK || !mean) return rc;
    hipLaunchKernelGGL(keep_tail_kernel, dim3(1), dim3(64), 0, st, wg_offsets, tiles, stats);
    return mv_check_launch();
}
