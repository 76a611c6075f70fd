// A scan from a structure-from-motion model on the GPU (the definition is sfm_math.h): the scores of all
// pairs of views over their common sparse points, every view's depth range and every view's source list.
//
//   mvster_sfm_pair_scores     sfm_zero_kernel       q [V,V] = 0
//                              pair_scores_kernel    point-centric: one lane per (point, pair within its track); item_ptr [P+1]
//                                                    is the prefix sum of L (L - 1) / 2.  A workgroup owns kTile consecutive items:
//                                                    it searches item_ptr once for the points its tile spans, then every lane
//                                                    searches only among those; the pair comes from the triangular index in
//                                                    integers (sfm::pair_of), rows first, so the lanes of a wave mostly add into
//                                                    one row of q at ascending columns.  One 64-bit integer atomic per item into the
//                                                    upper triangle.  No floating-point atomics: two runs give the same bytes.
//                              mirror_kernel         q[j][i] = q[i][j] for i < j
//   mvster_sfm_depth_ranges    depth_range_kernel    one workgroup per view: 8 passes of 8 bits from the top over the bit patterns
//                                                    of the view's kept depths, both ranks at once, histograms in LDS; the depths are
//                                                    formed again in every pass and never stored.  No sort, no global atomics.
//   mvster_sfm_select_sources  select_kernel         one wave per row: num_src rounds of an arg-max over (q, -j) among the entries
//                                                    behind the one picked last
#include "common.hpp"
#include "sfm_math.h"

namespace {

constexpr int kWG = 256;
constexpr int kItems = 8;                 // items per lane of pair_scores_kernel
constexpr int kTile = kWG * kItems;
constexpr int kBins = 256;
constexpr int kDigits = 8;

typedef unsigned long long u64;
typedef long long i64;

__global__ void __launch_bounds__(kWG) sfm_zero_kernel(u64* __restrict__ p, i64 n) {
    for (i64 i = (i64)blockIdx.x * kWG + threadIdx.x; i < n; i += (i64)gridDim.x * kWG) p[i] = 0;
}

// the last p in [lo, hi] with ptr[p] <= t (ptr[lo] <= t is the caller's)
__device__ __forceinline__ i64 find_point(const i64* __restrict__ ptr, i64 lo, i64 hi, i64 t) {
    while (lo < hi) {                                                           // at most 64 halvings
        const i64 mid = lo + (hi - lo + 1) / 2;
        if (ptr[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct PairArgs {
    const double* centres;            // [V,3]
    const double* points;             // [P,3]
    const i64* pt_ptr;                // [P+1]
    const int* pt_views;              // [nobs]
    const i64* item_ptr;              // [P+1]
    i64 P, nobs, total;
    int V;
    double theta0, sigma1, sigma2;
    u64* q;                           // [V,V]
};

// Nothing read from the device tables is trusted as an address: a point outside 0 .. P-1, a track that leaves pt_views, a
// pair outside its track or a view outside 0 .. V-1 adds nothing.
__global__ void __launch_bounds__(kWG) pair_scores_kernel(PairArgs a) {
    const i64 t0 = (i64)blockIdx.x * kTile;
    const i64 t1 = t0 + kTile < a.total ? t0 + kTile : a.total;
    if (t0 >= t1) return;
    const i64 p0 = find_point(a.item_ptr, 0, a.P - 1, t0);                      // the same in every lane
    const i64 p1 = find_point(a.item_ptr, p0, a.P - 1, t1 - 1);
#pragma unroll 1
    for (int k = 0; k < kItems; ++k) {
        const i64 t = t0 + (i64)k * kWG + threadIdx.x;
        if (t >= t1) continue;
        const i64 p = find_point(a.item_ptr, p0, p1, t);
        const i64 lo = a.pt_ptr[p], L = a.pt_ptr[p + 1] - lo, e = t - a.item_ptr[p];
        if (lo < 0 || L < 2 || L > a.V || lo + L > a.nobs || e < 0 || e >= sfm::pairs_of(L)) continue;
        i64 ia, ib;
        sfm::pair_of(e, L, ia, ib);
        if (ia < 0 || ib <= ia || ib >= L) continue;
        const int i = a.pt_views[lo + ia], j = a.pt_views[lo + ib];
        if (i < 0 || j <= i || j >= a.V) continue;
        const double x[3] = {a.points[p * 3 + 0], a.points[p * 3 + 1], a.points[p * 3 + 2]};
        const double ci[3] = {a.centres[(i64)i * 3 + 0], a.centres[(i64)i * 3 + 1], a.centres[(i64)i * 3 + 2]};
        const double cj[3] = {a.centres[(i64)j * 3 + 0], a.centres[(i64)j * 3 + 1], a.centres[(i64)j * 3 + 2]};
        double theta;
        const u64 qt = sfm::quantise(sfm::term(ci, cj, x, a.theta0, a.sigma1, a.sigma2, theta));
        if (qt) atomicAdd(&a.q[(i64)i * a.V + j], qt);
    }
}

__global__ void __launch_bounds__(kWG) mirror_kernel(u64* __restrict__ q, int V) {
    const i64 n = (i64)V * V;
    for (i64 t = (i64)blockIdx.x * kWG + threadIdx.x; t < n; t += (i64)gridDim.x * kWG) {
        const i64 r = t / V, c = t - r * V;
        if (r > c) q[t] = q[c * V + r];                                         // reads the upper triangle only, writes the lower
    }
}

// One histogram add per lane, or one per wave where every taking lane has the same digit (the top passes of a view's depths:
// sign and exponent agree, and 64 adds to one LDS word would queue up).
__device__ __forceinline__ void hist_add(unsigned* h, bool take, unsigned digit) {
    const u64 act = __ballot(take);
    if (!act) return;
    const int leader = __ffsll((i64)act) - 1;
    const unsigned first = (unsigned)__shfl((int)digit, leader, 64);
    const u64 same = __ballot(take && digit == first);
    if (same == act) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[first & (kBins - 1)], (unsigned)__popcll(act));
    } else if (take) {
        atomicAdd(&h[digit & (kBins - 1)], 1u);
    }
}

__global__ void __launch_bounds__(kWG) depth_range_kernel(const double* __restrict__ rt, const double* __restrict__ points, i64 P,
                                                          const i64* __restrict__ view_ptr, const int* __restrict__ view_pts,
                                                          i64 nobs, int* __restrict__ n_out, double* __restrict__ dmin,
                                                          double* __restrict__ dmax) {
    __shared__ unsigned h[2][kBins];
    __shared__ u64 prefix[2];
    __shared__ i64 rank[2];
    __shared__ i64 total;
    const int v = blockIdx.x;
    i64 lo = view_ptr[v], hi = view_ptr[v + 1];
    if (lo < 0) lo = 0;
    if (hi > nobs) hi = nobs;
    const double r[4] = {rt[(i64)v * 4 + 0], rt[(i64)v * 4 + 1], rt[(i64)v * 4 + 2], rt[(i64)v * 4 + 3]};
    if (threadIdx.x == 0) {
        prefix[0] = prefix[1] = 0;
        rank[0] = rank[1] = 0;
        total = 0;
    }
#pragma unroll 1
    for (int pass = 0; pass < kDigits; ++pass) {
        h[0][threadIdx.x] = 0u;
        h[1][threadIdx.x] = 0u;
        __syncthreads();                                                        // (also publishes prefix / rank of the pass before)
        const int shift = 56 - 8 * pass;
        const u64 pre0 = prefix[0], pre1 = prefix[1];
        for (i64 base = lo; base < hi; base += kWG) {                           // the same trip count in every lane
            const i64 k = base + threadIdx.x;
            bool kept = false;
            u64 bits = 0;
            if (k < hi) {
                const i64 p = view_pts[k];
                if (p >= 0 && p < P) {
                    const double x[3] = {points[p * 3 + 0], points[p * 3 + 1], points[p * 3 + 2]};
                    const double z = sfm::depth(r, x);
                    kept = sfm::depth_kept(z);
                    bits = sfm::depth_bits(z);
                }
            }
            const unsigned digit = (unsigned)(bits >> shift) & 255u;
            const u64 above = pass ? bits >> (shift + 8) : 0;
            hist_add(h[0], kept && above == (pass ? pre0 >> (shift + 8) : 0), digit);
            hist_add(h[1], kept && above == (pass ? pre1 >> (shift + 8) : 0), digit);
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            const int t = threadIdx.x;
            i64 want = rank[t];
            if (pass == 0) {
                i64 n = 0;
                for (int b = 0; b < kBins; ++b) n += h[t][b];                   // 256 bins: bounded
                want = t ? sfm::rank_max(n) : sfm::rank_min(n);
                if (t == 0) total = n;
            }
            i64 cum = 0;
            int digit = kBins - 1;
            for (int b = 0; b < kBins; ++b) {
                const i64 c = h[t][b];
                if (want < cum + c) {
                    digit = b;
                    break;
                }
                cum += c;
            }
            rank[t] = want - cum;
            prefix[t] |= (u64)digit << shift;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const i64 n = total;
        n_out[v] = (int)n;
        dmin[v] = n > 0 ? __longlong_as_double((i64)prefix[0]) : sfm::nan64();
        dmax[v] = n > 0 ? __longlong_as_double((i64)prefix[1]) : sfm::nan64();
    }
}

// (q, j) of the lanes folded to the first in the list's order; j = -1: none
__device__ __forceinline__ void wave_first(u64& q, int& j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 oq = __shfl_xor(q, o, 64);
        const int oj = __shfl_xor(j, o, 64);
        if (oj >= 0 && (j < 0 || sfm::before(oq, oj, q, j))) {
            q = oq;
            j = oj;
        }
    }
}

__global__ void __launch_bounds__(kWG) select_kernel(const u64* __restrict__ q, int V, int num_src, int* __restrict__ index,
                                                     u64* __restrict__ value, int* __restrict__ count) {
    const int row = blockIdx.x * (kWG / 64) + (threadIdx.x >> 6);               // the same in every lane of a wave
    const int lane = threadIdx.x & 63;
    if (row >= V) return;
    const u64* qr = q + (i64)row * V;
    u64 last_q = 0;
    int last_j = -1, found = 0;
#pragma unroll 1
    for (int s = 0; s < num_src; ++s) {
        u64 best_q = 0;
        int best_j = -1;
        for (int j = lane; j < V; j += 64) {
            const u64 c = qr[j];
            if (c == 0 || j == row) continue;
            if (last_j >= 0 && !sfm::before(last_q, last_j, c, j)) continue;    // listed already, or before what is listed
            if (best_j < 0 || sfm::before(c, j, best_q, best_j)) {
                best_q = c;
                best_j = j;
            }
        }
        wave_first(best_q, best_j);
        if (best_j >= 0) ++found;
        if (lane == 0) {
            index[(i64)row * num_src + s] = best_j;
            value[(i64)row * num_src + s] = best_j >= 0 ? best_q : 0;
        }
        if (best_j < 0) {                                                       // the same in every lane: the rest stays empty
            for (int r = s + 1 + lane; r < num_src; r += 64) {
                index[(i64)row * num_src + r] = -1;
                value[(i64)row * num_src + r] = 0;
            }
            break;
        }
        last_q = best_q;
        last_j = best_j;
    }
    if (lane == 0) count[row] = found;
}

unsigned capped_blocks(i64 n) {
    const i64 b = (n + kWG - 1) / kWG;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" int mvster_sfm_pair_scores(const double* centres, int V, const double* points, long P, const long* pt_ptr,
                                      const int* pt_views, long nobs, const long* item_ptr, long total, double theta0, double sigma1,
                                      double sigma2, unsigned long long* q, void* stream) {
    if (!centres || !q) return MVSTER_ERR_NULL;
    if (P > 0 && (!points || !pt_ptr || !item_ptr)) return MVSTER_ERR_NULL;
    if (nobs > 0 && !pt_views) return MVSTER_ERR_NULL;
    if (V < 1 || V > sfm::kMaxViews || P < 0 || P >= (1l << 31) || nobs < 0 || nobs > (1l << 34) || total < 0 || total > (1l << 40))
        return MVSTER_ERR_SHAPE;
    if ((P == 0 && total != 0) || !sfm::params_ok(theta0, sigma1, sigma2)) return MVSTER_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const i64 cells = (i64)V * V;
    hipLaunchKernelGGL(sfm_zero_kernel, dim3(capped_blocks(cells)), dim3(kWG), 0, st, q, cells);
    int rc = mv_check_launch();
    if (rc != MVSTER_OK || total == 0) return rc;
    PairArgs a;
    a.centres = centres;
    a.points = points;
    a.pt_ptr = reinterpret_cast<const i64*>(pt_ptr);
    a.pt_views = pt_views;
    a.item_ptr = reinterpret_cast<const i64*>(item_ptr);
    a.P = P;
    a.nobs = nobs;
    a.total = total;
    a.V = V;
    a.theta0 = theta0;
    a.sigma1 = sigma1;
    a.sigma2 = sigma2;
    a.q = q;
    hipLaunchKernelGGL(pair_scores_kernel, dim3((unsigned)((total + kTile - 1) / kTile)), dim3(kWG), 0, st, a);
    rc = mv_check_launch();
    if (rc != MVSTER_OK) return rc;
    hipLaunchKernelGGL(mirror_kernel, dim3(capped_blocks(cells)), dim3(kWG), 0, st, q, V);
    return mv_check_launch();
}

extern "C" int mvster_sfm_depth_ranges(const double* rt, int V, const double* points, long P, const long* view_ptr,
                                       const int* view_pts, long nobs, int* n, double* depth_min, double* depth_max, void* stream) {
    if (!rt || !view_ptr || !n || !depth_min || !depth_max) return MVSTER_ERR_NULL;
    if ((P > 0 && !points) || (nobs > 0 && !view_pts)) return MVSTER_ERR_NULL;
    if (V < 1 || V > sfm::kMaxViews || P < 0 || P >= (1l << 31) || nobs < 0 || nobs > (1l << 34)) return MVSTER_ERR_SHAPE;
    hipLaunchKernelGGL(depth_range_kernel, dim3((unsigned)V), dim3(kWG), 0, (hipStream_t)stream, rt, points, (i64)P,
                       reinterpret_cast<const i64*>(view_ptr), view_pts, (i64)nobs, n, depth_min, depth_max);
    return mv_check_launch();
}

extern "C" int mvster_sfm_select_sources(const unsigned long long* q, int V, int num_src, int* index, unsigned long long* value,
                                         int* count, void* stream) {
    if (!q || !index || !value || !count) return MVSTER_ERR_NULL;
    if (V < 1 || V > sfm::kMaxViews || num_src < 1 || num_src > sfm::kMaxSources) return MVSTER_ERR_SHAPE;
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)((V + kWG / 64 - 1) / (kWG / 64))), dim3(kWG), 0, (hipStream_t)stream, q, V,
                       num_src, index, value, count);
    return mv_check_launch();
}
