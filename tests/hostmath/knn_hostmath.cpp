// Host build of mvster_amd/csrc/knn_math.h -- TEST INFRASTRUCTURE ONLY.
// The k nearest points, the radius count, the statistical filter's means and statistics and the normals with the very functions
// the kernels of geo_knn.hip inline: a serial brute force over all pairs, which is the definition, and a serial search of a hash
// grid, which proves the stopping rule for a full list.  Never loaded by the product.
// Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/cloud_clean_cases.py).
#include <algorithm>
#include <cmath>
#include <limits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../mvster_amd/csrc/knn_math.h"

namespace {

typedef std::pair<double, long> Entry;        // (d2, index): std::pair orders lexicographically

struct Cloud {
    std::vector<long> idx;
    std::vector<unsigned long long> key;
    long dropped = 0;
};

Cloud valid_points(const float* p, long n, float cell) {
    Cloud c;
    for (long k = 0; k < n; ++k) {
        unsigned long long key;
        int t[3];
        if (vox::point_key(p + k * 3, cell, key, t)) {
            c.idx.push_back(k);
            c.key.push_back(key);
        } else {
            ++c.dropped;
        }
    }
    return c;
}

bool before(const Entry& a, const Entry& b) { return nn::better(a.first, a.second, b.first, b.second); }

// All candidates of query a (position `self`, or -1) among the valid targets, in ascending (d2, index) order.
std::vector<Entry> brute_candidates(const float* a, long self, const float* target, const Cloud& t, double limit) {
    std::vector<Entry> c;
    for (long j : t.idx) {
        if (j == self) continue;
        const float* b = target + j * 3;
        const double d2 = nn::dist2(a[0], a[1], a[2], b[0], b[1], b[2]);
        if (d2 <= limit) c.push_back(Entry(d2, j));
    }
    std::sort(c.begin(), c.end(), before);
    return c;
}

typedef std::unordered_map<unsigned long long, std::vector<long>> Cells;

Cells cells_of(const Cloud& t) {
    Cells grid;
    for (size_t n = t.idx.size(); n-- > 0;) grid[t.key[n]].push_back(t.idx[n]);      // DECREASING index inside a cell
    return grid;
}

// The k first candidates through the grid with the stopping rule of knn_math.h (k <= 0: every candidate, every shell).
std::vector<Entry> grid_candidates(const float* a, unsigned long long akey, long self, const float* target, const Cells& grid,
                                   float max_dist, float cell, int k, long& probes) {
    const long long ix = vox::key_axis(akey, 0), iy = vox::key_axis(akey, 1), iz = vox::key_axis(akey, 2);
    const double limit = nn::max_dist2(max_dist);
    const int R = nn::rings(max_dist, cell);
    std::vector<Entry> c;
    for (int r = 0; r <= R; ++r) {
        for (int dz = -r; dz <= r; ++dz)
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
                    if ((ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az)) != r) continue;          // shell r only
                    unsigned long long nk;
                    if (!nn::neighbour_key(ix, iy, iz, dx, dy, dz, nk)) continue;
                    ++probes;
                    const auto it = grid.find(nk);
                    if (it == grid.end()) continue;
                    for (long j : it->second) {
                        if (j == self) continue;
                        const float* b = target + j * 3;
                        const double d2 = nn::dist2(a[0], a[1], a[2], b[0], b[1], b[2]);
                        if (d2 <= limit) c.push_back(Entry(d2, j));
                    }
                }
        std::sort(c.begin(), c.end(), before);
        if (k > 0 && (long)c.size() > k) c.resize(k);
        if (r >= 1 && k > 0 && knn::ring_done(r, cell, (long)c.size() == k, c.empty() ? 0.0 : c.back().first)) break;
    }
    return c;
}

void knn_lists(const float* query, long Q, const float* target, long M, float max_dist, float cell, int k, int exclude_self,
               double* dist2, long* index, int* count, long* dropped, bool use_grid, long& probes) {
    const Cloud q = valid_points(query, Q, cell), t = valid_points(target, M, cell);
    dropped[0] = q.dropped;
    dropped[1] = t.dropped;
    for (long i = 0; i < Q * k; ++i) {
        dist2[i] = std::numeric_limits<double>::quiet_NaN();
        index[i] = -1;
    }
    for (long i = 0; i < Q; ++i) count[i] = 0;
    const Cells grid = use_grid ? cells_of(t) : Cells();
    const double limit = nn::max_dist2(max_dist);
    for (size_t n = 0; n < q.idx.size(); ++n) {
        const long i = q.idx[n];
        const long self = exclude_self ? i : -1;
        std::vector<Entry> c = use_grid ? grid_candidates(query + i * 3, q.key[n], self, target, grid, max_dist, cell, k, probes)
                                        : brute_candidates(query + i * 3, self, target, t, limit);
        const int m = (int)std::min<long>(k, (long)c.size());
        for (int j = 0; j < k; ++j) {
            dist2[i * k + j] = j < m ? c[j].first : knn::inf();
            index[i * k + j] = j < m ? c[j].second : -1;
        }
        count[i] = m;
    }
}

// one sum of the statistics in the fixed order of knn_math.h; PASS 1: squared deviations from mu
void stat_pass(const double* mean, long M, int pass, double mu, double& n_out, double& s_out) {
    const int rows = knn::stat_rows(M);
    const long len = knn::stat_len(M, rows);
    double n = 0.0, s = 0.0;
    for (int c = 0; c < rows; ++c) {
        const long lo = (long)c * len, hi = std::min(lo + len, M);
        double sum[knn::kStatWG], cnt[knn::kStatWG];
        for (int l = 0; l < knn::kStatWG; ++l) {
            sum[l] = cnt[l] = 0.0;
            for (long i = lo + l; i < hi; i += knn::kStatWG)
                if (knn::takes_part(mean[i])) {
                    cnt[l] = cnt[l] + 1.0;
                    sum[l] = sum[l] + (pass ? knn::sq_dev(mean[i], mu) : mean[i]);
                }
        }
        double ws[4], wc[4];
        for (int w = 0; w < 4; ++w) {
            double* v = sum + w * 64;
            double* u = cnt + w * 64;
            for (int o = 32; o > 0; o >>= 1)
                for (int i = 0; i < o; ++i) {
                    v[i] = v[i] + v[i + o];
                    u[i] = u[i] + u[i + o];
                }
            ws[w] = v[0];
            wc[w] = u[0];
        }
        n = n + ((wc[0] + wc[1]) + (wc[2] + wc[3]));
        s = s + ((ws[0] + ws[1]) + (ws[2] + ws[3]));
    }
    n_out = n;
    s_out = s;
}

}  // namespace

extern "C" {

// query [Q,3], target [M,3] -> dist2 [Q,k], index [Q,k], count [Q], dropped [2] = invalid queries, targets
void hm_knn_brute(const float* query, long Q, const float* target, long M, float max_dist, float cell, int k, int exclude_self,
                  double* dist2, long* index, int* count, long* dropped) {
    long probes = 0;
    knn_lists(query, Q, target, M, max_dist, cell, k, exclude_self, dist2, index, count, dropped, false, probes);
}

// the same through a hash grid with the stopping rule -> the cells probed
long hm_knn_grid(const float* query, long Q, const float* target, long M, float max_dist, float cell, int k, int exclude_self,
                 double* dist2, long* index, int* count, long* dropped) {
    long probes = 0;
    knn_lists(query, Q, target, M, max_dist, cell, k, exclude_self, dist2, index, count, dropped, true, probes);
    return probes;
}

// neighbours [M] of the radius filter (0 for an invalid point), brute force or through the grid
void hm_radius_count(const float* points, long M, float radius, float cell, int use_grid, int* neighbours) {
    const Cloud t = valid_points(points, M, cell);
    const Cells grid = use_grid ? cells_of(t) : Cells();
    const double limit = nn::max_dist2(radius);
    long probes = 0;
    for (long i = 0; i < M; ++i) neighbours[i] = 0;
    for (size_t n = 0; n < t.idx.size(); ++n) {
        const long i = t.idx[n];
        neighbours[i] = (int)(use_grid ? grid_candidates(points + i * 3, t.key[n], i, points, grid, radius, cell, 0, probes)
                                       : brute_candidates(points + i * 3, i, points, t, limit)).size();
    }
}

// count [M], mean [M] of the statistical filter; through the grid (the CPU tests prove grid = brute force on the lists)
void hm_knn_mean(const float* points, long M, float max_dist, float cell, int k, int use_grid, int* count, double* mean) {
    const Cloud t = valid_points(points, M, cell);
    const Cells grid = use_grid ? cells_of(t) : Cells();
    const double limit = nn::max_dist2(max_dist);
    long probes = 0;
    for (long i = 0; i < M; ++i) {
        count[i] = 0;
        mean[i] = std::numeric_limits<double>::quiet_NaN();
    }
    for (size_t n = 0; n < t.idx.size(); ++n) {
        const long i = t.idx[n];
        std::vector<Entry> c = use_grid ? grid_candidates(points + i * 3, t.key[n], i, points, grid, max_dist, cell, k, probes)
                                        : brute_candidates(points + i * 3, i, points, t, limit);
        const int m = (int)std::min<long>(k, (long)c.size());
        double sum = 0.0;
        for (int j = 0; j < m; ++j) sum = sum + sqrt(c[j].first);
        count[i] = m;
        mean[i] = m == k ? knn::mean_of(sum, k) : knn::inf();
    }
}

// stats [4] = n, mu, sigma, threshold; keep [M] uint8
void hm_knn_stats(const double* mean, long M, double std_ratio, double* stats, unsigned char* keep) {
    double n = 0.0, s = 0.0, n2 = 0.0, ss = 0.0;
    if (M > 0) stat_pass(mean, M, 0, 0.0, n, s);
    const double mu = knn::mu_of(s, n);
    if (M > 0) stat_pass(mean, M, 1, mu, n2, ss);
    const double sigma = knn::sigma_of(ss, n);
    stats[0] = n;
    stats[1] = mu;
    stats[2] = sigma;
    stats[3] = knn::threshold_of(mu, sigma, std_ratio);
    for (long i = 0; i < M; ++i) keep[i] = knn::stat_keep(mean[i], stats[3]) ? 1 : 0;
}

// normals [M,3] float32, valid [M] uint8, cov [M,6] float64 (the C of every valid normal: xx, xy, xz, yy, yz, zz; else zeros);
// toward [M,3] or NULL
void hm_knn_normals(const float* points, long M, float max_dist, float cell, int k, int use_grid, const float* toward,
                    float* normals, unsigned char* valid, double* cov) {
    const Cloud t = valid_points(points, M, cell);
    const Cells grid = use_grid ? cells_of(t) : Cells();
    const double limit = nn::max_dist2(max_dist);
    long probes = 0;
    for (long i = 0; i < M; ++i) {
        normals[i * 3] = normals[i * 3 + 1] = normals[i * 3 + 2] = 0.0f;
        valid[i] = 0;
        for (int j = 0; j < 6; ++j) cov[i * 6 + j] = 0.0;
    }
    for (size_t n = 0; n < t.idx.size(); ++n) {
        const long i = t.idx[n];
        const float* p = points + i * 3;
        std::vector<Entry> c = use_grid ? grid_candidates(p, t.key[n], i, points, grid, max_dist, cell, k, probes)
                                        : brute_candidates(p, i, points, t, limit);
        const int m = (int)std::min<long>(k, (long)c.size());
        knn::Moments s = knn::no_moments();
        for (int j = 0; j < m; ++j) knn::add(s, p, points + c[j].second * 3);
        const float* tw = toward ? toward + i * 3 : p;
        valid[i] = knn::normal(s, m, p[0], p[1], p[2], toward != nullptr, tw[0], tw[1], tw[2], normals[i * 3], normals[i * 3 + 1],
                               normals[i * 3 + 2]) ? 1 : 0;
        if (valid[i]) {
            const knn::Sym3 C = knn::covariance(s, m);
            cov[i * 6 + 0] = C.xx; cov[i * 6 + 1] = C.xy; cov[i * 6 + 2] = C.xz;
            cov[i * 6 + 3] = C.yy; cov[i * 6 + 4] = C.yz; cov[i * 6 + 5] = C.zz;
        }
    }
}

}  // extern "C"
