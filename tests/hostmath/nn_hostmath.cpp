// Host build of mvster_amd/csrc/nn_math.h -- TEST INFRASTRUCTURE ONLY.
// Cloud-to-cloud nearest distances twice, both with the very functions the kernels of geo_nn.hip inline (vox::point_key,
// nn::dist2, nn::better, nn::dist_of, nn::rings, nn::ring_done, nn::neighbour_key): a serial brute force over all pairs, which
// is the definition, and a serial search of a hash grid, which proves the ring bounds.  Never loaded by the product.
// Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/cloud_nn_cases.py).
#include <limits>
#include <unordered_map>
#include <vector>

#include "../../mvster_amd/csrc/nn_math.h"

namespace {

struct Cloud {
    std::vector<long> idx;                    // the valid points, increasing
    std::vector<unsigned long long> key;      // their cell keys
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

void prefill(long Q, float* dist, double* dist2, long* index) {
    for (long k = 0; k < Q; ++k) {
        dist[k] = std::numeric_limits<float>::quiet_NaN();
        dist2[k] = std::numeric_limits<double>::quiet_NaN();
        index[k] = -1;
    }
}

}  // namespace

extern "C" {

// query [Q,3], target [M,3] -> dist [Q] float32, dist2 [Q] float64, index [Q] int64, dropped [2] = invalid queries, targets
void hm_nn_brute(const float* query, long Q, const float* target, long M, float max_dist, float cell, float* dist, double* dist2,
                 long* index, long* dropped) {
    const Cloud q = valid_points(query, Q, cell), t = valid_points(target, M, cell);
    dropped[0] = q.dropped;
    dropped[1] = t.dropped;
    prefill(Q, dist, dist2, index);
    const double limit = nn::max_dist2(max_dist);
    for (long k : q.idx) {
        const float* a = query + k * 3;
        double best = std::numeric_limits<double>::infinity();
        long long best_index = -1;
        for (long j : t.idx) {
            const float* b = target + j * 3;
            const double d2 = nn::dist2(a[0], a[1], a[2], b[0], b[1], b[2]);
            if (d2 <= limit && nn::better(d2, j, best, best_index)) {
                best = d2;
                best_index = j;
            }
        }
        dist[k] = nn::dist_of(best);
        dist2[k] = best;
        index[k] = best_index;
    }
}

// The same through a hash grid of edge `cell`.  The targets of a cell are visited in DECREASING index, so a search that took
// the first of equal distances instead of the smallest index would be caught.  -> the cells probed, for the tests' information.
long hm_nn_grid(const float* query, long Q, const float* target, long M, float max_dist, float cell, float* dist, double* dist2,
                long* index, long* dropped) {
    const Cloud q = valid_points(query, Q, cell), t = valid_points(target, M, cell);
    dropped[0] = q.dropped;
    dropped[1] = t.dropped;
    prefill(Q, dist, dist2, index);
    std::unordered_map<unsigned long long, std::vector<long>> grid;
    for (size_t n = t.idx.size(); n-- > 0;) grid[t.key[n]].push_back(t.idx[n]);
    const double limit = nn::max_dist2(max_dist);
    const int R = nn::rings(max_dist, cell);
    long probes = 0;
    for (size_t n = 0; n < q.idx.size(); ++n) {
        const long k = q.idx[n];
        const float* a = query + k * 3;
        const long long ix = vox::key_axis(q.key[n], 0), iy = vox::key_axis(q.key[n], 1), iz = vox::key_axis(q.key[n], 2);
        double best = std::numeric_limits<double>::infinity();
        long long best_index = -1;
        for (int r = 0; r <= R; ++r) {
            for (int dz = -r; dz <= r; ++dz)
                for (int dy = -r; dy <= r; ++dy)
                    for (int dx = -r; dx <= r; ++dx) {
                        const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
                        if ((ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az)) != r) continue;      // shell r only
                        unsigned long long nk;
                        if (!nn::neighbour_key(ix, iy, iz, dx, dy, dz, nk)) continue;
                        ++probes;
                        const auto it = grid.find(nk);
                        if (it == grid.end()) continue;
                        for (long j : it->second) {
                            const float* b = target + j * 3;
                            const double d2 = nn::dist2(a[0], a[1], a[2], b[0], b[1], b[2]);
                            if (d2 <= limit && nn::better(d2, j, best, best_index)) {
                                best = d2;
                                best_index = j;
                            }
                        }
                    }
            if (r >= 1 && nn::ring_done(r, cell, best)) break;
        }
        dist[k] = nn::dist_of(best);
        dist2[k] = best;
        index[k] = best_index;
    }
    return probes;
}

int hm_nn_rings(float max_dist, float cell) { return nn::rings(max_dist, cell); }
int hm_nn_cell_ok(float max_dist, float cell) { return nn::cell_ok(max_dist, cell); }

}  // extern "C"
