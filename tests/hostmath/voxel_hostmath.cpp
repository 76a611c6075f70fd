// Host build of mvster_amd/csrc/voxel_math.h -- TEST INFRASTRUCTURE ONLY.
// A serial voxel-grid thinning with the very functions the kernels of geo_thin.hip inline (vox::point_key, vox::hash,
// vox::mean_coord, vox::mean_color), plus the per-point quantities and the hash on their own.  Never loaded by the product.
// Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/voxel_thin_cases.py).
#include <unordered_map>
#include <vector>

#include "../../mvster_amd/csrc/voxel_math.h"

extern "C" {

// points [M,3] -> valid [M] (0 / 1), key [M] (0 where invalid), t [M,3] (0 where invalid)
void hm_voxel_points(const float* points, long M, float v, unsigned char* valid, unsigned long long* key, int* t) {
    for (long k = 0; k < M; ++k) {
        unsigned long long kk = 0;
        int tt[3] = {0, 0, 0};
        const bool ok = vox::point_key(points + k * 3, v, kk, tt);
        valid[k] = ok;
        key[k] = ok ? kk : 0;
        for (int j = 0; j < 3; ++j) t[k * 3 + j] = ok ? tt[j] : 0;
    }
}

void hm_voxel_hash(const unsigned long long* key, long n, unsigned long long* out) {
    for (long k = 0; k < n; ++k) out[k] = vox::hash(key[k]);
}

// reduce 0 = mean, 1 = first.  Outputs have room for M rows.  -> U; *dropped = invalid points.
long hm_voxel_thin(const float* points, const unsigned char* colors, long M, float v, int reduce, float* out_points,
                   unsigned char* out_colors, int* out_counts, long* out_first, long* dropped) {
    struct Row { long long f; unsigned n; unsigned long long key, s[6]; };
    std::unordered_map<unsigned long long, long> rank;
    std::vector<Row> rows;
    *dropped = 0;
    for (long k = 0; k < M; ++k) {                                          // input order: ranks follow the first points
        unsigned long long key;
        int t[3];
        if (!vox::point_key(points + k * 3, v, key, t)) {
            ++*dropped;
            continue;
        }
        auto it = rank.find(key);
        if (it == rank.end()) {
            it = rank.emplace(key, (long)rows.size()).first;
            rows.push_back(Row{k, 0, key, {0, 0, 0, 0, 0, 0}});
        }
        Row& r = rows[it->second];
        ++r.n;
        for (int j = 0; j < 3; ++j) {
            r.s[j] += (unsigned long long)t[j];
            r.s[3 + j] += colors[k * 3 + j];
        }
    }
    for (size_t u = 0; u < rows.size(); ++u) {
        const Row& r = rows[u];
        out_first[u] = r.f;
        out_counts[u] = (int)r.n;
        for (int j = 0; j < 3; ++j) {
            if (reduce == 0) {
                out_points[u * 3 + j] = vox::mean_coord(vox::key_axis(r.key, j), r.s[j], r.n, v);
                out_colors[u * 3 + j] = vox::mean_color(r.s[3 + j], r.n);
            } else {
                out_points[u * 3 + j] = points[r.f * 3 + j];
                out_colors[u * 3 + j] = colors[r.f * 3 + j];
            }
        }
    }
    return (long)rows.size();
}

}  // extern "C"
