// Host build of mvster_amd/csrc/reg_math.h -- TEST INFRASTRUCTURE ONLY.
// The crop and transform, the 18 terms of a correspondence and the histogram bin with the very functions the kernels of
// geo_reg.hip inline, in serial loops.  Never loaded by the product.
// Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/tanks_eval_cases.py).
#include "../../mvster_amd/csrc/reg_math.h"

extern "C" {

// out [N,3] = (float)(T p); T NULL: the input's bits
void hm_reg_transform(const float* p, long N, const double* T, float* out) {
    for (long k = 0; k < N; ++k) {
        double q[3];
        if (T) reg::transform(T, p + k * 3, q);
        for (int j = 0; j < 3; ++j) out[k * 3 + j] = T ? (float)q[j] : p[k * 3 + j];
    }
}

// flags [N]; volume [2 + 2 P] = axis_min, axis_max, (u, v) of the vertices -> the kept count; out_points / out_index hold them
long hm_reg_crop(const float* p, long N, const double* T, const double* volume, int P, int axis, unsigned char* flags,
                 float* out_points, long* out_index) {
    long K = 0;
    for (long k = 0; k < N; ++k) {
        double q[3];
        if (T) reg::transform(T, p + k * 3, q);
        else reg::widen(p + k * 3, q);
        flags[k] = reg::inside(q, axis, volume[0], volume[1], volume + 2, P) ? 1 : 0;
        if (!flags[k]) continue;
        for (int j = 0; j < 3; ++j) out_points[K * 3 + j] = T ? (float)q[j] : p[k * 3 + j];
        out_index[K++] = k;
    }
    return K;
}

// terms [Q,18]: the pair's terms, zeros where index[i] is outside 0 .. M - 1
void hm_reg_terms(const float* source, const long* index, const double* dist2, long Q, const float* target, long M, double* terms) {
    for (long i = 0; i < Q; ++i) {
        double* t = terms + i * reg::kSums;
        for (int j = 0; j < reg::kSums; ++j) t[j] = 0.0;
        if (index[i] < 0 || index[i] >= M) continue;
        reg::pair_terms(source + i * 3, target + index[i] * 3, dist2[i], t);
    }
}

void hm_reg_histogram(const float* dist, long N, const double* edges, int bins, long* hist) {
    for (int b = 0; b < bins; ++b) hist[b] = 0;
    for (long k = 0; k < N; ++k) {
        const int b = reg::hist_bin((double)dist[k], edges, bins);
        if (b >= 0) ++hist[b];
    }
}

}  // extern "C"
