// Host build of mvster_amd/csrc/sfm_math.h -- TEST INFRASTRUCTURE ONLY.
// Pair scores, depth ranges and source lists with the very functions the kernels of geo_sfm.hip inline, as serial loops that
// follow the definition (all pairs of a track in a double loop, std::sort for the ranks and the lists), and the header's `term`
// next to long double libm for the error bound.  Never loaded by the product.
// Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/sfm_cases.py).
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "../../mvster_amd/csrc/sfm_math.h"

typedef unsigned long long u64;

extern "C" {

// q [V,V] (zeroed here, both triangles)
void hm_sfm_pair_scores(const double* centres, int V, const double* points, long P, const long* pt_ptr, const int* pt_views,
                        double theta0, double sigma1, double sigma2, u64* q) {
    std::fill(q, q + (long)V * V, 0ull);
    for (long p = 0; p < P; ++p) {
        for (long a = pt_ptr[p]; a < pt_ptr[p + 1]; ++a) {
            for (long b = a + 1; b < pt_ptr[p + 1]; ++b) {
                const int i = pt_views[a], j = pt_views[b];
                double theta;
                const u64 t = sfm::quantise(sfm::term(centres + 3l * i, centres + 3l * j, points + 3 * p, theta0, sigma1, sigma2, theta));
                q[(long)i * V + j] += t;
                q[(long)j * V + i] += t;
            }
        }
    }
}

void hm_sfm_depth_ranges(const double* rt, int V, const double* points, const long* view_ptr, const int* view_pts, int* n,
                         double* depth_min, double* depth_max) {
    std::vector<double> z;
    for (int v = 0; v < V; ++v) {
        z.clear();
        for (long k = view_ptr[v]; k < view_ptr[v + 1]; ++k) {
            const double d = sfm::depth(rt + 4l * v, points + 3l * view_pts[k]);
            if (sfm::depth_kept(d)) z.push_back(d);
        }
        std::sort(z.begin(), z.end());
        const long m = (long)z.size();
        n[v] = (int)m;
        depth_min[v] = m ? z[sfm::rank_min(m)] : sfm::nan64();
        depth_max[v] = m ? z[sfm::rank_max(m)] : sfm::nan64();
    }
}

void hm_sfm_select_sources(const u64* q, int V, int num_src, int* index, u64* value, int* count) {
    std::vector<std::pair<u64, int>> c;
    for (int i = 0; i < V; ++i) {
        c.clear();
        for (int j = 0; j < V; ++j)
            if (j != i && q[(long)i * V + j] > 0) c.push_back(std::make_pair(q[(long)i * V + j], j));
        std::sort(c.begin(), c.end(), [](const std::pair<u64, int>& a, const std::pair<u64, int>& b) {
            return sfm::before(a.first, a.second, b.first, b.second);
        });
        const int m = (int)std::min<size_t>(c.size(), (size_t)num_src);
        count[i] = m;
        for (int s = 0; s < num_src; ++s) {
            index[(long)i * num_src + s] = s < m ? c[s].second : -1;
            value[(long)i * num_src + s] = s < m ? c[s].first : 0ull;
        }
    }
}

// n triples ci, cj, x [n,3] each -> term, theta, q_term and err = term - the true value of the same inputs (long double: the
// angle from atan2l of |a x b| and a.b, expl), handed back as a double
void hm_sfm_terms(const double* ci, const double* cj, const double* x, long n, double theta0, double sigma1, double sigma2,
                  double* term, double* theta, u64* qterm, double* err) {
    const long double deg = 180.0L / acosl(-1.0L);
    for (long k = 0; k < n; ++k) {
        term[k] = sfm::term(ci + 3 * k, cj + 3 * k, x + 3 * k, theta0, sigma1, sigma2, theta[k]);
        qterm[k] = sfm::quantise(term[k]);
        long double a[3], b[3];
        for (int d = 0; d < 3; ++d) {
            a[d] = (long double)ci[3 * k + d] - (long double)x[3 * k + d];
            b[d] = (long double)cj[3 * k + d] - (long double)x[3 * k + d];
        }
        const long double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
        long double truth = 0.0L;
        if (aa > 0 && bb > 0) {
            const long double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
            const long double th = atan2l(sqrtl(cx * cx + cy * cy + cz * cz), a[0] * b[0] + a[1] * b[1] + a[2] * b[2]) * deg;
            const long double s = th <= (long double)theta0 ? sigma1 : sigma2;
            const long double d = th - (long double)theta0;
            truth = expl(-(d * d) / (2.0L * s * s));
        }
        err[k] = (double)((long double)term[k] - truth);
    }
}

// the pairs of a track of L views in the kernel's order: ab [L (L - 1) / 2, 2]
void hm_sfm_pairs(long L, long* ab) {
    for (long long e = 0; e < sfm::pairs_of(L); ++e) {
        long long a, b;
        sfm::pair_of(e, L, a, b);
        ab[2 * e] = (long)a;
        ab[2 * e + 1] = (long)b;
    }
}

void hm_sfm_pair_at(long e, long L, long* ab) {
    long long a, b;
    sfm::pair_of(e, L, a, b);
    ab[0] = (long)a;
    ab[1] = (long)b;
}

double hm_sfm_exp_neg(double x) { return sfm::exp_neg(x); }

}  // extern "C"
