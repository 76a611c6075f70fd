// Host build of mvster_amd/csrc/geo_math.h -- TEST INFRASTRUCTURE ONLY.
// A serial loop over a whole scan with the very functions geo_filter.hip and geo_scene.hip inline: votes, averaged depth,
// masks, and the survivors' world points and colours in the reference's emission order (reference views in pair order,
// pixels row-major).  Lets the CPU suite check the fusion arithmetic against oracle/geo_filter_oracle.py without a GPU.
// Never loaded by the product.  Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/test_fusion_scene_cpu.py).
#include "../../mvster_amd/csrc/geo_math.h"

extern "C" {

float hm_geo_remap_linear(const float* src, int H, int W, float x, float y) { return geo::remap_linear(src, H, W, x, y); }

// Layouts as for mvster_geo_scene_filter / _emit (include/mvster_hip.h); images [V,H,W,3] float32.  view_mask
// [R,Smax,H,W] (optional) = the per-(pixel, source view) votes.  points [R*H*W,3] / colors [R*H*W,3] capacity.
// -> number of points, or -1 for a view index outside [0, V).
long hm_geo_scene(const float* depth, const float* conf, const float* images, const int* pairs, const int* ref_view,
                  const double* ref_mats, const double* view_mats, int R, int Smax, int V, int H, int W, float conf_thres,
                  int thres_view, float pix_thres, float rel_thres, int* mask_sum, double* depth_avg,
                  unsigned char* photo_mask, unsigned char* geo_mask, unsigned char* final_mask, unsigned char* view_mask,
                  float* points, unsigned char* colors, long* counts) {
    const long hw = (long)H * W;
    long m = 0;
    for (int r = 0; r < R; ++r) {
        const int rv = ref_view[r];
        if (rv < 0 || rv >= V) return -1;
        const double* rm = ref_mats + (long)r * geo::kRefDoubles;
        counts[r] = 0;
        for (long p = 0; p < hw; ++p) {
            const int y = (int)(p / W), x = (int)(p - (long)y * W);
            const float dref = depth[(long)rv * hw + p];
            double rx, ry, rz;
            geo::lift_ref(rm, x, y, dref, rx, ry, rz);
            int count = 0;
            float dsum = 0.0f;
            for (int s = 0; s < Smax; ++s) {
                const int sv = pairs[(long)r * Smax + s];
                if (sv < 0) break;
                if (sv >= V) return -1;
                const geo::Vote vt = geo::view_vote(depth + (long)sv * hw, H, W, rm,
                                                    view_mats + ((long)r * Smax + s) * geo::kViewDoubles, x, y, dref, rx, ry,
                                                    rz, pix_thres, rel_thres);
                geo::accumulate(vt, count, dsum);
                if (view_mask) view_mask[((long)r * Smax + s) * hw + p] = vt.ok ? 1 : 0;
            }
            const bool photo = conf[(long)rv * hw + p] > conf_thres, g = count >= thres_view, fin = photo && g;
            const long o = (long)r * hw + p;
            mask_sum[o] = count;
            depth_avg[o] = geo::average(dsum, dref, count);
            photo_mask[o] = photo;
            geo_mask[o] = g;
            final_mask[o] = fin;
            if (!fin) continue;
            double wx, wy, wz;
            geo::backproject(rm, rm + 18, x, y, depth_avg[o], wx, wy, wz);
            points[m * 3 + 0] = (float)wx;
            points[m * 3 + 1] = (float)wy;
            points[m * 3 + 2] = (float)wz;
            const float* im = images + ((long)rv * hw + p) * 3;
            for (int c = 0; c < 3; ++c) colors[m * 3 + c] = geo::color_u8(im[c]);
            ++m;
            ++counts[r];
        }
    }
    return m;
}

}  // extern "C"
