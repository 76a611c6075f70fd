// Host build of the dynamic-consistency functions of mvster_amd/csrc/geo_math.h -- TEST INFRASTRUCTURE ONLY.
// A serial loop over a whole scan with the very functions geo_scene_dynamic_filter_kernel and geo_scene_emit_kernel
// inline (geo::dynamic_votes, geo::average, geo::backproject, geo::color_u8): level, votes, averaged depth, masks, and the
// survivors' world points and colours in emission order (reference views in pair order, pixels row-major).
// Never loaded by the product.  Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/dynamic_fusion_cases.py).
#include "../../mvster_amd/csrc/geo_math.h"

extern "C" {

// Layouts as for mvster_geo_scene_filter_dynamic / _emit (include/mvster_hip.h); images [V,H,W,3] float32.  points
// [R*H*W,3] / colors [R*H*W,3] capacity.  -> number of points, -1 for a reference view outside [0, V), -2 for more than
// 32 sources in a row.
long hm_geo_scene_dynamic(const float* depth, const float* conf, const float* images, const int* pairs, const int* ref_view,
                          const double* ref_mats, const double* view_mats, int R, int Smax, int V, int H, int W,
                          float conf_thres, int thres_view, float pix_base, float rel_base, int* mask_sum, double* depth_avg,
                          unsigned char* photo_mask, unsigned char* geo_mask, unsigned char* final_mask,
                          unsigned char* geo_level, float* points, unsigned char* colors, long* counts) {
    if (Smax > geo::kMaxLevelSources) return -2;
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
            const geo::DynamicVotes v = geo::dynamic_votes(depth, hw, H, W, pairs + (long)r * Smax, Smax, V, rm,
                                                           view_mats + (long)r * Smax * geo::kViewDoubles, x, y, dref, rx,
                                                           ry, rz, thres_view, pix_base, rel_base);
            const bool photo = conf[(long)rv * hw + p] > conf_thres, g = v.level != 0, fin = photo && g;
            const long o = (long)r * hw + p;
            mask_sum[o] = v.count;
            depth_avg[o] = geo::average(v.dsum, dref, v.count);
            photo_mask[o] = photo;
            geo_mask[o] = g;
            final_mask[o] = fin;
            geo_level[o] = (unsigned char)v.level;
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
