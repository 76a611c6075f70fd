// Per-pixel arithmetic of the evaluation loader's input scaling (general_eval4.py:92-109): cv2.resize(img, (Wd, Hd)) with
// default arguments (INTER_LINEAR) on the float32 image read_img returns, restated from OpenCV's resize.cpp (float path,
// scalar form).  Shared by stage_ops.hip (load_pack_images_u8_kernel) and a host build used only by the tests
// (tests/hostmath/resize_hostmath.cpp).
//
// The per-axis tables (first tap sx / sy, fraction fx / fy) are built on the host (formats.resize_tables), as OpenCV builds
// xofs / alpha before it touches a pixel: fx = (float)((dx + 0.5) * scale_x - 0.5) in double, sx = floor(fx), fx -= sx,
// clamped at both borders.  What runs per pixel is below: the horizontal pass on the two source rows, then the vertical
// one, every product and sum rounded to fp32 on its own (mv::*_rn: neither hipcc's contraction nor the host build, which
// compiles with -ffp-contract=off, changes a bit).  The loader never enlarges, so sx + 1 leaves the row only in the last
// column at scale 1, where fx = 0: the second tap is then taken from sx itself (OpenCV does not read it at all) and its
// weight 0 makes the result the first tap exactly -- x * 1.f + y * 0.f is x for the finite non-negative values involved.
#pragma once
#include "mvster_math.h"

namespace rsz {

// float32(u8) / 255.0f with a true division: read_img (general_eval4.py:81-86).  `k` = mv::make_recip(255.0f).
MV_HD float level(unsigned char b, const mv::Recip& k) { return mv::div_rn((float)b, k); }

// second tap of an axis: sx + 1, or sx in the last column / row (weight 0 there)
MV_HD int tap1(int s, int n) { return s + 1 < n ? s + 1 : s; }

// t = S[sx] * a0 + S[sx + 1] * a1 with a0 = 1.f - fx, a1 = fx
MV_HD float lerp(float s0, float s1, float f) {
    return mv::add_rn(mv::mul_rn(s0, mv::sub_rn(1.0f, f)), mv::mul_rn(s1, f));
}

// One channel of one output pixel from its four taps (s00 s01 / s10 s11 = rows y0, y1).  `area`: Ws == 2 Wd and
// Hs == 2 Hd, where OpenCV switches INTER_LINEAR to its area path: the mean of the 2 x 2 block.  (With fx = fy = 0.5
// the linear form gives the same bits -- scaling by a power of two commutes with rounding -- but the expression below is
// the one OpenCV evaluates.)
MV_HD float blend(float s00, float s01, float s10, float s11, float fx, float fy, bool area) {
    if (area) return mv::mul_rn(mv::add_rn(mv::add_rn(s00, s01), mv::add_rn(s10, s11)), 0.25f);
    return lerp(lerp(s00, s01, fx), lerp(s10, s11, fx), fy);
}

// One output pixel of an [Hs,Ws,3] 8-bit image: rows r0 / r1 point at the first byte of source rows sy / tap1(sy),
// x0 / x1 = sx / tap1(sx).  -> rgb[3]
MV_HD void pixel(const unsigned char* __restrict__ r0, const unsigned char* __restrict__ r1, int x0, int x1, float fx, float fy,
                 bool area, const mv::Recip& k, float* rgb) {
    const unsigned char* a = r0 + 3 * (long)x0;
    const unsigned char* b = r0 + 3 * (long)x1;
    const unsigned char* c = r1 + 3 * (long)x0;
    const unsigned char* d = r1 + 3 * (long)x1;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        rgb[ch] = blend(level(a[ch], k), level(b[ch], k), level(c[ch], k), level(d[ch], k), fx, fy, area);
}

// trunc(clip(x * 255, 0, 255)): the pixel the reference writes to images/*.jpg (test_mvs4.py:262-264), one fp32 product
MV_HD unsigned char to_u8(float x) {
    const float v = mv::mul_rn(x, 255.0f);
    return (unsigned char)(int)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v));
}

}  // namespace rsz
