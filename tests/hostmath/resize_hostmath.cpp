// Host build of mvster_amd/csrc/resize_math.h -- TEST INFRASTRUCTURE ONLY.
// A serial loop over a stack of 8-bit images with the very functions load_pack_images_u8_kernel inlines: the RGB0 float
// output and the 8-bit output of mvster_load_pack_images_u8 on full-image windows of one size, from the same host-built
// tables.  Lets the CPU suite check the resampling arithmetic against the NumPy restatements without a GPU, and the GPU
// suite compare the kernel byte for byte.
// Never loaded by the product.  Build: g++ -O2 -shared -fPIC -ffp-contract=off (tests/resize_cases.py).
#include "../../mvster_amd/csrc/resize_math.h"

extern "C" {

// Layouts as for mvster_load_pack_images_u8 (include/mvster_hip.h) on a packed stack: src [V,Hs,Ws,3], out [V,Hd,Wd,4],
// out_u8 [V,Hd,Wd,3] (optional).  -> 0, or -1 for a table entry outside the image (the kernel clamps; a test must never
// rely on that).
int hm_resize_pack(const unsigned char* src, const int* sx, const float* fx, const int* sy, const float* fy, float* out,
                   unsigned char* out_u8, int V, int Hs, int Ws, int Hd, int Wd) {
    const bool area = Ws == 2 * Wd && Hs == 2 * Hd;
    const mv::Recip k = mv::make_recip(255.0f);
    for (int x = 0; x < Wd; ++x)
        if (sx[x] < 0 || sx[x] >= Ws) return -1;
    for (int y = 0; y < Hd; ++y)
        if (sy[y] < 0 || sy[y] >= Hs) return -1;
    for (int v = 0; v < V; ++v) {
        const unsigned char* img = src + (long)v * Hs * Ws * 3;
        for (int y = 0; y < Hd; ++y) {
            const unsigned char* r0 = img + (long)sy[y] * Ws * 3;
            const unsigned char* r1 = img + (long)rsz::tap1(sy[y], Hs) * Ws * 3;
            for (int x = 0; x < Wd; ++x) {
                const long p = ((long)v * Hd + y) * Wd + x;
                float rgb[3];
                rsz::pixel(r0, r1, sx[x], rsz::tap1(sx[x], Ws), fx[x], fy[y], area, k, rgb);
                for (int c = 0; c < 3; ++c) {
                    out[p * 4 + c] = rgb[c];
                    if (out_u8) out_u8[p * 3 + c] = rsz::to_u8(rgb[c]);
                }
                out[p * 4 + 3] = 0.0f;
            }
        }
    }
    return 0;
}

}  // extern "C"
