// Host build of mvster_amd/csrc/conv_taps.h -- TEST INFRASTRUCTURE ONLY.
// One voxel's K walk with the very functions conv_mfma_kernel's load_step inlines, in the kernel's order: for each K step
// of a wave and each K slot, the tap, the slot's first channel, the tap's input offset and whether the tap is inside.
// Lets the CPU suite compare the scalar tap walk and the per-voxel masks with the emulator's decode
// (tests/conv_emulator.py) without a GPU.  Never loaded by the product.
// Build: g++ -O2 -shared -fPIC (tests/test_conv_taps_cpu.py).
#include "../../mvster_amd/csrc/conv_taps.h"

namespace {

template <int CIN>
int walk(int splitk, int wave, int nsteps_all, int KD, int KH, int KW, int Di, int Hi, int Wi, int iz0, int iy0, int ix0,
         int force_cmp, int* out) {
    using namespace mvtaps;
    const int ntaps = KD * KH * KW;
    const TapDivs dv = make_tap_divs(KH, KW);
    const bool fit = masks_fit(KD, KH, KW) && !force_cmp;
    const unsigned vmask = fit ? voxel_mask(iz0, iy0, ix0, KD, KH, KW, Di, Hi, Wi) : 0u;
    const int nsteps = wave_steps(nsteps_all, wave, splitk != 0);
    for (int si = 0; si < nsteps; ++si) {
        const int s = wave_step(si, wave, splitk != 0);
        for (int lq = 0; lq < 4; ++lq) {
            const int tap = step_tap<CIN>(s, lq);
            // (the kernel folds 4 * lq into the lane's base for CIN >= 16: chunk + 4 * lq is the slot's channel)
            const int c = CIN >= 16 ? s * 16 - tap * CIN + 4 * lq : step_channel<CIN>(s, lq);
            const bool tap_ok = CIN >= 16 || tap < ntaps;
            const Tap t = tap_decode(tap_ok ? tap : 0, KH, KW, dv);
            const bool ok = tap_ok && (fit ? tap_inside(vmask, tap_select(t, KD, KH))
                                           : tap_inside_cmp(iz0, iy0, ix0, t, Di, Hi, Wi));
            int* o = out + (si * 4 + lq) * 5;
            o[0] = s;
            o[1] = tap;
            o[2] = c;
            o[3] = tap_offset(t, Hi, Wi);
            o[4] = ok ? 1 : 0;
        }
    }
    return nsteps;
}

}  // namespace

extern "C" {

// out [steps of the wave][4 K slots][5] = (K step, tap, channel, tap offset in voxels, inside); -> steps of the wave, or -1
int hm_conv_tap_walk(int cin, int splitk, int wave, int nsteps_all, int KD, int KH, int KW, int Di, int Hi, int Wi, int iz0,
                     int iy0, int ix0, int force_cmp, int* out) {
#define MV_W(C_) if (cin == C_) return walk<C_>(splitk, wave, nsteps_all, KD, KH, KW, Di, Hi, Wi, iz0, iy0, ix0, force_cmp, out);
    MV_W(4) MV_W(8) MV_W(16) MV_W(32) MV_W(64) MV_W(80)
#undef MV_W
    return -1;
}

int hm_conv_masks_fit(int KD, int KH, int KW) { return mvtaps::masks_fit(KD, KH, KW) ? 1 : 0; }

}
