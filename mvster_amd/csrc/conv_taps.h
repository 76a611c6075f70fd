// Tap walk of the direct / split-K convolution kernel (conv_mfma.hip): which kernel tap and input channel a K step
// reads, where that tap lies relative to a voxel, and whether it falls into the zero padding.
//
// Small inline functions over plain integers, so that (a) conv_mfma_kernel and (b) a host build used only by the tests
// (tests/hostmath/conv_taps_hostmath.cpp) execute the same expressions.  In the kernel the arguments of the walk are
// wave-uniform for CIN >= 16 (a 16-wide K step lies inside one tap), so everything here except the per-voxel masks
// compiles to scalar instructions; for CIN 4 / 8 the K slot of a lane (lq) picks the tap and the same code runs per lane.
//
// Padding is decided once per voxel, not once per K step: a voxel carries one bit per kernel plane / row / column that is
// inside the input (axis_mask), the three sets packed into one word; a tap is inside iff its three bits are set
// (tap_select, tap_inside).  Kernels whose three extents do not fit one word (kd + kh + kw > 32) take the comparing form
// (tap_inside_cmp).
#pragma once

#if defined(__HIPCC__)
#define MVT_HD __host__ __device__ __forceinline__
#else
#define MVT_HD inline
#endif

namespace mvtaps {

// multiply-shift division by a kernel extent (constants from find_divisor / mv_fastdiv: exact for n < 2^31).  An extent of
// 1 has mul = 0 and one = ~0 (the dividend passes through), so that the walk has no branch on the divisor.
struct TapDivs {
    unsigned kw_mul, kw_shr, kw_one, kh_mul, kh_shr, kh_one;
};

struct Tap {
    int kz, ky, kx;
};

MVT_HD unsigned mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }

MVT_HD unsigned div_ms(unsigned n, unsigned mul, unsigned shr, unsigned one) { return (mulhi(n, mul) >> shr) | (n & one); }

// host side: the constants of one class (mul / shr as find_divisor makes them)
inline void make_tap_div(int d, unsigned& mul, unsigned& shr, unsigned& one) {
    mul = 0u; shr = 0u; one = ~0u;
    if (d <= 1) return;
    int lg = 31 - __builtin_clz((unsigned)d);
    if (d & (d - 1)) ++lg;                       // ceil(log2 d)
    const int p = 31 + lg;
    mul = (unsigned)(((1ull << p) + (unsigned)d - 1) / (unsigned)d);
    shr = (unsigned)(p - 32);
    one = 0u;
}
inline TapDivs make_tap_divs(int KH, int KW) {
    TapDivs dv;
    make_tap_div(KW, dv.kw_mul, dv.kw_shr, dv.kw_one);
    make_tap_div(KH, dv.kh_mul, dv.kh_shr, dv.kh_one);
    return dv;
}

// K step s, K slot lq (0..3) -> first of the slot's 4 consecutive K indices; K order is tap-major, channel-minor
template <int CIN>
MVT_HD int step_tap(int s, int lq) {
    return (int)(CIN >= 16 ? ((unsigned)s * 16u) / (unsigned)CIN : ((unsigned)s * 16u + (unsigned)lq * 4u) / (unsigned)CIN);
}
// ... and the slot's first channel.  For CIN >= 16 the tap does not depend on lq and the channel is chunk + 4 * lq.
template <int CIN>
MVT_HD int step_channel(int s, int lq) {
    return (int)(((unsigned)s * 16u + (unsigned)lq * 4u) % (unsigned)CIN);
}

// tap index -> (kz, ky, kx), kx fastest
MVT_HD Tap tap_decode(int tap, int KH, int KW, const TapDivs& dv) {
    const unsigned r = div_ms((unsigned)tap, dv.kw_mul, dv.kw_shr, dv.kw_one);
    const unsigned z = div_ms(r, dv.kh_mul, dv.kh_shr, dv.kh_one);
    Tap t;
    t.kx = tap - (int)r * KW;
    t.ky = (int)r - (int)z * KH;
    t.kz = (int)z;
    return t;
}

// linear input offset (voxels) of a tap
MVT_HD int tap_offset(const Tap& t, int Hi, int Wi) { return (t.kz * Hi + t.ky) * Wi + t.kx; }

MVT_HD bool masks_fit(int KD, int KH, int KW) { return KD + KH + KW <= 32; }

// bit k (k < K <= 31) set iff 0 <= i0 + k < extent
MVT_HD unsigned axis_mask(int i0, int K, int extent) {
    const int lo = i0 < 0 ? -i0 : 0;
    const int hi = extent - i0 < K ? extent - i0 : K;
    if (hi <= lo) return 0u;
    return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// the three axis sets of one voxel in one word: kz bits at 0, ky bits at KD, kx bits at KD + KH (masks_fit)
MVT_HD unsigned voxel_mask(int iz0, int iy0, int ix0, int KD, int KH, int KW, int Di, int Hi, int Wi) {
    return axis_mask(iz0, KD, Di) | (axis_mask(iy0, KH, Hi) << KD) | (axis_mask(ix0, KW, Wi) << (KD + KH));
}

MVT_HD unsigned tap_select(const Tap& t, int KD, int KH) {
    return (1u << t.kz) | (1u << (KD + t.ky)) | (1u << (KD + KH + t.kx));
}

MVT_HD bool tap_inside(unsigned vmask, unsigned sel) { return (vmask & sel) == sel; }

// the same decision by comparison (any kernel extent)
MVT_HD bool tap_inside_cmp(int iz0, int iy0, int ix0, const Tap& t, int Di, int Hi, int Wi) {
    return (unsigned)(iz0 + t.kz) < (unsigned)Di && (unsigned)(iy0 + t.ky) < (unsigned)Hi &&
           (unsigned)(ix0 + t.kx) < (unsigned)Wi;
}

// K steps of wave `wave` of a split-K workgroup (steps wave, wave + 4, ...); the plain walk has them all
MVT_HD int wave_steps(int nsteps_all, int wave, bool splitk) { return splitk ? (nsteps_all - wave + 3) / 4 : nsteps_all; }
MVT_HD int wave_step(int si, int wave, bool splitk) { return splitk ? wave + 4 * si : si; }

}  // namespace mvtaps
