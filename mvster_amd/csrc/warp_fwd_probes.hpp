// The forward forms kept for the record: the pixel-major kernel (variant 4) and the LDS-window kernel (variant 5), with
// their launchers.  Probe build only: warp_fwd.hip includes this file, inside its anonymous namespace, under MVSTER_PROBES.

// ------------------------------------------------------------------------------------------
// Pixel-major variant for the two fine stages (C <= 16, where the time is): lane = (pixel, sub), and the lane
// walks ALL D hypotheses of its pixel.  The wave-local kernel (warp_fwd.hip) is VALU-issue-bound (PMC: ~205 VALU
// instructions per (pixel, d, view) against 256 gathered bytes; 77 % of the SIMD issue cycles busy), so this one
// removes instructions rather than bytes:
//   * R*(x, y, 1) once per (pixel, view) instead of once per (pixel, d, view);
//   * the per-hypothesis scalar chain (r*depth + t, the IEEE division by z, the normalise / un-normalise round trip,
//     the fractional weights) runs on PAIRS of hypotheses in packed fp32 (v_pk_mul/add/fma_f32): same rounding per
//     element, half the issue slots;
//   * taps are fetched with raw buffer loads: ONE 32-bit offset per tap row ((y0*Ws + x0) << log2(4C), 24-bit
//     multiply-add), the other seven addresses are immediate offsets, and no index clamping at all -- a tap outside
//     the map either falls outside the descriptor (the hardware returns 0) or reads some other texel, and in both
//     cases its weight is already 0;
//   * the softmax over depth is in registers: no ds_bpermute, one reciprocal per pixel.
// Arithmetic per element and every summation order are those of warp_agg_fwd_kernel: bit-identical output.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ mv::f32x2 fma2(mv::f32x2 a, mv::f32x2 b, mv::f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ mv::f32x2 splat2(float v) { return (mv::f32x2){v, v}; }

struct Recip2 {
    mv::f32x2 d, r;
};
__device__ __forceinline__ Recip2 make_recip2(mv::f32x2 d) {
    Recip2 k;
    k.d = d;
    const mv::f32x2 r0 = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    k.r = fma2(fma2(-d, r0, splat2(1.0f)), r0, r0);
    return k;
}
// same sequence as mv::div_rn(float, Recip) on both elements
__device__ __forceinline__ mv::f32x2 div_rn2(mv::f32x2 a, const Recip2& k) {
    mv::f32x2 q = mv::mul_rn2(a, k.r);
    q = fma2(fma2(-k.d, q, a), k.r, q);
    return fma2(fma2(-k.d, q, a), k.r, q);
}
__device__ __forceinline__ mv::f32x2 div_rn2(mv::f32x2 a, const mv::Recip& k) {
    const mv::f32x2 d = splat2(k.d), r = splat2(k.r);
    mv::f32x2 q = mv::mul_rn2(a, r);
    q = fma2(fma2(-d, q, a), r, q);
    return fma2(fma2(-d, q, a), r, q);
}
__device__ __forceinline__ mv::f32x2 sub_rn2(mv::f32x2 a, mv::f32x2 b) {
#pragma clang fp contract(off)
    return a - b;
}

// DPL = hypotheses per lane (even): DPL = D is the form described above; DPL = 2 spreads the D / 2 hypothesis pairs of a
// pixel over QL = D / 2 lanes (twice / four times the waves, half / a quarter of the registers' worth of in-flight
// taps per lane), with the softmax over depth as an in-wave all-gather like the wave-local kernel.
template <int C, int G, int D, int DPL, int WPE>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, 8))) warp_agg_fwd_pix_kernel(WarpAggArgs a) {
    constexpr int LPP = C / 8;           // lanes per (pixel, hypothesis group): channel slices of 8
    constexpr int CG = C / G;            // channels per group
    constexpr int GPL = 8 / CG;          // whole groups per lane
    constexpr int QL = D / DPL;          // lanes (hypothesis groups) per pixel and channel slice
    constexpr int PPW = 64 / (LPP * QL); // pixels per wave (a workgroup is one wave: waves never talk to each other)
    constexpr int SH = C == 8 ? 5 : (C == 16 ? 6 : (C == 32 ? 7 : 8));   // log2(bytes per texel)
    static_assert(C % 8 == 0 && CG <= 8 && 8 % CG == 0 && DPL % 2 == 0 && D % DPL == 0 && PPW >= 1 &&
                  PPW * LPP * QL == 64 && D <= 8, "pixel split");

    const int lane = threadIdx.x;
    const int sub = lane % LPP, pl = (lane / LPP) % PPW, qg = lane / (LPP * PPW);
    const int b = blockIdx.y;
    const int hw = a.h * a.w;
    const int p = xcd_remap(blockIdx.x, gridDim.x) * PPW + pl;
    const bool valid = p < hw;
    const int pc = valid ? p : hw - 1;   // clamped: every lane takes part in the cross-lane sums
    const int y = pc / a.w;
    const int x = pc - y * a.w;
    const float xf = (float)x, yf = (float)y;
    const float* hp = a.hypo + ((long)b * D + qg * DPL) * hw + pc;
    mv::f32x2 depth2[DPL / 2];
#pragma unroll
    for (int q = 0; q < DPL / 2; ++q) depth2[q] = (mv::f32x2){hp[(long)(2 * q) * hw], hp[(long)(2 * q + 1) * hw]};
    const float* rp = a.ref + (long)b * a.ref_bs + (long)pc * C + sub * 8;
    const f32x4 R0 = ld4(rp), R1 = ld4(rp + 4);
    const mv::GridNorm gn = mv::make_grid_norm(a.Hs, a.Ws);
    const mv::Recip temp = mv::make_recip(a.attn_temp), sqrt_c = mv::make_recip(a.sqrt_c);
    const float xhi = (float)(a.Ws + 4), yhi = (float)(a.Hs + 4);
    const unsigned src_bytes = (unsigned)a.Hs * (unsigned)a.Ws * (unsigned)(C * 4);
    const int row_bytes = a.Ws << SH;

    float acc[DPL][GPL], wsum[DPL];
#pragma unroll
    for (int d = 0; d < DPL; ++d) {
        wsum[d] = 1e-8f;
#pragma unroll
        for (int k = 0; k < GPL; ++k) acc[d][k] = 0.0f;
    }

    for (int v = 0; v < a.NV; ++v) {
        const float* r = a.rt + ((long)b * a.NV + v) * 12;  // wave-uniform
        // rot @ (x, y, 1): the reference's sgemm FMA chain (mv::project), once per (pixel, view)
        const float rx = mv::add_rn(fmaf(r[1], yf, mv::mul_rn(r[0], xf)), r[2]);
        const float ry = mv::add_rn(fmaf(r[4], yf, mv::mul_rn(r[3], xf)), r[5]);
        const float rz = mv::add_rn(fmaf(r[7], yf, mv::mul_rn(r[6], xf)), r[8]);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.src + (long)v * a.src_vs + (long)b * a.src_bs), (short)0, (int)src_bytes, 0x00020000);

        float cg[DPL][GPL], score[DPL];
#pragma unroll
        for (int q = 0; q < DPL / 2; ++q) {
            // two hypotheses at a time through the scalar chain, packed
            const mv::f32x2 dz = depth2[q];
            const mv::f32x2 px = mv::add_rn2(mv::mul_rn2(splat2(rx), dz), splat2(r[9]));
            const mv::f32x2 py = mv::add_rn2(mv::mul_rn2(splat2(ry), dz), splat2(r[10]));
            mv::f32x2 pz = mv::add_rn2(mv::mul_rn2(splat2(rz), dz), splat2(r[11]));
            if (pz[0] == 0.0f) pz[0] = 1e-9f;
            if (pz[1] == 0.0f) pz[1] = 1e-9f;
            const Recip2 z = make_recip2(pz);
            // grid_roundtrip(): / half, - 1, + 1, * 0.5, * (size - 1)
            mv::f32x2 sx = sub_rn2(div_rn2(div_rn2(px, z), gn.halfw), splat2(1.0f));
            mv::f32x2 sy = sub_rn2(div_rn2(div_rn2(py, z), gn.halfh), splat2(1.0f));
            sx = mv::mul_rn2(mv::mul_rn2(mv::add_rn2(sx, splat2(1.0f)), splat2(0.5f)), splat2(gn.wm1));
            sy = mv::mul_rn2(mv::mul_rn2(mv::add_rn2(sy, splat2(1.0f)), splat2(0.5f)), splat2(gn.hm1));
            // make_taps(): clamp far-away / NaN positions, corner, fractional weights
            const mv::f32x2 cx = {__builtin_amdgcn_fmed3f(sx[0], -4.0f, xhi), __builtin_amdgcn_fmed3f(sx[1], -4.0f, xhi)};
            const mv::f32x2 cy = {__builtin_amdgcn_fmed3f(sy[0], -4.0f, yhi), __builtin_amdgcn_fmed3f(sy[1], -4.0f, yhi)};
            const mv::f32x2 fx = {floorf(cx[0]), floorf(cx[1])}, fy = {floorf(cy[0]), floorf(cy[1])};
            const mv::f32x2 wx1 = sub_rn2(cx, fx), wy1 = sub_rn2(cy, fy);
            const mv::f32x2 wx0 = sub_rn2(splat2(1.0f), wx1), wy0 = sub_rn2(splat2(1.0f), wy1);
            mv::f32x2 nw = mv::mul_rn2(wy0, wx0), ne = mv::mul_rn2(wy0, wx1);
            mv::f32x2 sw = mv::mul_rn2(wy1, wx0), se = mv::mul_rn2(wy1, wx1);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int d = 2 * q + e;
                const int x0 = (int)fx[e], y0 = (int)fy[e];
                const bool vx0 = (unsigned)x0 < (unsigned)a.Ws, vx1 = (unsigned)(x0 + 1) < (unsigned)a.Ws;
                const bool vy0 = (unsigned)y0 < (unsigned)a.Hs, vy1 = (unsigned)(y0 + 1) < (unsigned)a.Hs;
                const float wnw = (vy0 && vx0) ? nw[e] : 0.0f, wne = (vy0 && vx1) ? ne[e] : 0.0f;
                const float wsw = (vy1 && vx0) ? sw[e] : 0.0f, wse = (vy1 && vx1) ? se[e] : 0.0f;
                // byte offset of tap (y0, x0); |y0 * Ws + x0| < 2^24 (checked by the launcher), the shift may wrap for
                // negative corners: then the offset is out of the descriptor's range and the load returns 0
                const unsigned o0 = ((unsigned)__mul24(y0, a.Ws) + (unsigned)x0) << SH;
                const unsigned oa = o0 + (unsigned)(sub * 32), ob = oa + (unsigned)row_bytes;
                const f32x4 q0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa, 0, 0));
                const f32x4 q1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa + 16, 0, 0));
                const f32x4 q2 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa + (4 * C), 0, 0));
                const f32x4 q3 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa + (4 * C + 16), 0, 0));
                const f32x4 q4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob, 0, 0));
                const f32x4 q5 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob + 16, 0, 0));
                const f32x4 q6 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob + (4 * C), 0, 0));
                const f32x4 q7 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob + (4 * C + 16), 0, 0));
                float part[GPL];
                MV_CORRELATE_SLICE(part, wnw, wne, wsw, wse, q0, q1, q2, q3, q4, q5, q6, q7, R0, R1)
#pragma unroll
                for (int k = 0; k < GPL; ++k) cg[d][k] = mv::div_rn(part[k], (float)CG);   // .mean(2)
                MV_GROUP_SCORE(sc, cg[d], lane - sub)                                      // .sum(1)
                score[d] = a.fuse_d ? mv::div_rn(sc, temp) : sc;
            }
        }
        // softmax over depth (depth order, like the other launch forms): in registers, plus an in-wave all-gather over the
        // QL lanes that share the pixel when DPL < D
        float mx = score[0];
#pragma unroll
        for (int d = 1; d < DPL; ++d) mx = fmaxf(mx, score[d]);
        if (QL > 1) {
            const float own = mx;
#pragma unroll
            for (int j = 0; j < QL; ++j) mx = fmaxf(mx, __shfl(own, (j * PPW + pl) * LPP + sub));
        }
        float e[DPL], den = 0.0f;
#pragma unroll
        for (int d = 0; d < DPL; ++d) e[d] = expf(mv::sub_rn(score[d], mx));
#pragma unroll
        for (int j = 0; j < QL; ++j)
#pragma unroll
            for (int d = 0; d < DPL; ++d)
                den = mv::add_rn(den, QL == 1 ? e[d] : __shfl(e[d], (j * PPW + pl) * LPP + sub));
        const mv::Recip rden = mv::make_recip(den);
        const float wmax = mv::div_rn(1.0f, rden);   // attn_fuse_d = False: max_d softmax = exp(0) / sum
#pragma unroll
        for (int d = 0; d < DPL; ++d) {
            const float wgt = a.fuse_d ? mv::div_rn(mv::div_rn(e[d], rden), sqrt_c) : wmax;
            wsum[d] = mv::add_rn(wsum[d], wgt);
#pragma unroll
            for (int k = 0; k < GPL; ++k) acc[d][k] = mv::add_rn(acc[d][k], mv::mul_rn(wgt, cg[d][k]));
        }
    }

    if (valid) {
#pragma unroll
        for (int d = 0; d < DPL; ++d) {
            const long o = (((long)b * D + qg * DPL + d) * hw + p);
            float* op = a.out + o * G + sub * GPL;
            const mv::Recip rw = mv::make_recip(wsum[d]);
            if (GPL == 4) {
                st4(op, (f32x4){mv::div_rn(acc[d][0], rw), mv::div_rn(acc[d][GPL > 1 ? 1 : 0], rw),
                                mv::div_rn(acc[d][GPL > 2 ? 2 : 0], rw), mv::div_rn(acc[d][GPL > 3 ? 3 : 0], rw)});
            } else {
#pragma unroll
                for (int k = 0; k < GPL; ++k) op[k] = mv::div_rn(acc[d][k], rw);
            }
            if (a.wsum_out && sub == 0) a.wsum_out[o] = wsum[d];
        }
    }
}

// launch shape of the pixel-major kernel: hypotheses per lane (0 = all D) and the occupancy target handed to the
// register allocator; MVSTER_PIX_DPL / MVSTER_PIX_WPE override the defaults for experiments
static const bool g_pix = MV_PROBE_ENV("MVSTER_PIX") != nullptr;   // experiment switch: pixel-major kernel at the fine stages
[[maybe_unused]] static const int g_pix_dpl = MV_PROBE_ENV("MVSTER_PIX_DPL") ? atoi(MV_PROBE_ENV("MVSTER_PIX_DPL")) : 2;
[[maybe_unused]] static const int g_pix_wpe = MV_PROBE_ENV("MVSTER_PIX_WPE") ? atoi(MV_PROBE_ENV("MVSTER_PIX_WPE")) : 4;

template <int C, int G, int D, int DPL, int WPE>
int launch_fwd_pix_cfg(const WarpAggArgs& a, hipStream_t stream) {
    constexpr int PPW = 64 / ((C / 8) * (D / DPL));
    dim3 grid((a.h * a.w + PPW - 1) / PPW, a.B);
    MV_NOTE_KERNEL("warp_agg_fwd_pix_kernel<%d, %d, %d, %d, %d>", C, G, D, DPL, WPE);
    hipLaunchKernelGGL((warp_agg_fwd_pix_kernel<C, G, D, DPL, WPE>), grid, dim3(64), 0, stream, a);
    return mv_check_launch();
}

template <int C, int G, int D>
int launch_fwd_pix(const WarpAggArgs& a, hipStream_t stream) {
    // 24-bit multiply-add on texel indices, 32-bit byte offsets inside one (view, batch) map
    if ((long)a.Hs * a.Ws >= (1L << 23) || (long)a.Hs * a.Ws * C * 4 >= (1L << 31)) return MVSTER_ERR_SHAPE;
    if (g_pix_dpl == 2 || (C / 8) * (D / 2) > 64) {
        if constexpr ((C / 8) * (D / 2) <= 64) {
            if (g_pix_wpe >= 6) return launch_fwd_pix_cfg<C, G, D, 2, 6>(a, stream);
            if (g_pix_wpe == 5) return launch_fwd_pix_cfg<C, G, D, 2, 5>(a, stream);
            return launch_fwd_pix_cfg<C, G, D, 2, 4>(a, stream);
        }
    }
    if (g_pix_wpe >= 5) return launch_fwd_pix_cfg<C, G, D, D, 5>(a, stream);
    return launch_fwd_pix_cfg<C, G, D, D, 4>(a, stream);
}

template <int C, int G>
int dispatch_fwd_pix(const WarpAggArgs& a, hipStream_t stream) {
    if (a.D == 4) return launch_fwd_pix<C, G, 4>(a, stream);
    if (a.D == 8) return launch_fwd_pix<C, G, 8>(a, stream);
    return MVSTER_ERR_UNSUPPORTED;
}


// ------------------------------------------------------------------------------------------
// LDS-staged source windows (variant 5; C in {8, 16}: the two fine stages, where the time is).
// The wave-local kernel gathers every tap through the texture path: 4 taps x 32 bytes per (pixel, d, view), 671 MB
// through L1 per stage-4 launch against 80 MB of HBM traffic, texture-address unit 55 % busy, and inside the forward
// (features not cache-resident) it waits on many small dependent misses: 48 us against 30 us warm.  Here a workgroup
// owns a TW x TH tile of reference pixels and walks it in NP passes with the wave kernel's lane mapping; per view it
//   A. projects all its (pixel, d) pairs and reduces the bounding box of the taps that carry weight (wave butterfly +
//      four LDS atomics),
//   B. stages that source window once -- whole texel rows are contiguous in channels-last memory, so this is a handful
//      of fully coalesced 16-byte loads per thread -- into LDS, one plane per 16-byte channel quad (conflict-free reads),
//   C. serves the taps with ds_read_b128.  A lane whose weighted taps do not fit the window (capacity WCAP texels:
//      geometrically incoherent hypotheses) takes the buffer-load path of the wave kernel instead, lane by lane.
// Arithmetic, lane mapping and summation order are the wave kernel's: bit-identical output (a zero-weight tap may read
// another in-window texel: 0 * finite = 0 either way).  Pays off when neighbouring pixels carry similar depths (trained
// networks, stage 1 by construction); on unrelated winner-take-all depths most lanes fall back and the bounding-box
// pass is pure overhead -- the plan keeps the wave kernel there.
// ------------------------------------------------------------------------------------------
#ifndef MV_TILE_WAVES
#define MV_TILE_WAVES 3      // (measured: 2 -> 66.6 us, 3 -> 57.6 us, 4 -> 77.5 us at stage 4, smooth depths; the wave kernel: 32.3 us)
#endif
template <int C, int G, int D, int TW, int TH>
__global__ void __launch_bounds__(256, MV_TILE_WAVES) warp_agg_fwd_tile_kernel(WarpAggArgs a, int tiles_x, int tiles_y) {
    constexpr int LPP = C / 8, CG = C / G, GPL = 8 / CG, PPW = 64 / (LPP * D);
    constexpr int NP = (TW * TH) / (4 * PPW);                     // passes over the tile
    constexpr int NQ = C / 4;                                     // 16-byte quads per texel = LDS planes
    constexpr int WCAP = 24 * 1024 / (C * 4);                     // window capacity in texels (24 KB)
    static_assert(C % 8 == 0 && CG <= 8 && 8 % CG == 0 && PPW * LPP * D == 64 && NP * 4 * PPW == TW * TH, "tile split");
    __shared__ f32x4 win[NQ * WCAP];
    __shared__ int box[4];                                        // min x, min y, max x, max y of the weighted taps

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LPP, pl = (lane / LPP) % PPW, d = lane / (LPP * PPW);
    const int b = blockIdx.y;
    const int hw = a.h * a.w;
    const unsigned tile = xcd_remap(blockIdx.x, gridDim.x);
    const int ty0 = (int)(tile / (unsigned)tiles_x) * TH, tx0 = (int)(tile % (unsigned)tiles_x) * TW;
    const mv::GridNorm gn = mv::make_grid_norm(a.Hs, a.Ws);
    const mv::Recip temp = mv::make_recip(a.attn_temp), sqrt_c = mv::make_recip(a.sqrt_c);
    constexpr int SH = C == 8 ? 5 : 6;                            // log2(bytes per texel)
    const float xhi = (float)(a.Ws + 4), yhi = (float)(a.Hs + 4);
    const unsigned src_bytes = (unsigned)a.Hs * (unsigned)a.Ws * (unsigned)(C * 4);
    const int row_bytes = a.Ws << SH;

    // per pass: pixel, reference features, hypothesis
    int pix[NP];
    bool valid[NP];
    float depth[NP];
    f32x4 R0[NP], R1[NP];
    float acc[NP][GPL], wsum[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int q = (k * 4 + wave) * PPW + pl;                  // tile-local pixel index, row-major
        const int y = ty0 + q / TW, x = tx0 + q % TW;
        valid[k] = y < a.h && x < a.w;
        pix[k] = valid[k] ? y * a.w + x : hw - 1;                 // clamped: every lane takes part in the shuffles
        depth[k] = a.hypo[((long)b * D + d) * hw + pix[k]];
        const float* rp = a.ref + (long)b * a.ref_bs + (long)pix[k] * C + sub * 8;
        R0[k] = ld4(rp);
        R1[k] = ld4(rp + 4);
#pragma unroll
        for (int g = 0; g < GPL; ++g) acc[k][g] = 0.0f;
        wsum[k] = 1e-8f;
    }

    for (int v = 0; v < a.NV; ++v) {
        MV_LOAD_RT(m, a, b, v)
        if (threadIdx.x == 0) { box[0] = 1 << 30; box[1] = 1 << 30; box[2] = -1; box[3] = -1; }
        // ---- A: taps of every pass, bounding box of the ones that carry weight
        mv::Taps t[NP];
        int bx0 = 1 << 30, by0 = 1 << 30, bx1 = -1, by1 = -1;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int y = pix[k] / a.w, x = pix[k] - y * a.w;
            float sx, sy;
            mv::project(m, (float)x, (float)y, depth[k], gn, sx, sy);
            const float cx = __builtin_amdgcn_fmed3f(sx, -4.0f, xhi), cy = __builtin_amdgcn_fmed3f(sy, -4.0f, yhi);
            const float fx = floorf(cx), fy = floorf(cy);
            t[k].x0 = (int)fx;
            t[k].y0 = (int)fy;
            const float wx1 = mv::sub_rn(cx, fx), wy1 = mv::sub_rn(cy, fy);
            const float wx0 = mv::sub_rn(1.0f, wx1), wy0 = mv::sub_rn(1.0f, wy1);
            const bool vx0 = (unsigned)t[k].x0 < (unsigned)a.Ws, vx1 = (unsigned)(t[k].x0 + 1) < (unsigned)a.Ws;
            const bool vy0 = (unsigned)t[k].y0 < (unsigned)a.Hs, vy1 = (unsigned)(t[k].y0 + 1) < (unsigned)a.Hs;
            t[k].nw = (vy0 && vx0) ? mv::mul_rn(wy0, wx0) : 0.0f;
            t[k].ne = (vy0 && vx1) ? mv::mul_rn(wy0, wx1) : 0.0f;
            t[k].sw = (vy1 && vx0) ? mv::mul_rn(wy1, wx0) : 0.0f;
            t[k].se = (vy1 && vx1) ? mv::mul_rn(wy1, wx1) : 0.0f;
            if (valid[k] && (vx0 || vx1) && (vy0 || vy1)) {       // some tap lies inside the map
                bx0 = min(bx0, max(t[k].x0, 0));
                by0 = min(by0, max(t[k].y0, 0));
                bx1 = max(bx1, min(t[k].x0 + 1, a.Ws - 1));
                by1 = max(by1, min(t[k].y0 + 1, a.Hs - 1));
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            bx0 = min(bx0, __shfl_xor(bx0, off));
            by0 = min(by0, __shfl_xor(by0, off));
            bx1 = max(bx1, __shfl_xor(bx1, off));
            by1 = max(by1, __shfl_xor(by1, off));
        }
        __syncthreads();                                          // box initialised; previous view's window no longer read
        if (lane == 0 && bx1 >= 0) {
            atomicMin(&box[0], bx0);
            atomicMin(&box[1], by0);
            atomicMax(&box[2], bx1);
            atomicMax(&box[3], by1);
        }
        __syncthreads();
        // window = the box, cut to the capacity (anchored at its top-left corner); an empty box -> texel (0, 0)
        int wx0 = box[0], wy0 = box[1], wx = box[2] - wx0 + 1, wy = box[3] - wy0 + 1;
        if (box[2] < 0) { wx0 = 0; wy0 = 0; wx = 1; wy = 1; }
        wx = min(wx, WCAP);
        wy = min(wy, WCAP / wx);
        // ---- B: stage the window: thread -> (texel, quad), a window row is one contiguous run of wx * C * 4 bytes
        const float* sp = a.src + (long)v * a.src_vs + (long)b * a.src_bs;
        const int nst = wy * wx * NQ;
        for (int i = threadIdx.x; i < nst; i += 256) {
            const int qd = i % NQ, tx = (i / NQ) % wx, tyy = i / (NQ * wx);
            win[qd * WCAP + tyy * wx + tx] = ld4(sp + ((long)(wy0 + tyy) * a.Ws + (wx0 + tx)) * C + qd * 4);
        }
        __syncthreads();
        // ---- C: the wave kernel's arithmetic, taps from LDS where the lane's weighted taps lie inside the window
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(sp), (short)0, (int)src_bytes, 0x00020000);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const mv::Taps& tk = t[k];
            // in-window test on the clamped extent of the taps (taps outside the map carry no weight)
            const int ex0 = max(tk.x0, 0), ey0 = max(tk.y0, 0), ex1 = min(tk.x0 + 1, a.Ws - 1), ey1 = min(tk.y0 + 1, a.Hs - 1);
            const bool weighted = (ex0 <= ex1) && (ey0 <= ey1);
            const bool inwin = !weighted || (ex0 >= wx0 && ey0 >= wy0 && ex1 < wx0 + wx && ey1 < wy0 + wy);
            f32x4 q0, q1, q2, q3, q4, q5, q6, q7;
            if (inwin) {
                // (a tap outside the window has zero weight: it may read any staged texel)
                const int rx0 = min(max(tk.x0 - wx0, 0), wx - 1), rx1 = min(max(tk.x0 + 1 - wx0, 0), wx - 1);
                const int ry0 = min(max(tk.y0 - wy0, 0), wy - 1), ry1 = min(max(tk.y0 + 1 - wy0, 0), wy - 1);
                const f32x4* w0 = win + (sub * 2) * WCAP;
                const f32x4* w1 = w0 + WCAP;
                q0 = w0[ry0 * wx + rx0]; q1 = w1[ry0 * wx + rx0];
                q2 = w0[ry0 * wx + rx1]; q3 = w1[ry0 * wx + rx1];
                q4 = w0[ry1 * wx + rx0]; q5 = w1[ry1 * wx + rx0];
                q6 = w0[ry1 * wx + rx1]; q7 = w1[ry1 * wx + rx1];
            } else {
                const unsigned oa = (((unsigned)__mul24(tk.y0, a.Ws) + (unsigned)tk.x0) << SH) + (unsigned)(sub * 32);
                const unsigned ob = oa + (unsigned)row_bytes;
                q0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa, 0, 0));
                q1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa + 16, 0, 0));
                q2 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa + (4 * C), 0, 0));
                q3 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa + (4 * C + 16), 0, 0));
                q4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob, 0, 0));
                q5 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob + 16, 0, 0));
                q6 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob + (4 * C), 0, 0));
                q7 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob + (4 * C + 16), 0, 0));
            }
            float part[GPL];
            MV_CORRELATE_SLICE(part, tk.nw, tk.ne, tk.sw, tk.se, q0, q1, q2, q3, q4, q5, q6, q7, R0[k], R1[k])
            float cg[GPL];
#pragma unroll
            for (int g = 0; g < GPL; ++g) cg[g] = mv::div_rn(part[g], (float)CG);   // .mean(2)
            MV_GROUP_SCORE(score, cg, lane - sub)                                   // .sum(1)
            if (a.fuse_d) score = mv::div_rn(score, temp);
            float mx = score;
#pragma unroll
            for (int j = 0; j < D; ++j) mx = fmaxf(mx, __shfl(score, (j * PPW + pl) * LPP + sub));
            const float e = expf(mv::sub_rn(score, mx));
            float den = 0.0f;
#pragma unroll
            for (int j = 0; j < D; ++j) den = mv::add_rn(den, __shfl(e, (j * PPW + pl) * LPP + sub));
            const mv::Recip rden = mv::make_recip(den);
            float wgt;
            if (a.fuse_d)
                wgt = mv::div_rn(mv::div_rn(e, rden), sqrt_c);
            else
                wgt = mv::div_rn(1.0f, rden);
            wsum[k] = mv::add_rn(wsum[k], wgt);
#pragma unroll
            for (int g = 0; g < GPL; ++g) acc[k][g] = mv::add_rn(acc[k][g], mv::mul_rn(wgt, cg[g]));
        }
    }

#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (!valid[k]) continue;
        const long o = (((long)b * D + d) * hw + pix[k]);
        float* op = a.out + o * G + sub * GPL;
        const mv::Recip rw = mv::make_recip(wsum[k]);
        if (GPL == 4) {
            st4(op, (f32x4){mv::div_rn(acc[k][0], rw), mv::div_rn(acc[k][GPL > 1 ? 1 : 0], rw),
                            mv::div_rn(acc[k][GPL > 2 ? 2 : 0], rw), mv::div_rn(acc[k][GPL > 3 ? 3 : 0], rw)});
        } else {
#pragma unroll
            for (int g = 0; g < GPL; ++g) op[g] = mv::div_rn(acc[k][g], rw);
        }
        if (a.wsum_out && sub == 0) a.wsum_out[o] = wsum[k];
    }
}

template <int C, int G, int D>
int launch_fwd_tile(const WarpAggArgs& a, hipStream_t stream) {
    constexpr int TW = 32, TH = C == 8 ? 8 : 4;
    if ((long)a.Hs * a.Ws >= (1L << 23) || (long)a.Hs * a.Ws * C * 4 >= (1L << 31)) return MVSTER_ERR_SHAPE;
    const int tiles_x = (a.w + TW - 1) / TW, tiles_y = (a.h + TH - 1) / TH;
    MV_NOTE_KERNEL("warp_agg_fwd_tile_kernel<%d, %d, %d, %d, %d>", C, G, D, TW, TH);
    hipLaunchKernelGGL((warp_agg_fwd_tile_kernel<C, G, D, TW, TH>), dim3(tiles_x * tiles_y, a.B), dim3(256), 0, stream, a, tiles_x,
                       tiles_y);
    return mv_check_launch();
}

template <int C, int G>
int dispatch_fwd_tile(const WarpAggArgs& a, hipStream_t stream) {
    if (a.D == 4) return launch_fwd_tile<C, G, 4>(a, stream);
    if (a.D == 8) return launch_fwd_tile<C, G, 8>(a, stream);
    return MVSTER_ERR_UNSUPPORTED;
}

