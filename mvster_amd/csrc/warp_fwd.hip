// Fused homography warp + group correlation + epipolar attention aggregation (forward).
//
// Replaces, for one cascade stage and ALL source views in one launch, the reference's
//   homo_warping            models/mvs4net_utils.py:13-59
//   group / squared corr    models/mvs4net_utils.py:1037-1042
//   attention aggregation   models/mvs4net_utils.py:1048-1060
// without ever materialising the [B,C,D,h,w] warped volumes.
//
// Data layout (HBM):
//   ref feature  [B, h, w, C]        channels-last fp32
//   src features [NV][B, Hs, Ws, C]  channels-last fp32 (view / batch strides are arguments)
//   rt           [B, NV, 12]         relative projection rot(9) + trans(3)
//   hypo         [B, D, h, w]        depth hypotheses (API layout of `hypo_depth`)
//   out          [B, D, h, w, G]     aggregated correlation, channels-last (feeds conv0 of reg2d)
//
// Mapping: a workgroup is 64 consecutive reference pixels x D hypotheses; wave d handles
// hypothesis d for the 64 pixels (lane = pixel, so a wave's four bilinear taps fall on a
// short, contiguous run of source texels: one channels-last tap is C*4 bytes per lane and
// neighbouring lanes hit neighbouring texels).  The softmax over the depth axis is the
// only cross-wave step: each wave publishes its 64 scores in LDS (double-buffered by
// view parity, one barrier per view) and every lane reduces the D scores of its pixel.
//
// Roofline: HBM-bound.  Algorithmic bytes per launch = 4*[(NV+1)*C*hw + D*hw + G*D*hw]*B.
#include "warp_common.hpp"

namespace {

// PX pixels x D hypotheses per workgroup: 64 pixels for D <= 16 (the shipped cascade's fallback form), 32 / 16 pixels for up
// to 32 / 64 hypotheses per stage (free --ndepths of the reference; evaluation only, the backward keeps D <= 16).
template <int C, int G, bool GROUP, int DMAX, int PX = 64, bool IDX = false>
__global__ void __launch_bounds__(PX * DMAX) warp_agg_fwd_kernel(WarpAggArgs a) {
    static_assert(C % 8 == 0, "channels-last taps are read as float4 pairs");
    static_assert(GROUP ? (C % G == 0) : (C == G), "group layout");
    constexpr int CG = C / G;                // channels per correlation group
    constexpr int CB = CG > 8 ? CG : 8;      // channels gathered per loop iteration
    constexpr int GB = CB / CG;              // groups completed per iteration
    static_assert(C % CB == 0, "channel block");
    // per-view correlations live in LDS (G floats per thread) so that the gather loop can
    // stay rolled: ~45 VGPRs for every C instead of 4*C registers of in-flight taps
    __shared__ float sc[2][DMAX][PX];
    __shared__ float corL[G][DMAX * PX];

    const int tx = threadIdx.x;
    const int d = threadIdx.y;
    const int tid = d * PX + tx;
    const int b = blockIdx.y;
    const int hw = a.h * a.w;
    const int p = xcd_remap(blockIdx.x, gridDim.x) * PX + tx;
    const bool valid = p < hw;
    const int pc = valid ? p : hw - 1;  // clamped: every lane takes part in the barriers
    const int y = pc / a.w;
    const int x = pc - y * a.w;
    const float depth = a.hypo[((long)b * a.D + d) * hw + pc];
    const float* rp = ref_base<IDX>(a, b) + (long)pc * C;

    float acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0.0f;
    float wsum = 1e-8f;

    const int nv = source_count(a, b);
    for (int v = 0; v < nv; ++v) {
        MV_LOAD_RT(m, a, b, v)
        float sx, sy;
        mv::project(m, (float)x, (float)y, depth, a.Hs, a.Ws, sx, sy);
        mv::Taps t = mv::make_taps(sx, sy, a.Hs, a.Ws);
        const mv::TapsClamped tc = mv::clamp_taps(t, a.Hs, a.Ws);
        const float* sp = src_base<IDX>(a, b, v);
        const float* p00 = sp + ((long)tc.ya * a.Ws + tc.xa) * C;
        const float* p01 = sp + ((long)tc.ya * a.Ws + tc.xb) * C;
        const float* p10 = sp + ((long)tc.yb * a.Ws + tc.xa) * C;
        const float* p11 = sp + ((long)tc.yb * a.Ws + tc.xb) * C;

        float score = 0.0f;
#pragma unroll 2
        for (int cb = 0; cb < C / CB; ++cb) {
            const int cbase = cb * CB;
            float part[GB];
#pragma unroll
            for (int c0 = 0; c0 < CB; c0 += 4) {
                const f32x4 R = ld4(rp + cbase + c0);
                const f32x4 A = ld4(p00 + cbase + c0);
                const f32x4 Bq = ld4(p01 + cbase + c0);
                const f32x4 Cq = ld4(p10 + cbase + c0);
                const f32x4 Dq = ld4(p11 + cbase + c0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + j;  // channel within the block
                    const float wv = mv::blend(t, A[j], Bq[j], Cq[j], Dq[j]);
                    if (GROUP) {
                        const float pr = mv::mul_rn(wv, R[j]);
                        part[c / CG] = (c % CG == 0) ? pr : mv::add_rn(part[c / CG], pr);
                    } else {
                        const float df = mv::sub_rn(R[j], wv);
                        part[c] = mv::mul_rn(df, df);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                const float cg = GROUP ? mv::div_rn(part[k], (float)CG) : part[k];  // .mean(2)
                corL[cb * GB + k][tid] = cg;
                score = (cb == 0 && k == 0) ? cg : mv::add_rn(score, cg);           // .sum(1)
            }
        }
        MV_DEPTH_SOFTMAX(wgt, a, sc[v & 1], d, tx, true, score)
        wsum = mv::add_rn(wsum, wgt);
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = mv::add_rn(acc[g], mv::mul_rn(wgt, corL[g][tid]));
    }

    if (valid) {
        const long o = (((long)b * a.D + d) * hw + p);
        float* op = a.out + o * G;
#pragma unroll
        for (int g = 0; g < G; g += 4) {
            f32x4 r;
            r[0] = mv::div_rn(acc[g], wsum);
            r[1] = mv::div_rn(acc[g + 1], wsum);
            r[2] = mv::div_rn(acc[g + 2], wsum);
            r[3] = mv::div_rn(acc[g + 3], wsum);
            st4(op + g, r);
        }
        if (a.wsum_out) a.wsum_out[o] = wsum;
    }
}

// ------------------------------------------------------------------------------------------
// Lane-split variant for wide feature maps (C >= 16, group correlation).  At the coarse stages the
// map is small (5120 pixels at stage 1) but C is 64: one thread per (pixel, d) leaves most CUs idle
// and makes each thread walk 8 dependent gather rounds.  Here LPP = C/8 adjacent lanes share one
// (pixel, d): lane `sub` gathers channels 8*sub..8*sub+7 (= whole correlation groups, since C/G <= 8),
// so a tap of one pixel is LPP*32 contiguous bytes across neighbouring lanes, the chip sees LPP x more
// waves, and there is a single gather round per view.  The G correlations are all-gathered with wave
// shuffles and summed in group order, so scores are bit-identical to the one-thread form.
// ------------------------------------------------------------------------------------------
template <int C, int G, int DMAX, bool IDX = false>
__global__ void __launch_bounds__(64 * DMAX) warp_agg_fwd_lanes_kernel(WarpAggArgs a) {
    constexpr int LPP = C / 8;           // lanes per (pixel, d)
    constexpr int CG = C / G;            // channels per group
    constexpr int GPL = 8 / CG;          // whole groups per lane
    constexpr int PPB = 64 / LPP;        // pixels per workgroup
    static_assert(C % 8 == 0 && CG <= 8 && 8 % CG == 0 && LPP >= 1 && LPP <= 16, "lane split");
    __shared__ float sc[2][DMAX][PPB];

    const int tx = threadIdx.x;
    const int sub = tx % LPP, pl = tx / LPP;
    const int d = threadIdx.y;
    const int b = blockIdx.y;
    const int hw = a.h * a.w;
    const int p = xcd_remap(blockIdx.x, gridDim.x) * PPB + pl;
    const bool valid = p < hw;
    const int pc = valid ? p : hw - 1;
    const int y = pc / a.w;
    const int x = pc - y * a.w;
    const float depth = a.hypo[((long)b * a.D + d) * hw + pc];
    const float* rp = ref_base<IDX>(a, b) + (long)pc * C + sub * 8;
    const f32x4 R0 = ld4(rp), R1 = ld4(rp + 4);

    float acc[GPL];
#pragma unroll
    for (int k = 0; k < GPL; ++k) acc[k] = 0.0f;
    float wsum = 1e-8f;

    const int nv = source_count(a, b);
    for (int v = 0; v < nv; ++v) {
        MV_LOAD_RT(m, a, b, v)
        float sx, sy;
        mv::project(m, (float)x, (float)y, depth, a.Hs, a.Ws, sx, sy);
        mv::Taps t = mv::make_taps(sx, sy, a.Hs, a.Ws);
        const mv::TapsClamped tc = mv::clamp_taps(t, a.Hs, a.Ws);
        const float* sp = src_base<IDX>(a, b, v) + sub * 8;
        const float* p00 = sp + ((long)tc.ya * a.Ws + tc.xa) * C;
        const float* p01 = sp + ((long)tc.ya * a.Ws + tc.xb) * C;
        const float* p10 = sp + ((long)tc.yb * a.Ws + tc.xa) * C;
        const float* p11 = sp + ((long)tc.yb * a.Ws + tc.xb) * C;
        const f32x4 A0 = ld4(p00), A1 = ld4(p00 + 4), B0 = ld4(p01), B1 = ld4(p01 + 4);
        const f32x4 C0 = ld4(p10), C1 = ld4(p10 + 4), D0 = ld4(p11), D1 = ld4(p11 + 4);

        float part[GPL];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float wv = c < 4 ? mv::blend(t, A0[c & 3], B0[c & 3], C0[c & 3], D0[c & 3])
                                   : mv::blend(t, A1[c & 3], B1[c & 3], C1[c & 3], D1[c & 3]);
            const float pr = mv::mul_rn(wv, c < 4 ? R0[c & 3] : R1[c & 3]);
            part[c / CG] = (c % CG == 0) ? pr : mv::add_rn(part[c / CG], pr);
        }
        float cg[GPL];
#pragma unroll
        for (int k = 0; k < GPL; ++k) cg[k] = mv::div_rn(part[k], (float)CG);

        MV_GROUP_SCORE(score, cg, tx - sub)
        MV_DEPTH_SOFTMAX(wgt, a, sc[v & 1], d, pl, sub == 0, score)
        wsum = mv::add_rn(wsum, wgt);
#pragma unroll
        for (int k = 0; k < GPL; ++k) acc[k] = mv::add_rn(acc[k], mv::mul_rn(wgt, cg[k]));
    }

    if (valid) {
        const long o = (((long)b * a.D + d) * hw + p);
        float* op = a.out + o * G + sub * GPL;
#pragma unroll
        for (int k = 0; k < GPL; ++k) op[k] = mv::div_rn(acc[k], wsum);
        if (a.wsum_out && sub == 0) a.wsum_out[o] = wsum;
    }
}

// ------------------------------------------------------------------------------------------
// Wave-local variant (the default whenever D and C/8 are powers of two with D*C/8 <= 64, i.e. all
// four stages of the shipped cascade).  One wavefront owns PPW = 64/(D*C/8) pixels and ALL their
// depth hypotheses: lane = (d*PPW + pixel)*LPP + sub.  The softmax over depth is an in-wave
// all-gather (ds_bpermute), so there is no LDS, no barrier and no workgroup-level coupling: waves
// run free and the only thing a wave ever waits for is its own gather (8 independent 16-byte loads
// per lane and view).
// The kernel is VALU-bound, not HBM-bound (~200 instructions per (pixel, d, view) against 256 bytes
// gathered), hence the shared-reciprocal divisions, the single expf per lane and the packed blend.
// Arithmetic and summation order are those of the one-thread form: results are bit-identical to it.
// ------------------------------------------------------------------------------------------
// SCHED: 0 = the hypotheses are read from a.hypo; 1 = schedule_inverse_range of the previous stage's inverse bounds and
// 2 = init_inverse_range of depth_values, both computed per lane with the scheduler kernels' own per-hypothesis functions
// (mvster_math.h: bit-identical) and written to a.hypo_out by lane sub 0 -- one launch and one dependency edge less per
// stage (schedule_inverse_kernel ran alone for ~5 us three times per forward).
template <int C, int G, int D, int SCHED = 0, bool IDX = false>
__global__ void __launch_bounds__(256) warp_agg_fwd_wave_kernel(WarpAggArgs a) {
    constexpr int LPP = C / 8;           // lanes per (pixel, d)
    constexpr int CG = C / G;            // channels per group
    constexpr int GPL = 8 / CG;          // whole groups per lane
    constexpr int PPW = 64 / (LPP * D);  // pixels per wave
    static_assert(C % 8 == 0 && CG <= 8 && 8 % CG == 0 && PPW >= 1 && PPW * LPP * D == 64, "wave split");

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LPP, pl = (lane / LPP) % PPW, d = lane / (LPP * PPW);
    const int b = blockIdx.y;
    const int hw = a.h * a.w;
    const int p = (xcd_remap(blockIdx.x, gridDim.x) * 4 + wave) * PPW + pl;
    const bool valid = p < hw;
    const int pc = valid ? p : hw - 1;   // clamped: every lane takes part in the shuffles
    const int y = pc / a.w;
    const int x = pc - y * a.w;
    float depth;
    if constexpr (SCHED == 0) {
        depth = a.hypo[((long)b * D + d) * hw + pc];
    } else {
        if constexpr (SCHED == 1) {
            const int hi = a.h / 2, wi = a.w / 2;
            const mv::InvCorners cn = mv::schedule_inverse_corners(a.inv_min + (long)b * hi * wi, a.inv_max + (long)b * hi * wi,
                                                                   y, x, a.h, a.w, hi, wi);
            depth = mv::schedule_inverse_one(cn, D, d);
        } else {
            depth = mv::init_inverse_one(a.dvals[(long)b * a.ndv], a.dvals[(long)b * a.ndv + a.ndv - 1], D, d);
        }
        if (valid && sub == 0) a.hypo_out[((long)b * D + d) * hw + pc] = depth;
    }
    const float* rp = ref_base<IDX>(a, b) + (long)pc * C + sub * 8;
    const f32x4 R0 = ld4(rp), R1 = ld4(rp + 4);
    // per-launch divisors with their reciprocals (mvster_math.h: same bits as '/', 5 instead of 11 VALU ops)
    const mv::GridNorm gn = mv::make_grid_norm(a.Hs, a.Ws);
    const mv::Recip temp = mv::make_recip(a.attn_temp), sqrt_c = mv::make_recip(a.sqrt_c);
    constexpr int SH = C == 8 ? 5 : (C == 16 ? 6 : (C == 32 ? 7 : 8));   // log2(bytes per texel)
    const float xhi = (float)(a.Ws + 4), yhi = (float)(a.Hs + 4);
    const unsigned src_bytes = (unsigned)a.Hs * (unsigned)a.Ws * (unsigned)(C * 4);
    const int row_bytes = a.Ws << SH;

    float acc[GPL];
#pragma unroll
    for (int k = 0; k < GPL; ++k) acc[k] = 0.0f;
    float wsum = 1e-8f;

    const int nv = source_count(a, b);
    for (int v = 0; v < nv; ++v) {
        MV_LOAD_RT(m, a, b, v)
        float sx, sy;
        mv::project(m, (float)x, (float)y, depth, gn, sx, sy);
        // make_taps() with a single clamp instruction per coordinate (v_med3_f32; a NaN position ends up at -4)
        mv::Taps t;
        {
            const float cx = __builtin_amdgcn_fmed3f(sx, -4.0f, xhi), cy = __builtin_amdgcn_fmed3f(sy, -4.0f, yhi);
            const float fx = floorf(cx), fy = floorf(cy);
            t.x0 = (int)fx;
            t.y0 = (int)fy;
            const float wx1 = mv::sub_rn(cx, fx), wy1 = mv::sub_rn(cy, fy);
            const float wx0 = mv::sub_rn(1.0f, wx1), wy0 = mv::sub_rn(1.0f, wy1);
            const bool vx0 = (unsigned)t.x0 < (unsigned)a.Ws, vx1 = (unsigned)(t.x0 + 1) < (unsigned)a.Ws;
            const bool vy0 = (unsigned)t.y0 < (unsigned)a.Hs, vy1 = (unsigned)(t.y0 + 1) < (unsigned)a.Hs;
            t.nw = (vy0 && vx0) ? mv::mul_rn(wy0, wx0) : 0.0f;
            t.ne = (vy0 && vx1) ? mv::mul_rn(wy0, wx1) : 0.0f;
            t.sw = (vy1 && vx0) ? mv::mul_rn(wy1, wx0) : 0.0f;
            t.se = (vy1 && vx1) ? mv::mul_rn(wy1, wx1) : 0.0f;
        }
        // raw buffer loads: one 32-bit byte offset per tap row (24-bit multiply-add on the texel index), the other
        // addresses are immediate offsets; nothing is clamped -- a tap outside the map either falls outside the
        // descriptor (the hardware returns 0) or reads some other texel, and its weight is 0 in both cases
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(src_base<IDX>(a, b, v)), (short)0, (int)src_bytes, 0x00020000);
        const unsigned oa = (((unsigned)__mul24(t.y0, a.Ws) + (unsigned)t.x0) << SH) + (unsigned)(sub * 32);
        const unsigned ob = oa + (unsigned)row_bytes;
        const f32x4 q0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa, 0, 0));
        const f32x4 q1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa + 16, 0, 0));
        const f32x4 q2 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa + (4 * C), 0, 0));
        const f32x4 q3 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, oa + (4 * C + 16), 0, 0));
        const f32x4 q4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob, 0, 0));
        const f32x4 q5 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob + 16, 0, 0));
        const f32x4 q6 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob + (4 * C), 0, 0));
        const f32x4 q7 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ob + (4 * C + 16), 0, 0));
        // keep the eight loads together and ahead of their uses: left alone, the scheduler sinks each
        // load to its first use to save registers and the wave then eats eight memory latencies in a row
        __builtin_amdgcn_sched_barrier(0);

        // blend and correlate channel pairs (packed fp32 on the pairs the 16-byte loads deliver), then sum
        // each group in channel order
        float part[GPL];
        MV_CORRELATE_SLICE(part, t.nw, t.ne, t.sw, t.se, q0, q1, q2, q3, q4, q5, q6, q7, R0, R1)
        float cg[GPL];
#pragma unroll
        for (int k = 0; k < GPL; ++k) cg[k] = mv::div_rn(part[k], (float)CG);   // .mean(2)
        MV_GROUP_SCORE(score, cg, lane - sub)                                   // .sum(1)
        if (a.fuse_d) score = mv::div_rn(score, temp);
        // softmax over depth: the D scores of this pixel live in lanes (j*PPW + pl)*LPP + sub.  Each lane
        // exponentiates its own score once and the D terms are all-gathered and summed in depth order
        // (the other launch forms evaluate the same D expf calls in every thread).
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
            wgt = mv::div_rn(1.0f, rden);  // max_d softmax = exp(0) / sum
        wsum = mv::add_rn(wsum, wgt);
#pragma unroll
        for (int k = 0; k < GPL; ++k) acc[k] = mv::add_rn(acc[k], mv::mul_rn(wgt, cg[k]));
    }

    if (valid) {
        const long o = (((long)b * D + d) * hw + p);
        float* op = a.out + o * G + sub * GPL;
        const mv::Recip rw = mv::make_recip(wsum);
        if (GPL == 4) {
            st4(op, (f32x4){mv::div_rn(acc[0], rw), mv::div_rn(acc[GPL > 1 ? 1 : 0], rw),
                            mv::div_rn(acc[GPL > 2 ? 2 : 0], rw), mv::div_rn(acc[GPL > 3 ? 3 : 0], rw)});
        } else {
#pragma unroll
            for (int k = 0; k < GPL; ++k) op[k] = mv::div_rn(acc[k], rw);
        }
        if (a.wsum_out && sub == 0) a.wsum_out[o] = wsum;
    }
}

#ifdef MVSTER_PROBES   // pixel-major form (variant 4) and LDS-window form (variant 5): probe build only
#include "warp_fwd_probes.hpp"
#endif

template <int C, int G, int D>
int launch_fwd_wave(const WarpAggArgs& a, hipStream_t stream, int sched = 0) {
    constexpr int PPB = 4 * (64 / ((C / 8) * D));
    // 24-bit multiply-add on texel indices, 32-bit byte offsets inside one (view, batch) map
    if ((long)a.Hs * a.Ws >= (1L << 23) || (long)a.Hs * a.Ws * C * 4 >= (1L << 31)) return MVSTER_ERR_SHAPE;
    dim3 grid((a.h * a.w + PPB - 1) / PPB, a.B);
    if (sched == 1) {
        MV_NOTE_KERNEL("warp_agg_fwd_wave_kernel<%d, %d, %d, 1>", C, G, D);
        hipLaunchKernelGGL((warp_agg_fwd_wave_kernel<C, G, D, 1>), grid, dim3(256), 0, stream, a);
    } else if (sched == 2) {
        MV_NOTE_KERNEL("warp_agg_fwd_wave_kernel<%d, %d, %d, 2>", C, G, D);
        hipLaunchKernelGGL((warp_agg_fwd_wave_kernel<C, G, D, 2>), grid, dim3(256), 0, stream, a);
    } else if (a.views) {
        MV_NOTE_KERNEL("warp_agg_fwd_wave_kernel<%d, %d, %d, 0, true>", C, G, D);
        hipLaunchKernelGGL((warp_agg_fwd_wave_kernel<C, G, D, 0, true>), grid, dim3(256), 0, stream, a);
    } else {
        MV_NOTE_KERNEL("warp_agg_fwd_wave_kernel<%d, %d, %d>", C, G, D);
        hipLaunchKernelGGL((warp_agg_fwd_wave_kernel<C, G, D>), grid, dim3(256), 0, stream, a);
    }
    return mv_check_launch();
}

template <int C, int G>
int dispatch_fwd_wave(const WarpAggArgs& a, hipStream_t stream, int sched = 0) {
    if (a.D == 4) return launch_fwd_wave<C, G, 4>(a, stream, sched);
    if (a.D == 8) return launch_fwd_wave<C, G, 8>(a, stream, sched);
    return MVSTER_ERR_UNSUPPORTED;
}

template <int C, int G>
int launch_fwd_lanes(const WarpAggArgs& a, hipStream_t stream) {
    constexpr int PPB = 64 / (C / 8);
    if (a.D > 8) return MVSTER_ERR_UNSUPPORTED;
    dim3 block(64, a.D);
    dim3 grid((a.h * a.w + PPB - 1) / PPB, a.B);
    if (a.views) {
        if constexpr (kIndexedLanes<C, G>) {
            MV_NOTE_KERNEL("warp_agg_fwd_lanes_kernel<%d, %d, 8, true>", C, G);
            hipLaunchKernelGGL((warp_agg_fwd_lanes_kernel<C, G, 8, true>), grid, block, 0, stream, a);
        } else {
            return MVSTER_ERR_UNSUPPORTED;
        }
    } else {
        MV_NOTE_KERNEL("warp_agg_fwd_lanes_kernel<%d, %d, 8>", C, G);
        hipLaunchKernelGGL((warp_agg_fwd_lanes_kernel<C, G, 8>), grid, block, 0, stream, a);
    }
    return mv_check_launch();
}

// plain or indexed instantiation of the one-thread form (mvster_last_kernel reports the plain spelling for both)
template <int C, int G, bool GROUP, int DMAX, int PX>
void launch_fwd_form(const WarpAggArgs& a, dim3 grid, dim3 block, hipStream_t stream) {
    if constexpr (kIndexedOneThread<C>) {
        if (a.views) {
            hipLaunchKernelGGL((warp_agg_fwd_kernel<C, G, GROUP, DMAX, PX, true>), grid, block, 0, stream, a);
            return;
        }
    }
    hipLaunchKernelGGL((warp_agg_fwd_kernel<C, G, GROUP, DMAX, PX>), grid, block, 0, stream, a);
}

// maps views[b][k] of a level store -> out [1 + NV, B, map]: the view-major batch the plain entry reads (16 bytes per thread)
__global__ void __launch_bounds__(256) gather_views_kernel(const float* __restrict__ store, const int* __restrict__ views,
                                                          float* __restrict__ out, int B, int N, long map_quads) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= map_quads) return;
    const int k = blockIdx.y / B, b = blockIdx.y - k * B;            // out map k * B + b
    const long src = (long)views[b * N + k] * map_quads + q, dst = (long)blockIdx.y * map_quads + q;
    st4(out + dst * 4, ld4(store + src * 4));
}

template <int C, int G, bool GROUP>
int launch_fwd(const WarpAggArgs& a, hipStream_t stream) {
    dim3 block(64, a.D);
    dim3 grid((a.h * a.w + 63) / 64, a.B);
    if (a.views && !kIndexedOneThread<C>) return MVSTER_ERR_UNSUPPORTED;
    if (a.D <= 8) {
        MV_NOTE_KERNEL("warp_agg_fwd_kernel<%d, %d, %s, 8>", C, G, GROUP ? "true" : "false");
        launch_fwd_form<C, G, GROUP, 8, 64>(a, grid, block, stream);
    } else {
        // 1024-thread blocks; the per-thread correlations of the widest ungrouped case do not fit LDS
        if constexpr (G * kMaxD * 64 * 4 > 120 * 1024) return MVSTER_ERR_UNSUPPORTED;
        else if (a.D <= kMaxD) {
            MV_NOTE_KERNEL("warp_agg_fwd_kernel<%d, %d, %s, %d>", C, G, GROUP ? "true" : "false", kMaxD);
            launch_fwd_form<C, G, GROUP, kMaxD, 64>(a, grid, block, stream);
        } else if (a.D <= 32) {          // the same 1024 threads as 32 pixels x 32 hypotheses
            MV_NOTE_KERNEL("warp_agg_fwd_kernel<%d, %d, %s, 32, 32>", C, G, GROUP ? "true" : "false");
            launch_fwd_form<C, G, GROUP, 32, 32>(a, dim3((a.h * a.w + 31) / 32, a.B), dim3(32, a.D), stream);
        } else {                         // ... 16 pixels x 64 hypotheses
            MV_NOTE_KERNEL("warp_agg_fwd_kernel<%d, %d, %s, 64, 16>", C, G, GROUP ? "true" : "false");
            launch_fwd_form<C, G, GROUP, 64, 16>(a, dim3((a.h * a.w + 15) / 16, a.B), dim3(16, a.D), stream);
        }
    }
    return mv_check_launch();
}

}  // namespace

// mvster_warp_agg_fwd with the stage's hypothesis scheduling fused in (wave-local kernel only: group correlation, D in
// {4, 8}, C / 8 * D <= 64 -- every stage of the shipped cascade; MVSTER_ERR_UNSUPPORTED otherwise and the caller runs the
// scheduler launch + mvster_warp_agg_fwd).  mode 1: schedule_inverse_range of inv_min / inv_max [B, h/2, w/2]
// (models/mvs4net_utils.py:79-86); mode 2: init_inverse_range of depth_values [B, ndv] (:71-77).  hypo_out [B, D, h, w]
// receives the hypotheses (bit-identical to the scheduler kernels').
extern "C" int mvster_warp_agg_fwd_sched(const float* ref_feat, const float* src_feat, const float* rt, const float* inv_min,
                                         const float* inv_max, const float* depth_values, int ndv, float* hypo_out, float* out,
                                         float* wsum_out, int B, int NV, int C, int G, int D, int h, int w, int Hs, int Ws,
                                         long ref_batch_stride, long src_view_stride, long src_batch_stride, int attn_fuse_d,
                                         float attn_temp, int mode, void* stream) {
    if (!ref_feat || !src_feat || !rt || !hypo_out || !out) return MVSTER_ERR_NULL;
    if (mode == 1 ? (!inv_min || !inv_max) : (mode == 2 ? !depth_values : true)) return mode == 1 || mode == 2 ? MVSTER_ERR_NULL : MVSTER_ERR_SHAPE;
    if (B <= 0 || NV <= 0 || h <= 0 || w <= 0 || Hs <= 0 || Ws <= 0 || (mode == 1 && ((h | w) & 1)) || (mode == 2 && ndv < 2))
        return MVSTER_ERR_SHAPE;
    if (D != 4 && D != 8) return MVSTER_ERR_UNSUPPORTED;
    WarpAggArgs a = make_warp_args(ref_feat, src_feat, rt, nullptr, out, wsum_out, B, NV, C, D, h, w, Hs, Ws, ref_batch_stride,
                                   src_view_stride, src_batch_stride, attn_fuse_d, attn_temp);
    a.inv_min = inv_min; a.inv_max = inv_max; a.dvals = depth_values; a.hypo_out = hypo_out; a.ndv = ndv;
    hipStream_t s = (hipStream_t)stream;
    if (C == 8 && G == 4) return dispatch_fwd_wave<8, 4>(a, s, mode);
    if (C == 16 && G == 4) return dispatch_fwd_wave<16, 4>(a, s, mode);
    if (C == 32 && G == 8) return dispatch_fwd_wave<32, 8>(a, s, mode);
    if (C == 64 && G == 8) return dispatch_fwd_wave<64, 8>(a, s, mode);
    return MVSTER_ERR_UNSUPPORTED;
}

// the forward's argument checks and kernel choice, shared by the plain and the indexed entry (views != nullptr: ref_feat =
// src_feat = the level store, view stride store_vs, and the three plain strides are unused)
static int warp_agg_fwd_any(const float* ref_feat, const float* src_feat, const float* rt, const float* hypo,
                            float* out, float* wsum_out, int B, int NV, int C, int G, int D, int h, int w,
                            int Hs, int Ws, long ref_batch_stride, long src_view_stride, long src_batch_stride,
                            int group_cor, int attn_fuse_d, float attn_temp, int variant, const int* views, long store_vs,
                            const int* nsrc, void* stream) {
    if (!ref_feat || !src_feat || !rt || !hypo || !out) return MVSTER_ERR_NULL;
    if (B <= 0 || NV <= 0 || D <= 0 || D > kMaxFwdD || h <= 0 || w <= 0 || Hs <= 0 || Ws <= 0) return MVSTER_ERR_SHAPE;
    if (!group_cor && G != C) return MVSTER_ERR_SHAPE;
    WarpAggArgs a = make_warp_args(ref_feat, src_feat, rt, hypo, out, wsum_out, B, NV, C, D, h, w, Hs, Ws, ref_batch_stride,
                                   src_view_stride, src_batch_stride, attn_fuse_d, attn_temp);
    a.views = views; a.store_vs = store_vs; a.nsrc = nsrc;
    hipStream_t s = (hipStream_t)stream;
    if ((views || nsrc) && (variant == 4 || variant == 5)) return MVSTER_ERR_UNSUPPORTED;   // (forms kept for the record: plain only)
    // variant: 0 = choose; 1 = one thread per (pixel, d); 2 = workgroup-level lane split (C >= 16);
    // 3 = wave-local kernel (what 0 picks whenever it applies); 4 = pixel-major kernel (faster on cache-resident inputs,
    // slower inside the forward: kept as a tested alternative)
#ifdef MVSTER_PROBES
    if (!views && !nsrc && group_cor && (D == 4 || D == 8) && (variant == 4 || (variant == 0 && C <= 16 && g_pix))) {
        int rc = MVSTER_ERR_UNSUPPORTED;
        if (C == 8 && G == 4) rc = dispatch_fwd_pix<8, 4>(a, s);
        else if (C == 8 && G == 8) rc = dispatch_fwd_pix<8, 8>(a, s);
        else if (C == 16 && G == 4) rc = dispatch_fwd_pix<16, 4>(a, s);
        else if (C == 16 && G == 8) rc = dispatch_fwd_pix<16, 8>(a, s);
        else if (C == 32 && G == 8 && variant == 4) rc = dispatch_fwd_pix<32, 8>(a, s);
        else if (C == 32 && G == 4 && variant == 4) rc = dispatch_fwd_pix<32, 4>(a, s);
        if (rc != MVSTER_ERR_UNSUPPORTED && !(rc == MVSTER_ERR_SHAPE && variant == 0)) return rc;
        // (a map too large for the 24-bit index arithmetic falls through to the wave-local kernel)
    }
    if (group_cor && (D == 4 || D == 8) && variant == 5) {      // LDS-staged source windows (the two fine stages)
        if (C == 8 && G == 4) return dispatch_fwd_tile<8, 4>(a, s);
        if (C == 8 && G == 8) return dispatch_fwd_tile<8, 8>(a, s);
        if (C == 16 && G == 4) return dispatch_fwd_tile<16, 4>(a, s);
        if (C == 16 && G == 8) return dispatch_fwd_tile<16, 8>(a, s);
        return MVSTER_ERR_UNSUPPORTED;
    }
#else
    if (variant == 4 || variant == 5) return MVSTER_ERR_UNSUPPORTED;      // (the probe library has them)
#endif
    if (group_cor && (D == 4 || D == 8) && (variant == 0 || variant == 3)) {
        if (C == 8 && G == 4) return dispatch_fwd_wave<8, 4>(a, s);
        if (C == 8 && G == 8) return dispatch_fwd_wave<8, 8>(a, s);
        if (C == 16 && G == 4) return dispatch_fwd_wave<16, 4>(a, s);
        if (C == 16 && G == 8) return dispatch_fwd_wave<16, 8>(a, s);
        if (C == 32 && G == 8) return dispatch_fwd_wave<32, 8>(a, s);
        if (C == 32 && G == 4) return dispatch_fwd_wave<32, 4>(a, s);
        if (C == 64 && G == 8) return dispatch_fwd_wave<64, 8>(a, s);
    }
    if (group_cor && D <= 8 && variant != 1) {
        if (C == 64 && G == 8) return launch_fwd_lanes<64, 8>(a, s);
        if (C == 32 && G == 8) return launch_fwd_lanes<32, 8>(a, s);
        if (C == 16 && G == 4) return launch_fwd_lanes<16, 4>(a, s);
        if (C == 16 && G == 8) return launch_fwd_lanes<16, 8>(a, s);
    }
    return dispatch_layout(C, G, group_cor != 0, [&](auto c, auto g, auto gr) { return launch_fwd<c(), g(), gr()>(a, s); });
}

extern "C" int mvster_warp_agg_fwd(const float* ref_feat, const float* src_feat, const float* rt, const float* hypo,
                                   float* out, float* wsum_out, int B, int NV, int C, int G, int D, int h, int w,
                                   int Hs, int Ws, long ref_batch_stride, long src_view_stride, long src_batch_stride,
                                   int group_cor, int attn_fuse_d, float attn_temp, int variant, void* stream) {
    return warp_agg_fwd_any(ref_feat, src_feat, rt, hypo, out, wsum_out, B, NV, C, G, D, h, w, Hs, Ws, ref_batch_stride,
                            src_view_stride, src_batch_stride, group_cor, attn_fuse_d, attn_temp, variant, nullptr, 0, nullptr, stream);
}

// mvster_warp_agg_fwd reading its maps from a level store [V, h, w, C] through a DEVICE table views [B, 1 + NV] (column 0
// = the reference view); same kernels, same bits as the plain entry on a gathered copy.  The indices are NOT checked here
// (they are on the device): the caller validates 0 <= index < V before it uploads them.  MVSTER_ERR_UNSUPPORTED also for the
// forms listed at kIndexedOneThread / kIndexedLanes: gather (mvster_gather_views) and call the plain entry.
extern "C" int mvster_warp_agg_fwd_indexed(const float* store, const int* views, const float* rt, const float* hypo, float* out,
                                           float* wsum_out, int V, int B, int NV, int C, int G, int D, int h, int w,
                                           int group_cor, int attn_fuse_d, float attn_temp, int variant, void* stream) {
    if (!store || !views) return MVSTER_ERR_NULL;
    if (V <= 0 || C <= 0) return MVSTER_ERR_SHAPE;
    return warp_agg_fwd_any(store, store, rt, hypo, out, wsum_out, B, NV, C, G, D, h, w, h, w, 0, 0, 0, group_cor, attn_fuse_d,
                            attn_temp, variant, views, (long)h * w * C, nullptr, stream);
}

// The two entries above with a source count per batch item: nsrc is a DEVICE array [B], item b aggregates its first nsrc[b]
// sources (1 <= nsrc[b] <= NV, NOT checked here: the caller validates the counts before it uploads them, as it does the
// table).  NV stays the capacity -- rt is [B, NV, 12] and the table [B, 1 + NV] -- and the rt rows, table entries and maps of
// the slots beyond the count are never read.  Same kernels, and with count n the bits of the uncounted entry at NV = n on the
// first n sources.  MVSTER_ERR_UNSUPPORTED for the same forms as the uncounted entries.
extern "C" int mvster_warp_agg_fwd_counted(const float* ref_feat, const float* src_feat, const float* rt, const float* hypo,
                                           float* out, float* wsum_out, int B, int NV, int C, int G, int D, int h, int w,
                                           int Hs, int Ws, long ref_batch_stride, long src_view_stride, long src_batch_stride,
                                           int group_cor, int attn_fuse_d, float attn_temp, int variant, const int* nsrc,
                                           void* stream) {
    if (!nsrc) return MVSTER_ERR_NULL;
    return warp_agg_fwd_any(ref_feat, src_feat, rt, hypo, out, wsum_out, B, NV, C, G, D, h, w, Hs, Ws, ref_batch_stride,
                            src_view_stride, src_batch_stride, group_cor, attn_fuse_d, attn_temp, variant, nullptr, 0, nsrc, stream);
}

extern "C" int mvster_warp_agg_fwd_indexed_counted(const float* store, const int* views, const float* rt, const float* hypo,
                                                   float* out, float* wsum_out, int V, int B, int NV, int C, int G, int D, int h,
                                                   int w, int group_cor, int attn_fuse_d, float attn_temp, int variant,
                                                   const int* nsrc, void* stream) {
    if (!store || !views || !nsrc) return MVSTER_ERR_NULL;
    if (V <= 0 || C <= 0) return MVSTER_ERR_SHAPE;
    return warp_agg_fwd_any(store, store, rt, hypo, out, wsum_out, B, NV, C, G, D, h, w, h, w, 0, 0, 0, group_cor, attn_fuse_d,
                            attn_temp, variant, views, (long)h * w * C, nsrc, stream);
}

extern "C" int mvster_gather_views(const float* store, const int* views, float* out, int V, int B, int N, long map_floats,
                                   void* stream) {
    if (!store || !views || !out) return MVSTER_ERR_NULL;
    if (V <= 0 || B <= 0 || N <= 0 || map_floats <= 0 || map_floats % 4 || (long)B * N > 65535) return MVSTER_ERR_SHAPE;
    const long quads = map_floats / 4, blocks = (quads + 255) / 256;
    if (blocks > 0x7fffffffL) return MVSTER_ERR_SHAPE;
    hipLaunchKernelGGL(gather_views_kernel, dim3((unsigned)blocks, B * N), dim3(256), 0, (hipStream_t)stream, store, views, out, B, N,
                       quads);
    return mv_check_launch();
}

