// Backward of the fused warp + correlation + attention aggregation (forward: warp_fwd.hip): the window form
// (mvster_warp_agg_bwd) and the sorted scatter (mvster_warp_agg_bwd_sorted), which share warp_agg_bwd_kernel.
#include "warp_common.hpp"

namespace {

// ------------------------------------------------------------------------------------------
// Backward w.r.t. the features (training; autograd of mvs4net_utils.py:1036-1060).  The grid is
// not differentiated (torch.no_grad at :23).  Per (pixel, d) thread and per view: re-gather the
// taps, redo the depth softmax, form dL/dcor, then re-gather once more to scatter
//   d src[tap][c] += w_tap * dwarp[c]      (atomic, 4 taps x C)
//   d ref[c]      += ...                   (atomic, summed over d and views)
// Uses `out` and `wsum` saved by the forward.  Both attention forms (attn_fuse_d on: a weight per (pixel, d); off: one
// per pixel, the largest softmax value along depth, mvs4net_utils.py:1048-1051), up to 16 hypotheses.
// ------------------------------------------------------------------------------------------
// LDS accumulators of the backward are 64-bit FIXED POINT: on gfx950 a wave64 ds_add_f32 costs ~190 LDS cycles
// (scripts/probes/lds_atomic_probe.hip: it is executed lane by lane), ds_add_u64 ~7.  The scatter window and the
// reference-gradient tile therefore accumulate round(v * 2^k) with integer atomics -- which are also associative, so the
// sums no longer depend on the order in which the waves arrive -- and are converted back once.  2^k is chosen per
// launch from upper bounds on the operands (the largest |grad_out|, |ref|, |src|, reduced on the device just before):
// the largest single contribution lands below 2^37, leaving 26 bits of head room for the number of contributions per
// texel and >= 29 bits below the largest value actually seen (fp32 atomics keep 24).
typedef unsigned long long u64;

struct FixScale {
    float s, inv;
};

// maxima = {max |grad_out|, max |ref|, max |src|}
__device__ __forceinline__ FixScale make_fix_scale(const float* maxima, int G, int D, int CG, bool group, bool fuse, float temp) {
    const float gomax = maxima[0], fmax = fmaxf(maxima[1], maxima[2]);
    // |cor| <= cormax; |d L / d cor| <= gomax * (1 + 2 G (1 + D) cormax / temp)  (softmax Jacobian: |sig * dsig| <= 2 G gomax
    // cormax because W >= the view's own weight); a tap contribution is that times a feature value (/ CG), weights <= 1
    const float cormax = group ? fmax * fmax : 4.0f * fmax * fmax;
    const float dcor = gomax * (1.0f + 2.0f * (float)G * (float)(1 + D) * cormax / (fuse ? temp : 1.0f));
    const float bound = group ? dcor * fmax / (float)CG : 4.0f * fmax * dcor;
    FixScale f;
    int e = 0;
    if (bound > 0.0f && bound < INFINITY) frexpf(bound, &e);      // 2^(e-1) <= bound < 2^e
    e = min(max(37 - e, -60), 100);                               // one unit = 2^(e-37) <= bound * 2^-36, the documented resolution
    f.s = ldexpf(1.0f, e);
    f.inv = ldexpf(1.0f, -e);
    // A non-finite operand (absmax_kernel reports NaN for it) has no fixed-point image: integer conversion would turn it
    // into finite garbage.  Every value converted back then reads NaN instead -- the gradients of such a step are NaN, like
    // the reference's, never silently finite (the window forms, whose flush touches only the texels they hit: nan_grad_src
    // below).  (Resolution otherwise: absolute, at most bound * 2^-36 per contribution, i.e. the smallest gradients of a launch keep fewer bits than its largest; fp32 atomics would keep 24 relative to the running sum.)
    // (fmaxf above drops a NaN operand: the feature maxima are looked at themselves)
    if (!(bound < INFINITY) || !(maxima[1] + maxima[2] < INFINITY)) { f.s = 0.0f; f.inv = __builtin_nanf(""); }
    return f;
}
// round-to-nearest-even float -> 64-bit integer for |t| < 2^51 in four instructions (the library conversion takes ~12): adding
// 1.5 * 2^52 in double leaves round(t) in the low mantissa bits, two's complement included
__device__ __forceinline__ u64 fix_cvt(float t) {
    const double d = (double)t + 6755399441055744.0;
    return (u64)(__double_as_longlong(d) - 0x4338000000000000LL);
}
__device__ __forceinline__ void fix_add(u64* p, float v, float s) { atomicAdd(p, fix_cvt(v * s)); }
__device__ __forceinline__ float fix_get(u64 v, float inv) { return (float)(long long)v * inv; }

// max |x| of up to three arrays in one launch: workgroups [first[k], first[k+1]) reduce x[k] (n[k] floats, 16-byte aligned)
// into out[k] (a non-negative float orders like its bit pattern); out[] must start at 0.  ONE atomic per workgroup and at
// most ~1.5k workgroups per launch: atomics on one address retire ~13 ns apart on gfx950.
struct AbsMaxArgs {
    const float* x[3];
    long n[3];
    int first[4];
};
constexpr int kAbsMaxBlocks = 1536;

__device__ __forceinline__ void absmax_block(const AbsMaxArgs& a, float* __restrict__ out, int b) {
    __shared__ float wave_max[4];
    __shared__ int wave_bad[4];
    const int k = (b >= a.first[1] ? 1 : 0) + (b >= a.first[2] ? 1 : 0);
    const float* __restrict__ x = a.x[k];
    const long n = a.n[k];
    float m = 0.0f;
    bool bad = false;           // fmaxf drops NaN: non-finite elements are tracked separately and reported as NaN
    const long n4 = n >> 2;
    const long stride = (long)(a.first[k + 1] - a.first[k]) * 256;
    auto take = [&](const f32x4& v) {
        const float a0 = fabsf(v[0]), a1 = fabsf(v[1]), a2 = fabsf(v[2]), a3 = fabsf(v[3]);
        const float mv = fmaxf(fmaxf(a0, a1), fmaxf(a2, a3));
        m = fmaxf(m, mv);
        // (fmaxf drops a NaN operand: the sum below is NaN / Inf exactly if one of the four is)
        bad = bad || !((a0 + a1) + (a2 + a3) < INFINITY);
    };
    const long t0 = (long)(b - a.first[k]) * 256 + threadIdx.x;
    long i = t0;
    // four independent 16-byte loads in flight per thread
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const f32x4 v0 = ld4(x + i * 4), v1 = ld4(x + (i + stride) * 4), v2 = ld4(x + (i + 2 * stride) * 4),
                    v3 = ld4(x + (i + 3 * stride) * 4);
        take(v0);
        take(v1);
        take(v2);
        take(v3);
    }
    for (; i < n4; i += stride) take(ld4(x + i * 4));
    for (long j = (n4 << 2) + t0; j < n; j += stride) {
        m = fmaxf(m, fabsf(x[j]));
        bad = bad || !(fabsf(x[j]) < INFINITY);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    const bool any_bad = __any(bad);
    if ((threadIdx.x & 63) == 0) { wave_max[threadIdx.x >> 6] = m; wave_bad[threadIdx.x >> 6] = any_bad ? 1 : 0; }
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
        const bool wg_bad = (wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3]) != 0;
        // (as integers, positive floats order like their values and the quiet-NaN pattern lies above +Inf)
        if (m > 0.0f || wg_bad) atomicMax(reinterpret_cast<int*>(out + k), wg_bad ? 0x7fc00000 : __float_as_int(m));
    }
}

__global__ void __launch_bounds__(256) absmax_kernel(AbsMaxArgs a, float* __restrict__ out) { absmax_block(a, out, blockIdx.x); }

// the workgroup layout of launch_absmax, for kernels that carry the reduction beside other work
static AbsMaxArgs absmax_args(const float* const* x, const long* n, int count) {
    AbsMaxArgs a;
    long total = 0;
    for (int k = 0; k < count; ++k) total += n[k];
    a.first[0] = 0;
    for (int k = 0; k < 3; ++k) {
        a.x[k] = k < count ? x[k] : nullptr;
        a.n[k] = k < count ? n[k] : 0;
        long nb = 0;
        if (k < count) {
            nb = total > 0 ? (long)kAbsMaxBlocks * n[k] / total : 1;
            nb = std::min(nb, n[k] / 4096 + 1);
            nb = std::max(nb, 1L);
        }
        a.first[k + 1] = a.first[k] + (int)nb;
    }
    return a;
}

// workgroups in proportion to the arrays' sizes (they finish together), each array at least one
void launch_absmax(const float* const* x, const long* n, int count, float* out, hipStream_t s) {
    const AbsMaxArgs a = absmax_args(x, n, count);
    // (unused entries own no workgroups: first[k] == first[k+1] == gridDim.x, never selected)
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)a.first[3]), dim3(256), 0, s, a, out);
}

struct WarpAggBwdArgs {
    WarpAggArgs f;
    const float* fwd_out;   // [B, D, h, w, G]
    const float* wsum;      // [B, D, h, w]
    const float* grad_out;  // [B, D, h, w, G]
    float* grad_ref;        // [B, h, w, C]
    float* grad_src;        // [NV][B, Hs, Ws, C]  (same strides as src)
    // Deterministic, atomic-free accumulation of grad_src (both null: the window is flushed with global atomics):
    // every workgroup stores its scatter windows densely, windows [B][nblk][NV][C/8][WY][kWinX][8] and their origins
    // win_org [B][nblk][NV][2]; scatter_gather_kernel then sums, per source texel, the windows that cover it.
    float* windows;
    int* win_org;
    const float* maxima;    // {max |grad_out|, max |ref|, max |src|} (device; written just before this launch)
    // sorted scatter (mvster_warp_agg_bwd_sorted; REC instances of warp_agg_bwd_kernel): see the section below
    const int* rec_offset;  // [B*NV*ntiles + 1] exclusive prefix sums of the tiles' record counts
    int* rec_cursor;        // [B*NV*ntiles] running cursors (zero before the launch)
    float* rec;             // the records, kRecWords floats each
    int tiles_x, tiles_y;   // source tiles of kRecTileX x kRecTileY texels
};

// The window forms with a non-finite operand (make_fix_scale: inv is NaN): NaN onto EVERY texel of the batch item's source
// gradients, the ones no window or tap of this launch reaches included -- as atomic adds, so that they commute with the other
// workgroups' flushes, and before the gather pass, which adds onto what it finds.  (The sorted form stores every texel through
// fix_get and needs nothing.)  Workgroup `blk` of `nblk` takes every nblk-th stretch of nthr floats.
__device__ __forceinline__ void nan_grad_src(const WarpAggBwdArgs& ba, int C, int b, int blk, int nblk, int tid, int nthr, float nan) {
    const WarpAggArgs& a = ba.f;
    const long n = (long)a.Hs * a.Ws * C;
    for (int v = 0; v < a.NV; ++v) {
        float* g = ba.grad_src + (long)v * a.src_vs + (long)b * a.src_bs;
        for (long i = (long)blk * nthr + tid; i < n; i += (long)nblk * nthr) unsafeAtomicAdd(g + i, nan);
    }
}

// ------------------------------------------------------------------------------------------
// Sorted scatter of the source-view gradient (the adjoint of grid_sample, mvs4net_utils.py:13-59) WITHOUT global atomics.
// A (pixel, hypothesis, view) sample adds w_tap * dw[c] to four source texels.  With unrelated hypotheses on neighbouring
// pixels (random-winner depth maps) those texels are spread over hundreds of pixels of an epipolar line: the scatter
// windows above catch little and the rest are random-address global atomics, which the chip retires at ~370 G adds/s
// whatever the kernel does (0.92 ms for the 335 M adds of the full-resolution stage).  Here the samples are counting-sorted
// by SOURCE tile instead:
//   K0 warp_bwd_count_kernel   projects every sample and counts, per (batch, view, 32x32 source tile), the samples with a
//                              weighted tap in the tile (a sample on a tile border counts in up to four tiles)
//   K-scan                     exclusive prefix sums of the counts
//   K1 warp_agg_bwd_kernel<.., REC = true>   the backward's arithmetic as before, but instead of scattering it appends a
//                              48-byte record {corner, tap mask, east / south fractions, dw[8]} per 8-channel block to the
//                              list of every tile the sample touches (slots reserved per workgroup: one returning global
//                              atomic per touched tile and view, not per sample)
//   K2 warp_bwd_accum_kernel   one workgroup per (batch, view, channel block, tile): accumulates the tile's records in a
//                              64-bit fixed-point LDS window (integer adds: the order of the records does not matter) and
//                              writes the tile with plain coalesced stores -- every texel of grad_src exactly once, so
//                              the buffer needs no zero fill either.
// Deterministic by construction and independent of how smooth the depth maps are.
// ------------------------------------------------------------------------------------------
constexpr int kRecTileX = 32, kRecShiftX = 5, kRecTileY = 16, kRecShiftY = 4;     // source tile: 32 x 16 texels
constexpr int kRecWords = 12;            // {packed corner + mask, wx1, wy1, 0}, dw[0..3], dw[4..7]
constexpr int kRecMaxTiles = 4096;       // source tiles per map the workgroups' LDS histograms hold (4096 x 512 texels)

// bit k set: tap k carries weight (k = 0 nw (x0, y0), 1 ne (x0+1, y0), 2 sw (x0, y0+1), 3 se); t after clamp_taps()
__device__ __forceinline__ unsigned tap_mask(const mv::Taps& t) {
    return (t.nw != 0.0f ? 1u : 0u) | (t.ne != 0.0f ? 2u : 0u) | (t.sw != 0.0f ? 4u : 0u) | (t.se != 0.0f ? 8u : 0u);
}

// The tiles that hold a weighted tap of the sample: tile[k] = tile of tap k, or -1 where the tap carries no weight or an
// earlier tap already named the tile (statically indexed throughout: no compaction, nothing for the compiler to spill).
struct SampleTiles {
    int tile[4];
};

__device__ __forceinline__ SampleTiles sample_tiles(const mv::Taps& t, unsigned mask, int tiles_x) {
    SampleTiles s;
    const int tx0 = t.x0 >> kRecShiftX, tx1 = (t.x0 + 1) >> kRecShiftX;
    const int ty0 = t.y0 >> kRecShiftY, ty1 = (t.y0 + 1) >> kRecShiftY;
    const int id0 = ty0 * tiles_x + tx0, id1 = ty0 * tiles_x + tx1, id2 = ty1 * tiles_x + tx0, id3 = ty1 * tiles_x + tx1;
    s.tile[0] = (mask & 1u) ? id0 : -1;
    s.tile[1] = ((mask & 2u) && id1 != s.tile[0]) ? id1 : -1;
    s.tile[2] = ((mask & 4u) && id2 != s.tile[0] && id2 != s.tile[1]) ? id2 : -1;
    s.tile[3] = ((mask & 8u) && id3 != s.tile[0] && id3 != s.tile[1] && id3 != s.tile[2]) ? id3 : -1;
    return s;
}

// Scatter window: the source-view gradient of one workgroup (64 reference pixels of a row x all depths) and
// one view lands on a compact patch of the source map (a few rows around an epipolar segment), so it is
// accumulated in LDS (ds_add_f32) over a kWinX x kWinY texel window anchored at the workgroup's smallest tap
// coordinates, 8 channels at a time, and flushed with ONE global atomic per touched (texel, channel) instead
// of one per (pixel, depth, tap, channel): 5-8x fewer global atomics, which is what bounds this kernel.  Taps
// that fall outside the window (strongly rotated views) go to global memory directly.  grad_ref needs no
// atomics at all: each reference pixel belongs to exactly one workgroup, which sums over depths and views in
// LDS and stores once.
// Taps that fall outside the scatter window go to global memory with atomics.  Issued lane = pixel they would be 8
// successive instructions per tap, each lane walking its own texel's channels: the L2 atomic units then see one 4-byte
// request per lane and instruction, ~20 G adds/s whatever the address pattern (scripts/probes/global_atomic_probe.hip).
// Eight neighbouring lanes covering one texel's 32 contiguous bytes are merged into one request: 169 G adds/s.  So a
// wavefront parks the (offset, 8 values) records of its out-of-window lanes in LDS and drains them with
// lane = (record, channel).  Wave-local: no workgroup barrier, 64 records of 36 bytes per wavefront.
struct TapQueue {
    int off[64];
    float val[64][8];
};
constexpr int kQueueDirect = 4;      // up to this many out-of-window lanes of a wavefront issue their atomics themselves

__device__ __forceinline__ void queue_tap(TapQueue& q, float* __restrict__ gsp, bool outside, long off, float wt,
                                          const float (&dw8)[8]) {
    const unsigned long long mask = __ballot(outside);
    if (mask == 0) return;                                   // wave-uniform
    if (__popcll(mask) <= kQueueDirect) {                    // a few stragglers (smooth depth maps): not worth the detour
        if (outside) {
#pragma unroll
            for (int c = 0; c < 8; ++c) unsafeAtomicAdd(gsp + off + c, wt * dw8[c]);
        }
        return;
    }
    const int lane = threadIdx.x & 63;
    if (outside) {
        const int slot = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        q.off[slot] = (int)off;
#pragma unroll
        for (int c = 0; c < 8; ++c) q.val[slot][c] = wt * dw8[c];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int n = __popcll(mask) * 8;
    for (int i = lane; i < n; i += 64) unsafeAtomicAdd(gsp + q.off[i >> 3] + (i & 7), q.val[i >> 3][i & 7]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                         // the records are consumed before the next tap overwrites them
}

// The four taps of one pixel for one 8-channel pass: into the window (64-bit fixed-point LDS atomics) where they fall
// inside it, queued for the coalesced global atomics otherwise.  win = &window[0][0][0] with channel pitch `cpitch` and
// row pitch `rpitch` (u64 units).
struct TapPlace {
    int ax, bx, ay, by;
    bool iax, ibx, iay, iby;
    long o00, o01, o10, o11;
};

__device__ __forceinline__ void scatter_taps(u64* win, int cpitch, int rpitch, TapQueue& q, float* __restrict__ gsp, bool valid,
                                             const mv::Taps& t, const TapPlace& w, int cbase, const float (&dw8)[8],
                                             float fxs) {
    const bool wnw = valid && t.nw != 0.0f, wne = valid && t.ne != 0.0f;
    const bool wsw = valid && t.sw != 0.0f, wse = valid && t.se != 0.0f;
    if (wnw && w.iax && w.iay) {
#pragma unroll
        for (int cl = 0; cl < 8; ++cl) fix_add(win + cl * cpitch + w.ay * rpitch + w.ax, t.nw * dw8[cl], fxs);
    }
    if (wne && w.ibx && w.iay) {
#pragma unroll
        for (int cl = 0; cl < 8; ++cl) fix_add(win + cl * cpitch + w.ay * rpitch + w.bx, t.ne * dw8[cl], fxs);
    }
    if (wsw && w.iax && w.iby) {
#pragma unroll
        for (int cl = 0; cl < 8; ++cl) fix_add(win + cl * cpitch + w.by * rpitch + w.ax, t.sw * dw8[cl], fxs);
    }
    if (wse && w.ibx && w.iby) {
#pragma unroll
        for (int cl = 0; cl < 8; ++cl) fix_add(win + cl * cpitch + w.by * rpitch + w.bx, t.se * dw8[cl], fxs);
    }
    queue_tap(q, gsp, wnw && !(w.iax && w.iay), w.o00 + cbase, t.nw, dw8);
    queue_tap(q, gsp, wne && !(w.ibx && w.iay), w.o01 + cbase, t.ne, dw8);
    queue_tap(q, gsp, wsw && !(w.iax && w.iby), w.o10 + cbase, t.sw, dw8);
    queue_tap(q, gsp, wse && !(w.ibx && w.iby), w.o11 + cbase, t.se, dw8);
}

constexpr int kWinX = 96, kWinY = 6;
static const bool g_bwd_no_tiles = MV_PROBE_ENV("MVSTER_BWD_NO_TILES") != nullptr;   // experiment switch

// REC: the sorted-scatter form (see above) -- no scatter window, no tap queues; pass 2 appends records instead.
template <int C, int G, bool GROUP, int DMAX, bool REC = false>
__global__ void __launch_bounds__(64 * DMAX) warp_agg_bwd_kernel(WarpAggBwdArgs ba) {
    const WarpAggArgs& a = ba.f;
    constexpr int CG = C / G;
    constexpr int NB = C / 8;                // 8-channel blocks: one scatter-window pass each
    constexpr bool GO_REG = G <= 8;          // the pixel's G output gradients live in registers (else they are re-read)
    static_assert(C % 8 == 0 && (GROUP ? (C % G == 0 && G <= 8) : (C == G)), "layout");
    __shared__ float sc[2][DMAX][64];
    __shared__ float sd[2][DMAX][64];
    __shared__ u64 gref[C][64];
    __shared__ u64 win[REC ? 1 : 8][REC ? 1 : kWinY][REC ? 1 : kWinX];
    __shared__ int worg[2][2];
    __shared__ TapQueue tapq[REC ? 1 : DMAX];          // one per wavefront
    __shared__ int lcount[REC ? kRecMaxTiles : 1];     // REC: this workgroup's samples per source tile (one view at a time)
    __shared__ int lbase[REC ? kRecMaxTiles : 1];      //      and the first list position reserved for them
    const FixScale fx = make_fix_scale(ba.maxima, G, a.D, CG, GROUP, a.fuse_d != 0, a.attn_temp);

    const mv::GridNorm gn = mv::make_grid_norm(a.Hs, a.Ws);
    const int tx = threadIdx.x;
    const int d = threadIdx.y;
    const int tid = d * 64 + tx;
    const int nthr = 64 * blockDim.y;
    const int b = blockIdx.y;
    const int hw = a.h * a.w;
    const int p0 = xcd_remap(blockIdx.x, gridDim.x) * 64;
    const int p = p0 + tx;
    const bool valid = p < hw;
    const int pc = valid ? p : hw - 1;
    const int y = pc / a.w;
    const int x = pc - y * a.w;
    const long o = ((long)b * a.D + d) * hw + pc;
    const float depth = a.hypo[o];
    const float* rp = a.ref + (long)b * a.ref_bs + (long)pc * C;
    const float W = ba.wsum[o];
    const float invW = 1.0f / W;
    const float vmask = valid ? 1.0f : 0.0f;
    const float* gop = ba.grad_out + o * G;

    // go[g] = dL/d out[g] of this (pixel, d); common = sum_g go[g] * out[g]
    float go[GO_REG ? G : 1];
    float common = 0.0f;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float gv = gop[g] * vmask;
        common = fmaf(gv, ba.fwd_out[o * G + g], common);
        if (GO_REG) go[g] = gv;
    }
    for (int i = tid; i < C * 64; i += nthr) (&gref[0][0])[i] = 0;
    // narrow maps: this thread's share of the reference gradient is summed over the views in registers (integers: the same
    // bits as adding every view's term to LDS) and lands in LDS once
    constexpr bool GREF_REG = C <= 16;
    u64 gacc[GREF_REG ? C : 1];
#pragma unroll
    for (int c = 0; c < (GREF_REG ? C : 1); ++c) gacc[c] = 0;
    if (!REC)
        for (int i = tid; i < 8 * kWinY * kWinX; i += nthr) (&win[0][0][0])[i] = 0;
    const int ntiles = REC ? ba.tiles_x * ba.tiles_y : 0;
    if (REC)
        for (int i = tid; i < ntiles; i += nthr) lcount[i] = 0;
    __syncthreads();

    for (int v = 0; v < a.NV; ++v) {
        MV_LOAD_RT(m, a, b, v)
        float sx, sy;
        mv::project(m, (float)x, (float)y, depth, gn, sx, sy);      // (shared reciprocals: the forward kernels' form)
        mv::Taps t = mv::make_taps(sx, sy, a.Hs, a.Ws);
        const mv::TapsClamped tc = mv::clamp_taps(t, a.Hs, a.Ws);
        const long voff = (long)v * a.src_vs + (long)b * a.src_bs;
        const long o00 = ((long)tc.ya * a.Ws + tc.xa) * C, o01 = ((long)tc.ya * a.Ws + tc.xb) * C;
        const long o10 = ((long)tc.yb * a.Ws + tc.xa) * C, o11 = ((long)tc.yb * a.Ws + tc.xb) * C;
        const float* sp = a.src + voff;
        float* gsp = ba.grad_src + voff;
        // REC: the tiles this sample's weighted taps fall into, its tap mask and fractions (the record's header)
        unsigned tmask = 0;
        SampleTiles stl;
        stl.tile[0] = stl.tile[1] = stl.tile[2] = stl.tile[3] = -1;
        int li[4] = {0, 0, 0, 0};
        float wx1 = 0.0f, wy1 = 0.0f;
        if (REC) {
            tmask = valid ? tap_mask(t) : 0u;
            stl = sample_tiles(t, tmask, ba.tiles_x);
            mv::tap_fractions(sx, sy, a.Hs, a.Ws, wx1, wy1);
        }

        // pass 1: score (same arithmetic and order as the forward) and gdot = sum_g go[g] * cor[g]
        // (the warped feature of every channel stays in registers for pass 2 where the register file has room: with
        //  unrelated hypotheses on neighbouring pixels the taps are 32-byte gathers that miss L2, and the second gather
        //  round was half of this kernel's memory time)
        constexpr bool KEEP_WV = C <= 32;
        float wvk[KEEP_WV ? C : 1];
        float score = 0.0f, gdot = 0.0f, part = 0.0f;
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
            f32x4 gq[2];
            if (!GO_REG) { gq[0] = ld4(gop + cb * 8) * vmask; gq[1] = ld4(gop + cb * 8 + 4) * vmask; }
#pragma unroll
            for (int c0 = 0; c0 < 8; c0 += 4) {
                const f32x4 R = ld4(rp + cb * 8 + c0);
                const f32x4 A = ld4(sp + o00 + cb * 8 + c0), Bq = ld4(sp + o01 + cb * 8 + c0);
                const f32x4 Cq = ld4(sp + o10 + cb * 8 + c0), Dq = ld4(sp + o11 + cb * 8 + c0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = cb * 8 + c0 + j;
                    const float wv = mv::blend(t, A[j], Bq[j], Cq[j], Dq[j]);
                    if (KEEP_WV) wvk[KEEP_WV ? c : 0] = wv;
                    if (GROUP) {
                        const float pr = mv::mul_rn(wv, R[j]);
                        part = (c % CG == 0) ? pr : mv::add_rn(part, pr);
                        if (c % CG == CG - 1) {
                            const float cg = mv::div_rn(part, (float)CG);
                            score = (c / CG == 0) ? cg : mv::add_rn(score, cg);
                            gdot = fmaf(go[GO_REG ? c / CG : 0], cg, gdot);
                        }
                    } else {
                        const float df = mv::sub_rn(R[j], wv);
                        const float cg = mv::mul_rn(df, df);
                        score = (c == 0) ? cg : mv::add_rn(score, cg);
                        gdot = fmaf(GO_REG ? go[GO_REG ? c : 0] : gq[c0 / 4][j], cg, gdot);
                    }
                }
            }
        }
        if (a.fuse_d) score = mv::div_rn(score, a.attn_temp);
        sc[v & 1][d][tx] = score;
        if (tid == 0) { worg[v & 1][0] = 0x7fffffff; worg[v & 1][1] = 0x7fffffff; }
        __syncthreads();
        if (REC) {
            // position of this sample among the workgroup's samples of each tile it touches
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2)
                if (stl.tile[k2] >= 0) li[k2] = atomicAdd(&lcount[stl.tile[k2]], 1);
        }
        // window origin = smallest tap coordinates of the taps that carry weight (one LDS atomic per wave)
        if (!REC) {
            const bool any = valid && (t.nw != 0.0f || t.ne != 0.0f || t.sw != 0.0f || t.se != 0.0f);
            int mnx = any ? tc.xa : 0x7fffffff, mny = any ? tc.ya : 0x7fffffff;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                mnx = min(mnx, __shfl_xor(mnx, off));
                mny = min(mny, __shfl_xor(mny, off));
            }
            if (tx == 0) { atomicMin(&worg[v & 1][0], mnx); atomicMin(&worg[v & 1][1], mny); }
        }
        float mx = sc[v & 1][0][tx];
        int dstar = 0;
        for (int j = 1; j < a.D; ++j) {
            const float sj = sc[v & 1][j][tx];
            if (sj > mx) { mx = sj; dstar = j; }          // first maximum
        }
        float den = 0.0f;
        for (int j = 0; j < a.D; ++j) den += expf(sc[v & 1][j][tx] - mx);
        const float sig = expf(score - mx) / den;
        // dL/dw = (sum_g go[g]*cor[g] - sum_g go[g]*out[g]) / W  per (pixel, d); attn_fuse_d: one weight per (pixel, d),
        // w = softmax_d(score / temp) / sqrt(C); otherwise one weight per pixel, w = max_d softmax_d(score) = 1 / den
        float wgt, dscore;
        if (a.fuse_d) {
            wgt = sig / a.sqrt_c;
            const float dsig = (gdot - common) * invW / a.sqrt_c;
            sd[v & 1][d][tx] = sig * dsig;
            __syncthreads();
            float dot = 0.0f;
            for (int j = 0; j < a.D; ++j) dot += sd[v & 1][j][tx];
            dscore = sig * (dsig - dot) / a.attn_temp;   // d/d(sum_g cor[g])
        } else {
            wgt = 1.0f / den;
            sd[v & 1][d][tx] = gdot - common;
            __syncthreads();
            float dws = 0.0f;
            for (int j = 0; j < a.D; ++j) dws += sd[v & 1][j][tx];
            dscore = dws * invW * wgt * ((d == dstar ? 1.0f : 0.0f) - sig);
        }
        long slot0[4] = {0, 0, 0, 0};
        int cstride[4] = {0, 0, 0, 0};
        if (REC) {
            // reserve list space for the workgroup's samples: ONE returning global atomic per touched tile
            const long g0 = ((long)b * a.NV + v) * ntiles;
            for (int i = tid; i < ntiles; i += nthr) {
                const int c = lcount[i];
                if (c) {
                    lbase[i] = atomicAdd(ba.rec_cursor + g0 + i, c);
                    lcount[i] = 0;
                }
            }
            __syncthreads();
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2)
                if (stl.tile[k2] >= 0) {
                    const int off = ba.rec_offset[g0 + stl.tile[k2]];
                    cstride[k2] = ba.rec_offset[g0 + stl.tile[k2] + 1] - off;
                    slot0[k2] = (long)off * NB + lbase[stl.tile[k2]] + li[k2];
                }
        }
        const int wx0 = worg[v & 1][0], wy0 = worg[v & 1][1];
        // window coordinates of the four taps (negative / too large = outside -> global atomics)
        TapPlace tp;
        tp.ax = tc.xa - wx0; tp.bx = tc.xb - wx0; tp.ay = tc.ya - wy0; tp.by = tc.yb - wy0;
        tp.iax = (unsigned)tp.ax < (unsigned)kWinX; tp.ibx = (unsigned)tp.bx < (unsigned)kWinX;
        tp.iay = (unsigned)tp.ay < (unsigned)kWinY; tp.iby = (unsigned)tp.by < (unsigned)kWinY;
        tp.o00 = o00; tp.o01 = o01; tp.o10 = o10; tp.o11 = o11;

        // pass 2: re-gather, scatter the feature gradients, 8 channels per window pass (unrolled: go[] stays in registers)
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
            const int cbase = cb * 8;
            float dw8[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) dw8[j] = 0.0f;
            if (valid) {
                f32x4 gq[2];
                if (!GO_REG) { gq[0] = ld4(gop + cbase); gq[1] = ld4(gop + cbase + 4); }
#pragma unroll
                for (int c0 = 0; c0 < 8; c0 += 4) {
                    const f32x4 R = ld4(rp + cbase + c0);
                    f32x4 A = {0.f, 0.f, 0.f, 0.f}, Bq = A, Cq = A, Dq = A;
                    if (!KEEP_WV) {
                        A = ld4(sp + o00 + cbase + c0); Bq = ld4(sp + o01 + cbase + c0);
                        Cq = ld4(sp + o10 + cbase + c0); Dq = ld4(sp + o11 + cbase + c0);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int cl = c0 + j;               // channel within the pass
                        const int c = cbase + cl;
                        const float gv = GO_REG ? go[GO_REG ? (GROUP ? c / CG : c) : 0] : gq[c0 / 4][j];
                        const float dcor = fmaf(gv * invW, wgt, dscore);   // direct + through the softmax
                        const float wv = KEEP_WV ? wvk[KEEP_WV ? c : 0] : mv::blend(t, A[j], Bq[j], Cq[j], Dq[j]);
                        float dref;
                        if (GROUP) {
                            dw8[cl] = dcor * (1.0f / CG) * R[j];
                            dref = dcor * (1.0f / CG) * wv;
                        } else {
                            const float df = R[j] - wv;
                            dref = 2.0f * df * dcor;
                            dw8[cl] = -dref;
                        }
                        if (GREF_REG) gacc[GREF_REG ? c : 0] += fix_cvt(dref * fx.s);
                        else fix_add(&gref[c][tx], dref, fx.s);
                    }
                }
            }
            if (REC) {
                // one 48-byte record per touched tile into the list of (batch, view, tile), channel block cb
                const float hdr = __int_as_float((int)((unsigned)(t.x0 + 1) | ((unsigned)(t.y0 + 1) << 13) | (tmask << 26)));
#pragma unroll
                for (int k2 = 0; k2 < 4; ++k2)
                    if (stl.tile[k2] >= 0) {
                        float* r = ba.rec + (slot0[k2] + (long)cb * cstride[k2]) * kRecWords;
                        st4(r, f32x4{hdr, wx1, wy1, 0.0f});
                        st4(r + 4, f32x4{dw8[0], dw8[1], dw8[2], dw8[3]});
                        st4(r + 8, f32x4{dw8[4], dw8[5], dw8[6], dw8[7]});
                    }
                continue;
            }
            scatter_taps(&win[0][0][0], kWinY * kWinX, kWinX, tapq[d], gsp, valid, t, tp, cbase, dw8, fx.s);
            __syncthreads();
            if (ba.windows) {
                // store (and clear) the window densely, texel-major / channel-fastest; scatter_gather_kernel sums the
                // windows that cover a source texel in workgroup order: no atomics, the same bits on every run
                const long slot = (((long)b * gridDim.x + blockIdx.x) * a.NV + v) * NB + cb;
                float* wp = ba.windows + slot * (8 * kWinY * kWinX);
                for (int i = tid; i < 8 * kWinY * kWinX; i += nthr) {
                    const int cl = i % 8, tex = i / 8;
                    const int wxx = tex % kWinX, wyy = tex / kWinX;
                    wp[i] = fix_get(win[cl][wyy][wxx], fx.inv);
                    win[cl][wyy][wxx] = 0;
                }
                if (cb == 0 && tid == 0) {
                    int* op = ba.win_org + (((long)b * gridDim.x + blockIdx.x) * a.NV + v) * 2;
                    op[0] = wx0; op[1] = wy0;
                }
            } else {
                // flush (and clear) the window: one global atomic per touched (texel, channel), channel-fastest: the
                // atomics of a wave go to 8 neighbouring texels x 8 channels = 256 contiguous bytes
                for (int i = tid; i < 8 * kWinY * kWinX; i += nthr) {
                    const int cl = i % 8, tex = i / 8;
                    const int wxx = tex % kWinX, wyy = tex / kWinX;
                    const u64 raw = win[cl][wyy][wxx];
                    if (raw != 0) {
                        win[cl][wyy][wxx] = 0;
                        unsafeAtomicAdd(gsp + ((long)(wy0 + wyy) * a.Ws + (wx0 + wxx)) * C + cbase + cl, fix_get(raw, fx.inv));
                    }
                }
            }
            __syncthreads();
        }
    }
    if (GREF_REG) {
#pragma unroll
        for (int c = 0; c < (GREF_REG ? C : 1); ++c) atomicAdd(&gref[c][tx], gacc[c]);
    }
    if (REC || GREF_REG) __syncthreads();      // (the window form's last flush ends with a barrier, before these adds)
    // every reference pixel of this workgroup is complete: plain coalesced stores
    float* grp = ba.grad_ref + (long)b * a.ref_bs + (long)p0 * C;
    const int npix = min(64, hw - p0);
    for (int i = tid; i < npix * C; i += nthr) grp[i] = fix_get(gref[i % C][i / C], fx.inv);
    if (!REC && !(fx.inv == fx.inv)) nan_grad_src(ba, C, b, blockIdx.x, gridDim.x, tid, nthr, fx.inv);
}

// 2-D tile form for the full-resolution stage (C = 8, where this kernel's time is): one workgroup owns 64 columns x R
// consecutive reference rows and keeps ONE scatter window per view for all of them -- a bilinear footprint makes
// neighbouring reference rows hit the same two source rows, so R rows need R + 2 window rows instead of 3 R.  Same
// arithmetic as warp_agg_bwd_kernel; kTileWinX columns (the 64-bit accumulators double the window's LDS footprint; 80 is
// what leaves room for two workgroups per CU).
constexpr int kTileWinX = 80;

// NW = wavefronts (depth hypotheses) the LDS is sized for.  With NW = 4 (the shipped full-resolution stage) the kernel
// needs 80.7 KB: two workgroups per CU -- it is latency-bound.
template <int G, bool GROUP, int R, int NW>
__global__ void __launch_bounds__(64 * NW) warp_agg_bwd_tile_kernel(WarpAggBwdArgs ba, int tiles_x) {
    const WarpAggArgs& a = ba.f;
    constexpr int C = 8;
    constexpr int CG = C / G;
    constexpr int WY = R + 6;
    __shared__ float sc[2][NW][64];
    __shared__ float sd[2][NW][64];
    __shared__ u64 gref[R][C][64];
    __shared__ u64 win[8][WY][kTileWinX];
    __shared__ int worg[2];
    __shared__ TapQueue tapq[NW];            // one per wavefront
    const FixScale fx = make_fix_scale(ba.maxima, G, a.D, CG, GROUP, true, a.attn_temp);

    const int tx = threadIdx.x;
    const int d = threadIdx.y;
    const int tid = d * 64 + tx;
    const int nthr = 64 * blockDim.y;
    const int b = blockIdx.y;
    const int hw = a.h * a.w;
    const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int x0 = (int)(bid % tiles_x) * 64, y0 = (int)(bid / tiles_x) * R;
    const int x = min(x0 + tx, a.w - 1);
    const bool vcol = x0 + tx < a.w;

    for (int i = tid; i < R * C * 64; i += nthr) (&gref[0][0][0])[i] = 0;
    for (int i = tid; i < 8 * WY * kTileWinX; i += nthr) (&win[0][0][0])[i] = 0;

    for (int v = 0; v < a.NV; ++v) {
        MV_LOAD_RT(m, a, b, v)
        const long voff = (long)v * a.src_vs + (long)b * a.src_bs;
        const float* sp = a.src + voff;
        float* gsp = ba.grad_src + voff;
        // window origin over all rows of the tile
        if (tid == 0) { worg[0] = 0x7fffffff; worg[1] = 0x7fffffff; }
        __syncthreads();
        {
            int mnx = 0x7fffffff, mny = 0x7fffffff;
            for (int r = 0; r < R; ++r) {
                const int y = y0 + r;
                if (y >= a.h) break;
                const float depth = a.hypo[((long)b * a.D + d) * hw + (long)y * a.w + x];
                float sx, sy;
                mv::project(m, (float)x, (float)y, depth, a.Hs, a.Ws, sx, sy);
                mv::Taps t = mv::make_taps(sx, sy, a.Hs, a.Ws);
                const mv::TapsClamped tc = mv::clamp_taps(t, a.Hs, a.Ws);
                if (vcol && (t.nw != 0.0f || t.ne != 0.0f || t.sw != 0.0f || t.se != 0.0f)) {
                    mnx = min(mnx, tc.xa);
                    mny = min(mny, tc.ya);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                mnx = min(mnx, __shfl_xor(mnx, off));
                mny = min(mny, __shfl_xor(mny, off));
            }
            if (tx == 0) { atomicMin(&worg[0], mnx); atomicMin(&worg[1], mny); }
        }
        __syncthreads();
        const int wx0 = worg[0], wy0 = worg[1];

        for (int r = 0; r < R; ++r) {
            const int y = min(y0 + r, a.h - 1);
            const bool valid = vcol && y0 + r < a.h;
            const long o = ((long)b * a.D + d) * hw + (long)y * a.w + x;
            const float depth = a.hypo[o];
            const float* rp = a.ref + (long)b * a.ref_bs + ((long)y * a.w + x) * C;
            const float invW = 1.0f / ba.wsum[o];
            float go[G];
            float common = 0.0f;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                go[g] = valid ? ba.grad_out[o * G + g] : 0.0f;
                common = fmaf(go[g], ba.fwd_out[o * G + g], common);
            }
            float sx, sy;
            mv::project(m, (float)x, (float)y, depth, a.Hs, a.Ws, sx, sy);
            mv::Taps t = mv::make_taps(sx, sy, a.Hs, a.Ws);
            const mv::TapsClamped tc = mv::clamp_taps(t, a.Hs, a.Ws);
            const long o00 = ((long)tc.ya * a.Ws + tc.xa) * C, o01 = ((long)tc.ya * a.Ws + tc.xb) * C;
            const long o10 = ((long)tc.yb * a.Ws + tc.xa) * C, o11 = ((long)tc.yb * a.Ws + tc.xb) * C;

            // the eight channels of the reference pixel and of its warped source value stay in registers for both passes
            float Rv[8], wv[8];
#pragma unroll
            for (int c0 = 0; c0 < 8; c0 += 4) {
                const f32x4 Rq = ld4(rp + c0);
                const f32x4 A = ld4(sp + o00 + c0), Bq = ld4(sp + o01 + c0);
                const f32x4 Cq = ld4(sp + o10 + c0), Dq = ld4(sp + o11 + c0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    Rv[c0 + j] = Rq[j];
                    wv[c0 + j] = mv::blend(t, A[j], Bq[j], Cq[j], Dq[j]);
                }
            }
            // pass 1: score (same arithmetic and order as the forward) and gdot = sum_g go[g] * cor[g]
            float score = 0.0f, gdot = 0.0f, part = 0.0f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                if (GROUP) {
                    const float pr = mv::mul_rn(wv[c], Rv[c]);
                    part = (c % CG == 0) ? pr : mv::add_rn(part, pr);
                    if (c % CG == CG - 1) {
                        const float cg = mv::div_rn(part, (float)CG);
                        score = (c / CG == 0) ? cg : mv::add_rn(score, cg);
                        gdot = fmaf(go[c / CG], cg, gdot);
                    }
                } else {
                    const float df = mv::sub_rn(Rv[c], wv[c]);
                    const float cg = mv::mul_rn(df, df);
                    score = (c == 0) ? cg : mv::add_rn(score, cg);
                    gdot = fmaf(go[GROUP ? 0 : c], cg, gdot);
                }
            }
            score = mv::div_rn(score, a.attn_temp);
            const int par = r & 1;
            sc[par][d][tx] = score;
            __syncthreads();
            float mx = sc[par][0][tx];
            for (int j = 1; j < a.D; ++j) mx = fmaxf(mx, sc[par][j][tx]);
            float den = 0.0f;
            for (int j = 0; j < a.D; ++j) den += expf(sc[par][j][tx] - mx);
            const float sig = expf(score - mx) / den;
            const float wgt = sig / a.sqrt_c;
            const float dsig = (gdot - common) * invW / a.sqrt_c;
            sd[par][d][tx] = sig * dsig;
            __syncthreads();
            float dot = 0.0f;
            for (int j = 0; j < a.D; ++j) dot += sd[par][j][tx];
            const float dscore = sig * (dsig - dot) / a.attn_temp;
            TapPlace tp;
            tp.ax = tc.xa - wx0; tp.bx = tc.xb - wx0; tp.ay = tc.ya - wy0; tp.by = tc.yb - wy0;
            tp.iax = (unsigned)tp.ax < (unsigned)kTileWinX; tp.ibx = (unsigned)tp.bx < (unsigned)kTileWinX;
            tp.iay = (unsigned)tp.ay < (unsigned)WY; tp.iby = (unsigned)tp.by < (unsigned)WY;
            tp.o00 = o00; tp.o01 = o01; tp.o10 = o10; tp.o11 = o11;

            // pass 2: scatter into the tile's window (64-bit fixed-point LDS atomics; coalesced global atomics outside it)
            float dw8[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int g = GROUP ? c / CG : c;
                const float dcor = fmaf(go[g] * invW, wgt, dscore);
                float dref;
                if (GROUP) {
                    dw8[c] = dcor * (1.0f / CG) * Rv[c];
                    dref = dcor * (1.0f / CG) * wv[c];
                } else {
                    const float df = Rv[c] - wv[c];
                    dref = 2.0f * df * dcor;
                    dw8[c] = -dref;
                }
                if (valid) fix_add(&gref[r][c][tx], dref, fx.s);
            }
            scatter_taps(&win[0][0][0], WY * kTileWinX, kTileWinX, tapq[d], gsp, valid, t, tp, 0, dw8, fx.s);
        }
        __syncthreads();
        if (ba.windows) {
            // dense, texel-major / channel-fastest window for scatter_gather_kernel (fixed summation order)
            const long slot = ((long)b * gridDim.x + blockIdx.x) * a.NV + v;
            float* wp = ba.windows + slot * (8 * WY * kTileWinX);
            for (int i = tid; i < 8 * WY * kTileWinX; i += nthr) {
                const int cl = i % 8, tex = i / 8;
                const int wxx = tex % kTileWinX, wyy = tex / kTileWinX;
                wp[i] = fix_get(win[cl][wyy][wxx], fx.inv);
                win[cl][wyy][wxx] = 0;
            }
            if (tid == 0) { ba.win_org[slot * 2] = wx0; ba.win_org[slot * 2 + 1] = wy0; }
        } else {
            for (int i = tid; i < 8 * WY * kTileWinX; i += nthr) {
                const int cl = i % 8, tex = i / 8;
                const int wxx = tex % kTileWinX, wyy = tex / kTileWinX;
                const u64 raw = win[cl][wyy][wxx];
                if (raw != 0) {
                    win[cl][wyy][wxx] = 0;
                    unsafeAtomicAdd(gsp + ((long)(wy0 + wyy) * a.Ws + (wx0 + wxx)) * C + cl, fix_get(raw, fx.inv));
                }
            }
        }
        __syncthreads();
    }
    // reference gradients of the tile: plain stores
    for (int r = 0; r < R; ++r) {
        const int y = y0 + r;
        if (y >= a.h) break;
        float* grp = ba.grad_ref + (long)b * a.ref_bs + ((long)y * a.w + x0) * C;
        const int npix = min(64, a.w - x0);
        for (int i = tid; i < npix * C; i += nthr) grp[i] = fix_get(gref[r][i % C][i / C], fx.inv);
    }
    if (!(fx.inv == fx.inv)) nan_grad_src(ba, C, b, blockIdx.x, gridDim.x, tid, nthr, fx.inv);
}

// Second pass of the atomic-free backward: one workgroup per 32 x 4 tile of one source map; lane = (texel, channel
// quad).  The windows that overlap the tile are found by testing every workgroup's origin (a few thousand integer
// compares per tile, in index order through a ballot prefix so that the summation order is fixed) and summed in
// registers; the tile is then added onto grad_src, which holds what the first pass scattered directly (taps outside a
// window).  WY = window rows (kWinY for the row kernel, R + 6 for the tile kernel).
constexpr int kGatherList = 256;

template <int WY, int WX, int NBLK>
__global__ void __launch_bounds__(256) scatter_gather_kernel(const float* __restrict__ windows, const int* __restrict__ org,
                                                             float* __restrict__ grad_src, int nblk, int NV, int Hs, int Ws,
                                                             long src_vs, long src_bs, int tiles_x) {
    constexpr int C = NBLK * 8;
    __shared__ int list[kGatherList];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int v = blockIdx.y, b = blockIdx.z;
    const int tx0 = (int)(blockIdx.x % tiles_x) * 32, ty0 = (int)(blockIdx.x / tiles_x) * 4;
    const int half = tid & 1, tex = tid >> 1;
    const int tx = tx0 + (tex & 31), ty = ty0 + (tex >> 5);
    const bool inside = tx < Ws && ty < Hs;
    f32x4 acc[NBLK];
#pragma unroll
    for (int cb = 0; cb < NBLK; ++cb) acc[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const long slot0 = (long)b * nblk;

    int count = 0;                                   // entries in list (block-uniform)
    for (int base = 0; base < nblk || count > 0; base += 256) {
        if (base < nblk) {
            const int k = base + tid;
            bool hit = false;
            if (k < nblk) {
                const int* o = org + ((slot0 + k) * NV + v) * 2;
                const int wx0 = o[0], wy0 = o[1];
                hit = wx0 != 0x7fffffff && wx0 < tx0 + 32 && wx0 + WX > tx0 && wy0 < ty0 + 4 && wy0 + WY > ty0;
            }
            const unsigned long long m = __ballot(hit);
            if (lane == 0) wcnt[wave] = __popcll(m);
            __syncthreads();
            int off = count + __popcll(m & ((1ull << lane) - 1));
            for (int w = 0; w < wave; ++w) off += wcnt[w];
            if (hit) list[off] = k;                  // (count + 256 <= kGatherList is kept by draining below)
            count += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            __syncthreads();
        }
        // drain when the next chunk might not fit, and at the end
        if (count > kGatherList - 256 || base + 256 >= nblk) {
            for (int li = 0; li < count; ++li) {
                const int k = list[li];
                const int* o = org + ((slot0 + k) * NV + v) * 2;
                const int lx = tx - o[0], ly = ty - o[1];
                if ((unsigned)lx < (unsigned)WX && (unsigned)ly < (unsigned)WY) {
                    const float* wp = windows + ((slot0 + k) * NV + v) * ((long)NBLK * 8 * WY * WX) +
                                      ((long)ly * WX + lx) * 8 + half * 4;
#pragma unroll
                    for (int cb = 0; cb < NBLK; ++cb) acc[cb] += ld4(wp + (long)cb * (8 * WY * WX));
                }
            }
            __syncthreads();
            count = 0;
            if (base + 256 >= nblk) break;
        }
    }
    if (inside) {
        float* dst = grad_src + (long)v * src_vs + (long)b * src_bs + ((long)ty * Ws + tx) * C + half * 4;
#pragma unroll
        for (int cb = 0; cb < NBLK; ++cb) st4(dst + cb * 8, ld4(dst + cb * 8) + acc[cb]);
    }
}

template <int WY, int WX, int NBLK>
int launch_gather(const WarpAggBwdArgs& ba, int nblk, hipStream_t stream) {
    const WarpAggArgs& a = ba.f;
    const int tiles_x = (a.Ws + 31) / 32, tiles_y = (a.Hs + 3) / 4;
    hipLaunchKernelGGL((scatter_gather_kernel<WY, WX, NBLK>), dim3(tiles_x * tiles_y, a.NV, a.B), dim3(256), 0, stream, ba.windows,
                       ba.win_org, ba.grad_src, nblk, a.NV, a.Hs, a.Ws, a.src_vs, a.src_bs, tiles_x);
    return mv_check_launch();
}

// ---- sorted scatter: K0 (count), scan, K2 (accumulate) ---------------------------------------------------------------
// K0: thread = (pixel, hypothesis) of batch item blockIdx.y, all views; per view an LDS histogram over the source tiles,
// flushed with one global atomic per touched tile.
__device__ __forceinline__ void warp_bwd_count_block(const WarpAggArgs& a, int* __restrict__ count, int tiles_x, int tiles_y,
                                                     int bx, int b) {
    __shared__ int lcount[kRecMaxTiles];
    const int ntiles = tiles_x * tiles_y;
    const long hw = (long)a.h * a.w;
    const long i = (long)bx * 256 + threadIdx.x;                    // = pixel * D + d
    const mv::GridNorm gn = mv::make_grid_norm(a.Hs, a.Ws);
    const bool valid = i < hw * a.D;
    const long pc = valid ? i / a.D : hw - 1;
    const int d = valid ? (int)(i - pc * a.D) : 0;
    const int y = (int)(pc / a.w), x = (int)(pc - (long)y * a.w);
    const float depth = a.hypo[((long)b * a.D + d) * hw + pc];
    for (int t = threadIdx.x; t < ntiles; t += 256) lcount[t] = 0;
    __syncthreads();
    for (int v = 0; v < a.NV; ++v) {
        MV_LOAD_RT(m, a, b, v)
        float sx, sy;
        mv::project(m, (float)x, (float)y, depth, gn, sx, sy);      // (shared reciprocals: the forward kernels' form)
        mv::Taps t = mv::make_taps(sx, sy, a.Hs, a.Ws);
        mv::clamp_taps(t, a.Hs, a.Ws);
        const SampleTiles stl = sample_tiles(t, valid ? tap_mask(t) : 0u, tiles_x);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (stl.tile[k] >= 0) atomicAdd(&lcount[stl.tile[k]], 1);
        __syncthreads();
        int* gc = count + ((long)b * a.NV + v) * ntiles;
        for (int tl = threadIdx.x; tl < ntiles; tl += 256) {
            const int c = lcount[tl];
            if (c) {
                atomicAdd(gc + tl, c);
                lcount[tl] = 0;
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) warp_bwd_zero_kernel(int* __restrict__ a, long na, int* __restrict__ b, long nb) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < na) a[i] = 0;
    if (i < nb) b[i] = 0;
}

__global__ void __launch_bounds__(256) warp_bwd_count_kernel(WarpAggArgs a, int* __restrict__ count, int tiles_x, int tiles_y) {
    warp_bwd_count_block(a, count, tiles_x, tiles_y, blockIdx.x, blockIdx.y);
}

// The counting pass and the operand maxima of the fixed-point scale in ONE launch: they are independent, one is bound by
// instructions and the other by memory, and each alone leaves most of the chip idle for part of its time.  Workgroups
// [0, nabs) reduce the maxima, the rest count (per_b workgroups per batch item).
__global__ void __launch_bounds__(256) warp_bwd_prep_kernel(WarpAggArgs a, int* __restrict__ count, int tiles_x, int tiles_y,
                                                            AbsMaxArgs am, float* __restrict__ maxima, int nabs, int per_b) {
    if ((int)blockIdx.x < nabs) {
        absmax_block(am, maxima, blockIdx.x);
        return;
    }
    const int r = (int)blockIdx.x - nabs;
    warp_bwd_count_block(a, count, tiles_x, tiles_y, r % per_b, r / per_b);
}

// offset[0..n] = exclusive prefix sums of count[0..n) (offset[n] = total); one workgroup
__global__ void __launch_bounds__(1024) warp_bwd_scan_kernel(const int* __restrict__ count, int* __restrict__ offset, int n) {
    __shared__ int part[1024];
    const int chunk = (n + 1023) / 1024;
    const int lo = threadIdx.x * chunk, hi = min(lo + chunk, n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += count[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;                                 // exclusive
    for (int i = lo; i < hi; ++i) {
        offset[i] = run;
        run += count[i];
    }
    if (threadIdx.x == 1023) offset[n] = part[1023];
}

struct WarpBwdAccumArgs {
    const float* rec; const int* offset; const float* maxima; float* grad_src;
    long src_vs, src_bs;
    int NV, NB, C, Hs, Ws, tiles_x, tiles_y, G, D, CG, group, fuse;
    float attn_temp;
};

// K2: workgroup = (tile, view * NB + channel block, batch); lane = record.  The window is channel-major ([8] planes of
// 32 x 32 u64): the lanes of an atomic instruction hit one plane at (practically) random texels.
__global__ void __launch_bounds__(256) warp_bwd_accum_kernel(WarpBwdAccumArgs a) {
    __shared__ u64 win[8][kRecTileX * kRecTileY];
    const FixScale fx = make_fix_scale(a.maxima, a.G, a.D, a.CG, a.group != 0, a.fuse != 0, a.attn_temp);
    const int tile = blockIdx.x, v = blockIdx.y / a.NB, cb = blockIdx.y - v * a.NB, b = blockIdx.z;
    const int ntiles = a.tiles_x * a.tiles_y;
    const int tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
    for (int i = threadIdx.x; i < 8 * kRecTileX * kRecTileY; i += 256) (&win[0][0])[i] = 0;
    __syncthreads();
    const long g0 = ((long)b * a.NV + v) * ntiles + tile;
    const int off = a.offset[g0], cnt = a.offset[g0 + 1] - off;
    const float* base = a.rec + ((long)off * a.NB + (long)cb * cnt) * kRecWords;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const float* r = base + (long)i * kRecWords;
        const f32x4 h = ld4(r), d0 = ld4(r + 4), d1 = ld4(r + 8);
        const unsigned pk = (unsigned)__float_as_int(h[0]);
        const int x0 = (int)(pk & 0x1fffu) - 1, y0 = (int)((pk >> 13) & 0x1fffu) - 1;
        const unsigned mask = pk >> 26;
        float wt[4];
        mv::tap_weights(h[1], h[2], wt[0], wt[1], wt[2], wt[3]);
        const float dw[8] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int tx = x0 + (k & 1), ty = y0 + (k >> 1);
            if (((mask >> k) & 1u) && (tx >> kRecShiftX) == tile_x && (ty >> kRecShiftY) == tile_y) {
                const int idx = (ty & (kRecTileY - 1)) * kRecTileX + (tx & (kRecTileX - 1));
#pragma unroll
                for (int c = 0; c < 8; ++c) fix_add(&win[c][idx], wt[k] * dw[c], fx.s);
            }
        }
    }
    __syncthreads();
    // the tile's texels, every one exactly once: plain stores, channel-fastest (32 contiguous bytes per texel and block)
    float* gsp = a.grad_src + (long)v * a.src_vs + (long)b * a.src_bs;
    for (int i = threadIdx.x; i < 8 * kRecTileX * kRecTileY; i += 256) {
        const int c = i & 7, tex = i >> 3;
        const int ty = tile_y * kRecTileY + (tex >> kRecShiftX), tx = tile_x * kRecTileX + (tex & (kRecTileX - 1));
        if (ty < a.Hs && tx < a.Ws) gsp[((long)ty * a.Ws + tx) * a.C + cb * 8 + c] = fix_get(win[c][tex], fx.inv);
    }
}

constexpr int kTileR = 4;     // reference rows per workgroup of the tile kernel

// which first-pass kernel a configuration takes, its workgroups per batch item and its window height
static bool bwd_uses_tiles(int C, int G, int D, int fuse_d) {
    return C == 8 && C / G <= 8 && !g_bwd_no_tiles && fuse_d && D <= 8;
}
static int bwd_blocks(int C, int G, int D, int fuse_d, int h, int w) {
    return bwd_uses_tiles(C, G, D, fuse_d) ? ((w + 63) / 64) * ((h + kTileR - 1) / kTileR) : (h * w + 63) / 64;
}

template <int C, int G, bool GROUP>
int launch_bwd(const WarpAggBwdArgs& ba, hipStream_t stream) {
    const WarpAggArgs& a = ba.f;
    const int nblk = bwd_blocks(C, G, a.D, a.fuse_d, a.h, a.w);
    if constexpr (C == 8 && C / G <= 8) {
        if (bwd_uses_tiles(C, G, a.D, a.fuse_d)) {      // the shipped full-resolution stage
            const int tiles_x = (a.w + 63) / 64;
            if (a.D <= 4) {
                MV_NOTE_KERNEL("warp_agg_bwd_tile_kernel<%d, %s, %d, 4>", G, GROUP ? "true" : "false", kTileR);
                hipLaunchKernelGGL((warp_agg_bwd_tile_kernel<G, GROUP, kTileR, 4>), dim3(nblk, a.B), dim3(64, a.D), 0, stream,
                                   ba, tiles_x);
            } else {
                MV_NOTE_KERNEL("warp_agg_bwd_tile_kernel<%d, %s, %d, 8>", G, GROUP ? "true" : "false", kTileR);
                hipLaunchKernelGGL((warp_agg_bwd_tile_kernel<G, GROUP, kTileR, 8>), dim3(nblk, a.B), dim3(64, a.D), 0, stream,
                                   ba, tiles_x);
            }
            if (int rc = mv_check_launch()) return rc;
            return ba.windows ? launch_gather<kTileR + 6, kTileWinX, 1>(ba, nblk, stream) : MVSTER_OK;
        }
    }
    dim3 block(64, a.D);
    dim3 grid(nblk, a.B);
    if (a.D <= 8) {
        MV_NOTE_KERNEL("warp_agg_bwd_kernel<%d, %d, %s, 8>", C, G, GROUP ? "true" : "false");
        hipLaunchKernelGGL((warp_agg_bwd_kernel<C, G, GROUP, 8>), grid, block, 0, stream, ba);
    } else {
        MV_NOTE_KERNEL("warp_agg_bwd_kernel<%d, %d, %s, %d>", C, G, GROUP ? "true" : "false", kMaxD);
        hipLaunchKernelGGL((warp_agg_bwd_kernel<C, G, GROUP, kMaxD>), grid, block, 0, stream, ba);
    }
    if (int rc = mv_check_launch()) return rc;
    return ba.windows ? launch_gather<kWinY, kWinX, C / 8>(ba, nblk, stream) : MVSTER_OK;
}

// K1 of the sorted scatter: the row kernel's REC instance (all channel counts; the 2-D tile kernel's advantage was its
// shared scatter window, which this form does not have)
template <int C, int G, bool GROUP>
int launch_bwd_rec(const WarpAggBwdArgs& ba, hipStream_t stream) {
    const WarpAggArgs& a = ba.f;
    dim3 block(64, a.D);
    dim3 grid((a.h * a.w + 63) / 64, a.B);
    if (a.D <= 8) {
        MV_NOTE_KERNEL("warp_agg_bwd_kernel<%d, %d, %s, 8, true>", C, G, GROUP ? "true" : "false");
        hipLaunchKernelGGL((warp_agg_bwd_kernel<C, G, GROUP, 8, true>), grid, block, 0, stream, ba);
    } else {
        MV_NOTE_KERNEL("warp_agg_bwd_kernel<%d, %d, %s, %d, true>", C, G, GROUP ? "true" : "false", kMaxD);
        hipLaunchKernelGGL((warp_agg_bwd_kernel<C, G, GROUP, kMaxD, true>), grid, block, 0, stream, ba);
    }
    return mv_check_launch();
}

// what both entries fill the same way; the scratch of either form starts out unused
WarpAggBwdArgs make_bwd_args(const float* ref, const float* src, const float* rt, const float* hypo, const float* out,
                             const float* wsum, const float* grad_out, float* grad_ref, float* grad_src, int B, int NV, int C,
                             int D, int h, int w, int Hs, int Ws, long ref_bs, long src_vs, long src_bs, int fuse_d,
                             float attn_temp) {
    WarpAggBwdArgs ba{};
    ba.f = make_warp_args(ref, src, rt, hypo, nullptr, nullptr, B, NV, C, D, h, w, Hs, Ws, ref_bs, src_vs, src_bs, fuse_d, attn_temp);
    ba.fwd_out = out; ba.wsum = wsum; ba.grad_out = grad_out; ba.grad_ref = grad_ref; ba.grad_src = grad_src;
    return ba;
}

// operand maxima of strided batches: one launch per contiguous piece (each reduces into its operand's slot of mx)
void launch_absmax_strided(const WarpAggBwdArgs& ba, long n_go, long n_ref, long n_src, float* mx, hipStream_t s) {
    const WarpAggArgs& a = ba.f;
    launch_absmax(&ba.grad_out, &n_go, 1, mx, s);
    for (int bb = 0; bb < a.B; ++bb) {
        const float* p = a.ref + (long)bb * a.ref_bs;
        launch_absmax(&p, &n_ref, 1, mx + 1, s);
    }
    for (int v = 0; v < a.NV; ++v)
        for (int bb = 0; bb < a.B; ++bb) {
            const float* p = a.src + (long)v * a.src_vs + (long)bb * a.src_bs;
            launch_absmax(&p, &n_src, 1, mx + 2, s);
        }
}

}  // namespace

extern "C" int mvster_warp_agg_bwd_scratch(int B, int NV, int C, int G, int D, int h, int w, int attn_fuse_d,
                                          long* window_floats, long* origin_ints) {
    if (!window_floats || !origin_ints) return MVSTER_ERR_NULL;
    if (B <= 0 || NV <= 0 || C <= 0 || C % 8 || G <= 0 || D <= 0 || h <= 0 || w <= 0) return MVSTER_ERR_SHAPE;
    const long nblk = bwd_blocks(C, G, D, attn_fuse_d, h, w);
    const bool tiles = bwd_uses_tiles(C, G, D, attn_fuse_d);
    *window_floats = (long)B * nblk * NV * (C / 8) * 8 * (tiles ? (kTileR + 6) * kTileWinX : kWinY * kWinX);
    *origin_ints = (long)B * nblk * NV * 2 + 4;      // + the three operand maxima of the fixed-point scale
    return MVSTER_OK;
}

extern "C" int mvster_warp_agg_bwd(const float* ref_feat, const float* src_feat, const float* rt, const float* hypo,
                                   const float* out, const float* wsum, const float* grad_out, float* grad_ref,
                                   float* grad_src, float* windows, int* win_org, int B, int NV, int C, int G, int D, int h,
                                   int w, int Hs, int Ws, long ref_batch_stride, long src_view_stride,
                                   long src_batch_stride, int group_cor, int attn_fuse_d, float attn_temp, void* stream) {
    if (!ref_feat || !src_feat || !rt || !hypo || !out || !wsum || !grad_out || !grad_ref || !grad_src)
        return MVSTER_ERR_NULL;
    if (!win_org) return MVSTER_ERR_NULL;
    if (B <= 0 || NV <= 0 || D <= 0 || D > kMaxD || h <= 0 || w <= 0 || Hs <= 0 || Ws <= 0) return MVSTER_ERR_SHAPE;
    if (!group_cor && G != C) return MVSTER_ERR_SHAPE;
    WarpAggBwdArgs ba = make_bwd_args(ref_feat, src_feat, rt, hypo, out, wsum, grad_out, grad_ref, grad_src, B, NV, C, D, h, w, Hs,
                                      Ws, ref_batch_stride, src_view_stride, src_batch_stride, attn_fuse_d, attn_temp);
    ba.windows = windows; ba.win_org = win_org;
    hipStream_t s = (hipStream_t)stream;
    {
        // operand maxima for the fixed-point scale of the LDS accumulators: the last 4 ints of win_org
        long nf = 0, ni = 0;
        mvster_warp_agg_bwd_scratch(B, NV, C, G, D, h, w, attn_fuse_d, &nf, &ni);
        float* mx = reinterpret_cast<float*>(win_org + (ni - 4));
        // (zeroed by a kernel, not a memset node: see mvster_warp_agg_bwd_sorted)
        hipLaunchKernelGGL(warp_bwd_zero_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<int*>(mx), 4L, reinterpret_cast<int*>(mx), 0L);
        const long n_go = (long)B * D * h * w * G, n_ref = (long)h * w * C, n_src = (long)Hs * Ws * C;
        if (ref_batch_stride == n_ref && src_batch_stride == n_src && src_view_stride == n_src * B) {
            const float* xs[3] = {grad_out, ref_feat, src_feat};
            const long ns[3] = {n_go, n_ref * B, n_src * B * NV};
            launch_absmax(xs, ns, 3, mx, s);
        } else {
            launch_absmax_strided(ba, n_go, n_ref, n_src, mx, s);
        }
        ba.maxima = mx;
    }
    return dispatch_layout(C, G, group_cor != 0, [&](auto c, auto g, auto gr) { return launch_bwd<c(), g(), gr()>(ba, s); });
}

// ------------------------------------------------------------------------------------------------------------------
// mvster_warp_agg_bwd with the source-view gradient accumulated by the SORTED SCATTER (see the section above the kernels):
// no global atomics, bit-reproducible, independent of the smoothness of the depth maps, and grad_src needs no zero fill
// (every texel is written exactly once).  Scratch: rec = *rec_floats floats (the worst case: every sample on a tile corner,
// 4 records per sample and 8-channel block; typically 1.07 are used), ints = *ints ints (tile counts, cursors, offsets and
// the operand maxima of the fixed-point scale).  MVSTER_ERR_UNSUPPORTED for source maps of more than 2048 tiles of 32 x 32
// texels or beyond 8190 texels a side: the caller then takes mvster_warp_agg_bwd.
// ------------------------------------------------------------------------------------------------------------------
extern "C" int mvster_warp_agg_bwd_sorted_scratch(int B, int NV, int C, int D, int h, int w, int Hs, int Ws, long* rec_floats,
                                                 long* ints) {
    if (!rec_floats || !ints) return MVSTER_ERR_NULL;
    if (B <= 0 || NV <= 0 || C <= 0 || C % 8 || D <= 0 || h <= 0 || w <= 0 || Hs <= 0 || Ws <= 0) return MVSTER_ERR_SHAPE;
    const long tiles_x = (Ws + kRecTileX - 1) / kRecTileX, tiles_y = (Hs + kRecTileY - 1) / kRecTileY;
    if (tiles_x * tiles_y > kRecMaxTiles || Hs > 8190 || Ws > 8190) return MVSTER_ERR_UNSUPPORTED;
    const long n = (long)B * NV * tiles_x * tiles_y;
    const long samples = (long)B * h * w * D * NV;
    if (samples * 4 >= (1L << 31)) return MVSTER_ERR_UNSUPPORTED;          // (list positions are 32-bit)
    *rec_floats = samples * 4 * (C / 8) * kRecWords;
    *ints = 3 * n + 1 + 4;
    return MVSTER_OK;
}

extern "C" int mvster_warp_agg_bwd_sorted(const float* ref_feat, const float* src_feat, const float* rt, const float* hypo,
                                          const float* out, const float* wsum, const float* grad_out, float* grad_ref,
                                          float* grad_src, float* rec, int* ints, int B, int NV, int C, int G, int D, int h,
                                          int w, int Hs, int Ws, long ref_batch_stride, long src_view_stride,
                                          long src_batch_stride, int group_cor, int attn_fuse_d, float attn_temp, void* stream) {
    if (!ref_feat || !src_feat || !rt || !hypo || !out || !wsum || !grad_out || !grad_ref || !grad_src || !rec || !ints)
        return MVSTER_ERR_NULL;
    if (B <= 0 || NV <= 0 || D <= 0 || D > kMaxD || h <= 0 || w <= 0 || Hs <= 0 || Ws <= 0) return MVSTER_ERR_SHAPE;
    if (!group_cor && G != C) return MVSTER_ERR_SHAPE;
    long nf = 0, ni = 0;
    if (int rc = mvster_warp_agg_bwd_sorted_scratch(B, NV, C, D, h, w, Hs, Ws, &nf, &ni)) return rc;
    const int tiles_x = (Ws + kRecTileX - 1) / kRecTileX, tiles_y = (Hs + kRecTileY - 1) / kRecTileY;
    const long n = (long)B * NV * tiles_x * tiles_y;
    int* count = ints;
    int* cursor = ints + n;
    int* offset = ints + 2 * n;
    float* mx = reinterpret_cast<float*>(ints + 3 * n + 1);
    WarpAggBwdArgs ba = make_bwd_args(ref_feat, src_feat, rt, hypo, out, wsum, grad_out, grad_ref, grad_src, B, NV, C, D, h, w, Hs,
                                      Ws, ref_batch_stride, src_view_stride, src_batch_stride, attn_fuse_d, attn_temp);
    const WarpAggArgs& a = ba.f;
    ba.maxima = mx;
    ba.rec_offset = offset; ba.rec_cursor = cursor; ba.rec = rec; ba.tiles_x = tiles_x; ba.tiles_y = tiles_y;
    hipStream_t s = (hipStream_t)stream;
    // counts, cursors and the operand maxima start at zero: a kernel of our own, not hipMemsetAsync -- inside a captured
    // training step the memset node was seen to race with the kernels around it (garbage counts -> a memory fault on a
    // later replay); kernel nodes of one stream are strictly ordered
    hipLaunchKernelGGL(warp_bwd_zero_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, s, ints, 2 * n,
                       reinterpret_cast<int*>(mx), 4L);
    const long per_item = (long)h * w * D;
    const long per_b = (per_item + 255) / 256;
    {
        const long n_go = (long)B * D * h * w * G, n_ref = (long)h * w * C, n_src = (long)Hs * Ws * C;
        if (ref_batch_stride == n_ref && src_batch_stride == n_src && src_view_stride == n_src * B &&
            per_b * B < (1L << 30)) {
            // (contiguous operands: the maxima and the counting pass share a launch)
            const float* xs[3] = {grad_out, ref_feat, src_feat};
            const long ns[3] = {n_go, n_ref * B, n_src * B * NV};
            const AbsMaxArgs am = absmax_args(xs, ns, 3);
            hipLaunchKernelGGL(warp_bwd_prep_kernel, dim3((unsigned)(am.first[3] + per_b * B)), dim3(256), 0, s, a, count, tiles_x,
                               tiles_y, am, mx, am.first[3], (int)per_b);
        } else {
            launch_absmax_strided(ba, n_go, n_ref, n_src, mx, s);
            hipLaunchKernelGGL(warp_bwd_count_kernel, dim3((unsigned)per_b, B), dim3(256), 0, s, a, count, tiles_x, tiles_y);
        }
    }
    hipLaunchKernelGGL(warp_bwd_scan_kernel, dim3(1), dim3(1024), 0, s, count, offset, (int)n);
    if (int rc = dispatch_layout(C, G, group_cor != 0, [&](auto c, auto g, auto gr) { return launch_bwd_rec<c(), g(), gr()>(ba, s); }))
        return rc;
    WarpBwdAccumArgs k2{rec, offset, mx, grad_src, src_view_stride, src_batch_stride, NV, C / 8, C, Hs, Ws, tiles_x, tiles_y,
                        G, D, C / G, group_cor ? 1 : 0, attn_fuse_d ? 1 : 0, attn_temp};
    hipLaunchKernelGGL(warp_bwd_accum_kernel, dim3(tiles_x * tiles_y, NV * (C / 8), B), dim3(256), 0, s, k2);
    return mv_check_launch();
}
