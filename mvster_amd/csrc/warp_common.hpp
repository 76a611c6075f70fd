// What the warp kernels' translation units share: the launch arguments, the plain / indexed / counted address helpers, the
// device code that more than one kernel form repeats, and the host-side argument filling and (C, G, GROUP) dispatch.
//   warp_fwd.hip          forward forms (one-thread, lane-split, wave-local), their launchers and C entries
//   warp_fwd_probes.hpp   the forward forms kept for the record (pixel-major, LDS-window): probe build only
//   warp_bwd.hip          backward: window form, sorted scatter, their C entries
// Everything is in the anonymous namespace: each unit gets its own copy and the kernels keep their symbol names.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

#include "common.hpp"

namespace {

constexpr int kMaxD = 16;
constexpr int kMaxFwdD = 64;      // forward only (warp_agg_fwd_kernel with fewer pixels per workgroup)

struct WarpAggArgs {
    const float* ref;
    const float* src;
    const float* rt;
    const float* hypo;
    float* out;
    float* wsum_out;  // optional [B, D, h, w] (saved for the backward pass)
    long ref_bs;      // batch stride of ref (elements)
    long src_vs;      // view stride of src
    long src_bs;      // batch stride of src
    int B, NV, D, h, w, Hs, Ws;
    float attn_temp;
    float sqrt_c;
    int fuse_d;
    // fused hypothesis scheduling (wave-local kernel, SCHED != 0): the hypotheses are computed here instead of read, and
    // written to hypo_out [B, D, h, w] for the stage's selection and the API
    const float* inv_min;    // SCHED 1: previous stage's inverse_min_depth [B, h/2, w/2]
    const float* inv_max;    //          ... inverse_max_depth
    const float* dvals;      // SCHED 2: depth_values [B, ndv] (first and last column = the range)
    float* hypo_out;
    int ndv;
    // indexed form (mvster_warp_agg_fwd_indexed): ref = src = a level store [V, h, w, C] holding every view of a scan, and
    // batch item b reads maps views[b * (1 + NV) + 0] (reference) and [.. + 1 + v] (source v) of it
    const int* views;        // DEVICE table [B, 1 + NV]; nullptr in the plain forms
    long store_vs;           // view stride of the store (elements)
    // counted forms (mvster_warp_agg_fwd_counted / _indexed_counted): batch item b aggregates its first nsrc[b] sources; NV
    // stays the capacity (the strides of rt and of the table), and nothing of the slots v >= nsrc[b] is read
    const int* nsrc = nullptr;   // DEVICE [B], 1 <= nsrc[b] <= NV; nullptr: every item uses all NV sources
};

// Base address of a view's map: the ONLY difference between the plain and the indexed launch forms.  The table entry is
// uniform over the workgroup (b = blockIdx.y, v = the loop counter), i.e. one scalar load per view.
template <bool IDX>
__device__ __forceinline__ const float* ref_base(const WarpAggArgs& a, int b) {
    if constexpr (IDX) return a.ref + (long)a.views[b * (a.NV + 1)] * a.store_vs;
    else return a.ref + (long)b * a.ref_bs;
}
template <bool IDX>
__device__ __forceinline__ const float* src_base(const WarpAggArgs& a, int b, int v) {
    if constexpr (IDX) return a.src + (long)a.views[b * (a.NV + 1) + 1 + v] * a.store_vs;
    else return a.src + (long)v * a.src_vs + (long)b * a.src_bs;
}

// Sources of batch item b: uniform over the workgroup (b = blockIdx.y), one scalar load ahead of the view loop.
__device__ __forceinline__ int source_count(const WarpAggArgs& a, int b) { return a.nsrc ? a.nsrc[b] : a.NV; }

// Forms whose INDEXED instantiation leaves the register budget class of the plain one (compiler's counts, gfx950, -O3:
// one-thread form at C = 16: 72-80 -> 84-106 VGPRs, 6-7 -> 4-5 waves per SIMD; lane-split form at (16, 8) and (64, 8):
// 71 / 67 -> 79 / 73 VGPRs, 7 -> 6 waves).  They are not instantiated: the indexed entry answers MVSTER_ERR_UNSUPPORTED and
// the caller gathers the maps (mvster_gather_views) for the plain entry.  None of them is a kernel of the shipped cascade.
template <int C>
constexpr bool kIndexedOneThread = C != 16;
template <int C, int G>
constexpr bool kIndexedLanes = !((C == 16 && G == 8) || (C == 64 && G == 8));

// ---- device code that several kernel forms repeat, written once -------------------------------------------------------
// Macros on purpose.  As __forceinline__ functions the same statements reach the optimiser already simplified on their own,
// it then orders their uses differently, and the kernels' bytes change (the rt load alone: 184 of the 200 kernels, operands
// of commutative VALU instructions swapped -- the same arithmetic, but no longer the code object that was measured).  A
// macro expands to the very statements the forms used to spell out.  Names ending in _ are the macros' own.

// mv::RT m = relative projection of (batch item b, source v): rt row [rot(9), trans(3)]; wave-uniform, so scalar loads
#define MV_LOAD_RT(m, a, b, v)                                                      \
    mv::RT m;                                                                       \
    {                                                                               \
        const float* r_ = (a).rt + ((long)(b) * (a).NV + (v)) * 12;                 \
        _Pragma("unroll") for (int i_ = 0; i_ < 9; ++i_) m.r[i_] = r_[i_];          \
        _Pragma("unroll") for (int i_ = 0; i_ < 3; ++i_) m.t[i_] = r_[9 + i_];      \
    }

// Blend and correlate channels c, c + 1 of a lane's 8-channel slice (packed fp32 on the pairs the 16-byte loads deliver:
// elements j, j + 1 of the four taps A..Dq and of the reference R) and add them to their groups' sums part[] in channel
// order; CG is the kernel's constant.  MV_CORRELATE_SLICE: all eight channels, q0 / q1 = the two quads of tap nw, q2 / q3 of
// ne, q4 / q5 of sw, q6 / q7 of se.
#define MV_PAIR(part, nw, ne, sw, se, c, A, B, Cq, Dq, R, j)                                                   \
    {                                                                                                          \
        const mv::f32x2 wv = mv::blend2(nw, ne, sw, se, (mv::f32x2){A[j], A[j + 1]},                           \
                                        (mv::f32x2){B[j], B[j + 1]}, (mv::f32x2){Cq[j], Cq[j + 1]},            \
                                        (mv::f32x2){Dq[j], Dq[j + 1]});                                        \
        const mv::f32x2 p2 = mv::mul_rn2(wv, (mv::f32x2){R[j], R[j + 1]});                                     \
        part[(c) / CG] = ((c) % CG == 0) ? p2[0] : mv::add_rn(part[(c) / CG], p2[0]);                          \
        part[((c) + 1) / CG] = (((c) + 1) % CG == 0) ? p2[1] : mv::add_rn(part[((c) + 1) / CG], p2[1]);        \
    }
#define MV_CORRELATE_SLICE(part, nw, ne, sw, se, q0, q1, q2, q3, q4, q5, q6, q7, R0, R1) \
    MV_PAIR(part, nw, ne, sw, se, 0, q0, q2, q4, q6, R0, 0)                              \
    MV_PAIR(part, nw, ne, sw, se, 2, q0, q2, q4, q6, R0, 2)                              \
    MV_PAIR(part, nw, ne, sw, se, 4, q1, q3, q5, q7, R1, 0)                              \
    MV_PAIR(part, nw, ne, sw, se, 6, q1, q3, q5, q7, R1, 2)

// float score = the G correlations of one (pixel, d) -- GPL per lane in cg[], all-gathered over the LPP neighbouring lanes
// from lane0 that share it -- summed in group order: .sum(1), the same bits in every lane-split form as in the one-thread
// form.  LPP and GPL are the kernel's constants.
#define MV_GROUP_SCORE(score, cg, lane0)                                                        \
    float score = 0.0f;                                                                         \
    {                                                                                           \
        const int lane0_ = (lane0);                                                             \
        _Pragma("unroll") for (int j_ = 0; j_ < LPP; ++j_)                                      \
            _Pragma("unroll") for (int k_ = 0; k_ < GPL; ++k_) {                                \
                const float val_ = LPP == 1 ? (cg)[k_] : __shfl((cg)[k_], lane0_ + j_);         \
                score = (j_ == 0 && k_ == 0) ? val_ : mv::add_rn(score, val_);                  \
            }                                                                                   \
    }

// float wgt = attention weight of (pixel, d) by the workgroup-level softmax over depth of the one-thread and the lane-split
// form: row d publishes its score (a float variable; divided by attn_temp here) in column col of buf = sc[v & 1]
// (double-buffered by view parity, hence one barrier per view) and every thread reduces the D scores of its column.
#define MV_DEPTH_SOFTMAX(wgt, a, buf, d, col, publish, score)                                                     \
    float wgt;                                                                                                    \
    {                                                                                                             \
        if ((a).fuse_d) score = mv::div_rn(score, (a).attn_temp);                                                 \
        auto* buf_ = (buf);                                                                                       \
        if (publish) buf_[d][col] = score;                                                                        \
        __syncthreads();                                                                                          \
        float mx_ = buf_[0][col];                                                                                 \
        for (int j_ = 1; j_ < (a).D; ++j_) mx_ = fmaxf(mx_, buf_[j_][col]);                                       \
        float den_ = 0.0f;                                                                                        \
        for (int j_ = 0; j_ < (a).D; ++j_) den_ = mv::add_rn(den_, expf(mv::sub_rn(buf_[j_][col], mx_)));         \
        if ((a).fuse_d)                                                                                           \
            wgt = mv::div_rn(mv::div_rn(expf(mv::sub_rn(score, mx_)), den_), (a).sqrt_c);                         \
        else                                                                                                      \
            wgt = mv::div_rn(1.0f, den_); /* max_d softmax = exp(0) / sum */                                      \
    }

// ---- host side ----------------------------------------------------------------------------------------------------------

// The arguments every entry fills the same way; the scheduling, indexed and counted fields start out unused.
inline WarpAggArgs make_warp_args(const float* ref, const float* src, const float* rt, const float* hypo, float* out,
                                  float* wsum_out, int B, int NV, int C, int D, int h, int w, int Hs, int Ws, long ref_bs,
                                  long src_vs, long src_bs, int fuse_d, float attn_temp) {
    WarpAggArgs a{};
    a.ref = ref; a.src = src; a.rt = rt; a.hypo = hypo; a.out = out; a.wsum_out = wsum_out;
    a.ref_bs = ref_bs; a.src_vs = src_vs; a.src_bs = src_bs;
    a.B = B; a.NV = NV; a.D = D; a.h = h; a.w = w; a.Hs = Hs; a.Ws = Ws;
    a.attn_temp = attn_temp; a.sqrt_c = sqrtf((float)C); a.fuse_d = fuse_d;
    return a;
}

// The (C, G, GROUP) layouts the one-thread forward and both backward forms are instantiated for: f(C, G, GROUP) is called
// with the matching compile-time constants; MVSTER_ERR_UNSUPPORTED for every other layout.
template <class F>
int dispatch_layout(int C, int G, bool group, F&& f) {
#define MV_CASE(CC, GG, GR)                   \
    if (C == CC && G == GG && group == GR)    \
        return f(std::integral_constant<int, CC>{}, std::integral_constant<int, GG>{}, std::bool_constant<GR>{});
    MV_CASE(64, 8, true)
    MV_CASE(32, 8, true)
    MV_CASE(16, 4, true)
    MV_CASE(8, 4, true)
    MV_CASE(16, 8, true)
    MV_CASE(8, 8, true)
    MV_CASE(64, 4, true)
    MV_CASE(32, 4, true)
    MV_CASE(8, 8, false)
    MV_CASE(16, 16, false)
    MV_CASE(32, 32, false)
    MV_CASE(64, 64, false)
#undef MV_CASE
    return MVSTER_ERR_UNSUPPORTED;
}

}  // namespace
