/* C ABI of libmvster_hip.so -- the gfx950 kernels of the MVSTER cost-volume hot path.
 *
 * The reference (JeffWang987/MVSTER) is pure Python/PyTorch and has no FFI of its own; the
 * drop-in boundary is its Python module API (models/__init__.py:2, models/MVS4Net.py:9-111),
 * mirrored by the `mvster_amd` package, which calls the entry points below through ctypes
 * with raw device pointers (mvster_amd/_lib.py).  Each entry point names the reference code it
 * replaces (file:line under the reference tree).
 *
 * Conventions: every pointer is a DEVICE pointer to contiguous fp32 unless stated otherwise;
 * buffers are caller-owned; nothing is allocated, copied to the host or synchronised inside;
 * `stream` is a hipStream_t (NULL = default stream); the return value is 0 or a negative
 * MVSTER_ERR_* code.  All functions are stateless and re-entrant.
 */
#ifndef MVSTER_HIP_H
#define MVSTER_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MVSTER_OK 0
#define MVSTER_ERR_NULL (-1)        /* a required pointer is NULL */
#define MVSTER_ERR_SHAPE (-2)       /* inconsistent or out-of-range sizes */
#define MVSTER_ERR_UNSUPPORTED (-3) /* no kernel instance for this channel / tile combination */
#define MVSTER_ERR_LAUNCH (-4)      /* hipGetLastError() != hipSuccess after the launch */

/* proj_matrices [B,N,2,4,4] (extrinsic, intrinsic) -> rt [B,N-1,12]: rows 0..2 of
 * src_P @ inverse(ref_P) as rot(9)+trans(3), with X_P = K[:3,:3] @ E[:3,:4] (row 3 from E).
 * Replaces models/mvs4net_utils.py:1032-1035 (K@[R|t]) and :24-26 (inverse + matmul). */
int mvster_relative_projection(const float* proj_matrices, float* rt, int B, int N, void* stream);

/* Same for several cascade stages in one launch: proj_matrices = HOST array of nstage device pointers
 * (each [B,N,2,4,4]); rt [nstage,B,N-1,12]. */
int mvster_relative_projection_multi(const float* const* proj_matrices, int nstage, float* rt, int B, int N,
                                     void* stream);

/* imgs = HOST array of N device pointers, each [B,3,H,W] (the reference's `imgs` list, MVS4Net.py:60) ->
 * out [N*B,H,W,4] channels-last RGB0, view-major: the batch FPN4 runs on. */
int mvster_pack_images(const float* const* imgs, int N, float* out, int B, int H, int W, void* stream);

/* imgs uint8 [V,H,W,3] (what an image file decodes to; 4-byte aligned) -> out [V,1,H,W,4] float RGB0, value u8 / 255 with a
 * true division: the bits of read_img (datasets/general_eval4.py:81-86) followed by mvster_pack_images, for a whole scan in
 * one launch and from a quarter of the bytes. */
int mvster_pack_images_u8(const unsigned char* imgs, float* out, int V, int H, int W, void* stream);

/* mvster_pack_images_u8 with the image preparation of the reference's three evaluation loaders in the same pass, for a whole
 * scan in one launch: the input scaling of datasets/general_eval4.py:92-109 (cv2.resize with default arguments -- bilinear,
 * on read_img's floats), a crop (datasets/tanks.py:53-60) and a resize of every view from its own native size to one target
 * (datasets/eth3d.py:57-62).  buf: one ragged byte buffer (16-byte aligned, buf_bytes long) holding the decoded uint8
 * [Hs_v,Ws_v,3] images.  desc: V descriptors of 12 32-bit words each, on the DEVICE; desc_host: the same bytes on the HOST,
 * which is what is validated before the launch.  Words: [0],[1] byte offset of the image in buf (low, high; a multiple of
 * 16), [2] Hs, [3] Ws, [4] y0, [5] x0, [6] hw, [7] ww = the source window (the crop), [8] word offset into `tables` of that
 * window size's tap tables (a multiple of 4), [9] area flag: non-zero exactly where ww == 2 Wd and hw == 2 Hd (per view),
 * [10],[11] zero.  tables: table_words 32-bit words (16-byte aligned; may be NULL with table_words == 0).  One tap table is
 * 2 Wd + 2 Hd words -- first tap sx [Wd] (int32), fraction fx [Wd] (float32), then sy [Hd], fy [Hd] -- built on the host
 * for hw x ww -> Hd x Wd as OpenCV builds xofs / alpha (mvster_amd.formats.resize_tables), tap indices relative to the
 * window; arithmetic in csrc/resize_math.h.  Where the area flag is set, the 2 x 2 mean of OpenCV's area path.
 * out [V,1,Hd,Wd,4] float RGB0 and, where out_u8 is not NULL, out_u8 [V,Hd,Wd,3] = trunc(clip(x * 255, 0, 255)), the pixels
 * test_mvs4.py:262-264 writes to images/.  A window of hw == Hd and ww == Wd reads no table and gives the bits of
 * mvster_pack_images_u8 on the cropped image, whatever the alignment of its first byte and of the row pitch 3 Ws.  No path
 * enlarges: Hd > hw or Wd > ww is MVSTER_ERR_SHAPE, as are Hd / Wd that are not positive multiples of 64, an image that does
 * not lie inside buf, a window that does not lie inside its image, a table range outside `tables`, an area flag that does
 * not match the sizes, and V > 65535.  The tables are trusted for the values, not for the addresses: tap indices are
 * clamped into the window. */
int mvster_load_pack_images_u8(const unsigned char* buf, long buf_bytes, const int* desc_host, const int* desc, const void* tables,
                               long table_words, float* out, unsigned char* out_u8, int V, int Hd, int Wd, void* stream);

/* The three launches a forward starts with in one (MVS4Net.py:60-76): mvster_pack_images (imgs -> packed),
 * mvster_relative_projection_multi (proj_matrices -> rt) and mvster_init_range (depth_values [B,ndv] -> hypo [B,D,h,w], the
 * first stage's hypotheses; h*w <= H*W).  Same arithmetic as the three, bit for bit. */
int mvster_forward_prologue(const float* const* imgs, int N, float* packed, int B, int H, int W,
                            const float* const* proj_matrices, int nstage, float* rt, const float* depth_values, int ndv,
                            float* hypo, int D, int h, int w, int inverse, void* stream);

/* Fused homography warp + group-wise (or squared-difference) correlation + epipolar attention
 * aggregation over all NV source views.  Channels-last features:
 *   ref_feat [B,h,w,C] (batch stride given), src_feat view v / batch b at
 *   src_feat + v*src_view_stride + b*src_batch_stride as [Hs,Ws,C];
 *   rt [B,NV,12]; hypo [B,D,h,w]; out [B,D,h,w,G]; wsum_out optional [B,D,h,w].
 * group_cor=0 requires G == C.  variant: 0 = choose (the wave-local kernel whenever group_cor, D in {4, 8}
 * and C in {8, 16, 32, 64}); 1 = one thread per (pixel, d); 2 = workgroup-level lane split (C >= 16);
 * 3 = wave-local.  All forms return the same bits.  Replaces models/mvs4net_utils.py:13-59 (homo_warping),
 * :1037-1042 (correlation), :1048-1060 (attention aggregation). */
int mvster_warp_agg_fwd(const float* ref_feat, const float* src_feat, const float* rt, const float* hypo,
                        float* out, float* wsum_out, int B, int NV, int C, int G, int D, int h, int w, int Hs,
                        int Ws, long ref_batch_stride, long src_view_stride, long src_batch_stride, int group_cor,
                        int attn_fuse_d, float attn_temp, int variant, void* stream);

/* mvster_warp_agg_fwd reading its maps by index from a LEVEL STORE [V,h,w,C] (one pyramid level of every view of a scan):
 * the reference map of batch item b is map views[b][0] of the store and its NV source maps are views[b][1..NV]; `views`
 * is a DEVICE int32 table [B,1+NV] (a captured graph is replayed for another reference view after updating the table).
 * Repeated indices are legal.  Same kernels (one template parameter apart: how a view's base address is formed), same
 * (C, G, D, group_cor, attn_fuse_d, variant 0..3) combinations and the same bits as mvster_warp_agg_fwd on a gathered
 * copy.  The indices are NOT checked on the device: the caller validates 0 <= index < V before uploading them.
 * MVSTER_ERR_UNSUPPORTED (-3) where the plain entry returns it, and for the kernel forms whose indexed instantiation would
 * leave the plain one's register budget class (one thread per (pixel, d) at C = 16; the lane-split form at (C, G) = (16, 8)
 * and (64, 8) -- none of them in the shipped cascade): mvster_gather_views + mvster_warp_agg_fwd there. */
int mvster_warp_agg_fwd_indexed(const float* store, const int* views, const float* rt, const float* hypo, float* out,
                                float* wsum_out, int V, int B, int NV, int C, int G, int D, int h, int w, int group_cor,
                                int attn_fuse_d, float attn_temp, int variant, void* stream);

/* mvster_warp_agg_fwd / mvster_warp_agg_fwd_indexed with a source count per batch item: `nsrc` is a DEVICE int32 array [B]
 * and item b aggregates its first nsrc[b] sources, 1 <= nsrc[b] <= NV (NOT checked on the device: the caller validates the
 * counts before uploading them).  NV stays the capacity: rt is [B,NV,12] and the table [B,1+NV] with the same strides, and
 * nothing of the slots v >= nsrc[b] is read -- neither their rt rows, nor their table entries, nor their maps.  One captured
 * graph therefore serves reference views with any number of sources up to NV.  Same kernels and combinations as the
 * uncounted entries (the count is the bound of their view loop, one scalar load per workgroup); with count n the bits of the
 * uncounted entry called with NV = n on the first n sources.  MVSTER_ERR_NULL (-1) also for nsrc == NULL;
 * MVSTER_ERR_UNSUPPORTED (-3) where the uncounted entries return it. */
int mvster_warp_agg_fwd_counted(const float* ref_feat, const float* src_feat, const float* rt, const float* hypo,
                                float* out, float* wsum_out, int B, int NV, int C, int G, int D, int h, int w, int Hs,
                                int Ws, long ref_batch_stride, long src_view_stride, long src_batch_stride, int group_cor,
                                int attn_fuse_d, float attn_temp, int variant, const int* nsrc, void* stream);
int mvster_warp_agg_fwd_indexed_counted(const float* store, const int* views, const float* rt, const float* hypo, float* out,
                                        float* wsum_out, int V, int B, int NV, int C, int G, int D, int h, int w,
                                        int group_cor, int attn_fuse_d, float attn_temp, int variant, const int* nsrc,
                                        void* stream);

/* Maps views[b][k] (DEVICE int32 table [B,N], unchecked) of a level store [V, map_floats] -> out [N,B,map_floats]: the
 * view-major batch mvster_warp_agg_fwd reads (ref_feat = out, src_feat = out + B*map_floats).  map_floats % 4 == 0. */
int mvster_gather_views(const float* store, const int* views, float* out, int V, int B, int N, long map_floats, void* stream);

/* mvster_warp_agg_fwd with the stage's depth-hypothesis scheduling fused in: one launch instead of
 * (mvster_schedule_inverse_range | mvster_init_range) + mvster_warp_agg_fwd.  mode 1: the hypotheses are
 * schedule_inverse_range(inv_min, inv_max) of the previous stage's bounds [B,h/2,w/2] (models/mvs4net_utils.py:79-86);
 * mode 2: init_inverse_range of depth_values [B,ndv] (:71-77).  hypo_out [B,D,h,w] receives them, bit-identical to the
 * scheduler kernels' (the stage's selection and the API's `hypo_depth` read it).  Group correlation on the wave-local
 * kernel only: D in {4, 8}, (C, G) in {(8,4), (16,4), (32,8), (64,8)} -- the shipped cascade; MVSTER_ERR_UNSUPPORTED (-3)
 * otherwise: run the two launches.  Other arguments as mvster_warp_agg_fwd.  Reference call site: models/MVS4Net.py:88-99. */
int mvster_warp_agg_fwd_sched(const float* ref_feat, const float* src_feat, const float* rt, const float* inv_min,
                              const float* inv_max, const float* depth_values, int ndv, float* hypo_out, float* out,
                              float* wsum_out, int B, int NV, int C, int G, int D, int h, int w, int Hs, int Ws,
                              long ref_batch_stride, long src_view_stride, long src_batch_stride, int attn_fuse_d,
                              float attn_temp, int mode, void* stream);

/* Backward of mvster_warp_agg_fwd w.r.t. the features (the sampling grid carries no gradient,
 * models/mvs4net_utils.py:23).  grad_out/out [B,D,h,w,G], wsum [B,D,h,w] from the forward; both attention forms,
 * D <= 16.  grad_ref [B,h,w,C] is written; grad_src [NV][B,Hs,Ws,C] must be zero-initialised.
 * windows / win_org: scratch of the sizes mvster_warp_agg_bwd_scratch() reports (floats / ints, uninitialised).
 * win_org is required (it also holds the operand maxima of the fixed-point scale of the LDS accumulators).  With
 * `windows` the source gradient is accumulated without floating-point atomics for every tap inside a workgroup's
 * scatter window (integer LDS accumulation, dense windows, a gather pass in fixed order: bit-reproducible); with
 * windows == NULL the windows are flushed with global fp32 atomics.  Taps outside a window (strongly rotated views)
 * always use global atomics.
 * Autograd of models/mvs4net_utils.py:1036-1060. */
int mvster_warp_agg_bwd(const float* ref_feat, const float* src_feat, const float* rt, const float* hypo,
                        const float* out, const float* wsum, const float* grad_out, float* grad_ref,
                        float* grad_src, float* windows, int* win_org, int B, int NV, int C, int G, int D, int h, int w,
                        int Hs, int Ws, long ref_batch_stride, long src_view_stride, long src_batch_stride, int group_cor,
                        int attn_fuse_d, float attn_temp, void* stream);
int mvster_warp_agg_bwd_scratch(int B, int NV, int C, int G, int D, int h, int w, int attn_fuse_d, long* window_floats,
                                long* origin_ints);

/* mvster_warp_agg_bwd with the source-view gradient accumulated by a SORTED SCATTER instead of scatter windows + global
 * atomics (the adjoint of F.grid_sample in homo_warping, models/mvs4net_utils.py:13-59): the (pixel, hypothesis, view)
 * samples are counting-sorted by 32x32 source tile (count, prefix sums, 48-byte records appended per touched tile), then one
 * workgroup per (batch, view, 8-channel block, tile) accumulates its records in a 64-bit fixed-point LDS window and writes
 * the tile with plain stores.  Bit-reproducible, independent of the smoothness of the depth maps; grad_src needs NO zero
 * fill (every texel is written exactly once).  Same arguments as mvster_warp_agg_bwd except the scratch: rec (*rec_floats
 * floats: the worst case of 4 records per sample and channel block) and ints (*ints ints) as sized by the _scratch query.
 * MVSTER_ERR_UNSUPPORTED (from both) for source maps of more than 2048 tiles or 8190 texels a side: use mvster_warp_agg_bwd. */
int mvster_warp_agg_bwd_sorted_scratch(int B, int NV, int C, int D, int h, int w, int Hs, int Ws, long* rec_floats, long* ints);
int mvster_warp_agg_bwd_sorted(const float* ref_feat, const float* src_feat, const float* rt, const float* hypo,
                               const float* out, const float* wsum, const float* grad_out, float* grad_ref, float* grad_src,
                               float* rec, int* ints, int B, int NV, int C, int G, int D, int h, int w, int Hs, int Ws,
                               long ref_batch_stride, long src_view_stride, long src_batch_stride, int group_cor,
                               int attn_fuse_d, float attn_temp, void* stream);

/* depth_values [B,ndv] (columns 0 and ndv-1 used) -> out [B,D,h,w].
 * inverse=1: models/mvs4net_utils.py:71-77 (init_inverse_range); inverse=0: :61-69 (init_range). */
int mvster_init_range(const float* depth_values, int ndv, float* out, int B, int D, int h, int w, int inverse,
                      void* stream);

/* inv_min, inv_max [B,h/2,w/2] -> out [B,D,h,w].  models/mvs4net_utils.py:79-86. */
int mvster_schedule_inverse_range(const float* inv_min, const float* inv_max, float* out, int B, int D, int h,
                                  int w, void* stream);

/* cur_depth [B,h/2,w/2], interval [B] (device) -> out [B,D,h,w].  models/mvs4net_utils.py:88-99. */
int mvster_schedule_range(const float* cur_depth, const float* interval, float* out, int B, int D, int h, int w,
                          void* stream);

/* (optional 1x1x1 `prob` head) + softmax over D + first-max argmax + gather + max-prob confidence
 * + inverse-depth bounds.  Either logits [B,D,h,w] or feat [B,D,h,w,CF] (+ prob_w [CF], prob_b [1]).
 * attn [B,D,h,w], depth/conf/inv_min/inv_max [B,h,w] (conf, inv_* optional; inv_* need D >= 3),
 * logits_out optional [B,D,h,w].  models/mvs4net_utils.py:900 and :1068-1088. */
int mvster_select_depth(const float* logits, const float* feat, const float* prob_w, const float* prob_b, int CF,
                        const float* hypo, float* attn, float* depth, float* conf, float* inv_min, float* inv_max,
                        float* logits_out, int B, int D, int h, int w, float split_itv, void* stream);

/* Backward of mvster_select_depth's differentiable part (training): the 1x1x1 `prob` head + softmax over depth with respect
 * to the feature volume and the head's parameters, given gattn = d L / d attn [B,D,h,w] (depth, confidence and the
 * inverse bounds carry no gradient: argmax / detached in the reference, models/mvs4net_utils.py:1068-1088).
 * dfeat [B,D,h,w,CF] = dlogit * prob_w; partial [B * ceil(h*w/256), CF + 1] = per-workgroup sums of dlogit * feat (d prob_w)
 * and of dlogit (d prob_b): the caller adds the rows.  CF = 8, D <= 16. */
int mvster_select_depth_bwd(const float* attn, const float* gattn, const float* feat, const float* prob_w, float* dfeat,
                            float* partial, int B, int D, int h, int w, int CF, void* stream);

/* in [B,hi,wi] -> out [B,ho,wo], bilinear, align_corners=True.  models/mvs4net_utils.py:1077. */
int mvster_upsample_bilinear(const float* in, float* out, int B, int hi, int wi, int ho, int wo, void* stream);

/* n <= 8 maps of one batch to one output size in one launch: ins / outs / his / wis = HOST arrays (device pointers,
 * input sizes); ins[k] [B,his[k],wis[k]] -> outs[k] [B,ho,wo].  The coarse stages' confidence maps (MVS4Net.py:1077 per stage). */
int mvster_upsample_bilinear_multi(const float* const* ins, float* const* outs, const int* his, const int* wis, int n, int B,
                                   int ho, int wo, void* stream);

/* Channels-last implicit-GEMM convolution on the fp32 matrix cores with a fused
 * scale/shift (+ReLU, +skip) epilogue.  in [B,Di,Hi,Wi,cin]; wpk = weights packed by
 * mvster_amd/conv_plan.py; scale/shift [16*ntiles]; skip optional; zeros = >=16 B of zeros;
 * geom = HOST int32 array (layout: conv_plan.GEOM), woff = HOST int64 per-class weight offsets.
 * prob_w [8] / prob_b [1] (optional, cout == 8, variants 0/2): fuse the 1x1x1 `prob` head of reg2d
 * (models/mvs4net_utils.py:900) -- `out` is then the [B,Do,Ho,Wo] logits volume instead of the feature volume.
 * variant 0 = direct (operands from L1), 1 = LDS-staged input patch (ordinary convs, cin % 16 == 0,
 * mt in {2,4}: the workgroup tile is 2*mt rows x 32 columns), 2 = direct with the 4 waves of a workgroup
 * splitting K (small deep layers; cin >= 16, mt*nt <= 4), 5 = persistent workgroups with LDS-DMA double-buffered
 * input patches and workgroup-resident weights (ordinary convs, cin in {16, 32, 64}, cout % 16 == 0, kernels
 * (1|3)x3x3 and 1x5x5, in-plane stride 1 or 2, mt = 2; bits 8.. of `variant` = workgroups per CU, 0 = default),
 * 6 = persistent 1x1x1 kernel with all packed weights resident in LDS and the input read once (cin in {32, 64},
 * cout % 4 == 0, optional same-shape skip; nt is ignored: a wave walks all N tiles),
 * 7 = variant 5 with eight waves per workgroup in ping-pong (3x3, cin 16 / 32; measured no faster, kept for the record),
 * 8 = Winograd F(2x2, 3x3) on the persistent LDS-DMA frame: 1x3x3 stride 1 pad 1, cin in {16, 32}, cout % 16 == 0,
 * optional same-shape skip; `wpk` must be the array written by mvster_pack_wino_weights (not bit-identical to the other
 * variants: fp32 with a different operation order),
 * 9 = the same transform for deep layers: (1|3)x3x3 stride 1, cin in {16, 32, 64}; patch slices and transformed weights
 * stream through LDS rings one depth tap and 16-channel chunk at a time.
 * Conv3d/ConvTranspose3d/BatchNorm3d/ReLU of reg2d/reg3d (models/mvs4net_utils.py:870-965) and
 * Conv2d/BatchNorm2d/ReLU/upsample-add of FPN4 (:419-502). */
int mvster_conv_mfma(const float* in, const float* wpk, const float* scale, const float* shift, const float* skip,
                     const float* zeros, const float* prob_w, const float* prob_b, float* out, const int* geom,
                     int ngeom, const long* woff, int cin, int mt, int nt, int variant, void* stream);

/* 3x3 (pad 1, stride 1) convolution with 8 output channels and cin in {4, 8} on the fp32 VALU (packed FMA),
 * for the narrow full-resolution layers where the 16-wide MFMA tile is half padding.  in [NB,H,W,cin],
 * w [3,3,cin,8], scale/shift [8], skip optional [NB,H,W,8], out [NB,H,W,8] (depth slices folded into NB).
 * FPN4 conv0 (models/mvs4net_utils.py:427-428), reg2d conv0 (:875), the composed out4 tail (:459). */
int mvster_conv_small(const float* in, const float* w, const float* scale, const float* shift, const float* skip,
                      float* out, int NB, int H, int W, int cin, int relu, void* stream);

/* The same layers (same arguments, same result up to fp32 summation order) on the fp32 matrix cores: the empty half of
 * the 16-wide N tile holds the NEXT pixel's outputs (weights shifted by one tap column over a four-column K axis: 24
 * instead of 36 MFMAs per 32 pixels), persistent workgroups, inputs and the skip tile streamed through an LDS-DMA ring
 * three tiles ahead (csrc/conv_narrow.hip).  mt: tile rows / 4 (2, 4; 0 = by size); wpc: workgroups per CU (0 = default). */
int mvster_conv_narrow(const float* in, const float* w, const float* scale, const float* shift, const float* skip,
                       float* out, int NB, int H, int W, int cin, int relu, int mt, int wpc, void* stream);

/* The 8 -> 4 form of the same kernel (round 6): in [NB,H,W,8], w [3,3,8,8] with output columns 4..7 zero, scale / shift [8]
 * -> out [NB,H,W,4]; no skip.  The input gradient of reg2d's conv0 in training (autograd of models/mvs4net_utils.py:875). */
int mvster_conv_narrow4(const float* in, const float* w, const float* scale, const float* shift, float* out, int NB, int H,
                        int W, int relu, int mt, int wpc, void* stream);

/* FPN4.conv0 in ONE launch (round 6; models/mvs4net_utils.py:427-428: 3 -> 8 -> 8 channels, each conv3x3 + BatchNorm + ReLU):
 * in [NB,H,W,4] (RGB0), w1 [3,3,4,8], w2 [3,3,8,8], scale / shift [8] each -> out [NB,H,W,8].  The 8-channel intermediate
 * stays in LDS (14 x 64-pixel tiles, the first layer computed on the 16 x 66 halo tile, zero outside the image), so the pair
 * moves 78 MB instead of 183 MB at 5 x 512 x 640.  Same result as two mvster_conv_narrow calls up to fp32 summation order.
 * wpc: workgroups per CU (0 = default).  csrc/conv_narrow.hip. */
int mvster_conv_narrow_pair(const float* in, const float* w1, const float* scale1, const float* shift1, const float* w2,
                            const float* scale2, const float* shift2, float* out, int NB, int H, int W, int relu1, int relu2,
                            int wpc, void* stream);

/* mvster_pack_images + mvster_conv_narrow_pair in one launch, without the RGB0 copy: the loading waves read the planes of
 * imgs (N <= 8 views, each a contiguous [B,3,H,W] block, 4-byte aligned) themselves -> out [N*B,H,W,8] (batch index v*B+b),
 * bit for bit.  With proj_matrices non-null the launch also does the two small jobs of mvster_forward_prologue (same
 * arguments and bits): rt [nstage,B,N-1,12] and the first stage's hypotheses hypo [B,D,h,w], in a few workgroups dispatched
 * ahead of the tiles; with proj_matrices null the arguments from nstage to inverse are ignored. */
int mvster_conv_narrow_pair_planes(const float* const* imgs, int N, int B, int H, int W, const float* w1, const float* scale1,
                                   const float* shift1, const float* w2, const float* scale2, const float* shift2, float* out,
                                   int relu1, int relu2, int wpc, const float* const* proj_matrices, int nstage, float* rt,
                                   const float* depth_values, int ndv, float* hypo, int D, int h, int w, int inverse,
                                   void* stream);

/* ConvTranspose3d (1,3,3), stride (1,2,2), padding (0,1,1), output_padding (0,1,1) + BatchNorm scale/shift +
 * ReLU + skip add for (cin, cout) in {(16,8), (32,16)} on the VALU (the layers are HBM-bound).  in [NB,Hi,Wi,cin],
 * w [3,3,cin,cout], skip optional [NB,2Hi,2Wi,cout]; prob_w/prob_b optional (cout == 8): fuse the 1x1x1 head,
 * out = logits [NB,2Hi,2Wi] instead of [NB,2Hi,2Wi,cout].  reg2d conv9 / conv11 (models/mvs4net_utils.py:890-900). */
int mvster_deconv_small(const float* in, const float* w, const float* scale, const float* shift, const float* skip,
                        const float* prob_w, const float* prob_b, float* out, int NB, int Hi, int Wi, int cin,
                        int cout, int relu, void* stream);

/* reg2d's last layer and the depth selection in one launch (models/mvs4net_utils.py:897-900 and :1068-1088):
 * mvster_deconv_small (ConvTranspose 16 -> 8 + BatchNorm + ReLU + skip, fused 1x1x1 `prob` head) followed by
 * mvster_select_depth, bit for bit, without the logits volume going through HBM.  in [B*D,Hi,Wi,16] (slice b*D + d),
 * skip [B*D,2Hi,2Wi,8] or null, hypo [B,D,2Hi,2Wi] -> attn [B,D,2Hi,2Wi], depth / conf / inv_min / inv_max [B,2Hi,2Wi]
 * (conf and inv_* optional; inv_* need D >= 3), logits_out [B,D,2Hi,2Wi] optional.  2 <= D <= 16. */
int mvster_deconv_select(const float* in, const float* w, const float* scale, const float* shift, const float* skip,
                         const float* prob_w, const float* prob_b, const float* hypo, float* attn, float* depth, float* conf,
                         float* inv_min, float* inv_max, float* logits_out, int B, int D, int Hi, int Wi, int cin, int relu,
                         float split_itv, void* stream);

/* mvster_deconv_select followed by mvster_upsample_bilinear_multi, bit for bit, in one launch: workgroups behind the
 * selection's own interpolate up_ins[k] [B,up_his[k],up_wis[k]] -> up_outs[k] [B,ho,wo], k < n <= 3.  The maps must be
 * complete before the launch (the coarse stages' confidence maps at the last stage).  D in {4, 8}; any other D returns
 * MVSTER_ERR_UNSUPPORTED and launches nothing. */
int mvster_deconv_select_riders(const float* in, const float* w, const float* scale, const float* shift, const float* skip,
                                const float* prob_w, const float* prob_b, const float* hypo, float* attn, float* depth,
                                float* conf, float* inv_min, float* inv_max, float* logits_out, int B, int D, int Hi, int Wi,
                                int cin, int relu, float split_itv, const float* const* up_ins, float* const* up_outs,
                                const int* up_his, const int* up_wis, int n, int ho, int wo, void* stream);

/* FPN4 top-down tail, re-associated: G [NB,H/2,W/2,9*CO] = 1x1 conv of the half-resolution top-down
 * map with the 9 taps of the output conv stacked on the channel axis; vb [9,CO] = the taps applied to the
 * lateral conv's bias; P [NB,H,W,CO] = sum over in-bounds taps of (bilinear x2 align_corners upsample of
 * G_tap at p+tap, + vb[tap]).  Together with a 3x3 conv of the lateral input (composed weights, skip-add P)
 * this equals out4(F.interpolate(f) + inner3(c0)) of models/mvs4net_utils.py:488-489 without the
 * full-resolution 64-channel intermediate.  workspace: optional [NB,H,W/2,3*CO]; when given the gather runs as
 * two separable passes (vertical into the workspace, then horizontal), otherwise as one 36-tap pass. */
int mvster_fpn_tail_gather(const float* G, const float* vb, float* P, float* workspace, int NB, int H, int W,
                           int CO, void* stream);

/* Adjoint of mvster_fpn_tail_gather with respect to G (training): gP [NB,H,W,CO] -> gG [NB,H/2,W/2,pitch], channels
 * 9*CO..pitch-1 zero-filled (pitch >= 9*CO, multiple of 4); a gather over the <= 6x6 full-resolution positions that read
 * a half-resolution pixel, no atomics.  CO in {8, 16}. */
int mvster_fpn_tail_gather_bwd(const float* gP, float* gG, int NB, int H, int W, int CO, int pitch, void* stream);

/* Lateral 1x1 conv + top-down add of one FPN level, for a top-down map that is only held at the coarser
 * resolution (models/mvs4net_utils.py:485, after pushing the next level's 1x1 "tap" conv through it):
 * out [NB,H,W,CO] = bias [CO] + A [CO,CI] x [NB,H,W,CI] + bilinear x2 align_corners upsample of q [NB,H/2,W/2,CO].
 * (CI, CO) in {(16,72), (8,72)}. */
int mvster_fpn_lateral_up(const float* x, const float* A, const float* bias, const float* q, float* out, int NB,
                          int H, int W, int CI, int CO, void* stream);

/* mvster_fpn_lateral_up (16 -> 72) + mvster_fpn_tail_gather (CO = 8) of the finest FPN level in ONE launch: a workgroup builds
 * the half-resolution 72-channel patch its 8 x 32 output tile gathers from straight into LDS (lateral product on MFMA tiles,
 * bilinear x2 of q in the epilogue), so the 118 MB map between the two kernels never touches HBM.  x [NB,H/2,W/2,16],
 * A [72,16], bias [72], q [NB,H/4,W/4,72], vb [9,8] -> P [NB,H,W,8].  H, W multiples of 4, H >= 16, W >= 64, CI = 16;
 * MVSTER_ERR_UNSUPPORTED otherwise.  models/mvs4net_utils.py:485-489 (section 4.3 of DESIGN.md). */
int mvster_fpn_tail_fused(const float* x, const float* A, const float* bias, const float* q, const float* vb, float* P,
                          int NB, int H, int W, int CI, void* stream);

/* Packed-weight refresh on the device (training, once per layer and optimizer step): writes the fragment order
 * [K/16][N/16][64][4] that mvster_conv_mfma reads, Bm[tap*cin_pad + ci][n] = w[n*s_n + ci*s_c + kz*s_z + ky*s_y + kx*s_x]
 * (element strides of the parameter tensor; flip = 1 mirrors the taps: the input-gradient form of a stride-1 layer),
 * zero for ci >= cin and n >= cout.  wpk holds ceil(kd*kh*kw*cin_pad/16) * ceil(cout/16) * 256 floats. */
int mvster_pack_conv_weights(const float* w, float* wpk, int cout, int cin, int cin_pad, int kd, int kh, int kw, long s_n,
                             long s_c, long s_z, long s_y, long s_x, int flip, void* stream);

/* Transformed weights of the Winograd F(2x2, 3x3) kernels (variants 8 / 9 of mvster_conv_mfma, which take this array as
 * their `wpk`): U = G g G^T per (cout, cin, kz) of w [cout, cin, kd, 3, 3], kd in {1, 3} (element strides; flip = 1 mirrors
 * the taps), stored in the same fragment order with the 16 transform points in place of the in-plane taps:
 * kd * 16 * cin_pad/16 K steps x ceil(cout/16) x 256 floats.  Stands in for the weight side of nn.Conv2d(3x3) (models/mvs4net_utils.py:116-123). */
int mvster_pack_wino_weights(const float* w, float* wpk, int cout, int cin, int cin_pad, int kd, long s_n, long s_c, long s_z,
                             long s_y, long s_x, int flip, void* stream);

/* The same for every record of a DEVICE table in ONE launch (the training step re-transforms the weights of all its
 * Winograd layers after each optimizer update): 88-byte records {const float* w; float* wpk; long s_n, s_c, s_z, s_y, s_x;
 * int cout, cin_raw, cin_pad, kd, flip, ntile, first_block, pad}, ntile = ceil(cout / 16), first_block = prefix sum of
 * ceil(kd*16*cin_pad*ntile*16 / 256) over the earlier records, total_blocks = their sum. */
int mvster_pack_wino_batch(const void* descs, int ndesc, int total_blocks, void* stream);

/* The same refresh for a transposed layer (output-parity classes): w [cin, cout, kd, kh, kw] contiguous, ktot = kd*kh*kw
 * <= 27; class c packs the taps taps[c*27 .. c*27 + ntaps[c]) (flattened indices, input-offset order) at float offset
 * woff[c] of wpk. */
int mvster_pack_conv_weights_classes(const float* w, float* wpk, int cout, int cin, int cin_pad, int ktot, int nclass,
                                     const int* ntaps, const long* woff, const int* taps, void* stream);

/* Weight gradient of a channels-last convolution (training): for every kernel tap
 *   dW[tap][co][ci] = sum_o gy[o][co] * x[o*s - p + tap][ci]      (zero padding)
 * x [B,Di,Hi,Wi,CI], gy [B,Do,Ho,Wo,CO] with (Do,Ho,Wo) the conv output size for (k,s,p); CI, CO <= 64.
 * Workgroup slot n of `partial` [nblk][kd*kh*kw][COP][CIP] (COP/CIP = CO/CI rounded up to 16, 48 -> 64)
 * receives the sum over the output rows that workgroup visited; the caller adds the nblk slots.  packed = 1 (CI <= 8):
 * 16/CIP taps share one N tile (CIP = 4 or 8), partial [nblk][ceil(taps/(16/CIP))][COP][16], column = (tap % TPN)*CIP + ci.
 * With x and gy swapped it is the weight gradient of the transposed convolution.  Replaces autograd's conv weight gradients
 * of nn.Conv3d / nn.Conv2d / nn.ConvTranspose3d (models/mvs4net_utils.py:116-123, :224-251, :870-965, :419-502). */
int mvster_conv_wgrad(const float* x, const float* gy, float* partial, int nblk, int B, int Di, int Hi, int Wi, int CI,
                      int Do, int Ho, int Wo, int CO, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph,
                      int pw, int packed, void* stream);

/* Slot count (`nblk`) to give `partial` for a layer: > 0 where the persistent weight-gradient kernel applies (3x3 / 3x3x3,
 * stride 1, 16 / 32 / 64 channels on both sides: it fills exactly its workgroup count of slots) and for the 5x5 stride-2
 * layers (one resident round of workgroups), 0 = caller's choice.  The caller may use fewer slots, never more. */
int mvster_conv_wgrad_slots(int CI, int CO, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, int packed);

/* Finish of the weight gradient: adds the nblk slots (fixed order) and writes dW in the parameter's layout in one launch.
 * Slot element (g, row, col) of [ngrp][cop][width]: co = row; cip = 0: tap = g, ci = col; cip = 4 / 8 (packed): tap =
 * g*(16/cip) + col/cip, ci = col % cip.  Kept when tap < ntaps, co < co_lim, ci < ci_lim; flip mirrors the taps
 * (tap -> ntaps-1-tap); dw is [co_lim][ci_lim][ntaps], or [ci_lim][co_lim][ntaps] with swap (the mirrored narrow-output
 * form and nothing else needs both). */
int mvster_conv_wgrad_finish(const float* partial, float* dw, int nblk, int ngrp, int cop, int width, int ntaps, int cip,
                             int co_lim, int ci_lim, int swap, int flip, void* stream);

/* `count` finishes in ceil(count / 56) launches: recs = HOST array of 56-byte records {const float* partial; float* dw; int
 * nblk, ngrp, cop, width, ntaps, cip, co_lim, ci_lim, swap, flip} -- the arguments of mvster_conv_wgrad_finish.  The
 * training step defers the finishes of all its layers to the end of the backward pass (nothing reads a weight gradient
 * before) and issues them together. */
int mvster_conv_wgrad_finish_batch(const void* recs, int count, void* stream);

/* Training-mode BatchNorm + ReLU on channels-last activations (C a power of two, 4..64): the elementwise half of the
 * reference's conv -> BatchNorm -> ReLU blocks (models/mvs4net_utils.py:116-123, :224-251) and its autograd.
 * x [groups*rows, C]: `groups` independent statistics groups of `rows` rows each (the reference normalises every
 * view's batch on its own, MVS4Net.py:65-68); scale = gamma * rstd, shift = beta - mean * scale, mean, rstd are
 * [groups, C] (statistics from the caller: the pack of mvster_bn_train_fwd below, or a module's running statistics).
 *   fwd:         y = relu(x*scale + shift) (+ skip)                      (relu = 0: affine only; skip optional: the U-Net's
 *                same-shape skip connection, added after the activation, models/mvs4net_utils.py:893-895)
 *   bwd_reduce:  per-workgroup slots partial[g][n][0][c] / [g][n][1][c] = sum g_ and sum g_*xh; the last workgroup to
 *                arrive writes sums [groups][2][C] and the parameter gradients dbeta [C] = sum_g sum g_, dgamma [C] =
 *                sum_g sum g_*xh
 *   bwd_apply:   dx = scale * (g_ - sums[g][0]/rows - xh * sums[g][1]/rows),   g_ = gy * (y > 0), xh = (x - mean) * rstd;
 *                frozen = 1 (statistics are constants): dx = scale * g_
 * partial: [groups][mvster_bn_slots(rows, C, groups)][2][C] floats of scratch.  bwd_reduce is ONE launch:
 * the last workgroup to arrive (ticket: one device int, 0 before the call and 0 again after it) adds the slots in a fixed
 * order in fp64 and writes the results (slots published with write-through stores: no L2 write-back); groups*2C <= 2048.
 * Training-mode BatchNorm itself is mvster_bn_train_fwd / _bwd below; bwd_reduce + bwd_apply serve the backward of a
 * BatchNorm in eval mode inside a training graph (frozen = 1). */
int mvster_bn_relu_fwd(const float* x, const float* scale, const float* shift, const float* skip, float* y, long rows,
                       int C, int relu, int groups, void* stream);
int mvster_bn_slots(long rows, int C, int groups);
int mvster_bn_relu_bwd_reduce(const float* x, const float* gy, const float* scale, const float* shift, const float* mean,
                              const float* rstd, float* partial, float* sums, float* dgamma, float* dbeta, int* ticket,
                              long rows, int C, int relu, int groups, void* stream);
int mvster_bn_relu_bwd_apply(const float* x, const float* gy, const float* scale, const float* shift, const float* mean,
                             const float* rstd, const float* sums, float* dx, long rows, int C, int relu, int groups,
                             int frozen, void* stream);

/* out [C] = column sums of the channels-last x [rows, C], C in {4, 8, 16, 32, 64}: the bias gradient of the reference's
 * convolutions with bias (sum of the output gradient over every voxel; FPN laterals models/mvs4net_utils.py:485-487,
 * monocular heads :846-848).  partial: mvster_bn_slots(rows, C, 1) * 2 * C floats, ticket as above.  One launch. */
int mvster_col_sum(const float* x, float* partial, float* out, int* ticket, long rows, int C, void* stream);

/* Training-mode BatchNorm (+ ReLU, + skip): TWO launches per pass without a serial tail -- the reduction kernel only writes
 * its per-workgroup slots (forward: sum d and sum d^2, d = x - x[first row of the group]; backward: sum g_ and sum g_*xh),
 * the apply kernel's workgroups sum them in their prologue (every workgroup its group's, in the same fixed order, fp64), one
 * extra workgroup does the running-average updates (forward) / the parameter gradients (backward).
 *   train_fwd:  y = relu(x*scale + shift) (+ skip) with batch statistics; out [5][groups][C] = mean, biased var, rstd,
 *               scale, shift; running_mean / running_var (optional) get the groups' exponential-average updates in order
 *               (momentum, unbiased variance) and num_batches_tracked (optional, device int64) += groups -- what `groups`
 *               sequential nn.BatchNorm calls would do
 *   train_bwd:  dx as bwd_apply above with frozen = 0, dgamma / dbeta [C] summed over the groups; pack = the forward's `out`
 * partial: groups * mvster_bn_train_slots(rows, C, groups) * 2 * C floats; groups*2C <= 2048.
 * models/mvs4net_utils.py:116-123, :224-251 under autograd. */
int mvster_bn_train_slots(long rows, int C, int groups);
int mvster_bn_train_fwd(const float* x, const float* weight, const float* bias, float* running_mean, float* running_var,
                        long* num_batches_tracked, const float* skip, float* partial, float* y, float* out, long rows, int C,
                        int relu, int groups, float eps, float momentum, void* stream);
int mvster_bn_train_bwd(const float* x, const float* gy, const float* pack, float* partial, float* dgamma, float* dbeta, float* dx,
                        long rows, int C, int relu, int groups, void* stream);

/* Bilinear x2 up-sampling (align_corners=True) of a channels-last map, in [B,h,w,C] -> out [B,2h,2w,C], and its
 * adjoint gout [B,2h,2w,C] -> gin [B,h,w,C] as a gather (no atomics): the FPN top-down path in training
 * (models/mvs4net_utils.py:488-496 under autograd).  C % 4 == 0. */
int mvster_upsample2x_cl_fwd(const float* in, float* out, int B, int h, int w, int C, void* stream);
int mvster_upsample2x_cl_bwd(const float* gout, float* gin, int B, int h, int w, int C, void* stream);
/* Nearest x2 (F.interpolate(scale_factor=2, mode="nearest"), the mono head's up-sampling, models/mvs4net_utils.py:858):
 * backward = 0: in [B,h,w,C] -> out [B,2h,2w,C]; backward = 1: the adjoint, in = gout [B,2h,2w,C] -> out = gin [B,h,w,C]. */
int mvster_upsample2x_nearest_cl(const float* in, float* out, int B, int h, int w, int C, int backward, void* stream);

/* Sinkhorn optimal-transport loss per pixel and its gradient, fused (discrete form, ot_continous=False):
 * attn, hypo [B,D,HW], gt [B,HW] -> loss_pix [B,HW], jac [B,D,HW] = d loss_pix / d attn.  2 <= D <= 16,
 * iters <= 16.  Replaces the per-pixel part of `sinkhorn` (models/mvs4net_utils.py:1096-1142) and its autograd;
 * the masked mean over pixels stays with the caller. */
int mvster_sinkhorn(const float* attn, const float* hypo, const float* gt, float* loss_pix, float* jac, int B, int D,
                    long HW, int iters, float eps, void* stream);
/* The continuous form (ot_continous=True, models/mvs4net_utils.py:1111-1123): D + 1 target columns, all the mass on
 * the extra one, whose cost is the distance of every bin to the ground truth's fractional bin position (10 where
 * mask <= 0.5).  mask [B,HW] float; 3 <= D <= 8, iters <= 16. */
int mvster_sinkhorn_continuous(const float* attn, const float* hypo, const float* gt, const float* mask, float* loss_pix,
                               float* jac, int B, int D, long HW, int iters, float eps, void* stream);

/* The per-pixel terms of one stage of the training loss around the OT term, one pass (MVS4net_loss,
 * models/MVS4Net.py:131-151: the mask compare, F.l1_loss(mono_depth[mask], depth_gt[mask]) :136-137, mask_out_of_range
 * :141-147 and the masked mean of the OT loss).  hypo [B,D,HW] (D >= 3), gt, mask (float, > 0.5 = valid), loss_pix
 * [B,HW] (from mvster_sinkhorn*), mono [B,HW] or NULL -> terms [5][B*HW]: valid, valid*|mono-gt|, valid*(no hypothesis
 * within |t(hypo_2)-t(hypo_1)| of gt; t = 1/x when inverse_depth), valid*loss_pix, valid*sign(mono-gt).  The caller
 * sums the planes: l1 = S1/S0, range ratio = S2/S0, ot = S3/S0. */
int mvster_stage_loss_terms(const float* hypo, const float* gt, const float* mask, const float* loss_pix,
                            const float* mono, float* terms, int B, int D, long HW, int inverse_depth, void* stream);

/* Geometric-consistency filter of one reference view against NS source views, fused (test_mvs4.py:273-328 per
 * view pair + the sums of filter_depth :362-385).  depth_ref [H,W], depth_src [NS,H,W]; ref_mats = inv(K_ref)[9],
 * K_ref[9]; view_mats [NS][42] = (E_src inv(E_ref))[3x4], K_src[3x3], inv(K_src)[3x3], (E_ref inv(E_src))[3x4], all
 * row major, float32 values widened to double (the reference's dtype flow).  mask_sum [H,W] = number of consistent
 * views, depth_sum [H,W] = sum of their reprojected depths; view_mask / view_depth / x_src / y_src [NS,H,W] are
 * optional per-view outputs (the returns of check_geometric_consistency).  Source depth is sampled like
 * cv2.remap(INTER_LINEAR): 1/32-pixel coordinates, constant-0 border. */
int mvster_geo_filter(const float* depth_ref, const float* depth_src, const double* ref_mats, const double* view_mats,
                      int* mask_sum, float* depth_sum, unsigned char* view_mask, float* view_depth, float* x_src,
                      float* y_src, int NS, int H, int W, float pix_thres, float rel_thres, void* stream);

/* ---- depth-map fusion of a whole scan (csrc/geo_scene.hip): filter_depth of test_mvs4.py:331-421 in three launches ---- */

/* Number of workgroups (= survivor counts) the scene kernels use for R reference views of H x W pixels: the length of
 * wg_counts; wg_offsets holds one more.  MVSTER_ERR_SHAPE for non-positive sizes or more than 2^31 - 2 workgroups. */
int mvster_geo_scene_blocks(int R, int H, int W);

/* Filter pass + scan.  depth / confidence [V,H,W]: every view of the scan once; pairs [R,Smax] int32 = source views of
 * each reference view in pair-file order, padded with -1; ref_view [R] int32; ref_mats [R][30] = inv(K_ref)[9], K_ref[9],
 * inv(E_ref)[3x4]; view_mats [R][Smax][42] laid out as for mvster_geo_filter (rows behind the padding are not read).
 * One thread per (reference view, pixel) walks its source list like mvster_geo_filter (test_mvs4.py:362-385) and writes
 * mask_sum [R,H,W] int32, depth_avg [R,H,W] double = (float32 depth sum + depth_ref) / (votes + 1) (:385), and the 0 / 1
 * byte masks photo = confidence > conf_thres (:361), geo = votes >= thres_view (:387), final = both (:388).  wg_counts
 * [mvster_geo_scene_blocks()] int32 (scratch) = survivors per workgroup; wg_offsets [blocks + 1] int64 = their exclusive
 * scan, wg_offsets[blocks] = number of points M.  A workgroup covers 256 consecutive pixels of one view, so view r's
 * survivors are wg_offsets[(r + 1) * blocks / R] - wg_offsets[r * blocks / R].  View indices outside [0, V) are never
 * dereferenced (such a reference view keeps nothing; such a source entry ends the list).  Two launches, no atomics. */
int mvster_geo_scene_filter(const float* depth, const float* confidence, const int* pairs, const int* ref_view,
                            const double* ref_mats, const double* view_mats, int* mask_sum, double* depth_avg,
                            unsigned char* photo_mask, unsigned char* geo_mask, unsigned char* final_mask, int* wg_counts,
                            long* wg_offsets, int R, int Smax, int V, int H, int W, float conf_thres, int thres_view,
                            float pix_thres, float rel_thres, void* stream);

/* The same filter pass + scan under dynamic consistency checking instead of the fixed pixel /
 * relative-depth thresholds.  A source passes level n when its reprojection error is below n * pix_base (fp32 product,
 * compared in fp64) and its relative depth error below n * rel_base (fp32).  For a reference view with L real sources,
 * geo_level [R,H,W] uint8 = the smallest n in thres_view..L with at least n sources passing level n, 0 if there is none
 * (always 0 when L < thres_view); geo = geo_level != 0, final = photo & geo.  mask_sum = sources passing the loosest
 * level max(L, thres_view), depth_avg = (float32 sum of their reprojected depths in pair-file order + depth_ref) /
 * (mask_sum + 1).  Everything else -- layouts, wg_counts / wg_offsets, invalid view indices -- as for
 * mvster_geo_scene_filter, and mvster_geo_scene_emit takes the outputs as they are.  MVSTER_ERR_UNSUPPORTED for
 * Smax > 32 (the per-pixel level counts hold 32 sources), MVSTER_ERR_SHAPE for thres_view < 1 or a base that is not
 * finite and positive; all arguments are checked before any launch. */
int mvster_geo_scene_filter_dynamic(const float* depth, const float* confidence, const int* pairs, const int* ref_view,
                                    const double* ref_mats, const double* view_mats, int* mask_sum, double* depth_avg,
                                    unsigned char* photo_mask, unsigned char* geo_mask, unsigned char* final_mask,
                                    unsigned char* geo_level, int* wg_counts, long* wg_offsets, int R, int Smax, int V,
                                    int H, int W, float conf_thres, int thres_view, float pix_base, float rel_base,
                                    void* stream);

/* Emit pass: the pixels of final_mask, reference views in order and row-major inside a view, lifted to world space
 * with depth_avg in fp64 and rounded once -> points [M,3] float32 (test_mvs4.py:397-407, :413-415); colors [M,3] uint8 =
 * (image * 255) truncated (:395-396, :407).  images [V,H,W,3]: image_kind 0 = uint8 (copied: the float32 round trip
 * v / 255 * 255 is the identity on all 256 values), 1 = float32 in 0..1; anything else is MVSTER_ERR_UNSUPPORTED.
 * depth_avg / final_mask / ref_view / ref_mats / wg_offsets as written by (given to) mvster_geo_scene_filter with the
 * same R, H, W; M = wg_offsets[blocks] read back by the caller (points beyond M are dropped, M = 0 launches nothing). */
int mvster_geo_scene_emit(const double* depth_avg, const unsigned char* final_mask, const int* ref_view,
                          const double* ref_mats, const void* images, int image_kind, const long* wg_offsets, float* points,
                          unsigned char* colors, long M, int R, int V, int H, int W, void* stream);

/* ---- training-step glue (csrc/train_glue.hip): the reference's chains of small tensor expressions, one launch each ---- */

/* One stage of MVS4net_loss around the OT term (models/MVS4Net.py:126-153), forward: hypo [B,D,HW] (D >= 3), gt, mask
 * (float, > 0.5 = valid), loss_pix [B,HW] (from mvster_sinkhorn*), mono [B,HW] or NULL, total_in: device scalar or NULL ->
 * planes [2][B*HW] (valid, valid*sign(mono-gt): for the backward), partial [mvster_stage_loss_slots(B*HW)][4] (scratch),
 * out [6] = #valid, l1 = mean|mono-gt| (:136-137), out-of-range ratio (:141-147), ot = masked mean of loss_pix,
 * weighted = w_stage*(w_l1*l1 + w_ot*ot) (:151), total = total_in + weighted.  Two launches, deterministic. */
int mvster_stage_loss_slots(long n);
int mvster_stage_loss_fwd(const float* hypo, const float* gt, const float* mask, const float* loss_pix, const float* mono,
                          const float* total_in, float* planes, float* partial, float* out, int B, int D, long HW,
                          int inverse_depth, float w_l1, float w_ot, float w_stage, void* stream);

/* Its backward: jac [B,D,HW] = d loss_pix / d attn (mvster_sinkhorn*), planes / out from the forward; g_total / g_l1 /
 * g_ot = device scalars (NULL = 0), gradients of out[5] / out[1] / out[3]; w_l1 = w_stage*l1ot_lw[0], w_ot =
 * w_stage*l1ot_lw[1] -> g_attn [B,D,HW] (or NULL), g_mono [B,HW] (or NULL).  One launch. */
int mvster_stage_loss_bwd(const float* jac, const float* planes, const float* out, const float* g_total, const float* g_l1,
                          const float* g_ot, float w_l1, float w_ot, float* g_attn, float* g_mono, int B, int D, long HW,
                          void* stream);

/* Monocular head, disparity -> depth (models/mvs4net_utils.py:858-866): depth [B,HW] = 1 / (1/d_max[b] + (1/d_min[b] -
 * 1/d_max[b]) * sigmoid(z)); sig [B,HW] = sigmoid(z) is kept for the backward, gz = g * d depth / d z. */
int mvster_mono_depth_fwd(const float* z, const float* dmin, const float* dmax, float* depth, float* sig, int B, long HW,
                          void* stream);
int mvster_mono_depth_bwd(const float* g, const float* depth, const float* sig, const float* dmin, const float* dmax, float* gz,
                          int B, long HW, void* stream);

/* out [NB,H,W,Ca+Cb] = concat(nearest x2 up-sampling of a [NB,H/2,W/2,Ca], b [NB,H,W,Cb]) -- the input of the monocular
 * head's 3x3 convolutions (models/mvs4net_utils.py:854-857) -- and the adjoint g -> ga, gb.  H, W even; Ca, Cb % 4 == 0. */
int mvster_upcat_fwd(const float* a, const float* b, float* out, int NB, int H, int W, int Ca, int Cb, void* stream);
int mvster_upcat_bwd(const float* g, float* ga, float* gb, int NB, int H, int W, int Ca, int Cb, void* stream);

/* Composed weights of the re-associated finest FPN level (out4(up(f) + inner3(c0)), models/mvs4net_utils.py:496-498):
 * wo [CO,CM,3,3] = out4.weight, wi [CM,CI] = inner3.weight, bi [CM] = inner3.bias -> wg [9*CO,CM] (row tap*CO+o =
 * wo[o,:,tap]), wc [CO,CI,3,3] = sum_c wo[o,c,tap] wi[c,i], vb [9,CO] = sum_c wo[o,c,tap] bi[c]; and the adjoint
 * (g_wg / g_wc / g_vb may be NULL) -> g_wo, g_wi, g_bi.  One single-workgroup launch each. */
int mvster_fine_weights_fwd(const float* wo, const float* wi, const float* bi, float* wg, float* wc, float* vb, int CO, int CM,
                            int CI, void* stream);
int mvster_fine_weights_bwd(const float* wo, const float* wi, const float* bi, const float* g_wg, const float* g_wc,
                            const float* g_vb, float* g_wo, float* g_wi, float* g_bi, int CO, int CM, int CI, void* stream);

/* Adam update (torch.optim.Adam semantics with L2 weight decay, no amsgrad; train_mvs4.py:367) of `count` fp32 tensors:
 * params / grads = HOST arrays of `count` device pointers, sizes / state_offs = host int arrays (elements; offsets of a
 * tensor's moments in the flat exp_avg / exp_avg_sq buffers).  step_cells [2] device floats: cell 0 = number of updates
 * done so far, + 1 afterwards (cell 1 scratch); lr = one DEVICE float (a schedule reaches a captured step by rewriting
 * it between replays).  ceil(count / 128) launches (+ 1 when that is odd); the pointers travel as
 * kernel arguments, so a captured step records them with the launch.  Every pointer and size is checked before the first
 * launch: MVSTER_ERR_NULL (a null params[i] / grads[i]) or MVSTER_ERR_SHAPE (a negative size / offset) leave the tensors, the
 * moments and the step cells untouched. */
int mvster_fused_adam(const void* const* params, const void* const* grads, const int* sizes, const int* state_offs, int count,
                      float* exp_avg, float* exp_avg_sq, float* step_cells, const float* lr, double beta1, double beta2,
                      double eps, double weight_decay, void* stream);

/* Batched gather, one launch: for every record r of the DEVICE table `descs` (32-byte records {const float* src; float* dst;
 * const int* idx; int n; int first_block}), dst[i] = idx[i] > 0 ? src[idx[i] - 1] : 0, i < n (n % 4 == 0); first_block =
 * prefix sum of ceil(n / 1024), total_blocks their sum.  Refreshes all packed / permuted weight forms of the training step
 * from their parameters after an optimizer update (host-side plumbing: the reference's layers read the parameters directly). */
int mvster_gather_batch(const void* descs, int ndesc, int total_blocks, void* stream);

/* ---- voxel-grid thinning of a fused cloud (csrc/geo_thin.hip, csrc/voxel_math.h) ---- */

/* Workgroups (= leader counts) for a cloud of M points: the length of wg_counts; wg_offsets holds three more.
 * MVSTER_ERR_SHAPE for M <= 0 or M > 2^29 (a slot index and its leader mark share 32 bits). */
int mvster_voxel_thin_blocks(long M);

/* Insert + leaders + scan.  points [M,3] float32; voxel = the edge v, finite and > 0.  Per point and axis, in fp64:
 * q = p / v, i = floor(q); a point is valid iff -2^20 <= i < 2^20 on all axes; its voxel key is ((ix + 2^20) << 42) |
 * ((iy + 2^20) << 21) | (iz + 2^20).  keys [table_slots] uint64 / first [table_slots] int32 (scratch) = the open-addressing
 * table, filled here by a kernel; table_slots a power of two, >= 64, >= 2 * M, <= 2^30 -- anything else is
 * MVSTER_ERR_SHAPE before any launch.  slot [M] int32 (scratch): a point's slot, -2 - slot for the first point of a
 * voxel, -1 for an invalid point.  wg_counts [blocks] int32 (scratch); wg_offsets [blocks + 3] int64 = the exclusive scan
 * of the first points per workgroup, then U = occupied voxels, dropped = invalid points, status (non-zero: a point found
 * no slot, which a legal table_slots excludes) -- three neighbouring words, the caller's one read-back.  Four launches; the
 * probe loop runs at most table_slots iterations. */
int mvster_voxel_thin_insert(const float* points, long M, float voxel, unsigned long long* keys, int* first, long table_slots,
                             int* slot, int* wg_counts, long* wg_offsets, void* stream);

/* Rank + accumulate + emit, with first / slot / wg_offsets as mvster_voxel_thin_insert left them (first is overwritten by
 * ranks) and U read back by the caller.  Voxels in the order of their first point f: out_first [U] int64 = f, out_counts
 * [U] int32 = n, the voxel's valid points.  reduce 1 ("first"): out_points / out_colors = point f and its colour, bits
 * unchanged; sums may be NULL.  reduce 0 ("mean"): with t = min((int64)floor((q - i) * 65536), 65535) per point and axis,
 * S their sums and C the colour sums (sums [U,6] uint64, scratch), out_points = (float)((i + (S + 0.5 n) / (65536 n)) * v)
 * in fp64, out_colors = (2 C + n) / (2 n) in integers (round half up).  Integer atomics only: bit-reproducible.  U = 0
 * launches nothing; another reduce is MVSTER_ERR_UNSUPPORTED.  Four launches. */
int mvster_voxel_thin_emit(const float* points, const unsigned char* colors, long M, float voxel, int reduce, int* first,
                           const int* slot, const long* wg_offsets, unsigned long long* sums, float* out_points,
                           unsigned char* out_colors, int* out_counts, long* out_first, long U, void* stream);

/* ---- cloud-to-cloud nearest distances and scan scores (csrc/geo_nn.hip, csrc/nn_math.h) ---- */

/* The grid of a cloud from what mvster_voxel_thin_insert(points, M, cell, ...) left in first / slot / wg_offsets (the cells
 * are the voxels of edge `cell`).  ncells = the capacity of counts [ncells] int32 and starts [ncells + 1] int64: the
 * occupied cells U the caller read back, or M without a read-back.  Afterwards first [table_slots] holds the dense cell id
 * of every occupied slot (cells in the order of their first point), slot [M] a point's cell id (-1: invalid point), starts
 * the first record of every cell with starts[ncells] = the valid points, and records [M] the valid points in cell order as
 * 16-byte records (x, y, z as float32 bits, the point's index as int32).  The order inside a cell may differ between
 * runs.  local [M] int32 is scratch.  MVSTER_ERR_SHAPE for M outside 1 .. 2^29 or ncells outside 1 .. M.  Five launches. */
int mvster_cloud_grid_build(const float* points, long M, int* first, int* slot, const long* wg_offsets, int* counts, int* local,
                            long* starts, long ncells, void* records, void* stream);

/* Nearest target of every query up to max_dist (the definition: csrc/nn_math.h).  The queries come as the grid of their own
 * cloud: qrecords (NULL where it has no valid point) / qcell (= slot) / qtotal (= starts + ncells of that grid), Q its
 * points; the target as keys /
 * cell_of_slot (= first) / starts / records with ncells cells and nrecords records (0 cells: every valid query gets +inf).
 * Both grids must have been built with this `cell`; cell >= max_dist / 15.  Per query, at its original position: dist2 fp64
 * = the smallest d2 <= max_dist^2 over the valid targets, dist = (float)sqrt(d2), index = that target's index, the smallest
 * among equal d2; +inf / +inf / -1 without a candidate, NaN / NaN / -1 for an invalid query.  One launch, no atomics: the
 * result depends neither on the grid nor on the run.  Every hash probe loop runs at most table_slots iterations. */
int mvster_cloud_nn_query(const void* qrecords, const int* qcell, const long* qtotal, long Q, const unsigned long long* keys,
                          const int* cell_of_slot, long table_slots, const long* starts, const void* records, long ncells,
                          long nrecords, float max_dist, float cell, float* dist, double* dist2, long* index, void* stream);

/* Rows of `partial` for Q distances; MVSTER_ERR_SHAPE for Q outside 1 .. 2^29. */
int mvster_cloud_score_slots(long Q);

/* out [4] float64 over dist [Q]: the values that are not NaN, those <= max_dist, those < tau (0 <= tau <= max_dist) and the
 * fp64 sum of those <= max_dist.  partial [slots, 4] float64 (scratch): one row per workgroup, summed in row order -- no
 * atomics, two runs give the same bytes.  Two launches. */
int mvster_cloud_score(const float* dist, long Q, float max_dist, float tau, double* partial, double* out, void* stream);

/* ---- the DTU evaluation protocol (csrc/geo_eval.hip, csrc/eval_math.h) ---- */

/* state [M] int32 of the point reduction: 0 (undecided) for a valid point -- vox::point_key(p, dst) accepts it -- and 2
 * (dropped) for an invalid one; invalid [1] uint64 = the invalid points (zeroed here, one integer atomic per wave).
 * MVSTER_ERR_SHAPE for M outside 1 .. 2^29 or a dst that is not finite and > 0.  Two launches. */
int mvster_eval_reduce_init(const float* points, long M, float dst, int* state, unsigned long long* invalid, void* stream);

/* nrounds (1 .. 64) rounds of the reduction over the grid of the cloud at cell = cell_factor * dst (records [nrecords], keys /
 * cell_of_slot [table_slots], starts [ncells + 1] as mvster_cloud_grid_build left them); cell_factor 2 searches the 3 x 3 x 3
 * cells around a point's own, cell_factor 1 the 5 x 5 x 5 (csrc/eval_math.h proves both); anything else, or a cell that is not
 * finite, is MVSTER_ERR_SHAPE.  Point i has the priority (key_i, i): key_i = splitmix64(i, seed) (seed >= 0) where priority is
 * NULL, else priority [M] int64 in signed order.  In a round every undecided point looks at the points with d2 <= dst^2 and a
 * smaller priority: one of them kept (state 1) -> dropped (2); none kept and none undecided -> kept; otherwise unchanged.
 * States are read and written in place with relaxed atomics, each written once.  counts [nrounds] uint64: the points left
 * undecided after each round (zeroed here, one integer atomic per wave).  1 + nrounds launches; every hash probe loop runs at
 * most table_slots iterations. */
int mvster_eval_reduce_rounds(const void* records, long nrecords, const unsigned long long* keys, const int* cell_of_slot,
                              long table_slots, const long* starts, long ncells, float dst, int cell_factor, const long* priority,
                              long seed, long M, int* state, unsigned long long* counts, int nrounds, void* stream);

/* flags [N] uint8 of points [N,3]: bit 0 = in_obs_mask, bit 1 = above_plane, bit 2 = covered (csrc/eval_math.h), each only where
 * `which` (1 .. 7) has the bit.  mask [S1,S2,S3] uint8, C-contiguous (may be NULL without bit 0); params [12] float64 on the
 * device = BB1 (3), BB2 (3), Res, max_block, P (4).  counts [3] uint64 = the points with each bit (zeroed here, integer
 * atomics).  Two launches. */
int mvster_eval_flags(const float* points, long N, const unsigned char* mask, long S1, long S2, long S3, const double* params,
                      int which, unsigned char* flags, unsigned long long* counts, void* stream);

/* Rows of `partial` for N distances; MVSTER_ERR_SHAPE for N outside 1 .. 2^29. */
int mvster_eval_stats_slots(long N);

/* out [4] float64 = n, mean, var, median of d = sqrt(dist2 [N]) over the selected points: (flags[i] & need) == need, dist2
 * finite and d < max_dist (strict).  mean and var (second pass, / (n - 1)) from per-workgroup partials added in slot order;
 * the median from an exact radix selection of the two middle dist2 over their bit patterns (8 passes of 8 bits, integer
 * histograms).  n = 0 gives NaN, NaN, NaN.  Scratch: partial [slots, 2] float64, hist [8 * 2 * 256] uint32, work [6] uint64.
 * No floating-point atomics: two runs give the same bytes.  20 launches. */
int mvster_eval_stats(const double* dist2, const unsigned char* flags, long N, int need, float max_dist, double* partial,
                      unsigned* hist, unsigned long long* work, double* out, void* stream);

/* ---- the Tanks and Temples evaluation protocol (csrc/geo_reg.hip, csrc/reg_math.h) ---- */

/* Tiles of 256 points of a cloud of N points: the length of wg_counts; wg_offsets holds one more.  MVSTER_ERR_SHAPE for N
 * outside 1 .. 2^29. */
int mvster_reg_blocks(long N);

/* out [N,3] float32 = (float)(T p) for points [N,3] float32: T [12] float64 ON THE HOST (read before the call returns) = the
 * first three rows of a 4 x 4 matrix, q_a = ((T[4a] x + T[4a+1] y) + T[4a+2] z) + T[4a+3] in fp64.  One launch. */
int mvster_reg_transform(const float* points, long N, const double* T, float* out, void* stream);

/* flags [N] uint8 = 1 where q = T p (T as above, on the host; NULL: q = p) lies inside the crop volume: volume [2 + 2 P]
 * float64 on the device = axis_min, axis_max, then (u, v) of the P polygon vertices; axis 0 / 1 / 2 = the orthogonal axis
 * X / Y / Z (csrc/reg_math.h has the rule).  wg_counts [blocks] int32 (scratch); wg_offsets [blocks + 1] int64 = the exclusive
 * scan of the kept points per tile, its last word the kept count: the caller's one read-back.  max_grid: workgroups at most,
 * 0 for the default (2048), never more.  MVSTER_ERR_SHAPE before any launch for P outside 3 .. 1024, an axis outside 0 .. 2, N
 * outside 1 .. 2^29.  Two launches, no atomics. */
int mvster_reg_crop_flags(const float* points, long N, const double* T, const double* volume, int P, int axis, int max_grid,
                          unsigned char* flags, int* wg_counts, long* wg_offsets, void* stream);

/* The kept points in the input's order, with flags / wg_offsets as mvster_reg_crop_flags left them and K the kept count read
 * back: out_points [K,3] = (float)q (the input's bits where T is NULL), out_index [K] int64 = the position in the input,
 * out_colors [K,3] uint8 where colors is not NULL.  K = 0 launches nothing.  One launch. */
int mvster_reg_crop_emit(const float* points, const unsigned char* colors, long N, const double* T, const unsigned char* flags,
                         const long* wg_offsets, long K, int max_grid, float* out_points, unsigned char* out_colors,
                         long* out_index, void* stream);

/* Rows of `partial` for Q source points; MVSTER_ERR_SHAPE for Q outside 1 .. 2^29. */
int mvster_reg_sum_rows(long Q);

/* out [18] float64 over the source points i with 0 <= index[i] < M: n, sum d2, sum s (3), sum t (3), sum s.s, sum t_a s_b (9,
 * row a, column b); s = source [Q,3] float32 (already moved), t = target [M,3] float32 at index[i], d2 = dist2[i], index /
 * dist2 as mvster_cloud_nn_query gave them.  partial [rows, 18] float64 (scratch): one row per workgroup, added in row order.
 * No atomics: two runs give the same bytes.  Two launches. */
int mvster_reg_sums(const float* source, const long* index, const double* dist2, long Q, const float* target, long M,
                    double* partial, double* out, void* stream);

/* hist [bins] uint64 = np.histogram(dist, edges)[0]: dist [N] float32, edges [bins + 1] float64 on the device, non-decreasing;
 * edges[k] <= d < edges[k+1], the last bin closed on the right; NaN and values outside the edges are not counted.  1 <= bins <=
 * 4096.  hist is zeroed here.  Integer atomics (an LDS histogram per workgroup).  Two launches. */
int mvster_reg_histogram(const float* dist, long N, const double* edges, int bins, unsigned long long* hist, void* stream);

/* ---- cleaning a fused cloud: k nearest, outlier filters, normals (csrc/geo_knn.hip, csrc/knn_math.h) ---- */

/* The k nearest targets (1 <= k <= 32) of every query up to max_dist, in ascending (d2, index) order (the definition:
 * csrc/knn_math.h); the grids and max_dist / cell as for mvster_cloud_nn_query.  exclude_self (0 / 1; needs Q == M, the target's
 * points): the target whose index is the query's position is no candidate.  At the query's position: dist2 [Q,k] float64,
 * index [Q,k] int64, count [Q] int32 = min(k, candidates); unfilled places +inf / -1; an invalid query NaN / -1 / 0.  Every
 * check comes before the launch (MVSTER_ERR_SHAPE / MVSTER_ERR_NULL).  One launch, no atomics. */
int mvster_cloud_knn_query(const void* qrecords, const int* qcell, const long* qtotal, long Q, const unsigned long long* keys,
                           const int* cell_of_slot, long table_slots, const long* starts, const void* records, long ncells,
                           long nrecords, float max_dist, float cell, int k, int exclude_self, long M, double* dist2, long* index,
                           int* count, void* stream);

/* The same search of a cloud's grid (records / cell_of_point (= slot) / keys / cell_of_slot / starts of M points with ncells
 * cells and nrecords records) against itself with exclude_self, without the lists in memory: count [M] int32 and mean [M]
 * float64 = (the sum of sqrt(d2) in list order) / k, +inf where count < k, NaN for an invalid point.  One launch. */
int mvster_cloud_knn_mean(const void* records, const int* cell_of_point, long M, const unsigned long long* keys,
                          const int* cell_of_slot, long table_slots, const long* starts, long ncells, long nrecords, float max_dist,
                          float cell, int k, int* count, double* mean, void* stream);

/* The same search, then knn::normal per point: normals [M,3] float32 and valid [M] uint8 (zeros and 0 with fewer than two
 * neighbours or an invalid point).  points [M,3] = the cloud of the grid; toward [M,3] float32 or NULL (raw sign).  One launch. */
int mvster_cloud_knn_normals(const void* records, const int* cell_of_point, long M, const unsigned long long* keys,
                             const int* cell_of_slot, long table_slots, const long* starts, long ncells, long nrecords,
                             float max_dist, float cell, int k, const float* points, const float* toward, float* normals,
                             unsigned char* valid, void* stream);

/* neighbours [M] int32 = the valid points within `radius` of every point of the grid's cloud but the point itself (0 for an
 * invalid point): no list, every shell up to R.  One launch. */
int mvster_cloud_radius_count(const void* records, const int* cell_of_point, long M, const unsigned long long* keys,
                              const int* cell_of_slot, long table_slots, const long* starts, long ncells, long nrecords,
                              float radius, float cell, int* neighbours, void* stream);

/* Rows of `partial` for M means; MVSTER_ERR_SHAPE for M outside 1 .. 2^29. */
int mvster_cloud_knn_stats_rows(long M);

/* stats [0 .. 3] float64 = n, mu, sigma, threshold = mu + std_ratio * sigma over the means that take part (not +inf, not NaN):
 * two passes, partial [rows, 2] float64 (scratch), one row per workgroup, added in row order (csrc/knn_math.h has the order).
 * No atomics: two runs give the same bytes.  std_ratio finite.  Four launches. */
int mvster_cloud_knn_stats(const double* mean, long M, double std_ratio, double* partial, double* stats, void* stream);

/* flags [M] uint8 of the kept points, wg_counts [tiles] int32 and wg_offsets [tiles + 1] int64 over tiles of 256 points
 * (tiles = mvster_reg_blocks(M)) exactly as mvster_reg_crop_flags leaves them, so mvster_reg_crop_emit (T = NULL) compacts in
 * cloud order.  mean != NULL: keep iff mean takes part and mean <= stats[3]; stats[4] = the kept count as a float64 (one
 * read-back for all five).  mean == NULL: keep iff cell_of_point >= 0 and neighbours >= nb_points (>= 1).  No atomics. */
int mvster_cloud_keep_flags(const int* cell_of_point, const int* neighbours, int nb_points, const double* mean, double* stats,
                            long M, unsigned char* flags, int* wg_counts, long* wg_offsets, void* stream);

/* ---- a scan from a structure-from-motion model (csrc/geo_sfm.hip, csrc/sfm_math.h) ---- */

/* q [V,V] uint64 = the quantised pair scores (units of 2^-32) over the points two views share: q[i][j] = q[j][i] = the sum of
 * sfm::quantise(sfm::term(C_i, C_j, X_p)) over the points p both see, the diagonal 0.  centres [V,3] and points [P,3] float64;
 * pt_ptr [P+1] int64 / pt_views [nobs] int32: per point its sorted distinct views; item_ptr [P+1] int64 = the prefix sum of
 * L (L - 1) / 2 over the track lengths L, total = item_ptr[P] (the work items).  1 <= V <= 16384, P >= 0, total <= 2^40,
 * theta0 in 0 .. 180, sigma1, sigma2 >= 0.05 (degrees).  What the tables hold is never used as an address unchecked: an
 * entry out of range adds nothing.  q is zeroed here; integer atomics only, so two runs give the same bytes.  Three launches
 * (one when total = 0). */
int mvster_sfm_pair_scores(const double* centres, int V, const double* points, long P, const long* pt_ptr, const int* pt_views,
                           long nobs, const long* item_ptr, long total, double theta0, double sigma1, double sigma2,
                           unsigned long long* q, void* stream);

/* Per view n [V] int32 = its distinct points with a finite depth z > 0, z = ((r20 x + r21 y) + r22 z_p) + t2 with rt [V,4]
 * float64 = (r20, r21, r22, t2), and depth_min / depth_max [V] float64 = the z of rank n / 100 and (99 n) / 100 in ascending
 * order (NaN for n = 0): an exact radix selection over the bit patterns, one workgroup per view, no sort.  view_ptr [V+1] int64 /
 * view_pts [nobs] int32: per view its sorted distinct points; an entry outside 0 .. P-1 is skipped.  One launch. */
int mvster_sfm_depth_ranges(const double* rt, int V, const double* points, long P, const long* view_ptr, const int* view_pts,
                            long nobs, int* n, double* depth_min, double* depth_max, void* stream);

/* Per row i of q [V,V]: the first num_src (1 .. 64) views j != i with q[i][j] > 0 in (q descending, j ascending) order: index
 * [V,num_src] int32 (-1 where the list ends), value [V,num_src] uint64 (0 there), count [V] int32.  One wave per row.  One launch. */
int mvster_sfm_select_sources(const unsigned long long* q, int V, int num_src, int* index, unsigned long long* value, int* count,
                              void* stream);

/* ---- undistortion of a scan (csrc/geo_undistort.hip, csrc/undistort_math.h) ---- */

/* cams [C,12] float64 = per camera (model id 2 SIMPLE_RADIAL / 3 RADIAL / 4 OPENCV, W, H, fx, fy, cx, cy, k1, k2, p1, p2, pad)
 * -> out [C,8] float64 = the PINHOLE camera of its undistorted image (W', H', fx, fy, cx', cy'), the worst residual of the
 * inversion over the 2 (W + H) border pixel centres (normalised units) and the number of border points whose residual exceeds
 * 1e-9.  0 <= blank_pixels <= 1, 0 < min_scale <= max_scale <= 1024; scale_given != 0: the size comes from (scale_x, scale_y)
 * and the border is not walked (residual 0).  A record that is not a camera (another model, W or H outside 1 .. 2^20, a focal
 * length <= 0) gives zeros with residual +inf.  One workgroup per camera, min / max folds only: the bytes do not depend on the
 * order.  One launch. */
int mvster_undistort_cameras(const double* cams, int C, double blank_pixels, double min_scale, double max_scale, int scale_given,
                             double scale_x, double scale_y, double* out, void* stream);

/* N points xy [N,2] float64 in the pixels of their camera (camera_row [N] int32, rows of cams [C,12]) through its distortion
 * (direction 0) or its inverse (direction 1: ten Newton steps) -> out [N,2] in the same pixel units and residual [N] (0 for
 * direction 0; +inf where the inversion stopped, or the row is outside the table).  One lane per point.  One launch. */
int mvster_undistort_points(const double* cams, int C, const int* camera_row, long N, int direction, const double* xy, double* out,
                            double* residual, void* stream);

/* All views of a chunk in one launch.  views [V,8] int64 = per view (source byte offset into src, destination byte offset into
 * dst, byte offset into valid, Hs, Ws, Hd, Wd, its row in cams [C,12] and ucams [C,8] = the output of mvster_undistort_cameras);
 * the images are uint8 [H,W,3]; dst, valid and the destination and valid offsets are multiples of 16.  group_ptr [V+1] int64 =
 * the prefix sum of ceil(Hd Wd / 4), groups = group_ptr[V].  Every output pixel is the bilinear blend of its four source taps in
 * fp64 rounded to a byte, or (0, 0, 0) with valid = 0 where it looks outside the source.  A view whose extents leave the
 * buffers (src_bytes, dst_bytes, valid_bytes) writes nothing.  No atomics: two runs give the same bytes.  One launch. */
int mvster_undistort_images(const unsigned char* src, long src_bytes, unsigned char* dst, long dst_bytes, unsigned char* valid,
                            long valid_bytes, const long* views, const long* group_ptr, int V, long groups, const double* cams,
                            const double* ucams, int C, void* stream);

/* ---- meshing a scan: TSDF integration and marching tetrahedra (csrc/geo_mesh.hip, csrc/tsdf_math.h) ---- */

/* Tiles of 256 nodes of a grid of `nodes` nodes: the length of vcounts / tcounts; voffsets / toffsets hold one more.
 * MVSTER_ERR_SHAPE for nodes outside 8 .. 2^31 - 1. */
int mvster_mesh_blocks(long nodes);

/* All V views of a scan fused into the grid of nx x ny x nz nodes (each >= 2, at most 2^31 - 1 in all; node (i, j, k) at
 * origin + voxel (i, j, k), index i + nx (j + ny k)) in ONE launch: depth [V,H,W] float32, mask [V,H,W] uint8 (0 = not used),
 * images [V,H,W,3] uint8, views [V,21] float64 = K (9, row major; third row taken as 0 0 1), R (9), t (3), all on the device.
 * Per node, over the views in view order (csrc/tsdf_math.h has every step): the nearest pixel of its projection, the projective
 * distance sdf = d - c_z, dropped below -trunc, f = min(1, sdf / trunc) -> tsdf [n] float32 = the mean of f (1 where no view
 * counted), weight [n] int32 = the views counted, rgb [n,3] uint8 = the rounded mean of the pixels with sdf <= trunc,
 * has_color [n] uint8.  fp64, no atomics: two runs give the same bytes.  MVSTER_ERR_SHAPE before any launch for a bad grid, V, H
 * or W < 1, H or W above 2^20, a voxel or trunc that is not a positive finite number. */
int mvster_tsdf_integrate(const float* depth, const unsigned char* mask, const unsigned char* images, const double* views, int V,
                          int H, int W, double ox, double oy, double oz, double voxel, int nx, int ny, int nz, double trunc,
                          float* tsdf, int* weight, unsigned char* rgb, unsigned char* has_color, void* stream);

/* The counting passes of an extraction (a node is known iff weight >= min_weight, inside iff tsdf < 0; csrc/tsdf_math.h):
 * edge_mask [n] uint8 = bit d (1 .. 7) set where the edge from node n to the node at offset d (bits x, y, z) carries a vertex,
 * rank [n] uint16 = the vertices of the nodes before n in its tile, vcounts / tcounts [tiles] int32 (scratch), voffsets /
 * toffsets [tiles + 1] int64 = the exclusive scans of the vertices and the triangles per tile; their last words are the two
 * counts, the caller's one read-back.  Four launches, no atomics. */
int mvster_mesh_count(const float* tsdf, const int* weight, int nx, int ny, int nz, int min_weight, unsigned char* edge_mask,
                      unsigned short* rank, int* vcounts, int* tcounts, long* voffsets, long* toffsets, void* stream);

/* vertices [Nv,3] float32 and colors [Nv,3] uint8 in the order owner node, then d, with edge_mask / rank / voffsets as
 * mvster_mesh_count left them and Nv the count read back.  Nv = 0 launches nothing; Nv above 2^31 - 1 (the triangles hold int32
 * indices) is MVSTER_ERR_SHAPE and launches nothing.  One launch. */
int mvster_mesh_emit_vertices(const float* tsdf, const unsigned char* rgb, const unsigned char* has_color, double ox, double oy,
                              double oz, double voxel, int nx, int ny, int nz, const unsigned char* edge_mask,
                              const unsigned short* rank, const long* voffsets, long Nv, float* vertices, unsigned char* colors,
                              void* stream);

/* triangles [Nt,3] int32 (vertex numbers, counter-clockwise seen from the tsdf > 0 side) in the order cell, tetrahedron,
 * triangle.  Nt = 0 launches nothing; Nv above 2^31 - 1 is MVSTER_ERR_SHAPE.  One launch. */
int mvster_mesh_emit_triangles(const float* tsdf, const int* weight, int nx, int ny, int nz, int min_weight,
                               const unsigned char* edge_mask, const unsigned short* rank, const long* voffsets,
                               const long* toffsets, long Nv, long Nt, int* triangles, void* stream);

/* ---- brick-sparse TSDF volumes (csrc/geo_mesh_sparse.hip, csrc/tsdf_sparse_math.h).  The virtual grid
 * has nx x ny x nz nodes, each axis 2 .. 2^20 and no limit on the product; a brick is 8 x 8 x 8 nodes, brick (bi, bj, bk) has the
 * number bi + nbx (bj + nby bk) with nb = ceil(n / 8), and the grid may hold at most 2^27 bricks.  A sparse volume is bricks [Nb]
 * int32 (ascending brick numbers), brick_slot [nbricks] int32 (a brick's place in `bricks`, -1 = absent) and brick-major tsdf /
 * weight / has_color [Nb, 512], rgb [Nb, 512, 3]; a node's place in its brick is li + 8 (lj + 8 lk).  It means the dense volume of
 * the same grid with every node of an absent brick at weight 0, tsdf 1.  Every entry point validates before any HIP call; no
 * atomics: two runs give the same bytes. ---- */

/* The bricks of the virtual grid (the length of flags and brick_slot), or MVSTER_ERR_SHAPE where the grid is refused. */
int mvster_tsdf_sparse_bricks(int nx, int ny, int nz);

/* flags [nbricks] uint8 <- 1 for every brick that some pixel with mask != 0 and a finite depth > 0 allocates (its slab between
 * z = max(d - trunc, 0) and d + trunc, back-projected, widened by 2 nodes; K_10 is taken as 0), 0 elsewhere.  depth / mask
 * [V,H,W], views [V,21] as mvster_tsdf_integrate.  One memset and one launch. */
int mvster_tsdf_sparse_mark(const float* depth, const unsigned char* mask, const double* views, int V, int H, int W, double ox,
                            double oy, double oz, double voxel, int nx, int ny, int nz, double trunc, unsigned char* flags,
                            void* stream);

/* counts [ceil(nbricks / 512)] int32 (scratch) and offsets [that + 1] int64 = the exclusive scan of the flags set per tile of 512
 * bricks; its last word is Nb, the caller's one read-back of an allocation.  Two launches. */
int mvster_tsdf_sparse_compact_count(const unsigned char* flags, long nbricks, int* counts, long* offsets, void* stream);

/* brick_slot [nbricks] and bricks [Nb] from the flags and the offsets of mvster_tsdf_sparse_compact_count.  Nb = 0 still writes
 * brick_slot (all -1); bricks may then be NULL.  One launch. */
int mvster_tsdf_sparse_compact_emit(const unsigned char* flags, long nbricks, const long* offsets, long Nb, int* brick_slot,
                                    int* bricks, void* stream);

/* All V views fused into the bricks [Nb] (any ascending set in range) in ONE launch, one workgroup per brick, with
 * tsdf::add_view: the nodes carry exactly what mvster_tsdf_integrate gives them.  Words of a partial brick beyond the grid get
 * weight 0, tsdf 1, rgb 0, has_color 0.  Nb = 0 launches nothing. */
int mvster_tsdf_sparse_integrate(const float* depth, const unsigned char* mask, const unsigned char* images, const double* views,
                                 int V, int H, int W, double ox, double oy, double oz, double voxel, int nx, int ny, int nz,
                                 double trunc, const int* bricks, long Nb, float* tsdf, int* weight, unsigned char* rgb,
                                 unsigned char* has_color, void* stream);

/* The counting passes of a sparse extraction (min_weight >= 1, Nb >= 1): edge_mask [Nb,512] uint8, rank [Nb,512] uint16 = the
 * vertices of the nodes before a node in its brick, vcounts / tcounts [Nb] int32 (scratch), voffsets / toffsets [Nb + 1] int64;
 * their last words are Nv and Nt, the caller's one read-back.  Four launches. */
int mvster_mesh_sparse_count(const float* tsdf, const int* weight, const int* brick_slot, const int* bricks, long Nb, int nx, int ny,
                             int nz, int min_weight, unsigned char* edge_mask, unsigned short* rank, int* vcounts, int* tcounts,
                             long* voffsets, long* toffsets, void* stream);

/* vertices [Nv,3] float32, colors [Nv,3] uint8 and, where keys is not NULL, keys [Nv] int64 = global owner node * 8 + d, in the
 * order (brick, local node, d).  Nv = 0 launches nothing; Nv above 2^31 - 1 is MVSTER_ERR_SHAPE.  One launch. */
int mvster_mesh_sparse_emit_vertices(const float* tsdf, const int* weight, const unsigned char* rgb, const unsigned char* has_color,
                                     const int* brick_slot, const int* bricks, long Nb, double ox, double oy, double oz, double voxel,
                                     int nx, int ny, int nz, const unsigned char* edge_mask, const unsigned short* rank,
                                     const long* voffsets, long Nv, float* vertices, unsigned char* colors, long* keys, void* stream);

/* triangles [Nt,3] int32 in the order (brick, local cell, tetrahedron, triangle).  Nt = 0 launches nothing.  One launch. */
int mvster_mesh_sparse_emit_triangles(const float* tsdf, const int* weight, const int* brick_slot, const int* bricks, long Nb, int nx,
                                      int ny, int nz, int min_weight, const unsigned char* edge_mask, const unsigned short* rank,
                                      const long* voffsets, const long* toffsets, long Nv, long Nt, int* triangles, void* stream);

/* ---- cleaning a mesh: weld, components, compaction, vertex normals (csrc/geo_mesh_clean.hip, csrc/mesh_math.h; DESIGN.md
 * section 4.24).  A mesh is vertices [Nv,3] float32, triangles [Nt,3] int32 with every index in 0 .. Nv-1 (the caller checks
 * that; the kernels leave a triangle with another index out and never reach out of bounds), Nv and Nt at most 2^29. ---- */

/* The lengths of mvster_mesh_clean_plan's scratch, written to two HOST words: *work_ints (int32 entries; 8 Nv + 2 Nt + 3 B with
 * B workgroups of 256 over max(Nv, Nt)) and *work_longs (int64 entries; 3 (B + 1) + 8).  MVSTER_ERR_SHAPE for sizes outside
 * 0 .. 2^29.  The last 8 words of the work_longs buffer are the caller's ONE read-back: Nv', Nt', the components, the canonical
 * vertices, the triangles dropped, the components kept, the weld table's status (1 = full), and the greatest size key. */
int mvster_mesh_clean_work(long Nv, long Nt, long* work_ints, long* work_longs);
/* Workgroups of 256 over Nv vertices: the B of mvster_mesh_vertex_normals' scratch. */
int mvster_mesh_normals_blocks(long Nv);

/* Everything of a clean-up up to the counts.  weld (0 / 1): vertices whose coordinates compare equal become the one with the
 * smallest index, through the open-addressing table `table` [2 * table_slots] int32 (table_slots a power of two, >= max(64,
 * 2 Nv), <= 2^30; not read without weld).  vertices may be NULL without weld (no position is looked at: the components of an
 * index list).  A triangle with two equal canonical corners, or a corner that is not finite, is dropped; the others fall into
 * components by shared canonical vertices; a component is kept iff it has >= min_triangles triangles and, with largest_only,
 * is the one with the most (ties: the smallest root).  -> canon [Nv], labels [Nv] (the smallest vertex of the component; -1
 * for a vertex no kept triangle uses), tri_labels [Nt], tri_component [Nt] (the row in the table; -1 for a dropped triangle),
 * and the table roots / comp_vertices / comp_triangles with room for component_rows rows (min(Nv, Nt) always suffices), roots
 * ascending.  Integer atomics only; the result does not depend on the run.  Nv = 0 or Nt = 0 launches nothing. */
int mvster_mesh_clean_plan(const float* vertices, const int* triangles, long Nv, long Nt, int weld, long min_triangles,
                           int largest_only, int* table, long table_slots, int* canon, int* labels, int* tri_labels,
                           int* tri_component, int* roots, int* comp_vertices, int* comp_triangles, long component_rows,
                           int* work_ints, long* work_longs, void* stream);

/* The kept vertices (with colors [Nv,3] uint8, or NULL) and triangles, in input order, renumbered, with their input numbers in
 * vertex_index / triangle_index (int64), from canon and work_ints as mvster_mesh_clean_plan left them.  NvOut /
 * NtOut: the capacity of the buffers in entries (the counts read back); nothing is written behind them.  One launch; none
 * where both are 0. */
int mvster_mesh_clean_emit(const float* vertices, const unsigned char* colors, const int* triangles, long Nv, long Nt,
                           const int* canon, const int* work_ints, long NvOut, long NtOut,
                           float* out_vertices, unsigned char* out_colors, int* out_triangles, long* vertex_index,
                           long* triangle_index, void* stream);

/* Area-weighted vertex normals: normals [Nv,3] float32 and valid [Nv] uint8 (zeros and 0 where the length is 0 or not finite
 * or no triangle names the vertex).  A vertex sums (b - a) x (c - a) in fp64 over its triangles in ascending triangle index:
 * work_ints [2 Nv + B] int32, work_longs [B + 1] int64 (B = mvster_mesh_normals_blocks(Nv)) and rows [3 Nt] int32 are scratch
 * for the vertex -> triangle rows (integer counts, scan, fill, each row put in order by its lane).  No floating-point atomics;
 * the bytes do not depend on the run.  Nv = 0 launches nothing. */
int mvster_mesh_vertex_normals(const float* vertices, const int* triangles, long Nv, long Nt, int* work_ints, long* work_longs,
                               int* rows, float* normals, unsigned char* valid, void* stream);

/* ---- validation pass (csrc/val_ops.hip): test_sample_depth's metrics and its running averages, no host synchronisation ---- */

/* The depth metrics of a batch (utils.py:125-159: AbsDepthError_metrics, Thres_metrics) without boolean-mask gathers: est,
 * gt, mask [N,HW] (mask > 0.5 = valid), scale [N] or NULL, thres [K] on the HOST (1 <= K <= 8).  For a valid pixel
 * e = |est*s - gt*s| with s = scale[n] (|est - gt| without scale), every operation rounded on its own ->
 * partial [N][mvster_depth_metrics_slots(HW)][2+K] doubles (scratch), raw [N][2+K] doubles = valid pixels, sum of e
 * (fp64), #{e > thres[k]} (strict, IEEE: a NaN error counts for no threshold and makes the sum NaN, inf counts for all),
 * out [1+K] floats = abs_depth_error, thres_k errors: per image (float)(x / valid) with the quotient in double, then the
 * fp32 mean over the images in image order (compute_metrics_for_each_image, :126-136); an image without a valid pixel
 * gives NaN, like torch.mean of an empty tensor.  Two launches, no atomics: bit-reproducible. */
int mvster_depth_metrics_slots(long hw);
int mvster_depth_metrics(const float* est, const float* gt, const float* mask, const float* scale, const float* thres, int K,
                         int N, long HW, double* partial, double* raw, float* out, void* stream);

/* Blend_loss's error figures (MVS4Net.py:202-205) without a boolean-mask gather, pooled over ALL valid pixels of the batch
 * (not per image): arguments, e and the scratch as for mvster_depth_metrics; thres [K] on the HOST is read before the call
 * returns (the kernels get the values) -> raw [N][2+K] doubles = valid pixels, sum of e (fp64), #{e <= thres[k]} (counted
 * as such, IEEE: a NaN error at a valid pixel is in the denominator only, +inf is at-or-below nothing),
 * out [1+K] floats: with the columns of raw summed over the images in image order (counts exact, the sum fp64),
 * epe = (float)(sum_e / valid) and err_k = fl32(fl32(le_k / valid) * 100): the quotients in double, rounded once to fp32,
 * then an fp32 multiply; a batch without a valid pixel gives NaN.  Two launches, no atomics: bit-reproducible, whatever the
 * planes' alignment. */
int mvster_pooled_metrics(const float* est, const float* gt, const float* mask, const float* scale, const float* thres, int K,
                          int N, long HW, double* partial, double* raw, float* out, void* stream);

/* DictAverageMeter.update (utils.py:108-119) on the device: sums [n] doubles += row [n] floats, count [1] += 1 (Python
 * floats are doubles: the same sums in the same order); mvster_scalar_reset zeroes both (a kernel, not a memset node).
 * One single-workgroup launch each, reading and writing only through the arguments: capturable. */
int mvster_scalar_accumulate(const float* row, int n, double* sums, long* count, void* stream);
int mvster_scalar_reset(double* sums, int n, long* count, void* stream);

/* A training step's scalars, each a device tensor of its own, into one row and into the running sums in ONE launch: ptrs [n]
 * on the HOST holds the device address of every scalar (1 <= n <= 32, none NULL; read before the call returns) ->
 * row [n] floats = the scalars, sums [n] doubles += them, count [1] += 1 -- what torch.stack followed by
 * mvster_scalar_accumulate leaves.  Capturable: the addresses are kernel arguments. */
int mvster_scalar_gather_accumulate(const void* const* ptrs, int n, float* row, double* sums, long* count, void* stream);

/* Name of the kernel the most recent mvster_conv_mfma / mvster_conv_small / mvster_deconv_small / mvster_conv_wgrad /
 * mvster_warp_agg_fwd / mvster_warp_agg_bwd (first pass) call on the calling host thread launched, in the profiler's spelling with template arguments (e.g. "conv_lds_kernel<2, 1, 3, 1, 3>");
 * "" before the first call.  The pointer stays valid for the life of the library.  (bench.py attributes HIP-event timings
 * with it; there is no reference counterpart -- the reference's dispatch lives inside cuDNN.) */
const char* mvster_last_kernel(void);

/* Build flags of the loaded library: bit 0 = probe build (make -C mvster_amd/csrc probes).  The product library (0) reads no
 * environment variable and returns MVSTER_ERR_UNSUPPORTED for the kernel forms kept for the record only: warp variants 4
 * (pixel-major) and 5 (LDS-staged source windows), convolution variant 7 (ping-pong). */
int mvster_build_flags(void);

/* One v_mfma_f32_16x16x4_f32: A [16,4], B [4,16] -> D [16,16] (row major).  Test hook that pins the
 * fragment layout the convolution kernels assume. */
int mvster_mfma_probe(const float* A, const float* B, float* D, void* stream);

#ifdef __cplusplus
}
#endif
#endif
