"""Case table, inputs and fp64 references for the weight-gradient kernels (mvster_amd/csrc/conv_wgrad.hip,
conv_wgrad_pers.hip) -- importable without a GPU; test_wgrad_cases_cpu.py checks the table, test_gpu_wgrad.py runs it.

A case is one call of ``ops.conv_wgrad`` as the kernels see it: the operand in the x role [B,D,H,W,CI] (the shifted
tensor), the operand in the gy role [B,Do,Ho,Wo,CO], the tap shape, stride and padding, the channels to keep, an optional
cap on the slots of ``partial`` (ops.WGRAD_MAX_SLOTS) and the kernel instantiation the dispatch must pick.

The geometries come from the dispatch code, not from the network's shapes:
  * persistent kernel: a unit is R output rows x XC columns; XC = 80 where ceil(W / 80) * 80 wastes fewer columns than
    ceil(W / 64) * 64 (W = 65 .. 80, 129 .. 160), XC = 48 likewise for the 27-tap form (W = 47, 130); R = 4 or 2;
    H in {1, 3, 5, 7} leaves a row block shorter than R and a partial last block; a slot cap of 1 / 3 makes one workgroup
    walk many units (the double buffer's ``it & 1`` alternation), and at the default cap the small cases have more
    workgroups than units (the idle ones only zero-fill);
  * LDS-staged kernel: 64-column chunks of one output row, Wo in {1, 15, 63, 64, 65, 129}; stride 2 with odd input sizes
    and a second chunk (9 x 33, 10 x 130, 7 x 129); a slot cap of 5 on B * D * H = 2 * 3 * 7 rows wraps the ``advance``
    row step across a D and a B boundary;
  * per-tap kernels: what neither takes -- 27 taps at stride 2, channel counts that are no multiple of 4, 72 outputs with
    more than one tap; a slot cap of 2 on 11 rows wraps the ``gridDim.x * 4`` row loop with a remainder.
"""
import collections
import zlib

import torch
import torch.nn.functional as F

K111, K133, K333, K155 = (1, 1, 1), (1, 3, 3), (3, 3, 3), (1, 5, 5)
S111, S122, S222 = (1, 1, 1), (1, 2, 2), (2, 2, 2)
P_MAX = 1 << 20        # output voxels per case: with |x|, |gy| <= 2 every partial sum stays below 2^22 < 2^24, exact in fp32
KERNELS = {"pers": "conv_wgrad_pers_kernel", "lds": "conv_wgrad_lds_kernel", "packed": "conv_wgrad_packed_kernel",
           "tap": "conv_wgrad_kernel"}

Case = collections.namedtuple("Case", "name form CI CO kernel stride padding B D H W slots co_keep ci_keep kernel_name")


def C(name, form, CI, CO, kernel, stride, shape, kernel_name, slots=None, co_keep=None, ci_keep=None):
    """One table row.  ``shape`` = (B, D, H, W) of the operand in the x role; the padding is k // 2 everywhere (its own
    mirror image, k - 1 - p, for the mirrored form); ``kernel_name`` abbreviates the family ("pers<...>" etc.)."""
    family, args = kernel_name.split("<", 1)
    B, D, H, W = shape
    return Case(name, form, CI, CO, kernel, stride, tuple(k // 2 for k in kernel), B, D, H, W, slots,
                CO if co_keep is None else co_keep, CI if ci_keep is None else ci_keep, KERNELS[family] + "<" + args)


# form: "plain" / "transposed" / "mirrored" = the three branches of train_ops._ConvCL.backward (see layer_form; for the
# transposed form the x role is the layer's OUTPUT gradient), "direct" = a direct ops.conv_wgrad call no layer makes.
CASES = [
    # ---- persistent kernel, 9 taps: <MT, NT, 1, R, XC> --------------------------------------------------------------
    C("p1_16_16_w63_h3", "plain", 16, 16, K133, S111, (1, 1, 3, 63), "pers<1, 1, 1, 4, 64>"),
    C("p1_16_16_w64_h5", "plain", 16, 16, K133, S111, (2, 2, 5, 64), "pers<1, 1, 1, 4, 64>"),
    C("p1_16_16_w65_h1", "plain", 16, 16, K133, S111, (1, 1, 1, 65), "pers<1, 1, 1, 4, 80>"),
    C("p1_16_16_w80_h7", "plain", 16, 16, K133, S111, (1, 1, 7, 80), "pers<1, 1, 1, 4, 80>"),
    C("p1_16_16_w81_h5", "plain", 16, 16, K133, S111, (1, 1, 5, 81), "pers<1, 1, 1, 4, 64>"),
    C("p1_16_16_w100_h3", "plain", 16, 16, K133, S111, (1, 1, 3, 100), "pers<1, 1, 1, 4, 64>"),
    C("p1_16_16_w130_h3", "plain", 16, 16, K133, S111, (2, 2, 3, 130), "pers<1, 1, 1, 4, 80>"),
    C("p1_16_32_w63_h5", "plain", 16, 32, K133, S111, (1, 1, 5, 63), "pers<2, 1, 1, 4, 64>"),
    C("p1_16_32_w100_h3", "plain", 16, 32, K133, S111, (1, 1, 3, 100), "pers<2, 1, 1, 4, 64>"),
    C("p1_16_32_w65_h7", "plain", 16, 32, K133, S111, (1, 1, 7, 65), "pers<2, 1, 1, 4, 80>"),
    C("p1_16_32_w130_h5", "plain", 16, 32, K133, S111, (2, 2, 5, 130), "pers<2, 1, 1, 4, 80>"),
    C("p1_32_16_w64_h7", "plain", 32, 16, K133, S111, (1, 1, 7, 64), "pers<1, 2, 1, 4, 64>"),
    C("p1_32_16_w81_h1", "plain", 32, 16, K133, S111, (1, 1, 1, 81), "pers<1, 2, 1, 4, 64>"),
    C("p1_32_16_w80_h3", "plain", 32, 16, K133, S111, (1, 1, 3, 80), "pers<1, 2, 1, 2, 80>"),
    C("p1_32_16_w130_h5", "plain", 32, 16, K133, S111, (2, 2, 5, 130), "pers<1, 2, 1, 2, 80>"),
    C("p1_32_32_w63_h1", "plain", 32, 32, K133, S111, (1, 1, 1, 63), "pers<2, 2, 1, 2, 64>"),
    C("p1_32_32_w100_h5", "plain", 32, 32, K133, S111, (1, 1, 5, 100), "pers<2, 2, 1, 2, 64>"),
    C("p1_32_32_w80_h3", "plain", 32, 32, K133, S111, (2, 2, 3, 80), "pers<2, 2, 1, 2, 80>"),
    C("p1_32_32_w130_h7", "plain", 32, 32, K133, S111, (1, 1, 7, 130), "pers<2, 2, 1, 2, 80>"),
    C("p1_64_64_w64_h3", "plain", 64, 64, K133, S111, (1, 1, 3, 64), "pers<2, 2, 1, 2, 64>"),
    C("p1_64_64_w81_h7", "plain", 64, 64, K133, S111, (1, 1, 7, 81), "pers<2, 2, 1, 2, 64>"),
    C("p1_64_64_w65_h5", "plain", 64, 64, K133, S111, (1, 1, 5, 65), "pers<2, 2, 1, 2, 80>"),
    C("p1_64_64_w130_h1", "plain", 64, 64, K133, S111, (1, 1, 1, 130), "pers<2, 2, 1, 2, 80>"),
    C("p1_64_32_w63_h7", "plain", 64, 32, K133, S111, (2, 2, 7, 63), "pers<2, 2, 1, 2, 64>"),
    C("p1_64_32_w80_h5", "plain", 64, 32, K133, S111, (1, 1, 5, 80), "pers<2, 2, 1, 2, 80>"),
    C("p1_64_16_w100_h3", "plain", 64, 16, K133, S111, (1, 1, 3, 100), "pers<1, 2, 1, 4, 64>"),
    C("p1_64_16_w65_h3", "plain", 64, 16, K133, S111, (1, 1, 3, 65), "pers<1, 2, 1, 2, 80>"),
    # units per workgroup: 2 * 2 * ceil(7 / R) * 2 = 16 (R = 4) or 32 (R = 2) units on 1 slot and on 3 (6 + 5 + 5, 11 + 11 + 10)
    C("p1_16_16_w100_h7_s1", "plain", 16, 16, K133, S111, (2, 2, 7, 100), "pers<1, 1, 1, 4, 64>", slots=1),
    C("p1_16_16_w100_h7_s3", "plain", 16, 16, K133, S111, (2, 2, 7, 100), "pers<1, 1, 1, 4, 64>", slots=3),
    C("p1_16_32_w100_h7_s1", "plain", 16, 32, K133, S111, (2, 2, 7, 100), "pers<2, 1, 1, 4, 64>", slots=1),
    C("p1_16_32_w100_h7_s3", "plain", 16, 32, K133, S111, (2, 2, 7, 100), "pers<2, 1, 1, 4, 64>", slots=3),
    C("p1_32_16_w100_h7_s1", "plain", 32, 16, K133, S111, (2, 2, 7, 100), "pers<1, 2, 1, 4, 64>", slots=1),
    C("p1_32_16_w100_h7_s3", "plain", 32, 16, K133, S111, (2, 2, 7, 100), "pers<1, 2, 1, 4, 64>", slots=3),
    C("p1_32_32_w100_h7_s1", "plain", 32, 32, K133, S111, (2, 2, 7, 100), "pers<2, 2, 1, 2, 64>", slots=1),
    C("p1_32_32_w100_h7_s3", "plain", 32, 32, K133, S111, (2, 2, 7, 100), "pers<2, 2, 1, 2, 64>", slots=3),
    C("p1_32_32_w130_h7_s3", "plain", 32, 32, K133, S111, (2, 2, 7, 130), "pers<2, 2, 1, 2, 80>", slots=3),
    # ---- persistent kernel, 27 taps: <1, 1, 3, 2, XC>; D = 1, 2, 3: the depth padding meets both faces ---------------
    C("p3_16_w47_h3_d1", "plain", 16, 16, K333, S111, (1, 1, 3, 47), "pers<1, 1, 3, 2, 48>"),
    C("p3_16_w49_h5_d2", "plain", 16, 16, K333, S111, (1, 2, 5, 49), "pers<1, 1, 3, 2, 64>"),
    C("p3_16_w100_h3_d3", "plain", 16, 16, K333, S111, (2, 3, 3, 100), "pers<1, 1, 3, 2, 64>"),
    C("p3_16_w130_h5_d2", "plain", 16, 16, K333, S111, (1, 2, 5, 130), "pers<1, 1, 3, 2, 48>"),
    C("p3_32_w47_h5_d3", "plain", 32, 32, K333, S111, (1, 3, 5, 47), "pers<1, 1, 3, 2, 48>"),
    C("p3_32_w100_h3_d1", "plain", 32, 32, K333, S111, (1, 1, 3, 100), "pers<1, 1, 3, 2, 64>"),
    C("p3_32_w130_h3_d2", "plain", 32, 32, K333, S111, (2, 2, 3, 130), "pers<1, 1, 3, 2, 48>"),
    C("p3_64_w49_h3_d2", "plain", 64, 64, K333, S111, (1, 2, 3, 49), "pers<1, 1, 3, 2, 64>"),
    C("p3_64_w130_h3_d3", "plain", 64, 64, K333, S111, (1, 3, 3, 130), "pers<1, 1, 3, 2, 48>"),
    C("p3_64_w47_h5_d1", "plain", 64, 64, K333, S111, (2, 1, 5, 47), "pers<1, 1, 3, 2, 48>"),
    C("p3_16_w100_h3_d2_s1", "plain", 16, 16, K333, S111, (2, 2, 3, 100), "pers<1, 1, 3, 2, 64>", slots=1),
    C("p3_16_w100_h3_d2_s3", "plain", 16, 16, K333, S111, (2, 2, 3, 100), "pers<1, 1, 3, 2, 64>", slots=3),
    C("p3_32_w130_h5_d1_s3", "plain", 32, 32, K333, S111, (2, 1, 5, 130), "pers<1, 1, 3, 2, 48>", slots=3),
    # ---- LDS-staged kernel <MT, NT, TY, KW, PCB, SW>: 1x1 (8 -> 1 is the padded `prob` head, 64 -> 72 (pitch 80) the
    #      FPN gather) ----------------------------------------------------------------------------------------------------
    C("l1_64_64_w65", "plain", 64, 64, K111, S111, (2, 1, 3, 65), "lds<2, 4, 1, 1, 0, 1>"),
    C("l1_32_64_w129", "plain", 32, 64, K111, S111, (1, 1, 2, 129), "lds<4, 2, 1, 1, 0, 1>"),
    C("l1_16_64_w63", "plain", 16, 64, K111, S111, (1, 1, 5, 63), "lds<4, 1, 1, 1, 0, 1>"),
    C("l1_8_64_w15", "plain", 8, 64, K111, S111, (2, 1, 7, 15), "lds<4, 1, 1, 1, 0, 1>"),
    C("l1_8_1_w64", "plain", 8, 4, K111, S111, (1, 3, 3, 64), "lds<1, 1, 1, 1, 0, 1>", co_keep=1),
    C("l1_8_1_w1", "plain", 8, 4, K111, S111, (2, 2, 5, 1), "lds<1, 1, 1, 1, 0, 1>", co_keep=1),
    C("l1_64_72_w65", "direct", 64, 72, K111, S111, (1, 1, 3, 65), "lds<5, 2, 1, 1, 0, 1>"),
    C("l1_64_72_w15", "plain", 64, 80, K111, S111, (2, 1, 5, 15), "lds<5, 2, 1, 1, 0, 1>", co_keep=72),
    C("l1_8_72_w63", "direct", 8, 72, K111, S111, (1, 1, 3, 63), "lds<5, 1, 1, 1, 0, 1>"),
    C("l1_48_64_w64", "direct", 48, 64, K111, S111, (1, 1, 3, 64), "lds<2, 4, 1, 1, 0, 1>"),
    C("l1_16_48_w129", "direct", 16, 48, K111, S111, (1, 1, 1, 129), "lds<4, 1, 1, 1, 0, 1>"),
    C("l1_32_64_w15_s5", "plain", 32, 64, K111, S111, (2, 3, 7, 15), "lds<4, 2, 1, 1, 0, 1>", slots=5),
    # ---- 3x3 stride 2 (and the ConvTranspose twins: the x role is the up-sampled side) ----------------------------------
    C("l3s2_16_32_9x33", "plain", 16, 32, K133, S122, (2, 2, 9, 33), "lds<1, 1, 3, 3, 0, 2>"),
    C("l3s2_16_32_10x130", "plain", 16, 32, K133, S122, (1, 1, 10, 130), "lds<1, 1, 3, 3, 0, 2>"),
    C("l3s2_16_32_7x129", "plain", 16, 32, K133, S122, (1, 1, 7, 129), "lds<1, 1, 3, 3, 0, 2>"),
    C("l3s2_16_32_10x130_t", "transposed", 16, 32, K133, S122, (1, 2, 10, 130), "lds<1, 1, 3, 3, 0, 2>"),
    C("l3s2_16_32_13x33_s5", "plain", 16, 32, K133, S122, (2, 3, 13, 33), "lds<1, 1, 3, 3, 0, 2>", slots=5),
    C("l3s2_8_16_9x33", "plain", 8, 16, K133, S122, (1, 1, 9, 33), "lds<1, 1, 3, 3, 8, 2>"),
    C("l3s2_8_16_7x129", "plain", 8, 16, K133, S122, (2, 1, 7, 129), "lds<1, 1, 3, 3, 8, 2>"),
    C("l3s2_8_16_10x130", "plain", 8, 16, K133, S122, (1, 2, 10, 130), "lds<1, 1, 3, 3, 8, 2>"),
    C("l3s2_8_16_10x130_t", "transposed", 8, 16, K133, S122, (1, 1, 10, 130), "lds<1, 1, 3, 3, 8, 2>"),
    # (32 -> 64: one 16 x 16 tile pair per workgroup since the accumulator limit of 12 -- 41 KB of LDS, not the per-tap
    #  kernel that conv_wgrad.hip's note on layers above 64 KB still speaks of)
    C("l3s2_32_64_9x33", "plain", 32, 64, K133, S122, (2, 1, 9, 33), "lds<1, 1, 3, 3, 0, 2>"),
    C("l3s2_32_64_7x129", "plain", 32, 64, K133, S122, (1, 1, 7, 129), "lds<1, 1, 3, 3, 0, 2>"),
    C("l3s2_32_64_10x130_t", "transposed", 32, 64, K133, S122, (1, 2, 10, 130), "lds<1, 1, 3, 3, 0, 2>"),
    # ---- 5x5 stride 2: the staged patch is 131 pixels wide; unpacked it needs 65.4 KB (the 80 KB form) -----------------
    C("l5s2_8_16_9x33", "plain", 8, 16, K155, S122, (2, 1, 9, 33), "lds<1, 1, 5, 5, 8, 2>"),
    C("l5s2_8_16_10x130", "plain", 8, 16, K155, S122, (1, 1, 10, 130), "lds<1, 1, 5, 5, 8, 2>"),
    C("l5s2_8_16_7x129", "plain", 8, 16, K155, S122, (1, 1, 7, 129), "lds<1, 1, 5, 5, 8, 2>"),
    C("l5s2_16_32_9x33", "plain", 16, 32, K155, S122, (1, 1, 9, 33), "lds<1, 1, 5, 5, 0, 2>"),
    C("l5s2_16_32_10x130", "plain", 16, 32, K155, S122, (2, 1, 10, 130), "lds<1, 1, 5, 5, 0, 2>"),
    C("l5s2_16_32_7x129", "plain", 16, 32, K155, S122, (1, 1, 7, 129), "lds<1, 1, 5, 5, 0, 2>"),
    C("l5s2_16_32_13x33_s5", "plain", 16, 32, K155, S122, (2, 3, 13, 33), "lds<1, 1, 5, 5, 0, 2>", slots=5),
    C("l5s2_32_64_9x33", "plain", 32, 64, K155, S122, (1, 1, 9, 33), "lds<1, 1, 5, 5, 0, 2>"),
    C("l5s2_32_64_10x130", "plain", 32, 64, K155, S122, (1, 1, 10, 130), "lds<1, 1, 5, 5, 0, 2>"),
    C("l5s2_32_64_7x129", "plain", 32, 64, K155, S122, (2, 1, 7, 129), "lds<1, 1, 5, 5, 0, 2>"),
    C("l5s1_16_16_w65", "direct", 16, 16, K155, S111, (1, 1, 5, 65), "lds<1, 1, 5, 5, 0, 1>"),
    # ---- 27 taps: packed two (PCB 8) or four (PCB 4) per tile -- 27 is no multiple of either: dead tap columns ----------
    C("l27_8_8_w15_d1", "plain", 8, 8, K333, S111, (1, 1, 3, 15), "lds<1, 1, 9, 3, 8, 1>"),
    C("l27_8_8_w65_d2", "plain", 8, 8, K333, S111, (2, 2, 3, 65), "lds<1, 1, 9, 3, 8, 1>"),
    C("l27_8_8_w129_d3", "plain", 8, 8, K333, S111, (1, 3, 2, 129), "lds<1, 1, 9, 3, 8, 1>"),
    C("l27_8_8_w15_d3_s5", "plain", 8, 8, K333, S111, (2, 3, 7, 15), "lds<1, 1, 9, 3, 8, 1>", slots=5),
    C("l27_8_1_w63_d2", "plain", 8, 4, K333, S111, (1, 2, 3, 63), "lds<1, 1, 9, 3, 8, 1>", co_keep=1),
    C("l27_8_1_w1_d3", "plain", 8, 4, K333, S111, (2, 3, 5, 1), "lds<1, 1, 9, 3, 8, 1>", co_keep=1),
    C("l27_4_8_w64_d2", "plain", 4, 8, K333, S111, (1, 2, 3, 64), "lds<1, 1, 9, 3, 4, 1>"),
    C("l27_4_8_w65_d1", "plain", 4, 8, K333, S111, (2, 1, 2, 65), "lds<1, 1, 9, 3, 4, 1>"),
    C("l27_48_48_w65_d2", "direct", 48, 48, K333, S111, (1, 2, 3, 65), "lds<1, 1, 9, 3, 0, 1>"),
    # ---- 9 taps: packed (4 per tile leaves three dead columns), the mirrored narrow-output layers, 48 channels ----------
    C("l9_3_8_w63", "plain", 4, 8, K133, S111, (2, 1, 3, 63), "lds<1, 1, 3, 3, 4, 1>", ci_keep=3),
    C("l9_4_8_w129", "plain", 4, 8, K133, S111, (1, 1, 2, 129), "lds<1, 1, 3, 3, 4, 1>"),
    C("l9_8_8_w1", "plain", 8, 8, K133, S111, (2, 2, 5, 1), "lds<1, 1, 3, 3, 8, 1>"),
    C("l9_8_8_w65", "plain", 8, 8, K133, S111, (1, 1, 3, 65), "lds<1, 1, 3, 3, 8, 1>"),
    C("l9_8_8_w15_s5", "plain", 8, 8, K133, S111, (2, 3, 7, 15), "lds<1, 1, 3, 3, 8, 1>", slots=5),
    C("l9m_8_64_w64", "mirrored", 8, 64, K133, S111, (1, 2, 3, 64), "lds<2, 1, 3, 3, 8, 1>"),
    C("l9m_8_64_w15", "mirrored", 8, 64, K133, S111, (2, 1, 5, 15), "lds<2, 1, 3, 3, 8, 1>"),
    C("l9m_8_16_w65", "mirrored", 8, 16, K133, S111, (1, 1, 3, 65), "lds<1, 1, 3, 3, 8, 1>"),
    C("l9m_1_16_w63", "mirrored", 4, 16, K133, S111, (2, 1, 3, 63), "lds<1, 1, 3, 3, 4, 1>", ci_keep=1),
    C("l9m_1_32_w129", "mirrored", 4, 32, K133, S111, (1, 1, 2, 129), "lds<2, 1, 3, 3, 4, 1>", ci_keep=1),
    C("l9m_1_64_w15", "mirrored", 4, 64, K133, S111, (1, 2, 3, 15), "lds<4, 1, 3, 3, 4, 1>", ci_keep=1),
    C("l9m_1_64_w65", "mirrored", 4, 64, K133, S111, (2, 1, 2, 65), "lds<4, 1, 3, 3, 4, 1>", ci_keep=1),
    C("l9_48_16_w65", "direct", 48, 16, K133, S111, (1, 2, 3, 65), "lds<1, 1, 3, 3, 0, 1>"),
    C("l9_16_48_w15", "direct", 16, 48, K133, S111, (2, 1, 5, 15), "lds<1, 1, 3, 3, 0, 1>"),
    C("l9_16_8_w64", "direct", 16, 8, K133, S111, (1, 1, 3, 64), "lds<1, 1, 3, 3, 0, 1>", co_keep=6, ci_keep=12),
    # (five M tiles on the packed path: they do not halve, so one tile per workgroup -- the halving once left 2 x 2 tiles
    #  and rows 64 .. 79 of every slot unwritten)
    C("l9_8_72_w65", "direct", 8, 72, K133, S111, (1, 1, 3, 65), "lds<1, 1, 3, 3, 8, 1>"),
    C("l9_4_72_w15", "direct", 4, 80, K133, S111, (2, 1, 3, 15), "lds<1, 1, 3, 3, 4, 1>", co_keep=72),
    # ---- per-tap kernels: 27 taps at stride (2, 2, 2) (reg3d's down- and up-sampling layers) ----------------------------
    C("f27s2_8_16_w37", "plain", 8, 16, K333, S222, (1, 3, 9, 37), "packed<1, 8>"),
    C("f27s2_8_16_w16_t", "transposed", 8, 16, K333, S222, (2, 4, 10, 16), "packed<1, 8>"),
    C("f27s2_16_32_w17", "plain", 16, 32, K333, S222, (2, 2, 7, 17), "tap<2, 1>"),
    C("f27s2_16_32_w16_t", "transposed", 16, 32, K333, S222, (1, 4, 6, 16), "tap<2, 1>"),
    C("f27s2_32_64_w37", "plain", 32, 64, K333, S222, (1, 3, 5, 37), "tap<4, 2>"),
    C("f27s2_32_64_w16_t", "transposed", 32, 64, K333, S222, (2, 2, 4, 16), "tap<4, 2>"),
    # ---- per-tap kernels: channel counts that are no multiple of 4, 72 outputs with 9 taps, the wrapping row loop -------
    C("fd_3_6_k13_w17", "direct", 3, 6, K133, S111, (2, 1, 5, 17), "packed<1, 4>"),
    C("fd_16_1_k13_w37", "direct", 16, 1, K133, S111, (1, 1, 3, 37), "tap<1, 1>"),
    C("fd_3_1_k11_w16", "direct", 3, 1, K111, S111, (1, 2, 7, 16), "tap<1, 1>"),
    C("fd_32_6_k33_w5", "direct", 32, 6, K333, S111, (2, 2, 3, 5), "tap<1, 2>"),
    C("fd_64_72_k13_w17", "direct", 64, 72, K133, S111, (1, 1, 3, 17), "tap<5, 4>"),
    C("fd_3_64_k13_w37", "direct", 3, 64, K133, S111, (1, 1, 5, 37), "packed<4, 4>"),
    C("fd_6_32_k13_w16", "direct", 6, 32, K133, S111, (2, 1, 3, 16), "packed<2, 8>"),
    C("fd_3_6_k13_w17_s2", "direct", 3, 6, K133, S111, (1, 1, 11, 17), "packed<1, 4>", slots=2),
    C("fd_16_6_k13_w5_s2", "direct", 16, 6, K133, S111, (1, 1, 11, 5), "tap<1, 1>", slots=2),
    C("fd_6_16_k33_w16", "direct", 6, 16, K333, S222, (1, 3, 5, 16), "packed<1, 8>"),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]


def out_size(c):
    """(Do, Ho, Wo) of a case: the convolution's output size for (kernel, stride, padding)."""
    return tuple((n + 2 * p - k) // s + 1 for n, k, s, p in zip((c.D, c.H, c.W), c.kernel, c.stride, c.padding))


_ALLOWED_CIN = (4, 8, 16, 32, 64)      # train_ops._ALLOWED_CIN


def _cin_for(c):
    return next(a for a in _ALLOWED_CIN if c <= a)


def layer_form(module_kind, cin, cout, kernel, stride, padding=None):
    """The ``ops.conv_wgrad`` call that ``train_ops._ConvCL.backward`` makes for a layer (a mirror of its three-way branch):
    ``module_kind`` "conv" (nn.Conv2d / nn.Conv3d) or "convT" (nn.ConvTranspose3d), channels as the module has them, 3-D
    kernel and stride -> (form, CI, CO, kernel, stride, padding, co_keep, ci_keep) as conv_wgrad receives them."""
    kernel, stride = tuple(kernel), tuple(stride)
    padding = tuple(k // 2 for k in kernel) if padding is None else tuple(padding)
    cin_p, co_p = _cin_for(cin), _cin_for(cout)
    if module_kind == "convT":
        return ("transposed", co_p, cin_p, kernel, stride, padding, cin, cout)
    if stride == (1, 1, 1) and cout <= 8 < cin_p and kernel != (1, 1, 1):
        return ("mirrored", co_p, cin_p, kernel, stride, tuple(k - 1 - p for k, p in zip(kernel, padding)), cin, cout)
    return ("plain", cin_p, co_p, kernel, stride, padding, cout, cin)


def reference_dw(x, gy, kernel, stride, padding, co_keep=None, ci_keep=None, mirrored=False):
    """fp64 CPU reference of ``ops.conv_wgrad``: x [B,Di,Hi,Wi,CI], gy [B,Do,Ho,Wo,CO] channels-last -> autograd of
    F.conv3d on NCDHW doubles, dW [CO,CI,k] sliced [:co_keep, :ci_keep]; ``mirrored``: taps flipped, channel axes
    exchanged, [:ci_keep, :co_keep]."""
    CI, CO = x.shape[-1], gy.shape[-1]
    co_keep = CO if co_keep is None else co_keep
    ci_keep = CI if ci_keep is None else ci_keep
    xd = x.detach().cpu().double().permute(0, 4, 1, 2, 3).contiguous()
    w = torch.zeros((CO, CI) + tuple(kernel), dtype=torch.float64, requires_grad=True)
    y = F.conv3d(xd, w, None, stride=tuple(stride), padding=tuple(padding))
    gd = gy.detach().cpu().double().permute(0, 4, 1, 2, 3)
    assert tuple(y.shape) == tuple(gd.shape), (tuple(y.shape), tuple(gd.shape))
    y.backward(gd)
    dw = w.grad
    if mirrored:
        return dw.flip(2, 3, 4).transpose(0, 1)[:ci_keep, :co_keep].contiguous()
    return dw[:co_keep, :ci_keep].contiguous()


def make_inputs(c, exact):
    """(x, gy) of a case, fp32 on the CPU, seeded by its name.  ``exact``: integers uniform in {-2, ..., 2} -- every
    product is an integer of magnitude <= 4 and every partial sum of at most P_MAX of them is below 2^24, so any summation
    order gives the fp64 result bit for bit; else standard normal."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + (0 if exact else 1))
    Do, Ho, Wo = out_size(c)
    xs, gs = (c.B, c.D, c.H, c.W, c.CI), (c.B, Do, Ho, Wo, c.CO)
    if exact:
        return (torch.randint(-2, 3, xs, generator=g).float(), torch.randint(-2, 3, gs, generator=g).float())
    return torch.randn(xs, generator=g), torch.randn(gs, generator=g)


_REFERENCE = {}


def case_data(c, exact):
    """(x, gy, reference dW) of a case, computed once and shared (nobody writes into them)."""
    key = (c.name, bool(exact))
    if key not in _REFERENCE:
        x, gy = make_inputs(c, exact)
        _REFERENCE[key] = (x, gy, reference_dw(x, gy, c.kernel, c.stride, c.padding, c.co_keep, c.ci_keep, c.form == "mirrored"))
    return _REFERENCE[key]


def finish_reference(partial, ntaps, cip, co_lim, ci_lim, swap, flip):
    """The finish kernel in torch index arithmetic, after the layout comment above FinishArgs (conv_wgrad.hip):
    partial [nblk, ngrp, cop, width] -> the slot sum's kept elements, dw [co_lim, ci_lim, ntaps] (swap: [ci_lim, co_lim,
    ntaps]).  Dropped positions (tap >= ntaps, co >= co_lim, ci >= ci_lim) are never read."""
    nblk, ngrp, cop, width = partial.shape
    g, co, col = torch.meshgrid(torch.arange(ngrp), torch.arange(cop), torch.arange(width), indexing="ij")
    if cip:
        tap, ci = g * (16 // cip) + col // cip, col % cip
    else:
        tap, ci = g, col
    keep = (tap < ntaps) & (co < co_lim) & (ci < ci_lim)
    g, co, col, tap, ci = g[keep], co[keep], col[keep], tap[keep], ci[keep]
    vals = partial.double()[:, g, co, col].sum(0)
    if flip:
        tap = ntaps - 1 - tap
    dw = torch.full((ci_lim, co_lim, ntaps) if swap else (co_lim, ci_lim, ntaps), float("nan"), dtype=torch.float64)
    if swap:
        dw[ci, co, tap] = vals
    else:
        dw[co, ci, tap] = vals
    return dw
