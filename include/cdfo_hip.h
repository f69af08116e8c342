/* cdfo_hip.h -- C-ABI of libcdfo_hip.so: the MI355X (gfx950) kernels behind the CDFO CVSR_V8 forward path
 * and the ops/dcn deformable-convolution operator.
 *
 * Plain pointers (device memory), ints and a hipStream_t (passed as void*); no torch types.  Every entry
 * point returns 0 on success, a negative CDFO_E* code for a rejected argument, or the positive hipError_t of
 * a failed launch.  All activation tensors are fp32, "pixel-major" (N,H,W,C) with an explicit channel pitch
 * `ld` (floats between consecutive pixels), so a tensor may be a channel slice of a wider buffer.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   - every ATen call inside arch/SIDECVSR_our.py:4406-4481 (CVSR_V8.forward) and the modules it reaches;
 *   - ops/dcn/src/deform_conv_cuda.cpp:151-156 (deform_conv_forward_cuda) and :486-492
 *     (modulated_deform_conv_cuda_forward), i.e. the pybind module `deform_conv_cuda`
 *     (ops/dcn/src/deform_conv_cuda.cpp:681-695).
 */
#ifndef CDFO_HIP_H
#define CDFO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CDFO_EINVAL (-1)   /* bad shape / unsupported configuration */
#define CDFO_EALIGN (-2)   /* pointer or pitch not 16-byte aligned  */
#define CDFO_MAXSRC 8

enum { CDFO_ACT_NONE = 0, CDFO_ACT_LRELU = 1, CDFO_ACT_RELU = 2, CDFO_ACT_SIGMOID = 3 };
enum { CDFO_STORE_PLAIN = 0, CDFO_STORE_SHUFFLE2 = 1, CDFO_STORE_S2D = 2, CDFO_STORE_TAPS9 = 3, CDFO_STORE_OFFMASK = 4,
       CDFO_STORE_S2D_HS = 5 /* cdfo_conv3x3_c64_wino[_up2]: CDFO_STORE_S2D with half-split rows, see cdfo_conv_args.src_halfsplit */ };
enum { CDFO_DTYPE_F32 = 0, CDFO_DTYPE_F16 = 1, CDFO_DTYPE_F64 = 2 };   /* element type tag of the *_dt entry points */
enum { CDFO_PREC_F32 = 0, CDFO_PREC_BF16X3 = 1, CDFO_PREC_BF16 = 2, CDFO_PREC_FP16X2 = 3, CDFO_PREC_FP16 = 4, CDFO_PREC_FP16X1 = 5 };

/* ABI version / build info.  */
int cdfo_abi_version(void);
const char* cdfo_build_info(void);
/* The persistent kernels size their grids to the device's CU count; a host thread that runs two schedules beside each other on two
 * streams gives each a share: launches of the CALLING THREAD fill at most n CUs from now on (0 = all).  Returns the previous value.  */
int cdfo_set_cu_limit(int n);

/* Dense convolution as an implicit GEMM on the matrix cores (replaces F.conv2d for 1x1 / 3x3, stride 1|2;
 * arch/SIDECVSR_our.py e.g. :383-387 Block_.body, :4382, :4386, :4390-4391).
 * Input = channel-concatenation of up to CDFO_MAXSRC sources (replaces torch.cat(...,1) in front of a conv).
 * w: packed by cdfo_pack_conv_weight(); optional per-image weights (w_bstride != 0).
 * Epilogue: +bias -> act -> +res1 -> +res2 -> store (plain or 2x pixel-shuffle, arch.py:4473-4474).
 * CDFO_STORE_S2D writes output pixel (y,x), channel n to pixel (y/2,x/2), channel ((y&1)*2+(x&1))*Cout+n of a
 * [B,Ho/2,Wo/2,4*Cout] tensor (space-to-depth), the input format of the stride-2-composed conv of Block_'s 2x branch.  */
typedef struct {
  const float* src[CDFO_MAXSRC]; int ld[CDFO_MAXSRC]; int cs[CDFO_MAXSRC]; int nsrc;
  int B, H, W, Ho, Wo;
  int ks, stride, pad;
  int Cin, Cout, CoutP;
  const float* w; long long w_bstride; const float* bias;
  int act;
  const float* res1; int ldr1;
  const float* res2; int ldr2;
  float* out; int ldo; int store_mode;
  int prec;                   /* CDFO_PREC_*; bits 8 and up: developer ablation code of cdfo_conv3x3_ring / cdfo_conv3x3_bf16 (0 in the
                                 shipped library, which answers CDFO_EINVAL otherwise; -DCDFO_DEV_ABLATIONS builds compile the rest) */
  const float* ln_gamma; const float* ln_beta;   /* optional fused per-pixel LayerNorm of a single 64-channel source (1x1 only) */
  const unsigned* tap_mask;   /* optional, cdfo_conv3x3_bf16 only: per 16-channel chunk, bit t set = tap t has non-zero weights */
  int src_f16;                /* cdfo_conv3x3_bf16 only: the single source is an fp16 tensor (ld in halves); implies CDFO_PREC_FP16 */
  int out_f16;                /* cdfo_conv3x3_bf16 only: store the result as fp16 (ldo in halves); no residual inputs */
  void* out2_cp16;            /* optional, cdfo_conv3x3_ring only: second copy of the result as an fp16 chunk-planar tensor
                                 [B][Cout/16][H][W][16] (the next Block_'s body[0] source), Cout % 16 == 0 */
  int src_plane_wrap;         /* optional, cdfo_conv3x3_ring only: chunk c reads source plane c % src_plane_wrap (0 = plane c), so
                                 that a K-expanded product (a_hi | a_lo | a_hi) x (w_hi | w_hi | w_lo) needs no duplicated planes */
  const float* res_up2; int ldru;   /* optional, cdfo_conv3x3_ring only: a HALF-resolution residual [B][H/2][W/2][ldru] that is
                                 added after bilinear x2 up-sampling (align_corners=False), i.e. Block_'s x1/2 branch */
  int out2_lo;                /* cdfo_conv3x3_ring with out2_cp16: the copy is hi | lo planes [B][2*Cout/16][H][W][16] (fp16(v), then
                                 fp16(v - fp16(v))): the source of a split-fp16 convolution on the same kernel */
  /* CDFO_STORE_OFFMASK (cdfo_conv3x3_bf16 only, Cout = 3 * third, Wo % 4 == 0, no activation / residuals): the convolution is
   * MVDualAttAlignment's conv_offset[2] and its epilogue is the module's offset / mask assembly (arch/SIDECVSR_our.py:3336-3350),
   * written straight into the DCN operator's NCHW inputs -- out = offset [B][2*third][Ho][Wo], mask_out = mask [B][third][Ho][Wo]:
   *   off_accumulate == 0 (the first of the two heads):  offset[k] = off_mag * tanh(v[k]) + flow[b][1 - (k & 1)],  mask[k] = v[2*third + k]
   *   off_accumulate != 0 (the second head, in place):    offset[k] += off_mag * tanh(v[k]),  mask[k] = sigmoid(mask[k] + v[2*third + k])
   * flow: the motion field [B][2][Ho][Wo], image pitch flow_bstride floats (read by the first head only).  */
  float* mask_out; const float* flow; long long flow_bstride; float off_mag; int off_accumulate;
  const float* res2_pixscale;  /* optional, cdfo_conv1x1_bf16x3 only (its streaming form): res2 enters the sum as res2[p][c] * res2_pixscale[p],
                                 one factor per pixel [B][H*W] -- a spatial gate applied to the residual without writing the gated tensor */
  int src_halfsplit;           /* cdfo_conv3x3_ring only: the fp16 chunk-planar source's rows are stored as [8-channel half][W][8]
                                 (a row's first halves, then its second halves: what cdfo_conv3x3_c64_wino writes with
                                 CDFO_STORE_S2D_HS, 16 contiguous bytes per lane and pixel) instead of [W][16] */
  float* chan_sum_out;         /* optional, cdfo_conv1x1_bf16x3 only (plain store, Cout = CoutP = 64): per-image channel sums of the RESULT as
                                 partials [B][chan_sum_slots][64] in cdfo_chan_sum_partial's layout.  Zeroed by the caller; chan_sum_slots =
                                 cdfo_align_stats_slots(B, H*W).  The streaming kernel sums in its epilogue (one slot per image and
                                 workgroup segment, fixed order); any other form runs cdfo_chan_sum_partial(out) with nchunk = chan_sum_slots */
  int chan_sum_slots;
} cdfo_conv_args;
int cdfo_sizeof_conv_args(void);   /* sizeof(cdfo_conv_args) as the library was built: a binding checks its own mirror against it */
int cdfo_conv_igemm(const cdfo_conv_args* a, void* stream);

/* Pack an OIHW fp32 weight [Cout][Cin][ks][ks] (device) into the layout cdfo_conv_igemm reads:
 * [Cin/16][ks*ks][4][CoutP][4] floats, CoutP = Cout rounded up to 32, zero filled.
 * shuffle2 != 0 permutes output channels o = c*4+dy*2+dx -> (dy*2+dx)*(Cout/4)+c for CDFO_STORE_SHUFFLE2.
 * transposed != 0 reads an IOHW ConvTranspose2d weight and flips the taps (conv-equivalent form).  */
int cdfo_pack_conv_weight(const float* w_oihw, float* packed, int Cout, int Cin, int ks, int shuffle2,
                          int transposed, void* stream);

/* 3x3 / stride 1 / pad 1 convolution on the bf16 matrix cores, fp32 accumulate; same argument block and epilogue as
 * cdfo_conv_igemm.  a->prec = CDFO_PREC_BF16X3 (split-bf16, 3 passes, fp32-grade), CDFO_PREC_BF16 (plain bf16) -- both
 * with a->w packed by cdfo_pack_conv3x3_bf16 ([hi|lo] x [Cin/16][9][2][CoutP][8] bf16, CoutP = Cout up to 64) -- or
 * CDFO_PREC_FP16X2 (fp16 hi+lo activations x fp16 weights, 2 passes; a->w packed by cdfo_pack_conv3x3_f16, one block),
 * or CDFO_PREC_FP16 with a->src_f16 (the source already IS an fp16 tensor -- Block_'s 256-channel body intermediate,
 * whose rounding to fp16 does not move the forward's error -- one pass, staging is a plain 16-byte copy), or
 * CDFO_PREC_FP16X1 (fp32 source rounded once to fp16 while staging, fp16 weights, one pass: used for the convolutions
 * INSIDE Block_, where the oracle emulation shows the forward's error is set by the weight rounding alone).  */
int cdfo_conv3x3_bf16(const cdfo_conv_args* a, void* stream);
/* Image maps (csrc/image_map.h): a pixel-major fp32 operand [M][P][ld >= 64] whose images are not one dense block is described by its
 * first image's pointer and (Bi, s_b, s_g): image m starts at pointer + (m % Bi) s_b + (m / Bi) s_g floats (Bi > 0, strides >= 0 and
 * multiples of 4); inside an image nothing changes.  The *_map entry points read ONE named operand that way and give the bits their
 * dense forms give on the dense copy of those images; a launch outside a mapped form's contract is CDFO_EINVAL.
 * cdfo_conv3x3_bf16_map: cdfo_conv3x3_bf16 (a->prec = CDFO_PREC_BF16X3 or CDFO_PREC_FP16X2, fp32 sources, Cout > 32, plain store) with
 * source 0 mapped.  */
int cdfo_conv3x3_bf16_map(const cdfo_conv_args* a, int s0_Bi, long long s0_sb, long long s0_sg, void* stream);
int cdfo_pack_conv3x3_bf16(const float* w_oihw, void* packed, int Cout, int Cin, void* stream);
int cdfo_pack_conv3x3_f16(const float* w_oihw, void* packed, int Cout, int Cin, void* stream);

/* Block_.body[0] (arch/SIDECVSR_our.py:383-387, Conv2d(64, Cout, 3, 1, 1) + activation) as a persistent,
 * weights-stationary fp16 MFMA kernel: one workgroup per CU keeps the fp16 weights of 64 output channels in LDS and
 * streams pixel tiles past them.  src_cp16: fp16 "chunk-planar" tensor [B][4][H][W][16] (cdfo_to_cp16, or
 * cdfo_resample2 with out_f16 = 2); w_f16/CoutP: cdfo_pack_conv3x3_f16 packing and its padded channel count;
 * out_cp16: fp16 chunk-planar [B][Cout/16][H][W][16] (CDFO_STORE_PLAIN) or its space-to-depth form
 * [B][4*Cout/16][H/2][W/2][16], chunk = ((y&1)*2+(x&1))*Cout/16 + channel/16 (CDFO_STORE_S2D).
 * H even, Cout % 64 == 0, the source smaller than 2 GiB.  Since round 3 the call runs the ring-fed, wave-specialised form
 * (four producer waves feed two groups of four consumer waves, v_mfma_f32_16x16x32_f16); same operands, same result layout.
 * dbg: 0 (developer ablation flags otherwise -- compiled only into developer builds, -DCDFO_DEV_ABLATIONS, `python -m cdfo_amd.build --dev`;
 * the shipped library answers CDFO_EINVAL: 1 / 2 / 8 skip the MFMAs / the DMA / the epilogue; with dbg 32 clk_probe receives s_memtime stamps of the consumer waves, 256 x 12 x 4 x 8
 * 64-bit words; with dbg 128 -- private-halo form only -- per wave of the grid {shader-clock cycles, start, end in 100 MHz
 * real-time ticks}: 3 x 8 x 256 words; else pass NULL).  */
int cdfo_conv3x3_c64_ws(const void* src_cp16, int B, int H, int W, const void* w_f16, int CoutP, const float* bias,
                        int Cout, int act, void* out_cp16, int store_mode, int dbg, void* clk_probe, void* stream);
/* The same convolution (Block_.body[0], arch/SIDECVSR_our.py:383-387: 3x3, 64 -> Cout, stride 1, pad 1, + bias + activation; fp16
 * chunk-planar source and result exactly as cdfo_conv3x3_c64_ws) as a row-streaming Winograd F(2,3) product along x: 2/3 of the direct
 * form's MFMAs, weights stationary in REGISTERS (csrc/conv3x3_wino.hip).  w_wino: cdfo_pack_conv3x3_wino image (Cout x 64 x 12 fp16:
 * [Cout/16][dy 3][xi 4][K half 2][lane 64][8], element e of lane (kg, i) = U_xi[dy][channel 32 half + 8 kg + e][output channel 16 cb + i]
 * with U0 = g0, U1 = (g0 + g1 + g2)/2, U2 = (g0 - g1 + g2)/2, U3 = g2 over the kernel row g = w[:, :, dy, 0..2], formed in fp32).
 * Cout % 128 == 0, W even (H even for CDFO_STORE_S2D), one image of source / result smaller than 2 GiB; any B.  The transformed
 * inputs are up to 2x the source's magnitude in fp16: |src| must stay below 32752.  */
int cdfo_conv3x3_c64_wino(const void* src_cp16, int B, int H, int W, const void* w_wino, const float* bias, int Cout, int act,
                          void* out_cp16, int store_mode, void* stream);
int cdfo_pack_conv3x3_wino(const float* w_oihw, void* packed, int Cout, void* stream);
/* the same call with developer ablation bits (dbg != 0: developer builds only, -DCDFO_DEV_ABLATIONS, CDFO_EINVAL otherwise; WRONG
 * results; 1 no MFMAs, 2 no global loads, 4 no stores, 8 no epilogue arithmetic, 16 no barrier; 512 = timeline probe: clk_probe
 * receives s_memtime stamps [workgroup][wave][8] of one steady-state batch, 64-bit words, else NULL): tools/bench_wino.py, tools/wino_timeline.py */
/* Block_'s double-resolution branch (arch.py:398-404: body(up(x))) without its double-resolution source: src_lr_cp16
 * [B][4][H/2][W/2][16] = up.0(x) at the block's resolution (cdfo_block_prologue2's t16); H x W (multiples of 4) = the size of the x2
 * image the convolution runs on.  The bilinear x2 (align_corners = False, clamped taps; the convolution pads the x2 image with zeros)
 * is folded into the F(2,3) input transform.  Result as cdfo_conv3x3_c64_wino(..., store_mode) with store_mode = CDFO_STORE_S2D
 * ([B][4 Cout/16][H/2][W/2][16]) or CDFO_STORE_S2D_HS (the same planes with half-split rows [H/2][2][W/2][8]).  */
int cdfo_conv3x3_c64_wino_up2(const void* src_lr_cp16, int B, int H, int W, const void* w_wino, const float* bias, int Cout, int act,
                              void* out_cp16, int store_mode, void* stream);
int cdfo_conv3x3_c64_wino_dbg(const void* src_cp16, int B, int H, int W, const void* w_wino, const float* bias, int Cout, int act,
                              void* out_cp16, int store_mode, int dbg, void* clk_probe, void* stream);
/* MVDualAttAlignment's conv_offset[2] (3x3, 64 -> Cout = 27 dg, arch/SIDECVSR_our.py:3285-3289) on the weights-stationary kernel with
 * the module's offset / mask assembly (arch.py:3336-3350) as its epilogue -- the CDFO_STORE_OFFMASK contract of cdfo_conv_args above,
 * single-pass fp16 operands (src fp16 chunk-planar [B][4][H][W][16], weights from cdfo_pack_conv3x3_f16 with CoutP padded channels):
 * offset [B][2 Cout/3][H][W], mask [B][Cout/3][H][W] fp32 NCHW, flow [B][2][H][W] (image pitch flow_bstride floats).
 * accumulate == 0: first head; != 0: second head, in place.  H even; any W.  */
int cdfo_conv3x3_c64_ws_offmask(const void* src_cp16, int B, int H, int W, const void* w_f16, int CoutP, const float* bias, int Cout,
                                float* offset, float* mask, const float* flow, long long flow_bstride, float mag, int accumulate,
                                void* stream);

/* Residual form of cdfo_conv3x3_c64_ws (ResidualBlock_noBN's second convolution, arch.py:261-262):
 * out[B][H][W][ldo] (fp32, pixel-major) = act(conv + bias) + res1 (+ res2), res* fp32 pixel-major; optionally also the
 * fp16 chunk-planar copy out2_cp16 [B][Cout/16][H][W][16] (NULL to skip).  */
int cdfo_conv3x3_c64_ws_res(const void* src_cp16, int B, int H, int W, const void* w_f16, int CoutP, const float* bias,
                            int Cout, int act, float* out, int ldo, const float* res1, int ldr1, const float* res2,
                            int ldr2, void* out2_cp16, void* stream);
/* The same with res2 (required) read through an image map (see cdfo_conv3x3_bf16_map).  */
int cdfo_conv3x3_c64_ws_res_map(const void* src_cp16, int B, int H, int W, const void* w_f16, int CoutP, const float* bias,
                                int Cout, int act, float* out, int ldo, const float* res1, int ldr1, const float* res2,
                                int ldr2, int r2_Bi, long long r2_sb, long long r2_sg, void* out2_cp16, void* stream);
/* 3x3 / stride 1 / pad 1 convolution of an fp16 chunk-planar source (a->src[0] = [B][Cin/16][H][W][16], a->src_f16 = 1,
 * a->ld[0] = 16, a->cs[0] = Cin) as a persistent kernel fed by an LDS-DMA ring: Block_.body[2] (256 -> 64) and the
 * composed stride-2 convolution of Block_'s double-resolution branch.  a->w: fp16 [Cin/16][taps][2][CoutP][8] with
 * taps = 9 (cdfo_pack_conv3x3_f16) or, when a->tap_mask is given, taps = 4: only the chunk's four active taps, in
 * ascending tap order.  Epilogue and the other fields as cdfo_conv_igemm (fp32 or fp16 pixel-major result).  */
int cdfo_conv3x3_ring(const cdfo_conv_args* a, void* stream);
/* fp32 pixel-major [B][P][ldi] (C channels, C % 16 == 0) -> fp16 chunk-planar [B][C/16][P][16].  */
int cdfo_to_cp16(const float* in, int ldi, int B, long long P, int C, void* out_cp16, void* stream);

/* 1x1 convolution as an HBM-streaming GEMM in split-bf16 (3-pass, fp32-grade) arithmetic; same argument block and
 * epilogue as cdfo_conv_igemm with ks = 1 (fp32 packing of cdfo_pack_conv_weight, per-image weights, fused LayerNorm,
 * residuals, pixel-shuffle store).  Every source must be a multiple of 64 channels, CoutP a multiple of 64 (<= 256).
 * With a->out2_cp16 != NULL (Cout == 64, plain store): ln_gamma / ln_beta describe a LayerNorm64 of the RESULT, written there as
 * fp16 hi | lo chunk-planar planes [B][8][P][16] (what cdfo_layernorm64_cp16hl would produce from `out`); with out2_cp16 set and
 * ln_gamma == ln_beta == NULL (round 4) the second output is the result itself as fp16 chunk-planar [B][4][P][16] (= cdfo_to_cp16(out)).  */
int cdfo_conv1x1_bf16x3(const cdfo_conv_args* a, void* stream);
/* The same with one more 64-channel operand of the product that is a 3x3 stencil (zero padding) of a ONE-channel H x W plane and is
 * never materialised (streaming form only: plain store, Cout <= CoutP = 64, no out2_cp16, no res2_pixscale, H W + 2 W + 64 < 2^29;
 * CDFO_EINVAL otherwise -- there is no other kernel for it).  Image b's plane (dense fp32 rows) starts at plane + (b % plane_Bi) plane_sb
 * + (b / plane_Bi) plane_sg floats.  plane_w [CoutP][16] fp32, 16-byte aligned, image pitch plane_w_bstride floats (0: shared): row n =
 * sum_c W[n][c] w_s[c][0..8] | sum_c W[n][c] b_s[c] | six zeros, W the product's weights for that operand (the identity where the operand
 * is simply added to the result), (w_s, b_s) the stencil.  It enters the product as one split-bf16 k-step of 16 (the nine neighbours and a
 * constant 1, built in registers) before bias and activation; a->chan_sum_out works as without it.  */
int cdfo_conv1x1_bf16x3_plane(const cdfo_conv_args* a, const float* plane, int plane_Bi, long long plane_sb, long long plane_sg,
                              const float* plane_w, long long plane_w_bstride, void* stream);
/* cdfo_conv1x1_bf16x3 (plane == NULL) / cdfo_conv1x1_bf16x3_plane with operands read through image maps (see cdfo_conv3x3_bf16_map).
 * maps: CDFO_MAXSRC + 2 triples (Bi, s_b, s_g): entry i for source i, entries CDFO_MAXSRC and CDFO_MAXSRC + 1 for res1 and res2;
 * Bi == 0: that operand is dense.  Plain store, CoutP = 64, no out2_cp16, no LayerNorm, no res2_pixscale.  The streaming kernel takes
 * every such launch inside its own contract; outside it (Cin > 192) only mapped SOURCES of a product without plane, channel sums or
 * mapped residuals are taken.  cdfo_conv1x1_map_ok: 1 when a launch of Cin input channels with / without a plane operand, a mapped
 * residual, channel sums is taken (host arithmetic, no launch), else 0.  */
int cdfo_conv1x1_bf16x3_map(const cdfo_conv_args* a, const long long* maps, const float* plane, int plane_Bi, long long plane_sb,
                            long long plane_sg, const float* plane_w, long long plane_w_bstride, void* stream);
int cdfo_conv1x1_map_ok(int Cin, int with_plane, int with_res, int with_csum);

/* Upsampler tail without the HR feature map (arch.py:4474-4480).  cdfo_conv1x1_bf16x3 with a->store_mode =
 * CDFO_STORE_TAPS9 (upconv2: Cout = 256, pixel-shuffle weight packing, LeakyReLU; a->res2 = conv_last.weight
 * [1][64][3][3]) stores for every HR pixel the nine per-tap channel sums of conv_last into out[B][2H][2W][ldo >= 9];
 * cdfo_conv_last_taps then forms out[b][y][x] = bias + sum_k taps[(y,x) + delta_k][k] + bilinear_x4(x_center).  */
int cdfo_conv_last_taps(const float* taps, int ldt, const float* bias, const float* xc, long long xc_bstride, int B, int Hh,
                        int Wh, float* out, void* stream);
/* Layout changes at the module boundary (reference tensors are NCHW).  */
int cdfo_nchw_to_nhwc(const float* in, float* out, int B, int C, int H, int W, int ldo, void* stream);
int cdfo_nhwc_to_nchw(const float* in, int ldi, float* out, int B, int C, int H, int W, void* stream);
/* out[n][b] = in[b][n] for blocks of `block` floats (clip-major <-> frame-major feature stacks).  */
int cdfo_swap_outer(const float* in, float* out, int B, int N, long long block, void* stream);
/* Range probe of a dense fp32 buffer (n % 4 == 0): slots2[0] = max |x| over the finite elements (as the bit pattern of a
 * float, combined by atomicMax), slots2[1] |= 1 if any element is NaN / infinite.  Caller zeroes the two words. */
int cdfo_range_probe(const float* x, long long n, void* slots2, void* stream);

/* ---- bandwidth-bound pixel-major kernels (pointwise.hip) ------------------------------------------------- */
/* 3x3 conv 1 -> 64 channels on a single-channel plane [B][H][W] (image pitch img_bstride floats); raw OIHW weight
 * [64][1][3][3]; optional second output out2 = result + add; with out2, out may be NULL (the result itself is not written).
 * arch/SIDECVSR_our.py:4379-4384,4417-4418,4446-4449. */
int cdfo_stem_conv(const float* img, long long img_bstride, const float* w, const float* bias, int B, int H, int W,
                   int act, float* out, int ldo, const float* add, int lda, float* out2, int ldo2, void* stream);
/* two 1 -> 64 3x3 convolutions of the same plane in one pass: outA = conv(img; wA, bA) + add, outB = actB(conv(img; wB, bB))
 * (fea_com = fea_i + conv_expand_rms(rms), arch.py:4446-4449, and relu(conv_du_re.0(conv_expand_rms(rms))), arch.py:2148-2152,
 * 2200, with the 1x1 conv_du_re.0 composed into wB / bB by the caller: `rms_prior` is never written).  s2dB != 0: outB in
 * space-to-depth form [B][H/2 + 1][W/2 + 1][4 * 64] (phase-major channels; last row / column = the caller's zeros), over which
 * the stride-2 conv_du_re.2 is a stride-1 convolution with a 2x2 tap window. */
int cdfo_stem_conv2(const float* img, long long img_bstride, const float* wA, const float* bA, const float* add, int lda,
                    float* outA, int ldoA, const float* wB, const float* bB, int actB, float* outB, int ldoB, int s2dB, int B,
                    int H, int W, void* stream);
/* per-pixel LayerNorm over 64 channels (arch.py:1169-1198). */
int cdfo_layernorm64(const float* in, int ldi, const float* gamma, const float* beta, long long npix, float* out,
                     int ldo, void* stream);
/* the same LayerNorm written as an fp16 hi / lo pair in chunk-planar layout [B][8][P][16]: planes 0-3 = fp16(v) of channels
 * 0-63, planes 4-7 = fp16(v - fp16(v)): the source of a split-fp16 (fp32-grade) 3x3 convolution on cdfo_conv3x3_ring. */
int cdfo_layernorm64_cp16hl(const float* in, int ldi, const float* gamma, const float* beta, int B, long long P, void* out,
                            void* stream);
/* depthwise 3x3, pad 1, no bias; raw weight [C][1][3][3] (arch.py:1552). */
int cdfo_dwconv3x3(const float* in, int ldi, const float* w, int B, int H, int W, int C, float* out, int ldo,
                   void* stream);
/* flow_warp (arch.py:3068-3099); mv = [B][2][H][W] planes (x then y), image pitch mv_bstride floats. */
int cdfo_flow_warp(const float* in, int ldi, const float* mv, long long mv_bstride, int B, int H, int W, int C,
                   float* out, int ldo, void* stream);
/* bilinear x2 (up=1) or x0.5 (up=0), align_corners=False (arch.py:324-333); accumulate: out += result;
 * out_f16 (up only): 1 = `out` is an fp16 pixel-major tensor (ldo in halves) that feeds a single-pass fp16 convolution;
 * 2 = `out` is an fp16 chunk-planar tensor [B][C/16][2H][2W][16] (ldo ignored), the source of cdfo_conv3x3_c64_ws. */
int cdfo_resample2(const float* in, int ldi, int B, int H, int W, int C, float* out, int ldo, int up, int accumulate,
                   int out_f16, void* stream);
/* out = in * gate[b][c] (CALayer, arch.py:2041-2043); out_cp16 (optional, C % 16 == 0): the same values as the fp16
 * chunk-planar tensor [B][C/16][P][16] that cdfo_conv3x3_c64_ws reads. */
int cdfo_scale_channels(const float* in, int ldi, const float* gate, int B, long long P, int C, float* out, int ldo,
                        void* out_cp16, void* stream);
/* conv_last 3x3 64->1 (+bias) + bilinear x4 of the centre LR frame (arch.py:4476-4480); out = [B][Hh][Wh]. */
int cdfo_conv_last(const float* in, int ldi, const float* w, const float* bias, const float* xc, long long xc_bstride,
                   int B, int Hh, int Wh, float* out, void* stream);

/* ---- thin 16-channel layers of the prior U-net (smallconv.hip; arch.py:1815-1834, 2719-2730) --------------- */
int cdfo_small_conv16(const float* in, int ldi, const float* w, const float* bias, int B, int H, int W, int stride,
                      int pad, int out_pad, int transposed, int act, float* out, int ldo, void* stream);
/* the same, result as fp16 hi | lo planes [B][2][Ho*Wo][16] (chunk-planar): the split-fp16 source of cdfo_conv3x3_ring */
int cdfo_small_conv16_hl(const float* in, int ldi, const float* w, const float* bias, int B, int H, int W, int stride,
                         int pad, int out_pad, int transposed, int act, void* out_hl, void* stream);
/* lrelu(body.0(conv_second(img))): the prior U-net's first layer in the feature extractor's first round (arch.py:4420,
 * 1463-1468, 1819-1820) straight from the one-channel prior image -- conv_second's 64-channel result feeds only this
 * layer there and has no activation, so the two 3x3 convolutions are composed (exactly, borders included: a tap of body.0
 * outside the image sees zero, not conv_second's bias).  wc[t][u][o] = sum_c W0[o][c][t] W2[c][u] ([9][9][16]),
 * bt[t][o] = sum_c W0[o][c][t] b2[c] ([9][16]), b0 = body.0's bias.  img element [b][y][x] at img + b*img_bstride + y*W + x. */
int cdfo_udsa_head(const float* img, long long img_bstride, const float* wc, const float* bt, const float* b0, int B, int H,
                   int W, float* out, int ldo, void* stream);
int cdfo_spatial_gate16(const float* in, int ldi, const float* w, const float* bias, int B, int H, int W, float* out,
                        int ldo, void* stream);

/* ---- reductions + per-image weight folding of the channel attentions (stats.hip) --------------------------- */
int cdfo_chan_sum_partial(const float* in, int ldi, int B, long long P, int nchunk, float* partial, void* stream);
/* LLongRangAttention's mask statistics from the one-channel residual maps themselves (rdab_stats.hip; arch.py:2148-2152, 2200-2203):
 * partial [B][nchunk][64], cdfo_chan_sum_partial's layout (every slot written, fixed order: equal inputs give equal bits), of
 *   relu(conv3x3 stride 2 pad 2 (du0; w2, b2)) over its (H/2+1) x (W/2+1) output pixels,
 *   du0 = relu(stencil9(img; w0, b0)) on the H x W grid (the map zero-padded) and ZERO outside the grid,
 * with neither du0 nor the convolution's result written.  Split-bf16 MFMA in three passes, fp32 accumulation.  Image m's plane
 * (H x W fp32, dense rows) starts at img + (m % Bi) s_b + (m / Bi) s_g floats.  w0 [64][9], b0 [64]: the composed 1 -> 64 stencil;
 * w2_packed: the 3x3 weights as bf16 hi | lo, [2][9 taps][4 k-steps c][2 k-halves h][64 out][8], element j = input channel
 * 16 c + 8 (j >> 2) + 4 h + (j & 3) (147456 bytes, 16-byte aligned; kernels.py: pack_rdab_stats); b2 [64].  du0 is itself formed
 * by a split-bf16 product (the tap's nine neighbours and a constant 1 against [w0 | b0]).  H, W even, H W < 2^30, else CDFO_EINVAL. */
int cdfo_rdab_stats(const float* img, int Bi, long long s_b, long long s_g, const float* w0, const float* b0,
                    const void* w2_packed, const float* b2, int B, int H, int W, int nchunk, float* partial, void* stream);
int cdfo_gram_partial(const float* q, int ldq, const float* k, int ldk, int B, long long P, int ch_per_head, int nchunk,
                      float* partial, void* stream);
/* DualAttAlignment's statistics in one pass (arch/SIDECVSR_our.py:3455-3480): kf = act(W . [x0; x1] + bias) (1x1, 128 -> 64, split-bf16
 * MFMA like cdfo_conv1x1_bf16x3) is formed on the fly and never stored; the pass leaves
 *   gram_partial [B][nslots][64*(ch_per_head+2)]   cdfo_gram_partial(q, kf)'s layout
 *   sum0_partial / sum1_partial [B][nslots][64]    cdfo_chan_sum_partial(x0) / (x1)'s layout
 * for cdfo_align_fold (nchunk_g = nchunk_s = nslots).  x0, x1, q: pixel-major fp32 [B][P][ld >= 64] (64 channels each, 16-byte
 * aligned); w_packed: cdfo_pack_conv_weight's layout of the [64][128] weight; bias optional; act: NONE / LRELU / RELU;
 * ch_per_head: 8 | 16.  The three outputs are ZEROED BY THE CALLER, nslots >= cdfo_align_stats_slots(B, P): a persistent workgroup
 * stores its sums over its tiles of an image into its own slot with plain stores (no atomics: run-to-run identical).
 * cdfo_stream_slots_for_grid / cdfo_stream_slot_of: the slot arithmetic for a grid of `grid` workgroups, host only.  */
int cdfo_align_stats_slots(int B, long long P);
int cdfo_stream_slots_for_grid(int B, long long P, int grid);
int cdfo_stream_slot_of(int B, long long P, int grid, int wg, int b);
int cdfo_align_stats(const float* x0, int ld0, const float* x1, int ld1, const float* q, int ldq, const float* w_packed,
                     const float* bias, int act, int ch_per_head, int B, long long P, int nslots, float* gram_partial,
                     float* sum0_partial, float* sum1_partial, void* stream);
/* The same where x1 = stencil9(plane; w_s, b_s) (zero padding) of a ONE-channel W-pixel-wide plane per image and is never materialised:
 * image b's plane (dense fp32 rows, P = H W pixels) starts at plane + (b % plane_Bi) plane_sb + (b / plane_Bi) plane_sg floats.
 * w_packed / bias: as above (the 128 -> 64 packing; its second half is not read); plane_w [64][16] fp32: the product's second half
 * composed with the stencil, row n = sum_c W[n][64 + c] w_s[c][0..8] | sum_c W[n][64 + c] b_s[c] | six zeros, one split-bf16 k-step of
 * 16 behind the K block of x0; stencil_w [64][16] fp32: w_s[c][0..8] | b_s[c] | six zeros, from which sum1_partial[b][slot][c] =
 * sum_t w_s[c][t] S_t + b_s[c] count is formed out of the segment's nine tap sums S_t and its pixel count (fixed order).  Both tables
 * 16-byte aligned.  P % W == 0, P + 2 W + 64 < 2^29, else CDFO_EINVAL: there is no other kernel for this form.  */
int cdfo_align_stats_plane(const float* x0, int ld0, const float* q, int ldq, const float* w_packed, const float* bias, int act,
                           int ch_per_head, int B, long long P, int nslots, float* gram_partial, float* sum0_partial,
                           float* sum1_partial, const float* plane, int plane_Bi, long long plane_sb, long long plane_sg, int W,
                           const float* plane_w, const float* stencil_w, void* stream);
/* cdfo_align_stats (plane == NULL) / cdfo_align_stats_plane (x1 == NULL, ld1 unused) with q read through an image map (see
 * cdfo_conv3x3_bf16_map).  */
int cdfo_align_stats_map(const float* x0, int ld0, const float* x1, int ld1, const float* q, int ldq, int q_Bi, long long q_sb,
                         long long q_sg, const float* w_packed, const float* bias, int act, int ch_per_head, int B, long long P,
                         int nslots, float* gram_partial, float* sum0_partial, float* sum1_partial, const float* plane, int plane_Bi,
                         long long plane_sb, long long plane_sg, int W, const float* plane_w, const float* stencil_w, void* stream);
/* MDTA (arch.py:1555-1575): wout[b] = packed 1x1 weights (64->64) = project_out x blockdiag(softmax(...)). */
int cdfo_mdta_fold(const float* partial, int nchunk, const float* temperature, const float* proj_w, int B, float* wout,
                   void* stream);
/* DualAttAlignment (arch.py:3459-3491): wout[b] = packed 1x1 weights (192->64) over cat[warped, pred, x]. */
int cdfo_align_fold(const float* gram_partial, int nchunk_g, const float* sum_warp, const float* sum_pred, int nchunk_s,
                    long long P, const float* temperature, const float* du0_w, const float* du0_b, const float* du2_w,
                    const float* du2_b, const float* proj_w, const float* fusion_w, int B, float* wout, void* stream);
/* The same where pred = stencil9(plane; w_s, b_s) stays a one-channel plane (stencil_w [64][16]: w_s[c][0..8] | b_s[c] | zeros): with
 * [M1 | M2 | Wb] the three 64-column blocks of cdfo_align_fold's weights, wout[b] = packed 1x1 weights (128->64) [M1 | Wb] over
 * cat[warped, x] (bit-equal to those columns) and tables[b] = M2 . [w_s | b_s] as [64][16] fp32, columns 10..15 zero: the per-image
 * plane_w of cdfo_conv1x1_bf16x3_plane (image pitch 64 * 16).  wout, tables 16-byte aligned.  */
int cdfo_align_fold_plane(const float* gram_partial, int nchunk_g, const float* sum_warp, const float* sum_pred, int nchunk_s,
                          long long P, const float* temperature, const float* du0_w, const float* du0_b, const float* du2_w,
                          const float* du2_b, const float* proj_w, const float* fusion_w, const float* stencil_w, int B,
                          float* wout, float* tables, void* stream);
/* out[b] = act2(W2 act1(W1 mean_b + b1) + b2) from channel-sum partials (CALayer / conv_du_re2). */
int cdfo_vec_mlp(const float* sum_partial, int nchunk, long long P, const float* w1, const float* b1, int c1, int act1,
                 const float* w2, const float* b2, int c2, int act2, int B, float* out, void* stream);

/* ---- LLongRangAttention (attention.hip; arch.py:2179-2249) -------------------------------------------------- */
/* noise: the uniform draws of arch.py:2169 as [B][64][H*W]. */
int cdfo_rdab_prep(const float* xq, int ldx, const float* vmax, const float* noise, const float* wW, const float* bW,
                   int B, long long P, float* sq, int lds_, float* vrow, int ldv, float* qwin, int ldw, void* stream);
/* The same with the uniform draws generated inside the kernel (Philox4x32-10 keyed by seed, `draw` = index of the call
 * within the forward): the reference's default behaviour, torch.rand_like at arch.py:2169, without the 256 B/pixel noise
 * tensor.  noise_out: optional [B][64][H*W] copy of the drawn values (parity tests replay them through the oracle). */
int cdfo_rdab_prep_rng(const float* xq, int ldx, const float* vmax, long long seed, int draw, float* noise_out,
                       const float* wW, const float* bW, int B, long long P, float* sq, int lds_, float* vrow, int ldv,
                       float* qwin, int ldw, void* stream);
/* cdfo_rdab_prep_rng with the Philox key read from DEVICE memory (seed_dev: one 64-bit word, 8-byte aligned): a captured
 * HIP graph then draws fresh uniforms on every replay -- the caller rewrites the word between replays -- instead of
 * freezing a launch argument (the reference draws per forward, arch.py:2169). */
int cdfo_rdab_prep_rng_dev(const float* xq, int ldx, const float* vmax, const void* seed_dev, int draw, float* noise_out,
                           const float* wW, const float* bW, int B, long long P, float* sq, int lds_, float* vrow, int ldv,
                           float* qwin, int ldw, void* stream);
/* RDAB.input_conv (1x1, 64 -> 128) and cdfo_rdab_prep* in ONE launch: the 128-channel product is never written.  x [B][P][ldx]
 * fp32 (ldx >= 64), w_packed / bias: the convolution's fp32 packing [16][128][4] and bias [128] (NULL: none).  noise != NULL: the
 * injected draws (cdfo_rdab_prep); otherwise Philox keyed by *seed_dev (if non-NULL) or seed, with the optional noise_out.
 * vwin receives the v half of the product, which the two-kernel path reads from xq.  v_f16 (bit 0: vrow, bit 1: vwin): that output
 * is fp16, pitch in halves, each value rounded once -- what the attention modes 20-22 do to an fp32 V while staging.  Same bits as the streaming
 * form of cdfo_conv1x1_bf16x3 followed by cdfo_rdab_prep*.  P % 64 == 0. */
int cdfo_rdab_prep_fused(const float* x, int ldx, const float* w_packed, const float* bias, const float* vmax,
                         const float* noise, long long seed, const void* seed_dev, int draw, float* noise_out,
                         const float* wW, const float* bW, int B, long long P, float* sq, int lds_, void* vrow, int ldv,
                         float* qwin, int ldw, void* vwin, int ldvw, int v_f16, void* stream);
/* cdfo_rdab_prep_fused on x + stencil9(plane; w_s, b_s) (fea_com = fea + conv_expand_rms(rms), arch.py:4446-4449) with only x in
 * memory: the stencil's part joins the product as one split-bf16 k-step of 16 whose pixel operand (nine neighbours, zero padding, and a
 * constant 1) is built from the one-channel plane.  Image b's plane (P / W rows of W pixels, dense fp32) starts at plane +
 * (b % plane_Bi) plane_sb + (b / plane_Bi) plane_sg floats; plane_w [128][16] fp32, 16-byte aligned: row n = sum_c Wconv[n][c] w_s[c][0..8]
 * | sum_c Wconv[n][c] b_s[c] | six zeros.  The mask depends on vmax and the draws alone and is the same as on the materialised sum; q and
 * v agree with it to the product's fp32-grade rounding.  P + 2 W + 64 < 2^29. */
int cdfo_rdab_prep_fused_plane(const float* x, int ldx, const float* w_packed, const float* bias, const float* vmax,
                               const float* noise, long long seed, const void* seed_dev, int draw, float* noise_out,
                               const float* wW, const float* bW, int B, long long P, float* sq, int lds_, void* vrow, int ldv,
                               float* qwin, int ldw, void* vwin, int ldvw, int v_f16, const float* plane, int plane_Bi,
                               long long plane_sb, long long plane_sg, int W, const float* plane_w, void* stream);
/* cdfo_rdab_prep_fused_plane with x read through an image map (see cdfo_conv3x3_bf16_map).  */
int cdfo_rdab_prep_fused_plane_map(const float* x, int ldx, int x_Bi, long long x_sb, long long x_sg, const float* w_packed,
                                   const float* bias, const float* vmax, const float* noise, long long seed, const void* seed_dev,
                                   int draw, float* noise_out, const float* wW, const float* bW, int B, long long P, float* sq,
                                   int lds_, void* vrow, int ldv, float* qwin, int ldw, void* vwin, int ldvw, int v_f16,
                                   const float* plane, int plane_Bi, long long plane_sb, long long plane_sg, int W,
                                   const float* plane_w, void* stream);
int cdfo_colconv9(const float* in, int ldi, const float* wH, const float* bH, int B, int H, int W, float* out, int ldo,
                  void* stream);
/* Evaluation metrics on the device (metric/psnr_ssim.py:278-317 calculate_psnr, :320-399 _ssim / calculate_ssim): fp64
 * partial sums over [N][H][W] fp32 planes, values = plane * scale (optionally clamped to [0,255] / rounded to integers),
 * `crop` border pixels dropped.  metric 0: sum (a-b)^2;  metric 1: sum of the SSIM map (11x11 Gaussian, sigma 1.5,
 * valid positions).  partial receives [N][*nblocks_out] doubles (partial_cap = its capacity in doubles); the caller
 * adds them up in order and divides by the number of positions.  */
int cdfo_metric_partials(const float* a, const float* b, int N, int H, int W, int crop, float scale, int clamp, int round8,
                         int metric, double* partial, int partial_cap, int* nblocks_out, void* stream);
/* Block_ prologue (arch.py:378-406): from one read of the block input x [B][H][W][64] (H, W even) the fp16 chunk-planar
 * sources of its two resampled branches: u16 [B][4][2H][2W][16] = bilinear_x2(up.0(x)) and d16 [B][4][H/2][W/2][16] =
 * down.0(mean2x2(x)).  w_bf16: split-bf16 1x1 weights [hi|lo][4][2][128][8], rows 0-63 = up.0, 64-127 = down.0,
 * element (s,h,n,j) = W[n][16s+8h+j]; bias128 = [up.0 bias | down.0 bias].  x16 (optional): also the fp16 chunk-planar
 * copy [B][4][H][W][16] of x itself, the source of the block's own-resolution branch.  */
int cdfo_block_prologue(const float* x, int ldx, int B, int H, int W, const void* w_bf16, const float* bias128, void* u16,
                        void* d16, void* x16, void* stream);
/* The same with the double-resolution source left to its consumer: exactly one of u16 / t16 is given; t16 [B][4][H][W][16] receives
 * up.0(x) itself (fp16 chunk-planar, NOT resampled), which cdfo_conv3x3_c64_wino_up2 interpolates while it builds its transformed
 * inputs -- the 4x larger u16 is then never written or read.  */
int cdfo_block_prologue2(const float* x, int ldx, int B, int H, int W, const void* w_bf16, const float* bias128, void* u16, void* t16,
                         void* d16, void* x16, void* stream);
/* MDTA front end in one pass (arch.py:1169-1198 LayerNorm, :1551-1552 qkv + qkv_dwconv): out[B][H][W][192] =
 * depthwise3x3(conv1x1(LayerNorm64(x))).  w_bf16: split-bf16 weights [hi|lo][4][2][192][8], element (s,h,n,j) =
 * W[n][16s+8h+j] * gamma[16s+8h+j]; bias[192] = W @ beta (may be NULL); dw_w: raw [192][1][3][3] taps.
 * gram != NULL fuses the attention's Gram pass (arch.py:1561-1566): q and k are not written, `out` receives v only
 * (64 channels, ldo >= 64) and gram[B][gram_slots][640] -- zero-filled by the caller, gram_slots >=
 * cdfo_qkv_dw_gram_slots(B, H, W); per slot the layout of cdfo_gram_partial with 8 channels per head: [c*10 + j] =
 * sum_p q[c] k[head(c)*8 + j], [c*10 + 8] = sum q[c]^2, [c*10 + 9] = sum k[c]^2 -- receives each workgroup's partial
 * sums in its own slot (plain stores, fixed summation order: bit-reproducible); cdfo_mdta_fold(gram, gram_slots, ...)
 * reduces the slots.  */
int cdfo_qkv_dw_gram_slots(int B, int H, int W);
int cdfo_qkv_dw(const float* x, int ldx, int B, int H, int W, const void* w_bf16, const float* bias, const float* dw_w,
                float eps, float* out, int ldo, float* gram, int gram_slots, void* stream);
/* out = softmax(Q Q^T) V per row (mode 0), column (1) or 8x8 window (2) (arch.py:2179-2249), flash style on the matrix
 * cores: both products with fp16 hi + fp16 lo operands, three passes, fp32 accumulate (scores exact to ~1e-6 relative).
 * Modes 10 / 11 / 12: the plain-VALU forms of 0 / 1 / 2 (kept as A/B references for the tests).
 * Modes 20 / 21 / 22: modes 0 / 1 / 2 with the SECOND product (probabilities x values) on single-fp16 operands, one pass: an
 * output's error is bounded by 2^-11 * max|v| (probabilities sum to 1), ~1e-5 * |v| in practice; the scores keep three passes.
 * The forward's default fp16x2 arithmetic uses these (cdfo_amd/cvsr_v8.py); the fp32-grade modes and the training path do not. */
int cdfo_seq_attn(const float* q, int ldq, const float* v, int ldv, float* out, int ldo, int B, int H, int W, int mode,
                  void* stream);
/* Modes 20 / 21 / 22 with 16-bit operands.  v_f16: v is fp16 (ldv in halves) holding (_Float16)v, the rounding the fp32 form
 * applies while staging: same result bit for bit at half the bytes (ldv % 8 == 0, v 16-byte aligned).  out_f16 (mode 20 only): out is fp16 (ldo in halves) and
 * receives (_Float16)result -- the row attention's output as the V operand of the column attention.  Neither flag: cdfo_seq_attn. */
int cdfo_seq_attn_f16(const float* q, int ldq, const void* v, int ldv, void* out, int ldo, int B, int H, int W, int mode,
                      int v_f16, int out_f16, void* stream);

/* ---- deformable convolution forward (dcn.hip) --------------------------------------------------------------
 * Replaces deform_conv_forward_cuda (ops/dcn/src/deform_conv_cuda.cpp:151-156; mask == NULL, bias == NULL) and
 * modulated_deform_conv_cuda_forward (ops/dcn/src/deform_conv_cuda.cpp:486-492) of the pybind module
 * `deform_conv_cuda` (cpp:681-695).  NCHW fp32 contiguous tensors exactly as the reference passes them:
 * in [B,C,H,W], offset [B,2*dg*kh*kw,Ho,Wo], mask [B,dg*kh*kw,Ho,Wo] or NULL, weight [Co,C/groups,kh,kw],
 * bias [Co] or NULL, out [B,Co,Ho,Wo] (written, not accumulated).  The reference's `columns` scratch tensor
 * [C*kh*kw, Ho*Wo] has no counterpart (sampling and contraction are fused); `workspace` is an optional device scratch
 * of at least B*C*H*W*4 bytes (16-byte aligned) in which the kernel keeps a group-planar copy of `in` so that the
 * bilinear corners of a deformable group's channels are single 16-byte gathers; NULL selects the direct NCHW gathers
 * (same results, slower).  With cdfo_dcn_workspace_bytes(...) bytes (non-zero for groups == 1, (C/dg) % 4 == 0,
 * Co % 32 == 0, Co <= 128, kh*kw <= 64 -- the alignment module's shape) the fast kernel of dcn_fast.hip runs: whole-K
 * LDS staging and split-fp16 matrix products (fp32-grade, ~2^-22 relative; |in * mask| < 65504).  */
long long cdfo_dcn_workspace_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int groups, int deformable_groups);
int cdfo_dcn_forward(const float* in, const float* offset, const float* mask, const float* weight, const float* bias,
                     float* out, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                     int dh, int dw, int groups, int deformable_groups, void* workspace, long long workspace_bytes,
                     void* stream);

/* ---- deformable convolution backward (dcn_bwd.hip) -----------------------------------------------------------
 * One entry point behind the module's three backward functions: deform_conv_backward_input_cuda
 * (ops/dcn/src/deform_conv_cuda.cpp:260-266: grad_in + grad_offset; mask, grad_mask, grad_weight, grad_bias NULL),
 * deform_conv_backward_parameters_cuda (cpp:373-378: grad_weight only, `scale` multiplies the contribution) and
 * modulated_deform_conv_cuda_backward (cpp:566-573: all five).  Tensors as in cdfo_dcn_forward plus
 * grad_out [B,Co,Ho,Wo].  Any gradient pointer may be NULL (skipped).  grad_in, grad_weight and grad_bias are
 * ACCUMULATED into -- the reference's callers hand over zero-filled tensors (ops/dcn/deform_conv.py:71-72, 85,
 * 154-158) -- grad_offset and grad_mask are assigned.  kh*kw <= 64.  grad_in / grad_weight use fp32 hardware
 * atomics, so their summation order (not their value beyond fp32 rounding) varies between runs, as in the reference. */
int cdfo_dcn_backward(const float* in, const float* offset, const float* mask, const float* weight,
                      const float* grad_out, float* grad_in, float* grad_offset, float* grad_mask, float* grad_weight,
                      float* grad_bias, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph,
                      int pw, int dh, int dw, int groups, int deformable_groups, float scale, void* stream);
/* The same with a workspace of cdfo_dcn_backward_workspace_bytes(...) bytes (16-byte aligned; non-zero for groups == 1,
 * C/dg == 4, kh*kw <= 9, Co <= 64 -- the alignment module's shape; -1 on bad shapes): the weight gradient is then
 * contracted on the matrix cores inside the data-gradient kernel (grad_output x the column values it samples anyway)
 * instead of by a second sampling pass.  NULL / too small a workspace = cdfo_dcn_backward.  */
long long cdfo_dcn_backward_workspace_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph,
                                            int pw, int dh, int dw, int groups, int deformable_groups);
int cdfo_dcn_backward_ws(const float* in, const float* offset, const float* mask, const float* weight,
                         const float* grad_out, float* grad_in, float* grad_offset, float* grad_mask, float* grad_weight,
                         float* grad_bias, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph,
                         int pw, int dh, int dw, int groups, int deformable_groups, float scale, void* workspace,
                         long long workspace_bytes, void* stream);

/* ---- the operator's other dtypes (dcn_typed.hip) --------------------------------------------------------------
 * The reference instantiates its kernels for float, double and half (AT_DISPATCH_FLOATING_TYPES_AND_HALF,
 * ops/dcn/src/deform_conv_cuda_kernel.cu:258,352,450,780,812,845).  Same tensors and conventions as cdfo_dcn_forward /
 * cdfo_dcn_backward with elements of `dtype` (CDFO_DTYPE_*): F32 forwards to those; F16 = fp16 tensors, fp32 arithmetic
 * (operands widened into `workspace`, the fp32 kernels run, results narrowed once; accumulating gradients are added to the
 * fp16 tensors); F64 = fp64 VALU kernels, fp64 atomics (correctness-first).  F32 / F16 backward: the workspace also carries
 * what cdfo_dcn_backward_ws wants.  `workspace` must hold
 * cdfo_dcn_workspace_bytes_dt(...) bytes, 16-byte aligned (`backward` = 0 / 1; F64 needs none; returns -1 on bad shapes). */
long long cdfo_dcn_workspace_bytes_dt(int dtype, int backward, int B, int C, int H, int W, int Co, int kh, int kw, int sh,
                                      int sw, int ph, int pw, int dh, int dw, int groups, int deformable_groups);
int cdfo_dcn_forward_dt(int dtype, const void* in, const void* offset, const void* mask, const void* weight,
                        const void* bias, void* out, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw,
                        int ph, int pw, int dh, int dw, int groups, int deformable_groups, void* workspace,
                        long long workspace_bytes, void* stream);
int cdfo_dcn_backward_dt(int dtype, const void* in, const void* offset, const void* mask, const void* weight,
                         const void* grad_out, void* grad_in, void* grad_offset, void* grad_mask, void* grad_weight,
                         void* grad_bias, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                         int dh, int dw, int groups, int deformable_groups, float scale, void* workspace,
                         long long workspace_bytes, void* stream);

/* ---- backward kernels of the CVSR_V8 training path (train_ops.hip) ------------------------
 * cdfo_amd/autograd.py runs the module under torch autograd (train_LD_37.py:376-381): every Function's forward is one of
 * the exact-fp32 forward entry points above, its backward either the same entry points with adjoint operands (flipped /
 * transposed weights) or one of these.  fp32 pixel-major tensors with pitch ld (floats).
 * cdfo_conv_wgrad:   out[a][b][ky][kx] = sum_{n,y,x} S[n,y,x,a] * L[n, y*stride+ky-pad, x*stride+kx-pad, b]  -- a
 *                    convolution's weight gradient with S = grad_out, L = input (OIHW), a transposed convolution's with
 *                    S = input, L = grad_out (IOHW).  Split-K exact-fp32 MFMA into `slab`
 *                    (cdfo_conv_wgrad_slab_floats(...) floats), slices summed in a fixed order into
 *                    dw[(a*Btot + b_off + b)*ks*ks + tap] (b_off / Btot: channel offset of this source in a concatenated input).
 * cdfo_coldot:       out[img][c] = scale * sum_p a[img][p][c] * (b ? b[img][p][c] : 1)  (bias / gate / pooled gradients);
 *                    part = nimg*nchunk*C floats of scratch.
 * cdfo_ew:           mode 0 a*b, 1 a*(1-b), 2 a+b, 3 a*act'(y=b) (aux = CDFO_ACT_*), 4 out[p][c] = a[p/P][c]*scale.
 * cdfo_layernorm64_bwd, cdfo_dwconv3x3_wgrad, cdfo_spatial_gate16_bwd, cdfo_chanconv9 (9 taps along the channel axis,
 * flip = adjoint), cdfo_corr9 (weight gradient of a 9-tap convolution along the channel axis (0) or the image rows (1)),
 * cdfo_gumbel_mask (the hard mask of arch.py:2168-2195 as a tensor), cdfo_seq_attn_bwd (adjoint of cdfo_seq_attn, modes
 * 0-2, probabilities recomputed), cdfo_flow_warp_bwd (scatter with fp32 atomics into a zero-filled dx; the order of the sums, and
 * with it the low bits, change from run to run), cdfo_flow_warp_bwd_fixed (the same scatter as 64-bit fixed-point integer atomics
 * into a zero-filled `acc` [B][H][W][C], then one rounding into a zero-filled dx: equal inputs give equal bits; `slots2` are the two
 * words of cdfo_range_probe over a dense g, which set the scale -- a unit is 2^(ceil(log2(H W)) - 60) of the largest |g| -- and send
 * a g that holds a NaN or an infinity through the fp32 atomics; what the autograd path uses),
 * cdfo_resample2_bwd (adjoints of bilinear x2 / x0.5). */
long long cdfo_conv_wgrad_slab_floats(int A, int Bc, int ks, int nsplit);
int cdfo_conv_wgrad(const float* S, int lds_, int A, const float* L, int ldl, int Bc, int N, int Hs, int Ws, int Hl, int Wl,
                    int ks, int stride, int pad, int nsplit, float* slab, float* dw, int Btot, int b_off, void* stream);
/* the same contraction with both operands split into bf16 hi + lo on the fly (three MFMA passes, fp32 accumulate: ~16 operand
 * bits) -- the training path's default since round 3; prec = CDFO_PREC_F32 runs cdfo_conv_wgrad's exact kernel */
int cdfo_conv_wgrad_prec(const float* S, int lds_, int A, const float* L, int ldl, int Bc, int N, int Hs, int Ws, int Hl, int Wl,
                         int ks, int stride, int pad, int nsplit, float* slab, float* dw, int Btot, int b_off, int prec,
                         void* stream);
int cdfo_coldot(const float* a, int lda, const float* b, int ldb, int nimg, long long P, int C, int nchunk, float scale,
                float* part, float* out, void* stream);
int cdfo_ew(const float* a, int lda, const float* b, int ldb, long long rows, int C, int mode, int aux, float scale, long long P,
            float* out, int ldo, void* stream);
int cdfo_layernorm64_bwd(const float* x, int ldx, const float* g, int ldg, const float* gamma, long long npix, float* dx,
                         int ldo, float* part, int nblk, void* stream);
int cdfo_dwconv3x3_wgrad(const float* x, int ldx, const float* g, int ldg, int B, int H, int W, int C, float* part, int nblk,
                         void* stream);
int cdfo_spatial_gate16_bwd(const float* t, int ldt, const float* g, int ldg, const float* w, const float* bias, int B, int H,
                            int W, float* scratch, float* dt, int ldo, float* dw99, void* stream);
int cdfo_gumbel_mask(const float* vmax, const float* noise, long long seed, int draw, float* noise_out, int B, long long P,
                     float* mask, int ldm, void* stream);
int cdfo_chanconv9(const float* in, int ldi, const float* w9, const float* bias, int flip, long long npix, float* out, int ldo,
                   void* stream);
int cdfo_corr9(const float* in, int ldi, const float* g, int ldg, int axis, int B, int H, int W, float* part, int nblk,
               void* stream);
int cdfo_seq_attn_bwd(const float* q, int ldq, const float* v, int ldv, const float* o, int ldo, const float* g, int ldg,
                      float* dq, int lddq, float* dv, int lddv, int B, int H, int W, int mode, void* stream);
int cdfo_flow_warp_bwd(const float* g, int ldg, const float* mv, long long mv_bstride, int B, int H, int W, int C, float* dx,
                       int ldo, void* stream);
int cdfo_flow_warp_bwd_fixed(const float* g, int ldg, const float* mv, long long mv_bstride, int B, int H, int W, int C,
                             const void* slots2, long long* acc, float* dx, int ldo, void* stream);
int cdfo_resample2_bwd(const float* g, int ldg, int B, int H, int W, int C, int up, float* din, int ldo, void* stream);

/* ---- pixel-local operators of the CVSR_V7 forward (v7_ops.hip) ---------------------------
 * fp32 pixel-major activations [B,H,W,64] with pitch ld (floats).
 * cdfo_chan_pool:     ChannelPool (arch/SIDECVSR_our.py:1883-1885): out[p] = {max_c x[p][c], mean_c x[p][c]}.
 * cdfo_spatial_gate:  SpatialAttention (arch.py:2719-2730): out = x * sigmoid(conv_ksxks(pooled) + bias), zero padding
 *                     (ks-1)/2, w = the module's [1,2,ks,ks] weight; gate_scratch: B*H*W floats (the gate map, written
 *                     by a one-thread-per-pixel pass, then applied by a pure streaming pass).
 * cdfo_rdab_mix:      RDAB.forward's mixing step (arch.py:2836-2845): out = xf * (softmax_c(vmax[b][c] - log(-log(u)))
 *                     + sigmoid(conv3x3(pooled) + b3)); vmax [B,64]; noise u in the reference's NCHW order [B,64,H,W].
 * cdfo_shrink_planes: F.interpolate(scale_factor = 0.5 (level 1) or 0.25 (level 2), bilinear, align_corners=False) of
 *                     `planes` planes per image, divided by 2 resp. 4 (arch.py:4296-4303): dst [B,planes,H>>l,W>>l]
 *                     contiguous; src element [b][pl][y][x] at src[b*src_bstride + (pl*H + y)*W + x].
 * cdfo_lincomb:       out = ca*a + cb*b + cc*c over n floats (b, c may be NULL; out may alias an input). */
int cdfo_chan_pool(const float* x, int ld, long long npix, int C, float* out, void* stream);
/* The SAME SpatialAttention applied round after round to one tensor (PartitionTransformerBlock, arch.py:1350-1368): x_k = x_0 * G_k with
 * G_k = G_{k-1} * sigmoid(conv_ksxks(G_{k-1} * pooled_0) + bias) per pixel (the gates are positive, so pooling commutes with them).
 * pooled = cdfo_chan_pool(x_0) [B][H][W][2]; cum_in = G_{k-1} [B][H][W] or NULL (= 1); cum_out = G_k (must not alias cum_in).  */
int cdfo_gate_map_cumulative(const float* pooled, const float* cum_in, const float* w, const float* bias, int B, int H, int W, int ks,
                             float* cum_out, void* stream);
int cdfo_spatial_gate(const float* x, int ld, const float* pooled, const float* w, const float* bias, int B, int H, int W,
                      int C, int ks, float* gate_scratch, float* out, int ldo, void* stream);
int cdfo_rdab_mix(const float* xf, int ld, const float* pooled, const float* w3, const float* b3, const float* vmax,
                  const float* noise, int B, int H, int W, float* out, int ldo, void* stream);
int cdfo_shrink_planes(const float* src, long long src_bstride, int planes, int B, int H, int W, int level, float* dst,
                       void* stream);
int cdfo_lincomb(float* out, const float* a, float ca, const float* b, float cb, const float* c, float cc, long long n,
                 void* stream);

/* ---- small NCHW operators of the DCN consumer modules DSTA (ops/attentionlayer.py:86-156) and MVDualAttAlignment
 * (arch/SIDECVSR_our.py:3265-3352); contiguous NCHW fp32, one thread per output (nchw_ops.hip).  A kernel or pooling
 * window larger than the (padded) input is CDFO_EINVAL, here and in the backward; cdfo_maxpool_nchw propagates a NaN in
 * the window like torch.max_pool2d (and like the arg-max of its backward) ----------------------------------------- */
int cdfo_conv2d_nchw(const float* in, const float* w, const float* bias, int B, int C, int H, int W, int Co, int kh,
                     int kw, int stride, int pad, int act, float* out, void* stream);
int cdfo_maxpool_nchw(const float* in, int BC, int H, int W, int k, int stride, float* out, void* stream);
int cdfo_resize_bilinear_nchw(const float* in, int BC, int H, int W, int Ho, int Wo, int accumulate, float* out,
                              void* stream);
int cdfo_avgpool_nchw(const float* in, int BC, long long P, float* out, void* stream);
/* mode 0: a+b; 1: relu(a); 2: sigmoid(a); 3: x*sigmoid(a)*y[b][c] (P = H*W). */
int cdfo_ew_nchw(const float* a, const float* b, const float* x, const float* y, long long n, long long P, int mode,
                 float* out, void* stream);
/* arch.py:3336-3350: offset = mag*tanh(o1[:2/3]) + mag*tanh(o2[:2/3]) + flow.flip(1) tiled, mask = sigmoid(o1[2/3:]+o2[2/3:]);
 * o1,o2 pixel-major [B,H,W,3*third] (pitch ld), flow [B][2][H*W] planes, outputs NCHW. */
int cdfo_mv_offset_mask(const float* o1, const float* o2, int ld, const float* flow, long long flow_bstride, int B,
                        long long P, int third, float mag, float* offset, float* mask, void* stream);

/* ---- 3x3 / stride 1 / pad 1 convolution 64 -> 16 channels (conv3x3_n16.hip; round 4): the first layer of the feature extractor's prior
 * U-net (arch/SIDECVSR_our.py:1815-1834, body.0: Conv2d(64, 16, 3, 1, 1) + LeakyReLU) as a persistent stream on
 * v_mfma_f32_16x16x32_bf16, split-bf16 three-pass arithmetic (fp32-grade, as cdfo_conv3x3_bf16's "bf16x3").  x fp32 pixel-major
 * [B,H,W,>=64] (pitch ldx), out fp32 pixel-major [B,H,W,16] (pitch ldo).  w_packed: 36,864 bytes = [18 K steps = tap*2 + 32-channel
 * half][hi | lo][64 lanes][8 bf16], lane l = output channel l & 15, input channels 32 half + 8 (l >> 4) .. + 7
 * (cdfo_amd/kernels.py::pack_conv_n16). */
int cdfo_conv3x3_c64_n16(const float* x, int ldx, int B, int H, int W, const void* w_packed, const float* bias, int act, float* out,
                         int ldo, void* stream);

/* ---- backward of the same operators (nchw_bwd.hip): DSTA and MVDualAttAlignment under autograd, like their reference classes
 * (ops/attentionlayer.py:117-156, arch/SIDECVSR_our.py:3303-3352).  Gather kernels, fixed summation order, no atomics.
 * cdfo_conv2d_nchw_bwd: any of gin [B,C,H,W] (needs w), gw [Co,C,kh,kw] (needs in), gbias [Co] (needs gout alone, with or without
 *   gw) may be NULL; every output given is ASSIGNED.
 * cdfo_maxpool_nchw_bwd: idx_scratch = BC*Ho*Wo ints (the windows' arg-max, first maximum in scan order).
 * cdfo_ew_nchw_bwd modes: 1 g*(y>0) (y = relu output), 2 g*y*(1-y) (y = sigmoid output), 4 g[bc]/P (adjoint of the plane mean),
 *   5 / 6: the DSTA gate out = x*sigmoid(a)*yv[bc] w.r.t. a / w.r.t. x; cdfo_gate_nchw_bwd_y: w.r.t. yv ([BC]).
 * cdfo_mv_offset_mask_bwd: adjoint of cdfo_mv_offset_mask w.r.t. o1, o2 (g1, g2 pixel-major, pitch ld; the motion field is a
 *   network input and receives no gradient). */
int cdfo_conv2d_nchw_bwd(const float* in, const float* w, const float* gout, int B, int C, int H, int W, int Co, int kh, int kw,
                         int stride, int pad, float* gin, float* gw, float* gbias, void* stream);
int cdfo_maxpool_nchw_bwd(const float* in, const float* gout, int BC, int H, int W, int k, int stride, int* idx_scratch, float* gin,
                          void* stream);
int cdfo_resize_bilinear_nchw_bwd(const float* gout, int BC, int H, int W, int Ho, int Wo, float* gin, void* stream);
int cdfo_ew_nchw_bwd(const float* g, const float* y, const float* a, const float* x, const float* yv, long long n, long long P,
                     int mode, float* out, void* stream);
int cdfo_gate_nchw_bwd_y(const float* g, const float* a, const float* x, int BC, long long P, float* gy, void* stream);
int cdfo_mv_offset_mask_bwd(const float* o1, const float* o2, int ld, const float* goff, const float* gmask, int B, long long P,
                            int third, float mag, float* g1, float* g2, void* stream);

/* ---- backward-side kernels of CVSR_V7's own operators (v7_train.hip; cdfo_amd/cvsr_v7_train.py): fp32 pixel-major rows of 64
 * channels.  cdfo_chan_pool_bwd: adjoint of cdfo_chan_pool (dpooled [npix][2] = d max, d mean; the first maximum in channel order
 * receives d max).  cdfo_mul_plane: out[p][c] = x[p][c] * plane[p]; cdfo_dot_plane: out[p] = sum_c a[p][c] b[p][c].
 * cdfo_gumbel_softmax: r = softmax_c(v[b][c] - log(-log u)) with u the reference's NCHW noise [B][64][P] (arch.py:2813-2822);
 * cdfo_softmax64_bwd: dz = r * (dm - sum_c r dm). */
int cdfo_chan_pool_bwd(const float* x, int ld, const float* dpooled, long long npix, float* dx, int ldo, void* stream);
int cdfo_mul_plane(const float* x, int ld, const float* plane, long long npix, float* out, int ldo, void* stream);
int cdfo_dot_plane(const float* a, int lda, const float* b, int ldb, long long npix, float* out, void* stream);
int cdfo_gumbel_softmax(const float* v, const float* u, int B, long long P, float* out, int ldo, void* stream);
int cdfo_softmax64_bwd(const float* r, int ldr, const float* dm, int ldm, long long npix, float* dz, int ldo, void* stream);

/* ---- sequence-level input building of chunked inference (sequence.hip; cdfo_amd/streaming.py::StreamingSR.run_chunked) ----
 * cdfo_seq_flows:     the decoder's motion field mv [T][H][W][3] (element type `dtype`, one of CDFO_MV_*) -> the per-slot flows of
 *                     the K centre frames i0 .. i0+K-1, out [K][7][2][Hp][Wp] fp32, zero padded from H x W to Hp x Wp (Wp % 4 == 0).
 *                     Per pixel test_LD_22_FPS.py's mv2mvs (:100-122: components swapped, / -mv[2] with NaN -> 0 and inf kept,
 *                     x 3, 2, 1, 0, -1, -2, -3 with slot 3 forced to 0, / 128) on entry max(1, i) of the field (entry 0 if T == 1),
 *                     then modify_mv_for_end_frames (:200-225) for centre i in a sequence of T frames.  Every step is one correctly
 *                     rounded fp32 operation in the host function's order: bit-identical to cdfo_amd.streaming.mv2mvs +
 *                     modify_mv_for_end_frames.
 * cdfo_gather_frames: dst[j] = src[idx[j]], j < n_dst, over frames of frame_bytes bytes (a multiple of 16; src, dst 16-byte
 *                     aligned); idx: n_dst ints in DEVICE memory; an index outside [0, n_src) gives a frame of zeros.
 * cdfo_flow_warp_frames: cdfo_flow_warp with an indexed source, G neighbour slots of K windows in one launch: for g < G, k < K
 *                     out[g*K + k] = flow_warp(bank[idx[g*K + k]], mv + k*mv_kstride + (slot0 + g)*2*H*W), i.e. mv is the
 *                     [K][7][2][H][W] output of cdfo_seq_flows with mv_kstride = 14*H*W and slot0 the group's first slot.
 *                     bank: n_bank frames [H][W] of C channels at pixel pitch ldi, read in place; out: G*K dense frames at pitch
 *                     ldo; idx: G*K ints in DEVICE memory, an index outside [0, n_bank) gives a frame of zeros (the contract of
 *                     cdfo_gather_frames).  Per pixel the arithmetic of cdfo_flow_warp, bit for bit.  G*K <= 65535. */
#define CDFO_MV_F32 0
#define CDFO_MV_F64 1
#define CDFO_MV_F16 2
#define CDFO_MV_BF16 3
#define CDFO_MV_I8 4
#define CDFO_MV_U8 5
#define CDFO_MV_I16 6
#define CDFO_MV_I32 7
#define CDFO_MV_I64 8
int cdfo_seq_flows(const void* mv, int dtype, int T, int H, int W, int i0, int K, int Hp, int Wp, float* out, void* stream);
int cdfo_gather_frames(const void* src, int n_src, const int* idx, int n_dst, long long frame_bytes, void* dst, void* stream);
int cdfo_flow_warp_frames(const float* bank, int ldi, int n_bank, const int* idx, const float* mv, long long mv_kstride, int slot0,
                          int G, int K, int H, int W, int C, float* out, int ldo, void* stream);

/* ---- input building of live sequence inference (live.hip; cdfo_amd/live.py::LiveSR) ----
 * Frames arrive one at a time into rings of cap frames (frame t in slot t mod cap) that keep the files' sample types.
 * cdfo_live_planes:   every plane a chunk of K centre frames reads from the sample rings, in one launch.  Rings of cap dense frames
 *                     [H][W]: lr and ufs of sample_bytes = 1 (peak <= 255) or 2 bytes per sample, pms of one byte, rms fp32.
 *                     table: 14 K + 2 E ints in DEVICE memory, ring slots: win_frame[K][7], win_prior[K][7], new_frame[E],
 *                     new_prior[E].  Outputs, dense fp32, zero padded from H x W to Hp x Wp (Wp % 4 == 0, 16-byte aligned):
 *                     x [K][7] = lr[win_frame] / peak, r = rms[win_prior] / peak, u = ufs[win_prior] / peak, lr_new [E] =
 *                     lr[new_frame] / peak, p_new [E] = pms[new_prior] / 255, r_new [E] = rms[new_prior] / peak.  r and r_new may
 *                     each be null (not written); E may be 0 (then lr_new and p_new may be null too).  Every quotient is ONE
 *                     correctly rounded fp32 division.  A slot outside [0, cap) gives a plane of zeros (cdfo_gather_frames'
 *                     contract).  21 K + 3 E <= 65535; offsets inside a frame and a plane are 32-bit (else CDFO_EINVAL).
 * cdfo_seq_flows_ring: cdfo_seq_flows reading a ring [cap][H][W][3] of fp32 motion fields.  T_known: the sequence's length once the
 *                     stream has closed, else 0 = not known yet: no end rule of modify_mv_for_end_frames applies and T > 1.  Centre
 *                     i reads entry e = (T_known == 1 ? 0 : max(1, i)) from slot e mod cap.  out [K][7][2][Hp][Wp], bit-identical to
 *                     cdfo_seq_flows on the whole field of T_known frames (for T_known = 0: of any length >= i0 + K + 3). */
int cdfo_live_planes(const void* lr, const void* ufs, const unsigned char* pms, const float* rms, int sample_bytes, int cap, int H, int W,
                     const int* table, int K, int E, int Hp, int Wp, int peak, float* x, float* r, float* u, float* lr_new, float* p_new,
                     float* r_new, void* stream);
int cdfo_seq_flows_ring(const float* ring, int cap, int H, int W, int i0, int K, int T_known, int Hp, int Wp, float* out, void* stream);

/* ---- the random-access forms of the two flow builders (seq_flows_ra.hip; StreamingSR / LiveSR with coding="RA") ----
 * cdfo_seq_flows_ra:  cdfo_seq_flows from BOTH lists' fields mv0, mv1 [T][H][W][3] (one element type `dtype`, any CDFO_MV_*), for a model
 *                     trained on the random-access loader's field (opt/data_RA_bi.py, cdfo_train_batch_ra).  Centre i reads both lists
 *                     at entry max(1, i) (entry 0 if T == 1).  Per pixel, (a, b, ref) converted to fp32 first, every step one correctly
 *                     rounded fp32 operation:
 *                         p2 = (b0 / (ref0 * -1), a0 / (ref0 * -1))      NaN -> +0, an infinity stays
 *                         p4 = (b1 / ref1,        a1 / ref1)             NaN -> +0, an infinity stays
 *                         ref0 == -99: p2 = -p4;   then ref1 == -99: p4 = -p2
 *                         slots 0, 1, 2 = fl(p2 * w) / 128, w = 3, 2, 1;  slot 3 = +0;  slots 4, 5, 6 = fl(p4 * w) / 128, w = 1, 2, 3
 *                     then modify_mv_for_end_frames for centre i in a sequence of T frames, zero padded from H x W to Hp x Wp
 *                     (Wp % 4 == 0).  The marker is tested on the converted value (== -99.0f): an unsigned field never marks.  Nothing
 *                     is clipped.  out [K][7][2][Hp][Wp] fp32, 16-byte aligned; bit-identical to cdfo_amd.streaming.mv2mvs_ra +
 *                     modify_mv_for_end_frames.  K <= 65535; offsets inside a field are 32-bit (else CDFO_EINVAL).
 * cdfo_seq_flows_ra_ring: cdfo_seq_flows_ra reading two fp32 rings [cap][H][W][3] (entry e of both lists in slot e mod cap), with
 *                     T_known as in cdfo_seq_flows_ring (0: the end is not known yet, no end rule applies and T > 1).  Bit-identical to
 *                     cdfo_seq_flows_ra on the whole fields of T_known frames (for T_known = 0: of any length >= i0 + K + 3). */
int cdfo_seq_flows_ra(const void* mv0, const void* mv1, int dtype, int T, int H, int W, int i0, int K, int Hp, int Wp, float* out,
                      void* stream);
int cdfo_seq_flows_ra_ring(const float* ring0, const float* ring1, int cap, int H, int W, int i0, int K, int T_known, int Hp, int Wp,
                           float* out, void* stream);

/* ---- the output side of sequence evaluation (finish.hip; cdfo_amd/evaluate.py) ----
 * cdfo_finish_frames: K fp32 frames, read in place (frame k, row y at src + k*src_fstride + y*src_pitch, in elements; src 16-byte
 *                     aligned, pitch and stride multiples of 4), -> K 8-bit frames dst [K][Ho][Wo], packed (Wo % 4 == 0, dst 16-byte
 *                     aligned).  Per pixel, each step one correctly rounded fp32 operation: clamp to [0,1] (NaN -> 0), x 255, then
 *                     CDFO_QUANT_TRUNC: truncation, the reference's `.astype(np.uint8)` (test_LD_37.py:179-180), or
 *                     CDFO_QUANT_NEAREST: round to nearest even.  gt != NULL: in the same pass the PSNR numerator against 8-bit
 *                     ground truth (frame k, row y at gt + k*gt_fstride + y*gt_pitch bytes, Hgt x Wgt): the sum of (u8 - gt)^2 over
 *                     [crop, Hm-crop) x [crop, Wm-crop), Hm = min(Ho, Hgt), Wm = min(Wo, Wgt) (psnr_ssim.py:462-468), as exact
 *                     64-bit integers: partial receives [K][*nblocks_out] sums (partial_cap = its capacity; K * 1024 always
 *                     suffices), which the caller adds up.  gt == NULL: partial and nblocks_out are not touched.
 * cdfo_metric_partials_u8: cdfo_metric_partials (metric 0: sum (a-b)^2; 1: sum of the SSIM map; fp64 partials [N][*nblocks_out],
 *                     `crop`) on two stacks of N 8-bit frames with their own sizes, pitches and frame strides (bytes), compared
 *                     over their common Hm x Wm = min(Ha, Hb) x min(Wa, Wb).
 * Offsets inside a frame are 32-bit: rows * pitch beyond 2^31 - 1 is CDFO_EINVAL. */
#define CDFO_QUANT_TRUNC 0
#define CDFO_QUANT_NEAREST 1
int cdfo_finish_frames(const float* src, int src_pitch, long long src_fstride, int K, int Ho, int Wo, unsigned char* dst, int mode,
                       const unsigned char* gt, int gt_pitch, long long gt_fstride, int Hgt, int Wgt, int crop, long long* partial,
                       int partial_cap, int* nblocks_out, void* stream);
int cdfo_metric_partials_u8(const unsigned char* a, int a_pitch, long long a_fstride, int Ha, int Wa, const unsigned char* b,
                            int b_pitch, long long b_fstride, int Hb, int Wb, int N, int crop, int metric, double* partial,
                            int partial_cap, int* nblocks_out, void* stream);

/* ---- chroma of YUV 4:2:0 evaluation (chroma.hip; cdfo_amd/evaluate.py: evaluate_yuv) ----
 * cdfo_chroma_up4: N 8-bit planes h x w, read in place (plane n, row y at src + n*src_pstride + y*src_pitch bytes), -> N 8-bit planes
 *                     dst [N][4h][4w], packed (dst 4-byte aligned).  Centre-aligned x4 Catmull-Rom in integers: output index 4q + r
 *                     takes four taps from q-2 (r = 0, 1) or q-1 (r = 2, 3), indices clamped to the plane, coefficients / 128
 *                     (-6,50,93,-9), (-1,12,123,-6), (-6,123,12,-1), (-9,93,50,-6) for r = 0..3; along x and y in 32-bit integers
 *                     without intermediate rounding, then clamp((v + 8192) >> 14, 0, 255), the shift arithmetic.  gt != NULL: in the
 *                     same pass the sum of (out - gt)^2 over [crop, Hm-crop) x [crop, Wm-crop), Hm = min(4h, Hgt), Wm = min(4w, Wgt),
 *                     as exact 64-bit integers: partial receives [N][*nblocks_out] sums (partial_cap = its capacity; N * 1024 always
 *                     suffices), which the caller adds up.  gt == NULL: partial and nblocks_out are not touched.
 * Offsets inside a plane are 32-bit: rows * pitch (and 16 h w) beyond 2^31 - 1 is CDFO_EINVAL. */
int cdfo_chroma_up4(const unsigned char* src, int src_pitch, long long src_pstride, int N, int h, int w, unsigned char* dst,
                    const unsigned char* gt, int gt_pitch, long long gt_pstride, int Hgt, int Wgt, int crop, long long* partial,
                    int partial_cap, int* nblocks_out, void* stream);

/* ---- high-bit-depth samples (finish.hip, chroma.hip; evaluate_yuv at 10, 12 and 16 bits) ----
 * The three kernels above on 16-bit samples (unsigned short, the value in the low bits) of a peak of 1 .. 65535 (2^depth - 1; else
 * CDFO_EINVAL).  Pitches and strides are in SAMPLES, sample pointers 2-byte aligned, destinations 16-byte aligned (else CDFO_EALIGN);
 * the 32-bit-offset guards and the partial / nblocks_out contracts are their 8-bit twins'.
 * cdfo_finish_frames_u16: cdfo_finish_frames with `x peak` for `x 255`: clamp to [0,1] (NaN -> 0), one correctly rounded fp32 multiply
 *                     by (float)peak, truncation or round to nearest even; Wo % 4 == 0, so a row is at least 8 bytes.  gt != NULL: the
 *                     sum of (u16 - gt)^2 as exact 64-bit integers (one square reaches 65535^2 > 2^31: squared unsigned).
 * cdfo_ssim_partials_u16: metric 1 of cdfo_metric_partials_u8 (the sum of the SSIM map, fp64 partials [N][*nblocks_out]) with
 *                     C1 = (0.01 peak)^2, C2 = (0.03 peak)^2 in fp64.  There is no metric 0: fp64 partial sums of squares are not
 *                     exact at 16 bits, the two kernels beside it give that sum in integers.
 * cdfo_chroma_up4_u16: cdfo_chroma_up4 with clamp((v + 8192) >> 14, 0, peak); the 32-bit sums hold up to 16 bits
 *                     (|v| <= 65535 * 158^2 = 1 636 015 740 < 2^31 - 8192). */
int cdfo_finish_frames_u16(const float* src, int src_pitch, long long src_fstride, int K, int Ho, int Wo, unsigned short* dst, int peak,
                           int mode, const unsigned short* gt, int gt_pitch, long long gt_fstride, int Hgt, int Wgt, int crop,
                           long long* partial, int partial_cap, int* nblocks_out, void* stream);
int cdfo_ssim_partials_u16(const unsigned short* a, int a_pitch, long long a_fstride, int Ha, int Wa, const unsigned short* b,
                           int b_pitch, long long b_fstride, int Hb, int Wb, int N, int crop, int peak, double* partial,
                           int partial_cap, int* nblocks_out, void* stream);
int cdfo_chroma_up4_u16(const unsigned short* src, int src_pitch, long long src_pstride, int N, int h, int w, unsigned short* dst,
                        int peak, const unsigned short* gt, int gt_pitch, long long gt_pstride, int Hgt, int Wgt, int crop,
                        long long* partial, int partial_cap, int* nblocks_out, void* stream);

/* ---- five-scale MS-SSIM of the luma (finish.hip; cdfo_amd/metrics.py: msssim_u8, msssim_u16; DESIGN.md has the definition) ----
 * cdfo_msssim_partials_u8 / _u16: two stacks of N frames as cdfo_metric_partials_u8 / cdfo_ssim_partials_u16 take them, compared over
 *                     Hc x Wc = their common size less `crop` on every side; Hc, Wc >= CDFO_MSSSIM_MIN_SIZE, else CDFO_EINVAL (there is
 *                     no metric with fewer scales).  Level 0 is that region, level j + 1 the 2x2 mean of level j (from the top-left
 *                     sample, a trailing odd row or column dropped), exact.  Per level j = 0..4 and frame the call leaves two sums
 *                     over the level's valid 11x11-Gaussian map of (Hc >> j) - 10 by (Wc >> j) - 10 positions: of
 *                     cs = (2 s12 + C2) / (s1^2 + s2^2 + C2) and of l * cs, l = (2 m1 m2 + C1) / (m1^2 + m2^2 + C1), in fp64.
 *                     partial: frame n's row is partial[n * row .. (n + 1) * row), row = 2 * (nblocks_out[0] + .. + nblocks_out[4]);
 *                     in it level 0's nblocks_out[0] pairs (cs sum, l cs sum) come first, then level 1's, ...; the caller adds each
 *                     level's pairs up in order and divides by the map's size.  nblocks_out: 5 ints.  partial_cap: capacity in
 *                     doubles, N * 10240 always suffices (less is CDFO_EINVAL when it does not).  partial 8-byte aligned.
 *                     pyramid: scratch of pyramid_bytes >= cdfo_msssim_pyramid_bytes(Hc, Wc, N), 4-byte aligned, overwritten by every
 *                     call (calls that share it must be ordered, e.g. by one stream).  Three launches whatever N.
 * cdfo_msssim_pyramid_bytes: 2 N * 4 * sum_{j=1..4} (Hc >> j)(Wc >> j); 0 for a region below the minimum or N <= 0. */
#define CDFO_MSSSIM_MIN_SIZE 176
long long cdfo_msssim_pyramid_bytes(int Hc, int Wc, int N);
int cdfo_msssim_partials_u8(const unsigned char* a, int a_pitch, long long a_fstride, int Ha, int Wa, const unsigned char* b,
                            int b_pitch, long long b_fstride, int Hb, int Wb, int N, int crop, float* pyramid, long long pyramid_bytes,
                            double* partial, int partial_cap, int* nblocks_out, void* stream);
int cdfo_msssim_partials_u16(const unsigned short* a, int a_pitch, long long a_fstride, int Ha, int Wa, const unsigned short* b,
                             int b_pitch, long long b_fstride, int Hb, int Wb, int N, int crop, int peak, float* pyramid,
                             long long pyramid_bytes, double* partial, int partial_cap, int* nblocks_out, void* stream);

/* ---- NIQE's block features of 8-bit luma frames (niqe.hip; cdfo_amd/metrics.py: niqe_features_u8; DESIGN.md has the definition) ----
 * Every buffer but the frames is fp64 and 8-byte aligned (else CDFO_EALIGN); sizes, pitches and strides are in samples; K <= 65535
 * frames per launch, all on `stream`.  The region R x C is the frames' top-left 96 floor(H/96) x 96 floor(W/96); nothing outside it is
 * read.
 * cdfo_niqe_mscn_u8 / _f64: dst [K][R][C] = (x - mu) / (sigma + 1), mu = sum h x and sigma = sqrt(|sum h x^2 - mu^2| + 2^-52) over the
 *                     7 x 7 window `window` (49 doubles in HOST memory, row-major, copied into the launch), the samples beyond the
 *                     region's edge replaced by the edge sample.  src: frame n at src + n fstride, rows at `pitch` >= C.
 * cdfo_niqe_half:     dst [K][R/2][C/2]: x / 255.0, the taps (-3, -9, 29, 111, 111, 29, -9, -3) / 256 at the inputs 2i-3 .. 2i+4 down
 *                     the columns, then along the rows, mirrored at the region's edge with the edge sample repeated, times 255.0.
 *                     R and C even, at least 8.
 * cdfo_niqe_block_sums: mscn dense [K][R][C], B x B blocks (2 <= B <= 96 divides R and C); sums [K][nb][5][6], nb = (R/B)(C/B), block
 *                     (ih, iw) at iw (R/B) + ih: for the maps x and x * x[(i-a) mod B][(j-b) mod B], (a,b) = (0,1), (1,0), (1,1), (1,-1),
 *                     the counts of v < 0 and v > 0, the sums of v^2 over each, of |v| and of v^2.  Fixed order, no atomics: equal
 *                     inputs give equal bits.
 * cdfo_niqe_features: from those sums of blocks of `count` samples and the device table (gam [CDFO_NIQE_TABLE], then r_gam
 *                     [CDFO_NIQE_TABLE]) the 18 features of each block into features[(n nb + b) 36 + 18 scale ...], scale 0 or 1:
 *                     the index is the first minimum of |r_gam - rn|, 0 when rn is NaN.
 * cdfo_niqe_mscn_u16 / cdfo_niqe_half_u16: the two sample readers on 16-bit frames of `peak` = 2^depth - 1 (1 .. 65535, else
 *                     CDFO_EINVAL; src 2-byte aligned): x = (255.0 v) / peak in fp64, an exact product and ONE correctly rounded
 *                     division (no reciprocal), v not clamped; every statement behind x is the 8-bit one, the same template.  v = 257 k
 *                     at peak 65535 gives k exactly, so such frames give the bits of the 8-bit frames k. */
#define CDFO_NIQE_TABLE 9801
int cdfo_niqe_mscn_u8(const unsigned char* src, int pitch, long long fstride, int K, int R, int C, const double* window, double* dst,
                      void* stream);
int cdfo_niqe_mscn_f64(const double* src, int pitch, long long fstride, int K, int R, int C, const double* window, double* dst,
                       void* stream);
int cdfo_niqe_half(const unsigned char* src, int pitch, long long fstride, int K, int R, int C, double* dst, void* stream);
int cdfo_niqe_mscn_u16(const unsigned short* src, int pitch, long long fstride, int K, int R, int C, const double* window, double* dst,
                       int peak, void* stream);
int cdfo_niqe_half_u16(const unsigned short* src, int pitch, long long fstride, int K, int R, int C, double* dst, int peak,
                       void* stream);
int cdfo_niqe_block_sums(const double* mscn, int K, int R, int C, int B, double* sums, void* stream);
int cdfo_niqe_features(const double* sums, int K, int nb, int count, const double* table, int scale, double* features, void* stream);

/* ---- BRISQUE's 36 features of 8-bit luma frames (brisque.hip; cdfo_amd/metrics.py: brisque_features_u8; DESIGN.md has the definition) ----
 * NIQE's sibling over the WHOLE H x W frame.  Every buffer but the frames is fp64 and 8-byte aligned (else CDFO_EALIGN); sizes, pitches
 * and strides are in samples; K <= 65535 frames per launch, all on `stream`.
 * cdfo_brisque_mscn_u8 / _f64: dst [K][H][W] = (x - mu) / (sigma + 1), mu = sum h x and sigma = sqrt(|sum h x^2 - mu^2| + 2^-23) over
 *                     the 7 x 7 window `window` (49 doubles in HOST memory, row-major, copied into the launch), the samples beyond the
 *                     FRAME's edge ZERO.  src: frame n at src + n fstride, rows at `pitch` >= W.
 * cdfo_brisque_half:  dst [K][ceil(H/2)][ceil(W/2)]: the taps (-3, -9, 29, 111, 111, 29, -9, -3) / 256 on x itself at the inputs
 *                     2i-3 .. 2i+4 down the columns, then along the rows, mirrored at the frame's edge with the edge sample repeated;
 *                     not rounded.  H and W at least 8, odd sizes included.
 * cdfo_brisque_sums:  mscn dense [K][H][W] (H, W >= 2); partials [K][G][5][6], G = ceil(H / CDFO_BRISQUE_STRIP), strip g the rows
 *                     16 g .. 16 g + 15: for the maps x and x * x[(i-a) mod H][(j-b) mod W], (a,b) = (0,1), (1,0), (1,1), (-1,1), the
 *                     counts of v < 0 and v > 0, the sums of v^2 over each, of |v| and of v^2.  G depends on the shape alone, the
 *                     order is fixed and there are no atomics: equal inputs give equal bits on any device.
 * cdfo_brisque_features: adds the G strips in index order and writes, from those sums over `count` = H W samples and the device table
 *                     (gam, r_gam, r_ggd, CDFO_BRISQUE_TABLE entries each), the 18 features of each frame into
 *                     features[n 36 + 18 scale ...], scale 0 or 1: the map's symmetric fit (first minimum of |r_ggd - rho|), its four
 *                     products' asymmetric fits (|r_gam - rn|); index 0 where the searched value is NaN.
 * cdfo_brisque_mscn_u16 / cdfo_brisque_half_u16: the two sample readers on 16-bit frames of `peak` (1 .. 65535, else CDFO_EINVAL; src
 *                     2-byte aligned), x = (255.0 v) / peak as cdfo_niqe_mscn_u16 forms it; the half image filters x itself. */
#define CDFO_BRISQUE_TABLE 9801
#define CDFO_BRISQUE_STRIP 16
int cdfo_brisque_mscn_u8(const unsigned char* src, int pitch, long long fstride, int K, int H, int W, const double* window, double* dst,
                         void* stream);
int cdfo_brisque_mscn_f64(const double* src, int pitch, long long fstride, int K, int H, int W, const double* window, double* dst,
                          void* stream);
int cdfo_brisque_half(const unsigned char* src, int pitch, long long fstride, int K, int H, int W, double* dst, void* stream);
int cdfo_brisque_mscn_u16(const unsigned short* src, int pitch, long long fstride, int K, int H, int W, const double* window, double* dst,
                          int peak, void* stream);
int cdfo_brisque_half_u16(const unsigned short* src, int pitch, long long fstride, int K, int H, int W, double* dst, int peak,
                          void* stream);
int cdfo_brisque_sums(const double* mscn, int K, int H, int W, double* partials, void* stream);
int cdfo_brisque_features(const double* partials, int K, int G, int count, const double* table, int scale, double* features,
                          void* stream);

/* ---- tOF: the dense Farneback flow of 8-bit luma pairs and the distance of two flows (tof.hip; cdfo_amd/metrics.py: farneback_u8,
 * tof_frames_u8; DESIGN.md has the definition, the project's own: cv2 parity unpinned) ----
 * Pairs are the batch dimension.  Every buffer but the frames is fp64, dense and 8-byte aligned, the flows 16-byte aligned (else
 * CDFO_EALIGN); sizes, pitches and strides are in samples; at most 65535 pairs (32767 for the level images) per launch, all on
 * `stream`.  Grids depend on the shapes alone, every sum has a fixed order and there are no atomics: equal inputs give equal bits.
 * cdfo_tof_level_u8:  dst [K][2][h][w]: for pair j the level image of its previous frame, then of its current one, frame `cur + j
 *                     cstride` with rows at `cpitch`.  The previous frame is `prev + j pstride` when `first` is NULL; else it is
 *                     `first` (rows at `fpitch`) for pair 0 and `prev + (j - 1) pstride` beyond, the form of a chunk whose pair j
 *                     is (frame j - 1, frame j) with a carried frame in front.  The H x W region of each frame (at least
 *                     CDFO_TOF_MIN each way) is smoothed with the `ntaps` (odd, 3 .. CDFO_TOF_MAX_TAPS; doubles in HOST memory)
 *                     down the columns and then along the rows, reflect-101, and resized to h x w (h <= H, w <= W) bilinearly: the
 *                     source coordinate (i + 1/2) (N / n) - 1/2, both taps clamped, the weight from the unclamped floor.
 * cdfo_tof_level_u16: the same of 16-bit frames of `peak` (1 .. 65535, else CDFO_EINVAL; 2-byte aligned): Farneback runs on
 *                     x = (255.0 v) / peak as cdfo_niqe_mscn_u16 forms it.
 * cdfo_tof_polyexp:  img [N][h][w] -> R [N][5][h][w] = (b_x, b_y, a_xx, a_yy, a_xy), the edge sample repeated.  `kernels`: 37 doubles
 *                     in HOST memory: the 11 taps g, x g, x^2 g, then the inverse Gram matrix's entries [1][1], [0][3], [3][3], [5][5].
 * cdfo_tof_matrices:  R [N][2][5][h][w] (a pair's previous, then current expansion) and flow [N][h][w][2] (dx, dy; NULL: zeros) ->
 *                     M [N][5][h][w], the normal equations' planes with the border factors applied.
 * cdfo_tof_blur_solve: M -> flow [N][h][w][2]: the 15 x 15 box mean of each plane (direct sums, rows first, the edge sample
 *                     repeated, / 225), then the 2 x 2 solve with 1e-3 added to the determinant.
 * cdfo_tof_flow_up:   src [N][hp][wp][2] -> dst [N][h][w][2]: the bilinear resize above, times 2.
 * cdfo_tof_epe:       flows a, b [K][h][w][2] -> out [K]: the mean over h w pixels of |a - b|; partials [K][G], G = ceil(h /
 *                     CDFO_TOF_STRIP), holds the strips' sums, which one workgroup per frame adds in index order (two launches). */
#define CDFO_TOF_MIN 32
#define CDFO_TOF_MAX_TAPS 19
#define CDFO_TOF_STRIP 16
int cdfo_tof_level_u8(const unsigned char* prev, int ppitch, long long pstride, const unsigned char* cur, int cpitch, long long cstride,
                      const unsigned char* first, int fpitch, int K, int H, int W, int h, int w, const double* taps, int ntaps,
                      double* dst, void* stream);
int cdfo_tof_level_u16(const unsigned short* prev, int ppitch, long long pstride, const unsigned short* cur, int cpitch, long long cstride,
                       const unsigned short* first, int fpitch, int K, int H, int W, int h, int w, const double* taps, int ntaps,
                       double* dst, int peak, void* stream);
int cdfo_tof_polyexp(const double* img, int N, int h, int w, const double* kernels, double* R, void* stream);
int cdfo_tof_matrices(const double* R, const double* flow, int N, int h, int w, double* M, void* stream);
int cdfo_tof_blur_solve(const double* M, int N, int h, int w, double* flow, void* stream);
int cdfo_tof_flow_up(const double* src, int N, int hp, int wp, int h, int w, double* dst, void* stream);
int cdfo_tof_epe(const double* a, const double* b, int K, int h, int w, double* partials, double* out, void* stream);

/* ---- LPIPS: what a VGG-shaped trunk needs beside cdfo_conv_igemm, and the distance of two feature stacks (lpips.hip;
 * cdfo_amd/metrics.py: lpips_layers_u8; DESIGN.md has the definition, the project's own: parity with the lpips package unpinned) ----
 * Activations are dense NHWC fp32, 16-byte aligned (else CDFO_EALIGN); everything behind the features is fp64.  Grids and summation
 * orders depend on the shapes alone and there are no atomics: equal inputs give equal bits, the distance of equal stacks is exactly
 * 0 and swapping the stacks keeps its bits.  All on `stream`; at most 65535 frames per launch of the stem and of the distance.
 * cdfo_lpips_stem_u8: N 8-bit frames, frame j at `src + j fstride` with rows at `pitch`, region h x w -> dst [N][h][w][C0] =
 *                     ReLU(conv1_1): a sample v becomes x = v / 255, with `normalize` 2 x - 1, then the three channels (x -
 *                     shift_c) / scale_c, shift = (-.030, -.088, -.188), scale = (.458, .448, .450); the SCALED tensor is padded
 *                     with zeros; weight [C0][3][3][3] and bias [C0] fp32 on the device, C0 a multiple of 16, at most
 *                     CDFO_LPIPS_STEM_MAXC.
 * cdfo_lpips_stem_u16: the same of 16-bit frames of `peak` (1 .. 65535, else CDFO_EINVAL; src 2-byte aligned): x = (float)v /
 *                     (float)peak, one correctly rounded fp32 division, where the 8-bit form has (float)v / 255.f; v not clamped.
 * cdfo_lpips_pool2:  src [N][H][W][C] -> dst [N][H/2][W/2][C], the maximum of each 2 x 2 block (odd sizes floor; a NaN wins), C a
 *                     multiple of 4.  Bit-exact.
 * cdfo_lpips_dist:    fa, fb [N][h][w][C], lin [C] fp64 -> partials [N][G], G = ceil(h / CDFO_LPIPS_STRIP): per strip of rows the
 *                     sum over its pixels of sum_c lin[c] (fa_c / (|fa| + 1e-10) - fb_c / (|fb| + 1e-10))^2, |.| the root of the
 *                     pixel's sum of squares over the channels.  C a multiple of 4.
 * cdfo_lpips_fold:    partials: the layers' [N][strips[k]] blocks one behind the other -> out [N][layers], the strips of (frame,
 *                     layer) added in index order and divided by counts[k].  `strips` and `counts` are in HOST memory, at most
 *                     CDFO_LPIPS_MAX_LAYERS of each.
 * The training loss (cdfo_amd/loss.py: lpips_loss) and its adjoint; the gradient goes to the result's samples only:
 * cdfo_lpips_stem_f32: cdfo_lpips_stem_u8 of fp32 samples (src 4-byte aligned) used as x themselves: no division, no clamp, no
 *                     quantisation.  Samples k / 255 (correctly rounded) give the bits of the 8-bit form on k.
 * cdfo_lpips_dist_bwd: fa, fb [N][h][w][C], lin [C] fp64, gscale [N] fp32 (the upstream gradient of each frame's layer distance),
 *                     gin [N][h][w][C] or null (the gradient that arrives at this tap from the deeper stage) -> gout [N][h][w][C]:
 *                     per pixel in fp64, r = 1 / (|fa| + 1e-10), u_c = fa_c / (|fa| + 1e-10) - fb_c / (|fb| + 1e-10) (two quotients
 *                     as in cdfo_lpips_dist: equal stacks give exactly 0), q = sum_c lin_c u_c fa_c,
 *                     t_c = gscale_n / (h w) 2 r (lin_c u_c - (r q / |fa|) fa_c), gout_c = fa_c > 0 ? (float)(t_c + gin_c) : +0
 *                     -- a select: a NaN or an infinity under a ReLU output that is not positive is dropped, the 0 / 0 of a pixel
 *                     whose tap is zero in every channel included.  C a multiple of 16.
 * cdfo_lpips_pool2_bwd: x [N][H][W][C] (the pool's input), g [N][H/2][W/2][C] -> gx [N][H][W][C]: g goes to the element
 *                     cdfo_lpips_pool2 took (the first maximum in the order (0,0), (0,1), (1,0), (1,1); a NaN takes the cell, the
 *                     last one if there are several), +0 to the other three and to the row and column the floor drops.  Exact.
 * cdfo_lpips_stem_bwd: g [N][h][w][C0] (already masked by the stem's output), wf [C0][3][3] fp32 on the device -> gx [N][h][w] =
 *                     sum_o sum_ky sum_kx wf[o][ky][kx] g[y + 1 - ky][x + 1 - kx][o], g zero outside: the adjoint of the scaling
 *                     and conv1_1 with wf[o][ky][kx] = k sum_c weight[o][c][ky][kx] / scale_c, k = 2 with `normalize`, else 1,
 *                     formed by the caller.  C0 as for the stem.
 * Every element of every output is written; nothing is atomic. */
#define CDFO_LPIPS_MIN 16
#define CDFO_LPIPS_STRIP 2
#define CDFO_LPIPS_STEM_MAXC 256
#define CDFO_LPIPS_MAX_LAYERS 8
int cdfo_lpips_stem_u8(const unsigned char* src, int pitch, long long fstride, int N, int h, int w, const float* weight,
                       const float* bias, int C0, int normalize, float* dst, void* stream);
int cdfo_lpips_stem_u16(const unsigned short* src, int pitch, long long fstride, int N, int h, int w, const float* weight,
                        const float* bias, int C0, int normalize, float* dst, int peak, void* stream);
int cdfo_lpips_pool2(const float* src, int N, int H, int W, int C, float* dst, void* stream);
int cdfo_lpips_dist(const float* fa, const float* fb, const double* lin, int N, int h, int w, int C, double* partials, void* stream);
int cdfo_lpips_fold(const double* partials, int N, int layers, const int* strips, const long long* counts, double* out, void* stream);
int cdfo_lpips_stem_f32(const float* src, int pitch, long long fstride, int N, int h, int w, const float* weight,
                        const float* bias, int C0, int normalize, float* dst, void* stream);
int cdfo_lpips_dist_bwd(const float* fa, const float* fb, const double* lin, const float* gscale, const float* gin, int N, int h,
                        int w, int C, float* gout, void* stream);
int cdfo_lpips_pool2_bwd(const float* x, const float* g, int N, int H, int W, int C, float* gx, void* stream);
int cdfo_lpips_stem_bwd(const float* g, const float* wf, int N, int h, int w, int C0, float* gx, void* stream);

/* ---- training batches and the training loss (train_batch.hip; cdfo_amd/train_data.py, cdfo_amd/loss.py) ----
 * cdfo_train_batch:   the resident clip set -- lr, pms, hr unsigned and rms signed 8-bit [S][T][H][W] ([S][T][4H][4W] for hr), ufs
 *                     [S][T][Hu][W] with Hu >= H rows indexed from the top, mvl0 signed 8-bit [S][T][H][W][3] (a, b, ref), all dense --
 *                     -> B samples in ONE launch.  plan: B rows of 8 ints on the device, (seq, first, top, left, hflip, vflip, rot, 0):
 *                     frames first .. first + 6 of sequence seq, cut at (top, left) to crop x crop (hr: frame first + 3, 4 crop each
 *                     way from (4 top, 4 left)).  out[y][x] = P[top + i'][left + j'] / 255 (correctly rounded), (i, j) = rot ? (x, y)
 *                     : (y, x), i' = vflip ? n-1-i : i, j' = hflip ? n-1-j : j.  x, pms_out: [B][7][1][c][c]; rms_out, ufs_out:
 *                     [B][1][7][c][c]; hr_out: [B][1][4c][4c]; mvs0: [B][7][2][c][c] from mvl0 of frame first + 3 through the same
 *                     index map: m0 = b, m1 = a, hflip negates m0, vflip m1, rot swaps them, p = m / (ref * -1) with NaN -> 0 (an
 *                     infinity stays, as in cdfo_seq_flows), slot k = fl(p * (3 - k)) / 128, slot 3 = +0.  crop % 4 == 0,
 *                     crop <= min(H, W), T >= 7, B <= 65535, else CDFO_EINVAL; outputs 16-byte aligned.  The caller validates the
 *                     plan's rows; a row that does not fit the set writes nothing.
 * cdfo_train_batch_ra: the random-access form (opt/data_RA_bi.py).  cdfo_train_batch's arguments plus mvl1, the second list's field,
 *                     signed 8-bit [S][T][H][W][3] like mvl0 (null is CDFO_EINVAL); the six plane outputs, the grid and every check
 *                     are cdfo_train_batch's.  mvs: [B][7][2][c][c] from both fields of frame first + 3, each through the index map
 *                     and the m0 / m1 rules above: p2 = m(list 0) / (ref0 * -1), p4 = m(list 1) / ref1, NaN -> +0, an infinity stays;
 *                     then ref0 == -99: p2 = -p4, and after that ref1 == -99: p4 = -p2 (both marked: p4 stays, p2 = -p4; the
 *                     negations give -0 where the reference's do).  Slots 0, 1, 2 = fl(p2 * w) / 128 with w = 3, 2, 1, slot 3 = +0,
 *                     slots 4, 5, 6 = fl(p4 * w) / 128 with w = 1, 2, 3.  The reference's mvs1 equals this field: it is written once.
 * cdfo_charbonnier:  sr, hr: n fp32 values each.  grad[i] = d / sqrt(d^2 + eps), d = sr[i] - hr[i]; *loss = the sum of
 *                     sqrt(d^2 + eps), accumulated in fp64 (partials per workgroup, added in a fixed order by a second launch: no
 *                     atomics, equal inputs give equal bits), rounded once to fp32.  Square root and division correctly rounded;
 *                     non-finite values propagate.  partial: scratch of partial_cap doubles, 8-byte aligned; min(ceil(n / 1024),
 *                     CDFO_CHARBONNIER_MAX_BLOCKS) are used, so CDFO_CHARBONNIER_MAX_BLOCKS always suffice (less is CDFO_EINVAL when
 *                     it does not).  Two launches whatever n. */
#define CDFO_CHARBONNIER_MAX_BLOCKS 1024
int cdfo_train_batch(const unsigned char* lr, const unsigned char* pms, const signed char* rms, const unsigned char* ufs,
                     const signed char* mvl0, const unsigned char* hr, int S, int T, int H, int W, int Hu, const int* plan, int B,
                     int crop, float* x, float* pms_out, float* rms_out, float* ufs_out, float* mvs0, float* hr_out, void* stream);
int cdfo_train_batch_ra(const unsigned char* lr, const unsigned char* pms, const signed char* rms, const unsigned char* ufs,
                        const signed char* mvl0, const signed char* mvl1, const unsigned char* hr, int S, int T, int H, int W, int Hu,
                        const int* plan, int B, int crop, float* x, float* pms_out, float* rms_out, float* ufs_out, float* mvs,
                        float* hr_out, void* stream);
int cdfo_charbonnier(const float* sr, const float* hr, long long n, float eps, float* grad, double* partial, int partial_cap,
                     float* loss, void* stream);

/* ---- the focal frequency loss and its 2-D FFT pair (ffl.hip; cdfo_amd/loss.py: focal_frequency_loss) ----
 * Frames are dense fp32 [N][H][W]; H and W are powers of two from CDFO_FFL_MIN to CDFO_FFL_MAX and may differ, 1 <= N <= 65535.  A
 * spectrum F is complex fp32 [N][H][W] (re, im interleaved, 8-byte aligned), bin (ky, kx) = sum_yx d[y][x] exp(-2 pi i (ky y / H +
 * kx x / W)) / sqrt(H W): the full spectrum of numpy's fft2(norm="ortho").  tw_h, tw_w: the twiddle tables of the two lengths on the
 * device, n / 2 pairs (cos, sin)(2 pi k / n) in fp32 for length n, computed in fp64 and rounded once by the caller, 8-byte aligned
 * (one pointer serves both when H == W).  Every entry point checks its arguments before any HIP call: a null pointer, N, H or W
 * outside the above, a scratch capacity that is too small and an alpha that is negative or not finite are CDFO_EINVAL.
 * cdfo_ffl_tiles:    P(H, W) = W / 16 (W / 8 when H = 512), the column tiles of a frame; cdfo_ffl_strips: S(H, W) = max(1, H W /
 *                    4096), the strips of the weight pass.  Functions of the shape alone; CDFO_EINVAL for a size outside the set.
 * cdfo_ffl_spectrum: d = sr - hr (one fp32 subtraction) -> F = fft2(d) / sqrt(H W), the scale applied once in fp64, and pmax [N][P]
 *                    fp64: per column tile the maximum of D = re^2 + im^2 of the ROUNDED fp32 bins, formed in fp64 (a NaN is
 *                    skipped).  pmax_cap >= N P doubles.  Two launches.
 * cdfo_ffl_weight:   F and pmax [N][P] (any P >= 1 values per frame whose maximum is the frame's largest D) -> loss[n] = sum_bins(w D)
 *                    / (H W), D as above, w = M / max M with M = sqrt(D)^alpha (alpha == 1: no pow; 0^0 = 1), NaN -> 0, clamped to
 *                    [0, 1]; w, the terms and the sum in fp64, strips of 4096 bins added in index order, one rounding to fp32.  With
 *                    `apply` F is overwritten by w F (product in fp64, rounded once).  partial: scratch of partial_cap >= N S
 *                    doubles.  A frame with a non-finite bin gets a NaN loss; other frames are untouched.  Two launches.
 * cdfo_ffl_inverse:  F -> g [N][H][W] = 2 / (H W) Re(ifft2(F) sqrt(H W)), i.e. the gradient of the loss when F holds w F; the scale
 *                    is applied once in fp64, the imaginary part is dropped.  F IS OVERWRITTEN (the column pass works in place).
 *                    Two launches.
 * Radix-2 transforms in LDS; no atomics, grids are functions of (N, H, W) alone, equal inputs give equal bits.  Every element of
 * every output is written. */
#define CDFO_FFL_MIN 16
#define CDFO_FFL_MAX 512
int cdfo_ffl_tiles(int H, int W);
int cdfo_ffl_strips(int H, int W);
int cdfo_ffl_spectrum(const float* sr, const float* hr, int N, int H, int W, const float* tw_h, const float* tw_w, float* F,
                      double* pmax, int pmax_cap, void* stream);
int cdfo_ffl_weight(float* F, const double* pmax, int P, int N, int H, int W, float alpha, int apply, double* partial,
                    int partial_cap, float* loss, void* stream);
int cdfo_ffl_inverse(float* F, int N, int H, int W, const float* tw_h, const float* tw_w, float* g, void* stream);

/* ---- Adam on the device (adam.hip; cdfo_amd/optim.py: DeviceAdam) ----
 * The moments of all parameters live in one fp32 buffer m and one fp32 buffer v of `total` elements each (16-byte aligned, total a
 * multiple of 4); parameters and gradients stay the caller's fp32 tensors.
 * table:      [ntensors][4] 64-bit words (p, g, offset, n) on the device: tensor t has n elements at p, its gradient at g, and
 *             owns [offset, offset + n) of m and v; offset is a multiple of 4.  table_host is the host copy the caller uploaded: the
 *             entry points validate IT (a null p or g, n < 0 or above INT_MAX, an offset that is negative, not a multiple of 4 or,
 *             in cdfo_adam_step, with offset + n > total are CDFO_EINVAL; p or g not 4-byte aligned is CDFO_EALIGN) and never read
 *             the device table on the host.  p and g need not be 16-byte aligned: such a tensor takes a scalar path.
 * chunks:     [nchunks][2] ints (tensor, first element) on the device: every run of at most CDFO_ADAM_CHUNK elements of every
 *             tensor once, first a multiple of CDFO_ADAM_CHUNK (cdfo_amd/optim.py: chunk_table).  A row that lies outside its
 *             tensor, or outside m and v, touches nothing.
 * cdfo_grad_norm_partials: partials[c] = sum of g^2 over chunk c, products and sums in fp64, in a fixed order (adam.hip).
 * cdfo_adam_scalars:       one workgroup adds the partials in a fixed order and writes scalars [6] (fp64): [0] norm = sqrt(sum),
 *             [1] coef = 1 when max_norm <= 0 or norm <= max_norm, else max_norm / (norm + 1e-6), rounded to fp32, [2] step_size =
 *             lr / (1 - beta1^step), [3] 1 / sqrt(1 - beta2^step), [4] skip = !isfinite(sum), [5] the sum of norm over the
 *             unskipped steps so far.  counters [2] (64-bit): unless skipping, step = ++counters[0] before [2] and [3] are formed
 *             from it; when skipping ++counters[1] and [1..3], [5] keep their values.  lr < 0 or NaN, a beta outside [0, 1) and a
 *             NaN max_norm are CDFO_EINVAL.
 * cdfo_adam_step:          returns at once when scalars[4] is set (p, m, v keep their bits); else per element in fp32
 *             g' = coef g + wd p;  m += (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g' g';  p -= step_size (m / (sqrt(v)
 *             inv_bc2_sqrt + eps)), torch.optim.Adam's single-tensor statement (L2 weight decay, no amsgrad).  g is not written.
 * Every entry point: a null pointer, ntensors <= 0, nchunks <= 0 are CDFO_EINVAL.  One launch each, no atomics, grids are functions
 * of the sizes alone, equal inputs give equal bits. */
#define CDFO_ADAM_CHUNK 4096
int cdfo_grad_norm_partials(const long long* table_host, const long long* table, int ntensors, const int* chunks, int nchunks,
                            double* partials, void* stream);
int cdfo_adam_scalars(const double* partials, int nchunks, double lr, double beta1, double beta2, double max_norm,
                      long long* counters, double* scalars, void* stream);
int cdfo_adam_step(const long long* table_host, const long long* table, int ntensors, const int* chunks, int nchunks, float* m,
                   float* v, long long total, const double* scalars, double beta1, double beta2, double eps, double weight_decay,
                   void* stream);

/* ---- SSIM and MS-SSIM as training losses (ssim_loss.hip; cdfo_amd/loss.py: ssim_loss, msssim_loss) ----
 * A frame is dense fp32 [H][W], a stack [N][H][W], 1 <= N <= 65535.  `levels` is 1 (SSIM: H, W >= 11) or 5 (MS-SSIM: H, W >=
 * CDFO_MSSSIM_MIN); H, W <= 16384 are the sizes of LEVEL 0 in every call; level j is (H >> j) x (W >> j), and x, y of a call with
 * `level` are that level's stacks.  peak: finite and > 0; C1 = (0.01 peak)^2, C2 = (0.03 peak)^2 in fp64.  Per valid position of a
 * level, with the 11-tap Gaussian of cdfo_metric_partials, behind the fp32 loads in fp64: m1 = G*x, m2 = G*y, e11 = G*x^2, e22 =
 * G*y^2, e12 = G*xy, cs = (2 (e12 - m1 m2) + C2) / ((e11 - m1^2) + (e22 - m2^2) + C2), l = (2 m1 m2 + C1) / (m1^2 + m2^2 + C1).
 * Every entry point checks its arguments before any HIP call: a null pointer, N, H, W, levels, level or peak outside the above and a
 * capacity that is too small are CDFO_EINVAL, a misaligned pointer (4 bytes for fp32, 8 for fp64) CDFO_EALIGN.
 * cdfo_ssim_loss_tiles:   T(H, W, levels), the tiles of 16 x 32 valid positions of all levels of a frame; no launch.
 * cdfo_ssim_loss_level:   partial [N][T][2] fp64 (partial_cap >= 2 N T doubles): the level's tiles, behind those of the levels before
 *                         it, get (sum cs, sum l cs) over the tile, added in a fixed order.  One launch.
 * cdfo_ssim_loss_pool:    x, y [N][h][w] (h, w >= 22) -> xn, yn [N][h / 2][w / 2]: fp32(((a + b) + c) + d in fp64, times 0.25) of the
 *                         2 x 2 block from the top-left sample; a trailing odd row or column is dropped.  One launch.
 * cdfo_ssim_loss_combine: partial (every level written) -> means [N][levels][2] = (M_cs, M_ssim), the tiles added in index order;
 *                         loss [N] fp32 = 1 - M_ssim[0] (levels 1) or 1 - prod_{j<4} M_cs[j]^w[j] M_ssim[4]^w[4], rounded once;
 *                         coef [N][levels][2] = (d loss / d M_cs[j], d loss / d M_ssim[j]).  If any of the five means used is <= 0
 *                         the loss is exactly 1 and the frame's coefficients are 0.  One launch.
 * cdfo_ssim_loss_pqr:     pqr [N][3][h - 10][w - 10] fp64 (pqr_cap doubles) of the level: P = d/d m1, Q = d/d e11, R = d/d e12 of
 *                         (coef[n][level][0] sum cs + coef[n][level][1] sum l cs) / ((h - 10)(w - 10)).  One launch.
 * cdfo_ssim_loss_adjoint: the level's gradient by x: (Gt*P + 2 x Gt*Q) + y Gt*R, Gt* the full correlation (the adjoint of the valid
 *                         one), plus, for level < levels - 1, a quarter of coarse [N][h / 2][w / 2] (the next level's gradient,
 *                         fp64, required) at (row / 2, column / 2) where that exists.  Level 0 writes g32 [N][H][W], rounded once;
 *                         a level above 0 writes g64 [N][h][w].  The pointer the level does not use is ignored.  One launch.
 * No atomics, grids are functions of (N, H, W) alone, equal inputs give equal bits.  Every element of every output is written. */
#define CDFO_MSSSIM_MIN 176
int cdfo_ssim_loss_tiles(int H, int W, int levels);
int cdfo_ssim_loss_level(const float* x, const float* y, int N, int H, int W, int levels, int level, double peak, double* partial,
                         long long partial_cap, void* stream);
int cdfo_ssim_loss_pool(const float* x, const float* y, int N, int h, int w, float* xn, float* yn, void* stream);
int cdfo_ssim_loss_combine(const double* partial, long long partial_cap, int N, int H, int W, int levels, double* means, double* coef,
                           float* loss, void* stream);
int cdfo_ssim_loss_pqr(const float* x, const float* y, int N, int H, int W, int levels, int level, double peak, const double* coef,
                       double* pqr, long long pqr_cap, void* stream);
int cdfo_ssim_loss_adjoint(const double* pqr, const float* x, const float* y, int N, int H, int W, int levels, int level,
                           const double* coarse, double* g64, float* g32, void* stream);

/* ---- optional per-launch HIP-event timing on the launch stream (bench.py's live roofline figures) ----------- */
int cdfo_prof_begin(int max_records);
int cdfo_prof_end(int* launches, double* ms, double* flops, double* bytes, int nkid);
int cdfo_prof_kid_count(void);

#ifdef __cplusplus
}
#endif
#endif
