/*
 * ica_hip.h — C ABI of libica_hip.so, the MI355X (gfx950) drop-in for the
 * adversarial-attack hot path of tongxyh/ImageCompression_Adversarial.
 *
 * Conventions
 *   - All tensor arguments are device pointers (fp32) allocated and owned by
 *     the caller (PyTorch's caching allocator); the library never allocates
 *     or frees caller memory and never synchronises the stream.
 *   - Activation tensors on the hot path use the nChw4c layout
 *     [N][ceil(C/4)][H][W][4]; padded channels are zero.  Image-domain tensors
 *     (noise, im_s, output_s, m, v) are plain NCHW [B][3][H][W].
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream).
 *   - Every function returns 0 on success, a hipError_t from the launch, or a
 *     negative code for an unsupported shape/variant (-2 channel multiple,
 *     -3 channel tile, -4 epilogue/shape mismatch, -5 epilogue id, -6 kernel
 *     geometry).  The Python layer turns non-zero into RuntimeError.
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   conv / deconv layers + autograd dgrad .......... anchors/utils.py:112-130 (via CompressAI g_a/g_s, h_a/h_s)
 *   GDN / IGDN (fwd + bwd) .......................... utils/ops.py:58-97  (== compressai.layers.GDN)
 *   Low_bound / Up_bound (clamp + pass-through) ..... utils/ops.py:28-56
 *   attack step (box, clamp, L2 loss, branch, Adam)  attack_rd.py:496-559, attack_our :332-379
 *   C&W-style search (gate, Adam, both bisections) . attack_cw.py:115-199, 238-259; attack_cw_fast.py:100-183, 222-243
 *   I-FGSM / MI-FGSM update + projection ........... attack_ifgsm.py:348-362, 405-419
 *   EntropyBottleneck / GaussianConditional lik. ... anchors/model.py:86-108, anchors/balle.py:31-55 (CompressAI)
 *   bpp ............................................. attack_rd.py:419, self_ensemble.py:222
 *   MS-SSIM (pytorch_msssim / utils.torch_msssim) .. attack_rd.py:336,362; utils/torch_msssim.py:26-71
 *   entropy coding (CompressAI compress/decompress, the _quantized_cdf / _offset / _cdf_length buffers
 *     anchors/balle.py:57-72 restores) ............. ica_gc_symbols / ica_eb_symbols / ica_dequantize /
 *                                                     ica_pmf_to_quantized_cdf / ica_rans_encode / ica_rans_decode
 */
#ifndef ICA_HIP_H
#define ICA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

/* ---- conv engine (ica_conv.hip) ------------------------------------------- */
/* epilogue ids */
enum { ICA_EPI_BIAS = 0, ICA_EPI_RELU = 1, ICA_EPI_GDN = 2, ICA_EPI_IGDN = 3, ICA_EPI_GDN_BWD = 4, ICA_EPI_IGDN_BWD = 5 };

/* 32-channel MFMA row tiles per wave the launchers use for `cout` output channels. */
int ica_conv_it(int cout);
/* floats needed for the packed fragments of a weight viewed as W[O][C][KS][KS], chunk CC (4|16),
 * it = 32-channel row tiles per wave (0: ica_conv_it(O)); conv launches must use the same it. */
size_t ica_pack_conv_weight_size(int O, int C, int KS, int CC, int it);
/* Pack W (element (o,c,ky,kx) at w[o*so + c*sc + ky*KS + kx]); order 0 = conv_down, 1 = conv_up.
 * flip != 0 reverses the taps (W[o][c][KS-1-ky][KS-1-kx]): the dgrad of a stride-1 conv as a conv_down. */
int ica_pack_conv_weight(const float* w, float* dst, int O, int C, int KS, long so, long sc, int CC, int order,
                         int flip, int it, hipStream_t stream);
/* GDN reparametrisation + fragment packing: gamma' = max(gamma,2^-18)^2 - 2^-36 (transpose 0: gamma', 1: gamma'^T),
 * beta_eff = max(beta, beta_bound)^2 - 2^-36.  gp holds (C/32)^2 * 1024 floats. */
int ica_pack_gdn(const float* gamma, const float* beta, float* gp, float* beta_eff, int C, int transpose,
                 float beta_bound, hipStream_t stream);
/* bf16-operand packs for ica_conv_ex launches with prec = 1 (the bf16 MFMA conv path).
 * ica_pack_conv_weight_bf16: the fragment order of ica_pack_conv_weight with CC = 16, each element rounded to
 *   bf16 (RNE); dst holds ica_pack_conv_weight_size(O, C, KS, 16, it) bf16 values.
 * ica_pack_gdn_bf16: gamma' (or gamma'^T) as bf16 hi/lo pairs in the k order of accumulator-as-operand MFMAs
 *   (the GDN normaliser / GDN-bwd GEMMs use the hi part: bf16 is what the stored y and s carry; the lo part is
 *   packed for a bf16x3 variant); gpb holds (C/32)^2 * 2048 bf16. */
int ica_pack_conv_weight_bf16(const float* w, void* dst, int O, int C, int KS, long so, long sc, int order,
                              int flip, int it, hipStream_t stream);
int ica_pack_gdn_bf16(const float* gamma, const float* beta, void* gpb, float* beta_eff, int C, int transpose,
                      float beta_bound, hipStream_t stream);
/* fp32-accurate bf16x6 packs for ica_conv_ex launches with prec = 2 (ica_conv_x6.hip; the anchors/utils.py:112-130
 * k5 s2 conv / deconv layers of g_a and g_s and their input gradients).  Each weight w is split exactly into three
 * bf16 parts w = hi + mid + lo; dst holds three planes (hi, mid, lo), each in the CC = 16 fragment order of
 * ica_pack_conv_weight (order 0: conv_down, 1: conv_up) with row tiles it (> 0).  For KS = 5, it = 4 the buffer
 * continues with the tap-pair pack of the 8-wave conv_down (three planes of [cb][K step][it][lane] fragments; lane half
 * h of a step = tap 2 s + h of an 8-channel chunk, chunk pairs sharing a tap-24 step; filled for order 0);
 * ica_pack_conv_weight_x6_size(O, C, KS, it) bf16 values in all.  Order 2 (KS = 5, C <= 3: the RGB-side conv_down
 * of g_a.0 forward / the g_s.6 input gradient, 128 output channels) packs the dense tap-row K of conv_rgb5_x6
 * instead: three planes of [cb][ky][it][lane] fragments, k = 8 h + e of step ky holding (kx, c) = h 0: (0..1, 0..2),
 * (4, 0..1); h 1: (2..3, 0..2), (4, 2), zero; it fits in the size above.  Returns -2 for order 2 with other shapes. */
int ica_pack_conv_weight_x6(const float* w, void* dst, int O, int C, int KS, long so, long sc, int order, int it,
                            hipStream_t stream);
size_t ica_pack_conv_weight_x6_size(int O, int C, int KS, int it);
/* The fp32 gamma' (or gamma'^T) pack of ica_pack_gdn split exactly into three bf16 planes for the x6 GDN / IGDN
 * epilogues (their normaliser GEMMs run as bf16x6 MFMAs too); ica_pack_gdn_x6_size(C) bytes. */
int ica_pack_gdn_x6(const float* gp, void* dst, int C, hipStream_t stream);
size_t ica_pack_gdn_x6_size(int C);
/* bf16 values ica_pack_conv_weight_bf16 writes.  C <= 4 (an RGB conv input; conv_down only) packs "tap groups":
 * k = 8h + j of MFMA tg is tap 4tg + 2h + (j>>2), channel j&3 (7 MFMAs per 32-row tile for 5x5 taps). */
size_t ica_pack_conv_weight_bf16_size(int O, int C, int KS, int it);
/* cheng2020 g_a.0 input gradient, fused (replaces the backward of compressai ResidualBlockWithStride(3, N)'s conv1 =
 * conv3x3(3, N, stride 2) and skip = conv1x1(3, N, stride 2), reference anchors/model.py:76-77 -> cheng2020_anchor):
 * dx [N][1][Hout][Wout][4] = conv3x3_s2^T(g1) + conv1x1_s2^T(gs), g1 / gs [N][Cg/4][Hin][Win][4] row-major, Hin =
 * ceil(Hout / 2), Win = ceil(Wout / 2), Cg % 16 == 0; x6 operands.  Weights: conv1 [Cg][3][3][3], skip [Cg][3][1][1]
 * -> ica_pack_up3k3_x6 (ica_pack_up3k3_x6_size(Cg) bytes). */
int ica_pack_up3k3_x6(const float* w1, const float* ws, void* dst, int Cg, hipStream_t stream);
size_t ica_pack_up3k3_x6_size(int Cg);
int ica_conv_up3k3_x6(const float* g1, const float* gs, const void* wp, float* dx, int N, int Cg, int Hin, int Win,
                      int Hout, int Wout, hipStream_t stream);
/* bf16 conv path activations are bf16 nChw4c (8 B per channel quad): every prec = 1 conv_down / conv_up reads
 * bf16 x (except 4-channel RGB inputs, fp32), writes bf16 y / save_s and reads bf16 in_x / in_s; the Z-gather
 * kernel reads bf16 x and writes fp32 y.  Casts for the tensors that leave the path (n % 4 == 0): */
int ica_cast_f32_bf16(const float* x, void* y, long n, hipStream_t stream);
int ica_cast_bf16_f32(const void* x, float* y, long n, hipStream_t stream);

/* ---- eval-time defences (ica_defend.hip; self_ensemble.py:34-83) ------------------- */
/* NCHW planes (planes = batch * channels).  op 0 flip rows, 1 flip columns, 2 torch.rot90(k=1, dims [2,3]),
 * 3 rot90(k=-1); ops 2/3 write W x H planes. */
int ica_flip_rot(const float* x, float* y, long planes, int H, int W, int op, hipStream_t stream);
/* y = round_half_even(x * scale) / scale (self_ensemble.bitdepth_reduction, inference=True; scale = 2^bits - 1) */
int ica_bitdepth(const float* x, float* y, long n, float scale, hipStream_t stream);
/* one separable pass of the antialiased bicubic resize (F.interpolate(..., "bicubic", antialias=True)):
 * axis 1 maps columns W -> out_len, axis 0 rows H -> out_len; out[o] = sum_{k<xsize[o]} w[o*K+k] in[xmin[o]+k];
 * the tables are device arrays built on the host (self_ensemble.aa_table). */
int ica_resample_axis(const float* x, float* y, long planes, int H, int W, int axis, int out_len, const int* xmin,
                      const int* xsize, const float* w, int K, hipStream_t stream);
/* Attacking through the defence (self_ensemble.py --adv, :253-270):
 * y = (x * scale + u) / scale (bitdepth_reduction(inference=False), :66-69, u given) and its input gradient
 * gx = (g / scale) * scale; y = a + b (training-mode "noise" quantisation of the latent);
 * ensemble branch loss gradient g = [0 <= o <= 1] * 2 invN (out_s - clamp(o, 0, 1)) (:112, :261-270). */
int ica_bitdepth_noise(const float* x, const float* u, float* y, long n, float scale, hipStream_t stream);
int ica_bitdepth_noise_bwd(const float* g, float* gx, long n, float scale, hipStream_t stream);
int ica_add(const float* a, const float* b, float* y, long n, hipStream_t stream);
int ica_ensemble_grad(const float* o, const float* out_s, float* g, long n, float invN, hipStream_t stream);
/* Entropy coding (CompressAI EntropyBottleneck / GaussianConditional compress + decompress).
 * Device: symbols / CDF indexes of nChw4c latents in NCHW order (int32), and dequantisation back to nChw4c.
 *   ica_gc_symbols: idx = T-1 - #{j<T-1: max(scale, bound) <= table[j]}, sym = round(y - mean) (means4 may be NULL)
 *   ica_eb_symbols: sym = round(z - medians[c]), idx = c
 *   ica_dequantize: out = sym + (means4 ? means4 : medians ? medians[c] : 0)
 * Host (plain pointers, no stream): 16-bit quantised CDFs and the 64-bit rANS coder (32-bit words, 4-bit bypass
 * coding of values outside a table's range).  cdfs: n_cdfs rows of `stride` int32, row k valid for cdf_sizes[k]
 * entries, offsets[k] = the value of slot 0.  ica_rans_encode returns the byte count (-7: cap too small, *needed
 * holds the size; -5 bad table); ica_rans_decode returns 0 (-8 truncated / corrupt stream, -5 bad table). */
int ica_gc_symbols(const float* y4, const float* scales4, const float* means4, const float* table, int T, float bound,
                   int32_t* symbols, int32_t* indexes, int B, int C, int H, int W, hipStream_t stream);
int ica_eb_symbols(const float* z4, const float* medians, int32_t* symbols, int32_t* indexes, int B, int C, int H,
                   int W, hipStream_t stream);
int ica_dequantize(const int32_t* symbols, const float* means4, const float* medians, float* out4, int B, int C, int H,
                   int W, hipStream_t stream);
int ica_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int32_t* cdf_out);
long ica_rans_encode(const int32_t* symbols, const int32_t* indexes, long n, const int32_t* cdfs, int stride,
                     const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, uint8_t* out, long cap,
                     long* needed);
int ica_rans_decode(const uint8_t* data, long nbytes, const int32_t* indexes, long n, const int32_t* cdfs, int stride,
                    const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int32_t* symbols);
/* Incremental decoding (context models: one latent position of every image per call, because the next position's
 * CDF rows depend on the symbols just decoded).  open: *decoder = a decoder over one bitstream (-8 and NULL for a
 * malformed one); step: n symbols from each of B decoders (indexes / symbols [B][n]; the first error, its image in
 * *bad); close frees one decoder. */
int ica_rans_dec_open(const uint8_t* data, long nbytes, void** decoder);
int ica_rans_dec_step(void* const* decoders, int B, const int32_t* indexes, long n, const int32_t* cdfs, int stride,
                      const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int32_t* symbols, int* bad);
int ica_rans_dec_close(void* decoder);

/* Autoregressive coding of the context models' latents (mbt2018 / cheng2020; CompressAI
 * JointAutoregressiveHierarchicalPriors._compress_ar / _decompress_ar, anchors/model.py:97-106): one workgroup
 * per image walks the latent raster; per position the type-A 5x5 masked context conv over the 12 causal taps of
 * the zero-padded y_hat, entropy_parameters (1x1: 4M -> E1 -> E2 -> 2M, LeakyReLU 0.01), scales / means, CDF row
 * index (as ica_gc_symbols) and, encoding, symbol = round(y - mean), y_hat = symbol + mean.
 *   y, params  nChw4c latents [B][M/4][H][W][4] and h_s output [B][2M/4][H][W][4]
 *   yhat       [B][M][H+4][W+4] float, zero-initialised by the caller (the padded y_hat)
 *   sym, idx   mode 0: [B][H W M] (position-major, the bitstream order); mode 1: idx [B][M] of position p0
 *   sym_in     mode 1: [B][M] decoded symbols of position p0 - 1 (applied first when p0 > 0); means [B][M]
 *   wc [2M][12M] (k = tap * M + c, taps: rows 0-1 of the window, then row 2 columns 0-1), bc [2M],
 *   w1 [E1][4M], w2 [E2][E1], w3 [2M][E2] and biases: the entropy_parameters 1x1 weights
 * mode 0 encodes positions [p0, p1); mode 1 is one decode step (p1 <= p0 + 1).  Returns 0, -2 bad sizes, -4 mode. */
typedef struct ica_ar_args {
  const float* y;
  const float* params;
  float* yhat;
  int32_t* sym;
  int32_t* idx;
  const int32_t* sym_in;
  float* means;
  const float* wc;
  const float* bc;
  const float* w1;
  const float* b1;
  const float* w2;
  const float* b2;
  const float* w3;
  const float* b3;
  const float* table;
  int T;
  float bound;
  int B, M, H, W, E1, E2;
} ica_ar_args;
size_t ica_ar_lds_bytes(int M, int E1, int E2);
int ica_ar_step(const ica_ar_args* args, int p0, int p1, int mode, hipStream_t stream);
/* The conv launch (all geometries / epilogues / extras).  kind 0 = conv_down (stride-S KSxKS conv, pad KS/2;
 * (KS,S) in {(5,2),(3,1),(3,2),(1,2),(1,1),(5,1)}), kind 1 = conv_up (stride-2 transposed conv, pad KS/2,
 * output_padding 1; KS in {5,3,1} — the input-gradient of a stride-2 conv).  Epilogues add ICA_EPI_LRELU (6,
 * slope 0.01) and ICA_EPI_LRELU_BWD (7: y = acc * (in_x > 0 ? 1 : 0.01)).  Optional extras:
 *   res        forward: y = act(acc + bias) + res;  GDN_BWD/IGDN_BWD: acc += res first
 *   save_x     forward: act output before the residual;  GDN_BWD/IGDN_BWD: acc + res
 *   ps         PixelShuffle(2) store (rho-ordered rows: rho = 16*c4 + 4*q + e -> channel 4*c4+e, sub-pixel q)
 *   fill_mode  conv_down input view: 1 = x * leaky_relu'(mask), 2 = PixelUnshuffle(2) of a (2H)x(2W) x
 *   it         32-channel row tiles per wave (0 = ica_conv_it(Cout)); 6 runs C = 192 GDN layers in one wave.
 * GDN / IGDN: gp = gamma' fragments, beta = beta_eff, optional save_s output (y = x * s is the layer's output).
 * GDN_BWD / IGDN_BWD: x holds dL/dy of the GDN behind this conv's output, gp = gamma'^T fragments, in_x / in_s = that
 * GDN's saved (y, s); y receives dL/dx.  save_t (may be NULL) receives t = dL/dn, n = beta' + gamma' x^2 the GDN
 * norm, from which the GDN parameter gradients follow (ica_channel_sum, ica_wgrad KS=1).
 * Reference: CompressAI cheng2020-anchor blocks (anchors/model.py:76-77). */
enum { ICA_EPI_LRELU = 6, ICA_EPI_LRELU_BWD = 7 };
/* Fragment orders of a packed weight (ica_conv_args.order).  DOWN / UP: the `order` argument of the packers (conv_down
 * [cb][chunk][tap], conv_up [cb][tap][chunk]); RGB5: the dense tap-row pack (order 2 of ica_pack_conv_weight_bf16 /
 * _x6); TG: the tap groups ica_pack_conv_weight_bf16 writes for C <= 4 with order 0; UP3: the Z-gather pack of
 * ica_pack_up3 (read by ica_conv_up3 only, never by ica_conv_ex). */
enum { ICA_ORDER_DOWN = 0, ICA_ORDER_UP = 1, ICA_ORDER_RGB5 = 2, ICA_ORDER_TG = 3, ICA_ORDER_UP3 = 4 };
typedef struct ica_conv_args {
  const float* x;
  float* y;
  const float* wp;
  const float* bias;
  const float* gp;
  const float* beta;
  float* save_x;
  float* save_s;
  const float* in_x;
  const float* in_s;
  float* save_t;
  const float* res;
  const float* mask;
  int N, Cin, Hin, Win, Cout, Hout, Wout;
  int kind, KS, S, epi, it, fill_mode, ps;
  int prec; /* 0: fp32 operands (exact fp32 MFMA); 1: bf16 operands, fp32 accumulate (wp / gp from the _bf16
             * packers; bmshj2018 k5 s2 layers: conv_down BIAS/GDN/IGDN_BWD, conv_up BIAS/IGDN/GDN_BWD);
             * 2: fp32-accurate bf16x6 operands (wp from ica_pack_conv_weight_x6, gp from ica_pack_gdn_x6, fp32
             * x / y / saved tensors; k5 s2, Cin >= 16: conv_down BIAS/GDN/IGDN_BWD, conv_up BIAS/IGDN/GDN_BWD, 128 output channels,
             * or 96-multiples with the bias epilogue; k3 s1 conv_down (kind 0, it 4 or 6): every epilogue and fill
             * mode except a save_t output, gp from ica_pack_gdn_x6 as well);
             * 3: bf16 operands over fp32 tensors on the k3 conv_downs (kind 0, KS 3: stride 1 as for prec 2, stride
             * 2 plain-fill bias / leaky-ReLU forwards; it 4 or 6): wp from ica_pack_conv_weight_x6, of which only
             * the hi plane (RNE bf16 of the weight) is read; the activation is rounded to bf16 (RNE) as it is
             * staged; fp32 accumulate; GDN epilogue GEMMs on the ica_pack_gdn_x6 pack (cheng2020 --precision bf16,
             * attack_rd.py:712-715) */
  int layout; /* parity-split pixel order (k5 s2, plain fill, no ps; 0 = row-major everywhere): bit 0 = x, bit 1 = y and
               * every other output-layout tensor (save_x / save_s, in_x / in_s, save_t, res).  A parity-split
               * H x W plane (H, W even) stores the four (y & 1, x & 1) sub-planes of (H/2) x (W/2) pixels one after
               * another, so a transposed conv's output-parity classes write and read dense lines */
  int order; /* ICA_ORDER_* of wp.  Each route reads one order: kind 1 UP; kind 0 DOWN, but TG for prec 1 with Cin <= 4
              * and RGB5 for the prec 1 / 2 RGB-side k5 s2 conv_down (Cin <= 3, 128 outputs, BIAS/GDN/IGDN_BWD, plain
              * fill, no extras).  Any other order returns -4: a pack is never read as a layout it does not have */
} ica_conv_args;
int ica_conv_ex(const ica_conv_args* args, hipStream_t stream);
/* Evidence, not compute: the kernel and grid of the calling thread's last kernel launch (any entry point of this
 * library), and how many launches there were since the previous call, which consumes the record.  name receives the
 * demangled kernel name as rocprofv3 prints it (truncated to cap - 1 chars), *threads the grid size in threads
 * (rocprofv3's Grid_Size).  Returns the launch count (0: none since the previous call; name and *threads untouched).
 * bench.py matches its PMC traffic stamps (profiles/pmc_traffic*.json) against the launch it timed, and only when the
 * timed region held exactly one launch. */
int ica_last_launch(char* name, int cap, unsigned long long* threads);
/* Tiling the x6 k5 s2 pickers take (process-wide; for tests and A/B runs): 0 = their own choice from the grid (the
 * default), 1 = the large-grid kernel a layer ran before it had a second one, whatever the grid, 2 = the newer one
 * wherever a layer has it (ica_conv_x6.hip: g_x6_tiling); 1 and 2 skip the small-grid kernels.  The large-grid
 * kernels of a layer give the same bits as each other; the small-grid kernels sum in another order, so for maps of
 * <= 32 x 32 pixels modes 1 / 2 match mode 0 to fp32 rounding only.  Read once per launch (atomic); nothing in the
 * package sets it.  Returns -2 for another mode. */
int ica_x6_tiling(int mode);
/* Transposed conv to 3 channels (Z-gather kernel; g_s's last layer, deconv(N, 3) of anchors/utils.py:122-130, and the
 * input gradient of g_a's first, conv(3, N) of anchors/utils.py:112-119): w view [Cin][3][5][5], Cin % 16 == 0.
 * prec as ica_conv_args.prec, for the pack and the launch alike (another value returns -4 before any device call):
 * 0 = fp32 (dst: ica_pack_up3_size(Cin) floats); 1 = bf16 operands (dst: as many bf16; x is bf16 nChw4c, y fp32);
 * 2 = fp32-accurate bf16x6 (dst: three bf16 planes of the fp32 fragment order, 3 * ica_pack_up3_size(Cin) values).
 * layout: 1 = x parity-split (ica_conv_args.layout bit 0; even Hin / Win), 0 = row-major; the 3-channel output is
 * always row-major. */
size_t ica_pack_up3_size(int Cin);
int ica_pack_up3(const float* w, void* dst, int Cin, int prec, hipStream_t stream);
int ica_conv_up3(const float* x, float* y, const void* wp, const float* bias, int N, int Cin, int Hin, int Win,
                 int layout, int prec, hipStream_t stream);

/* ---- elementwise / attack step / entropy (ica_elem.hip) -------------------- */
int ica_elem_blocks_per_image(void);
int ica_nchw_to_nc4(const float* src, float* dst, int N, int C, int H, int W, hipStream_t stream);
int ica_nc4_to_nchw(const float* src, float* dst, int N, int C, int H, int W, hipStream_t stream);
/* out[b] = scale * sum_k part[b*nblk + k] (deterministic order). */
int ica_reduce_rows(const float* part, float* out, int B, int nblk, float scale, hipStream_t stream);
/* im_in4 = Up(Low(im_s + Up(Low(noise,-eps),eps), 0), 1) (nChw4c) ; part = per-image partial sum (im_s-im_in)^2. */
int ica_attack_prologue(const float* noise, const float* im_s, float* im_in4, float* part, int B, int H, int W,
                        float eps, hipStream_t stream);
/* ica_attack_prologue with clamp_in = 0: im_in4 = im_s + Up(Low(noise,-eps),eps), no [0, 1] clamp (the debug model,
 * attack_rd.py:514-515). */
int ica_attack_prologue_ex(const float* noise, const float* im_s, float* im_in4, float* part, int B, int H, int W,
                           float eps, int clamp_in, hipStream_t stream);
/* mode 0: dL/dx_hat of 1 - mean((os - bound01(x_hat))^2) (clamp optional); mode 1: of mean((os - x_hat)^2). */
int ica_attack_loss(const float* xhat4, const float* out_s, float* grad4, float* part, int B, int H, int W,
                    float invN, int clamp, int mode, hipStream_t stream);
/* Per-image branch (loss_i[b] > thr), bounds backward, torch-Adam step on noise/m/v (in place). */
int ica_attack_adam(float* noise, const float* im_s, const float* gnet4, const float* loss_i, const float* cheap_grad,
                    float* m, float* v, float* im_in_out, int B, int H, int W, float eps, float thr, float invN,
                    float bc2s, float neg_step, int* branch, const int* gpos, int* census, hipStream_t stream);
/* ica_attack_adam with clamp_in = 0: no [0, 1] bound on im_in, so none in the backward (the debug model). */
int ica_attack_adam_ex(float* noise, const float* im_s, const float* gnet4, const float* loss_i,
                       const float* cheap_grad, float* m, float* v, float* im_in_out, int B, int H, int W, float eps,
                       float thr, float invN, float bc2s, float neg_step, int* branch, const int* gpos, int* census,
                       int clamp_in, hipStream_t stream);
/* ---- universal perturbation (ica_universal.hip; DESIGN.md §8 "Universal perturbation") ----
 * One noise [1][3][H][W] (with its m, v) for B images: attack_rd.attack_ with a noise that broadcasts over the batch.
 * ica_universal_prologue: im_in4[b] = Up(Low(im_s[b] + Up(Low(noise,-eps),eps), 0), 1) and the partial sums of
 * (im_s - im_in)^2, the ops, block-to-pixel mapping and partial layout of ica_attack_prologue (noise stride 0).
 * ica_universal_adam: cheap = loss_i[0] > thr for the whole batch (the coupled loop has written the batch mean into
 * every entry; branch[b], census[b] are written for every b); per noise element g_b = cheap ? -2 fl(gscale (s_b -
 * ii_b)) : gnet4[b] through image b's [0, 1] pass-through, G = ((g_0 + g_1) + ...) + g_{B-1} in that order, then the
 * noise bounds' pass-through and ica_attack_adam's Adam on noise / m / v.  gnet4 [B][1][H][W][4] is read on the
 * expensive branch only; im_in_out (optional) [B][3][H][W] gets every image's im_in.  H * W < 2^27. */
int ica_universal_prologue(const float* noise, const float* im_s, float* im_in4, float* part, int B, int H, int W,
                           float eps, hipStream_t stream);
int ica_universal_adam(float* noise, const float* im_s, const float* gnet4, const float* loss_i, float* m, float* v,
                       float* im_in_out, int B, int H, int W, float eps, float thr, float gscale, float bc2s,
                       float neg_step, int* branch, int* census, hipStream_t stream);
/* Branch compaction: sel[0] = E = #images with loss_i <= thr (the network branch, attack_rd.py:334), sel[1..E] =
 * their indexes in order, gpos[b] = row of image b in the compacted sub-batch (-1: cheap branch, no network).
 * ica_attack_adam / ica_roi_adam read the network gradient of image b from row gpos[b] (gpos null: row b) and,
 * with census non-null, add the cheap flag into census[b] (per-image count of cheap-branch steps). */
int ica_branch_select(const float* loss_i, float thr, int B, int* sel, int* gpos, hipStream_t stream);
/* dst[r] = src[idx[r]], r < E, whole images of floats_per_image floats (a multiple of 4). */
int ica_gather_images(const float* src, float* dst, const int* idx, int E, long floats_per_image, hipStream_t stream);
/* Targeted / ROI attack (README "attack with ROI", attack_cv.py:153-163 mask box,
 * attack_data.py:202-226 target / masked losses; semantics fixed in DESIGN.md).  Box [y0,y1) x [x0,x1) is the
 * target region; w_* are the per-element weights of the masked means (1 / count, la_x / count).
 * prologue: im_in4 as ica_attack_prologue, part = box-weighted input distortion (loss_i after ica_reduce_rows).
 * loss: grad4 = d/dx_hat [w_out_tar * sum_tar (out_t - o)^2 + w_out_bkg * sum_bkg (out_s - o)^2], o = bound01(x_hat).
 * adam: ica_attack_adam with the box-weighted cheap-branch gradient. */
int ica_roi_prologue(const float* noise, const float* im_s, float* im_in4, float* part, int B, int H, int W, float eps,
                     int x0, int x1, int y0, int y1, float w_in_tar, float w_in_bkg, hipStream_t stream);
int ica_roi_loss(const float* xhat4, const float* out_s, const float* out_t, float* grad4, float* part, int B, int H,
                 int W, int x0, int x1, int y0, int y1, float w_out_tar, float w_out_bkg, int clamp, hipStream_t stream);
int ica_roi_adam(float* noise, const float* im_s, const float* gnet4, const float* loss_i, float* m, float* v,
                 float* im_in_out, int B, int H, int W, float eps, float thr, float bc2s, float neg_step, int* branch,
                 int x0, int x1, int y0, int y1, float w_in_tar, float w_in_bkg, const int* gpos, int* census,
                 hipStream_t stream);
int ica_ifgsm_step(float* x, const float* im_s, const float* grad4, float* gacc, const float* l1, int B, int H, int W,
                   float alpha, float eps, int momentum, hipStream_t stream);
int ica_l1_partial(const float* g4, float* part, int B, int H, int W, hipStream_t stream);
int ica_gc_likelihood(const float* y, const float* scales, const float* means, const float* qnoise, float* y_hat,
                      float* lik, float* part, int B, int C, int H, int W, int training, hipStream_t stream);
int ica_eb_likelihood(const float* z, const float* prm, const float* med, const float* qnoise, float* z_hat,
                      float* lik, float* part, int B, int C, int H, int W, int training, hipStream_t stream);
/* params: host array of 15 device pointers (_matrix0..4, _bias0..4, _factor0..3, quantiles). */
int ica_pack_eb(const float* const* params, float* prm, float* med, int C, hipStream_t stream);
int ica_abs(const float* x, float* y, long n, hipStream_t stream);
/* y = rint(x) (round half to even == torch.round): eval-mode quantize(y, "dequantize"), means = None. */
int ica_round(const float* x, float* y, long n, hipStream_t stream);
int ica_clamp01(const float* x, float* y, long n, hipStream_t stream);
int ica_sqdiff_partial(const float* a, const float* b, float* part, int B, long len, int clamp_a, hipStream_t stream);
int ica_nc4_bound_to_nchw(const float* x4, float* out, int B, int H, int W, int clamp, hipStream_t stream);
int ica_bound_bwd_nc4(const float* x4, const float* g, float* g4, int B, int H, int W, int clamp, hipStream_t stream);

/* ---- C&W-style binary-search attack (ica_cw.hip) ---------------------------
 * Replaces, per image of a batch and with the search state on the device:
 *   attack_cw.py:115-140 (attack_cw: step loss and the gate on c), :142-199 (search_noise: the step loop with
 *   torch.optim.Adam and the bisection on c), :238-259 (attack_: the outer search on the level);
 *   attack_cw_fast.py:100-125, :127-183 (the width / residual rule that ends a level), :222-243.
 * Per-image state, field-major (field f of image b at [f * B + b]), allocated by the caller on the device:
 *   sd   double [6][B]   0 c_l, 1 c_r, 2 c, 3 level, 4 min, 5 max
 *   lold float  [B]      loss_i_old
 *   si   int    [5][B]   0 t (Adam steps of the current level), 1 round (rounds done in the level),
 *                        2 levels (levels completed), 3 active, 4 reset
 * Start of a run: c_l = 0, c_r = c = la, level = max = the start level, min = noise, lold = 0, si = 0 but active = 1.
 * A step is ica_attack_prologue_ex + ica_reduce_rows (loss_i), g_a / g_s / ica_attack_loss (mode 0, part) and the
 * network backward, then ica_cw_gate and ica_cw_adam; after every `steps` steps ica_cw_round and ica_cw_reset. */
/* mse_o[b] = invN * sum part[b][0..nblk) (ica_reduce_rows' order); c_eff[b] = mse_o[b] > 1.1 * level[b] ? 0 : c[b];
 * t[b] += 1.  Images with active[b] == 0: c_eff[b] = 0, mse_o[b] and t[b] unchanged. */
int ica_cw_gate(const float* part, int nblk, float invN, const double* sd, int* si, float* mse_o, float* c_eff, int B,
                hipStream_t stream);
/* g = -2 fl(invN (im_s - im_in)) + c_eff[b] * gnet4 (the network's gradient of loss_o at unit weight), the [0, 1]
 * (clamp_in) and +-eps pass-through gates, torch-Adam on noise / m / v with (bc2s, neg_step) = tab[t[b] - 1]
 * (tab: ntab float pairs on the device).  Images with active[b] == 0 are left untouched.  im_in_out (optional):
 * im_in of the active images.  Returns -2 unless H * W is a multiple of 4. */
int ica_cw_adam(float* noise, const float* im_s, const float* gnet4, const float* c_eff, float* m, float* v,
                float* im_in_out, int B, int H, int W, float eps, float invN, const float* tab, int ntab, const int* si,
                int clamp_in, hipStream_t stream);
/* End of a round for the active images: bisection on c (mse_o < 0.99 level: c_l = c, else c_r = c), end of the
 * level (fast 0: after ssteps rounds; fast 1: attack_cw_fast's rule; either: after max_rounds rounds), the stop
 * test and the bisection on the level with loss_i, active = 0 when the image is done.  reset[b] is rewritten for
 * every image: 1 when it starts a new level.  *n_active = images still active.  cfg: HOST array {la, noise}. */
int ica_cw_round(const float* loss_i, const float* mse_o, double* sd, float* lold, int* si, int* n_active, int B,
                 int fast, int ssteps, int max_rounds, const double* cfg, hipStream_t stream);
/* noise = m = v = 0 for the images with reset[b] (floats_per_image a multiple of 4).  The flag is not cleared
 * here (every block of the image reads it); the next ica_cw_round rewrites it. */
int ica_cw_reset(float* noise, float* m, float* v, const int* si, int B, long floats_per_image, hipStream_t stream);

/* ---- latent range profile, clamp defence and detector (ica_latent.hip) ------
 * The per-channel range of the latent y = g_a(x), the paper's "safe zone".  y4 / out4 / g4 are fp32 nChw4c
 * [B][C/4][H][W][4]; cmax / cmin are the profile's channel_max / channel_min, float [C].  Every entry returns -2
 * unless C is a multiple of 4, allocates nothing and runs on `stream`. */
/* feature_range.py:19-21: out_max / out_min / out_absmax [B][C] = amax / amin / amax(abs) of each (image, channel)
 * plane, the bits of torch.amax / torch.amin (a NaN in a plane gives NaN); out_absmax may be NULL.  One caveat: where
 * the extreme of a plane is zero and the plane holds zeros of both signs, the sign of the returned zero is the
 * hardware max / min's choice, which torch's CPU reduction (whose choice depends on its vector order) need not
 * share; the value is equal either way. */
int ica_latent_range(const float* y4, int B, int C, int H, int W, float* out_max, float* out_min, float* out_absmax,
                     hipStream_t stream);
/* clamp_value_naive (attack_rd.py:53-73, search.py:25-36): t = y > cmax ? cmax : y; out = t < cmin ? cmin : t
 * (torch.where twice: a NaN passes through).  out4 may be y4.  nclamped (int [B], may be NULL) is zeroed and then
 * counts the elements of each image with out != y. */
int ica_latent_clamp(const float* y4, const float* cmax, const float* cmin, float* out4, int B, int C, int H, int W,
                     int* nclamped, hipStream_t stream);
/* The autograd of those two selects with respect to y, in place on g4: g where !(y > cmax) && !(t < cmin), else 0. */
int ica_latent_clamp_bwd(float* g4, const float* y4, const float* cmax, const float* cmin, int B, int C, int H, int W,
                         hipStream_t stream);
/* detect (search.py:137-146) per image, from the image's channel extremes imax / imin [B][C]:
 * score[b] = max_c(clamp(imax - cmax, min=0) / (cmax + 1)) + max_c|clamp(imin - cmin, max=0) / (cmin + 1)|, each
 * step one correctly rounded fp32 operation, NaN propagating as in torch.max. */
int ica_latent_detect(const float* imax, const float* imin, const float* cmax, const float* cmin, float* score, int B,
                      int C, hipStream_t stream);

/* ---- latent distribution (ica_distrib.hip) ----------------------------------
 * visual_distribution.py's numbers for one batch, from the tensors of the eval forward: y4, scales4, means4 (NULL:
 * mu = 0, the hyperprior model) and lik4 (NULL: no bits) are fp32 nChw4c [B][C/4][H][W][4], 16-byte aligned.  Bin k
 * of nbins (1 .. 64) unit bins covers [vmin + k, vmin + k + 1), the last one closed on the right; vmax = vmin + nbins
 * in fp32.
 *   hist [B][C][nbins] int32 = torch.histc(y[b, c], nbins, vmin, vmax) of a float CPU tensor, exact counts:
 *     pos = (int)(((v - vmin) * nbins) / (vmax - vmin)) in fp32, pos == nbins -> nbins - 1; values outside
 *     [vmin, vmax], NaN and +-inf are skipped.  hist is zeroed first.
 *   pred [B][C][nbins] = mean over (H, W) of max(cdf(vmin + k + 1) - cdf(vmin + k), pred_floor) with
 *     cdf(v) = 0.5 * (1 + erff(((v - mu) * (1 / sigma)) / sqrt(2))), sigma = max(scale, scale_floor): the operation
 *     order of torch.distributions.Normal.cdf (visual_distribution.py:85-101), in fp32.  The edge vmin + j is one
 *     rounded fp32 sum: equal to the reference's (vmin + 0.5 + k) -/+ 0.5 when those sums are exact (integer or
 *     half-integer vmin), within one ulp of the edge otherwise.
 *   bits [B][C] (written only with lik4) = sum over (H, W) of -log2f(lik).
 * work: scratch of ica_latent_distrib_ws_size floats (0 for an unsupported problem).  pred and bits are fixed-order
 * sums over min(ceil(H * W / 256), 64) partials per row, a function of the plane alone: a row's numbers are the same
 * bits alone and in a batch, run to run.  Status: 0; -2 unless C is a positive multiple of 4; -5 for nbins outside
 * 1 .. 64, a non-finite vmin, B < 1, B * ceil(nbins / 16) > 65535, C > 4 * 65535, H * W > 2^29 - 1, B * C * H * W >= 2^47,
 * more than 2^31 - 1 partials, a missing pointer or one that is not 16-byte aligned; -7 for an output that overlaps
 * an input or another output.  Nothing is launched then. */
size_t ica_latent_distrib_ws_size(int B, int C, int H, int W, int nbins);
int ica_latent_distrib(const float* y4, const float* scales4, const float* means4, const float* lik4, int B, int C,
                       int H, int W, float vmin, int nbins, float scale_floor, float pred_floor, int* hist,
                       float* pred, float* bits, float* work, hipStream_t stream);

/* ---- layer-wise error propagation (ica_layers.hip) ----------------------------
 * The sums behind layer_compare (anchors/utils.py:132-166) for every layer of a side in one launch.  A descriptor
 * names up to three fp32 nChw4c tensors [B][ceil(C/4)][H][W][4] (16-byte aligned, each a contiguous run of B images:
 * the halves or thirds of one batched forward) and a mode; per (layer, image) two sums come back, sums[layer][B][2]:
 *   ICA_LAYER_PAIR    sum (a - b)^2,        0                         (c ignored)
 *   ICA_LAYER_QUANT   sum (a - rne(b))^2,   sum (rne(a) - rne(b))^2   (c ignored; rne = round half to even, the
 *                                                                      bits of torch.round; nothing rounded is stored)
 *   ICA_LAYER_TRIPLE  sum (a - c)^2,        sum (b - c)^2             (c read once)
 * The tensors of a descriptor must share one storage layout (row-major or the parity-split order of
 * ica_conv_args.layout): the sums run over whole planes, so which of the two does not change what is summed.
 * Padding lanes (c >= C) add nothing whatever they hold.  layers is a HOST array of n <= ICA_LAYERS_MAX descriptors,
 * copied into the kernel arguments (no device table).  work: scratch of ica_layer_sums_ws_size(n, B) floats.
 * Fixed-order sums (ica_reduce.h, then ica_reduce_rows), no float atomics, and the ica_layer_sums_blocks(C, H, W)
 * partials of an image are a function of the layer's size alone: an image's numbers are the same bits alone and in
 * a batch, with any other layers in the table, run to run.  Status: 0; -5 for n outside 1 .. 16, B outside
 * 1 .. 65535, an unknown mode, C / H / W <= 0, more than 2^31 - 1 channel quads an image or 2^47 elements a tensor, a missing or
 * misaligned pointer; -7 for an output that overlaps an input or the other output.  Nothing is launched then. */
enum { ICA_LAYER_PAIR = 0, ICA_LAYER_QUANT = 1, ICA_LAYER_TRIPLE = 2 };
enum { ICA_LAYERS_MAX = 16 };
typedef struct ica_layer_desc {
  const float* a;
  const float* b;
  const float* c;
  int C, H, W, mode;
} ica_layer_desc;
int ica_layer_sums_blocks(int C, int H, int W);
size_t ica_layer_sums_ws_size(int n, int B);
int ica_layer_sums(const ica_layer_desc* layers, int n, int B, float* sums, float* work, hipStream_t stream);

/* ---- bitrate attack: entropy-model value gradients (ica_rate.hip) -----------
 * The expensive branch of attack_rd -r minimises  L = scale * sum ln lik  (scale = 1 / (ln 2 * H_img * W_img) > 0,
 * so L = -bpp of the relaxed codec): the train-mode likelihoods of the UNROUNDED latents with zero noise
 * (CompressAI GaussianConditional / EntropyBottleneck, likelihood LowerBound 1e-9, scale LowerBound 0.11, the
 * detached EntropyBottleneck sign).  Both launches read fp32 nChw4c tensors [B][ceil(C/4)][H][W][4] (16-byte
 * aligned), write the gradient with respect to the values only (padding lanes c >= C: 0) and per-block partial sums
 * of ln lik; ica_reduce_rows(part, sumln, B, blocks, 1) gives sum ln lik per image.  Fixed-order sums, no float
 * atomics: an image's numbers are the same bits alone and in a batch.  Status: 0; -5 for a non-positive or oversized
 * shape (B or ceil(C/4) > 65535, H * W > 2^28 - 1, >= 2^47 elements), scale not in (0, inf), a missing or misaligned
 * pointer; -7 for an output that overlaps an input or the other output.  Nothing is launched then.
 *
 * ica_rate_gc: lik = max(Phi((.5 - |y|) / s) - Phi((-.5 - |y|) / s), 1e-9), s = max(sigma, 0.11).  gy = dL/dy,
 * gsig = dL/dsigma with the scale bound's pass-through rule and the backward of the ReLU that produced sigma folded
 * in (sigma <= 0: 0).  part: B * ica_rate_gc_blocks() floats.
 * ica_rate_eb: lik = max(|sigmoid(sg F(v + .5)) - sigmoid(sg F(v - .5))|, 1e-9) with prm[C][58] of ica_pack_eb.
 * gv = dL/dv.  part: B * ica_rate_eb_blocks(C, H, W) floats. */
int ica_rate_gc_blocks(void);
int ica_rate_eb_blocks(int C, int H, int W);
int ica_rate_gc(const float* y4, const float* sigma4, float* gy4, float* gsig4, float* part, int B, int C, int H,
                int W, float scale, hipStream_t stream);
int ica_rate_eb(const float* v4, const float* prm, float* gv4, float* part, int B, int C, int H, int W, float scale,
                hipStream_t stream);

/* ---- RD evaluation: the loss side of batch_test (ica_rdeval.hip) -------------
 * RateDistortionLoss(training=False) (train.py:50-70) on what the eval forward left on the device, per image, in one
 * launch: xhat4 fp32 nChw4c [B][1][H][W][4], target NCHW [B][3][H][W], liky4 [B][ceil(Cy/4)][Hy][Wy][4] and the
 * optional likz4 likewise (NULL with Cz = Hz = Wz = 0 for the factorized model).  out [B][3][H][W] receives
 * clamp(x_hat, 0, 1); part (3 * B * ica_rd_metrics_blocks() floats) the per-block partials [B][3][blocks] of
 * sse = sum (clamp(x_hat) - target)^2, lny = sum ln max(lik_y, 2^-16) and lnz (0 without z):
 * ica_reduce_rows(part, sums, 3 * B, blocks, 1) gives sums[B][3].  nclamp [B] (int32, zeroed by the call) counts the
 * likelihood elements below 2^-16.  Padding lanes (c >= C) add nothing.  Fixed-order sums, no float atomics: an
 * image's numbers are the same bits alone and in a batch; the census uses integer atomics.  Status: 0; -5 for a
 * non-positive or oversized shape (B or ceil(C/4) > 65535, H * W > 2^28 - 1, >= 2^47 elements), a z shape without a
 * z plane, a missing required pointer or a misaligned nChw4c pointer; -7 for an output that overlaps an input.
 * Nothing is launched then. */
int ica_rd_metrics_blocks(void);
int ica_rd_metrics(const float* xhat4, const float* target, const float* liky4, const float* likz4, float* out,
                   float* part, int* nclamp, int B, int H, int W, int Cy, int Hy, int Wy, int Cz, int Hz, int Wz,
                   hipStream_t stream);
/* ica_val_metrics: the trainer's validation (validate.py; the reference's test_epoch scores an eval forward with
 * RateDistortionLoss(training=True), train.py:217-229).  The same tensors, partials and status codes as
 * ica_rd_metrics, with three differences: sse = sum (x_hat - target)^2 of the UNCLAMPED reconstruction; out receives
 * the unclamped x_hat as NCHW and may be NULL, which skips the store (only the ms-ssim metric reads it); there is no
 * census.  part: 3 * B * ica_rd_metrics_blocks() floats, reduced by ica_reduce_rows as above. */
int ica_val_metrics(const float* xhat4, const float* target, const float* liky4, const float* likz4, float* out,
                    float* part, int B, int H, int W, int Cy, int Hy, int Wy, int Cz, int Hz, int Wz,
                    hipStream_t stream);

/* ---- patch-wise VI localisation (ica_patch.hip) ----------------------------
 * psnr_partial (attack_patch.py:119-146) on four planar NCHW fp32 tensors [B][3][H][W], per image.  With
 * nh = (H - win) / stride + 1 and nw likewise: mse_in / mse_out [B][nh][nw] are the means over the 3 * win^2 window
 * elements of (im_s - im_adv)^2 and (out_s - out_adv)^2; vi = mse_out / mse_in, 0 on the `border` rows and columns
 * at each edge and where mse_in == 0; val[B] / pos[B][2] (row, col of the map; pixel origin = pos * stride) are
 * the largest vi and its first row-major position.  Accepted: stride in {1, 2, 4}, win % stride == 0, win <= 128,
 * H, W >= win, W % 4 == 0, border >= 0, W / stride <= 8192; anything else returns -5 and launches nothing.
 * ws: ica_patch_vi_ws_size floats; key_ws: 8 * B bytes (both scratch). */
size_t ica_patch_vi_ws_size(int B, int H, int W, int win, int stride);
int ica_patch_vi(const float* im_adv, const float* out_adv, const float* im_s, const float* out_s, int B, int H, int W,
                 int win, int stride, int border, float* ws, void* key_ws, float* mse_in, float* mse_out, float* vi,
                 float* val, int* pos, hipStream_t stream);
/* patches[B][4][3][win][win] = (im_adv, out_adv, im_s, out_s) cut at pos * stride, pos [B][2] read on the device. */
int ica_patch_gather(const float* im_adv, const float* out_adv, const float* im_s, const float* out_s, const int* pos,
                     float* patches, int B, int H, int W, int win, int stride, hipStream_t stream);

/* ---- image-space degradations (ica_degrade.hip) -----------------------------
 * random_noise.py's blur, sigma scan and additive noise on planar NCHW fp32 tensors [B][3][H][W] (16-byte aligned).
 * Status: 0, -5 for an unsupported problem or a missing / misaligned pointer, -7 for an output that overlaps the
 * input of the blur; nothing is launched then.  Every workspace is scratch, in floats, sized by its *_ws_size query
 * (0 for an unsupported problem).  All reductions are fixed-order: an image's numbers do not depend on the batch.
 *
 * ica_gauss_blur: torchvision gaussian_blur.  Reflect padding without edge repeat (kx / 2 columns, ky / 2 rows),
 * then out = sum_{i, j} (wy[b][i] * wx[b][j]) * x_padded[y + i][x + j] per channel, the weight one rounded fp32
 * product, the sum one fmaf chain in row-major tap order.  wx [B][kx], wy [B][ky] on the device; kx, ky odd in
 * 1 .. 9, W % 4 == 0, H > ky / 2, W > kx / 2.  clamp != 0 clamps out to [0, 1].  ref (optional, with mse and ws):
 * mse[b] = mean((out - ref)^2). */
size_t ica_gauss_blur_ws_size(int B, int H, int W);
int ica_gauss_blur(const float* x, const float* wx, const float* wy, int B, int H, int W, int kx, int ky, int clamp,
                   const float* ref, float* out, float* mse, float* ws, hipStream_t stream);
/* ica_blur_sweep: S <= ica_blur_sweep_chunk() candidate kernels wx [S][kx], wy [S][ky] shared by all images; for
 * every image with done[b] == 0: mse[b * ld + s0 + s] = mean((clamp(blur_s(x), 0, 1) - x)^2) (the arithmetic of
 * ica_gauss_blur; no image is written), then idx[b] = s0 + (first s with mse <= budget) and done[b] = 1 if there is
 * one.  remaining[0] = images still without an answer.  Images with done[b] != 0 cost nothing and keep their mse
 * row.  The caller zeroes done and sets idx to -1 before the first chunk. */
int ica_blur_sweep_chunk(void);
size_t ica_blur_sweep_ws_size(int B, int H, int W);
int ica_blur_sweep(const float* x, const float* wx, const float* wy, int S, int B, int H, int W, int kx, int ky,
                   float budget, int s0, float* mse, long ld, int* idx, int* done, int* remaining, float* ws,
                   hipStream_t stream);
/* ica_noise_apply (random_noise.py:80): out = clamp(im + noise, 0, 1) (out a third buffer), noise_power[b] =
 * mean(noise^2), mse_in[b] = mean((out - im)^2).  W % 4 == 0. */
size_t ica_noise_apply_ws_size(int B, int H, int W);
int ica_noise_apply(const float* im, const float* noise, float* out, int B, int H, int W, float* noise_power,
                    float* mse_in, float* ws, hipStream_t stream);

/* ---- JPEG round trip (ica_jpeg.hip) -----------------------------------------
 * The baseline-JPEG transform round trip of DESIGN.md "JPEG round trip" on planar NCHW fp32 tensors [B][3][H][W]
 * (16-byte aligned): 8-bit levels, JFIF YCbCr, 4:2:0 box mean, per 8x8 block DCT / quantise / dequantise / inverse
 * DCT, triangle chroma upsampling, RGB levels / 255.  No bitstream.  sub is 420 or 444; H and W are multiples of 16
 * (420) or 8 (444).  A table pair is 128 floats: the luminance table [64] then the chrominance table [64], row-major
 * (row = vertical frequency), integer values >= 1 built on the host.  Status: 0, -5 for an unsupported problem or a
 * missing / misaligned pointer, -7 for an out that overlaps x or ref; nothing is launched then.  ws: scratch of the *_ws_size floats (0 for an unsupported
 * problem): the partial sums, then the decoded Y, Cb and Cr planes as bytes.  No float atomics, fixed-order
 * reductions: an image's numbers do not depend on the batch, run to run the same bits.
 *
 * ica_jpeg_roundtrip: tabs [B][128], one pair per image.  out is a buffer of its own.  ref (optional, with mse): mse[b] =
 * mean((out - ref)^2). */
size_t ica_jpeg_roundtrip_ws_size(int B, int H, int W, int sub);
int ica_jpeg_roundtrip(const float* x, const float* tabs, int B, int H, int W, int sub, const float* ref, float* out,
                       float* mse, float* ws, hipStream_t stream);
/* ica_jpeg_roundtrip_bwd: g_x = the vector-Jacobian product of the round trip at x with g_out, under a surrogate
 * (DESIGN.md "JPEG round trip", "The attack through it"): a sample rounding has derivative 1, a clamp passes the
 * gradient iff the rounded value lies in 0 .. 255 (step 1: iff 0 <= x <= 1), the coefficient quantiser q roundf(c / q)
 * has derivative 1 (ICA_JPEG_STE) or 3 r^2, r = c / q - roundf(c / q) (ICA_JPEG_CUBIC); everything else is transposed.
 * Stateless: it runs the forward's block pass into ws (ica_jpeg_roundtrip_bwd_ws_size floats: the fp32 gradient
 * planes gY [B][H][W] and gC [B][2][Hc][Wc], then the decoded byte planes) and takes the masks and r from the
 * forward's own values.  x, tabs, B, H, W, sub as for ica_jpeg_roundtrip; g_out and g_x [B][3][H][W], 16-byte
 * aligned.  -5: unsupported shape, null or misaligned pointer, unknown surrogate; -7: g_x overlaps x or g_out.  No
 * atomics: an image's gradient does not depend on the batch or the tiling, run to run the same bits. */
#define ICA_JPEG_STE 0
#define ICA_JPEG_CUBIC 1
size_t ica_jpeg_roundtrip_bwd_ws_size(int B, int H, int W, int sub);
int ica_jpeg_roundtrip_bwd(const float* x, const float* tabs, const float* g_out, int B, int H, int W, int sub,
                           int surrogate, float* g_x, float* ws, hipStream_t stream);
/* ica_jpeg_sweep: S <= ica_jpeg_sweep_chunk() candidate table pairs tabs [S][128] shared by all images.  The forward
 * DCT of a block is computed once per launch; for every image with done[b] == 0: mse[b * ld + s0 + s] =
 * mean((roundtrip_s(x) - x)^2) (no image is written), then idx[b] = s0 + (first s with mse <= budget) and done[b] = 1
 * if there is one.  remaining[0] = images still without an answer.  Images with done[b] != 0 cost nothing and keep
 * their mse row.  The caller zeroes done and sets idx to -1 before the first chunk. */
int ica_jpeg_sweep_chunk(void);
size_t ica_jpeg_sweep_ws_size(int B, int H, int W, int sub);
int ica_jpeg_sweep(const float* x, const float* tabs, int S, int B, int H, int W, int sub, float budget, int s0,
                   float* mse, long ld, int* idx, int* done, int* remaining, float* ws, hipStream_t stream);

/* ---- perturbation transfer (ica_transfer.hip) -------------------------------
 * The pair loop of transfer_noise.py for N noises x M target images of one size, pair (i, j) at index i * M + j.
 * Status as above: -5 for an unsupported problem (N, M < 1, M > 65535, N > 4 * 65535, N * M >= 2^21, H * W >= 2^29) or a
 * missing / misaligned pointer, -7 for an im_in that overlaps im or noise; nothing is launched then.  ws: scratch of
 * the *_ws_size floats (0 for an unsupported problem).  Reductions are fixed-order and a pair's blocks depend on
 * (H, W) only: a pair's numbers are the same bits alone (N = M = 1) and in any block of pairs.
 *
 * ica_transfer_apply (transfer_noise.py:88-89): im [M][3][H][W], noise [N][3][H][W] planar NCHW fp32, W % 4 == 0;
 * im_in[i * M + j] = clamp(im[j] + noise[i], 0, 1) ([N * M][3][H][W]), mse_in[i][j] = mean((im_in - im[j])^2).
 * ica_transfer_score (transfer_noise.py:96, :133): x_hat4 [N * M][H][W][4], x_s4 [M][H][W][4] nChw4c fp32 of 3
 * channels; mse_out[i][j] = mean over the 3 real channels of (c(x_hat4[i * M + j]) - c(x_s4[j]))^2 with c = clamp to
 * [0, 1] if `clamp`, else the identity.  The padding lane is loaded and never used. */
size_t ica_transfer_apply_ws_size(int N, int M, int H, int W);
int ica_transfer_apply(const float* im, const float* noise, float* im_in, int N, int M, int H, int W, float* mse_in,
                       float* ws, hipStream_t stream);
size_t ica_transfer_score_ws_size(int N, int M, int H, int W);
int ica_transfer_score(const float* x_hat4, const float* x_s4, int N, int M, int H, int W, int clamp, float* mse_out,
                       float* ws, hipStream_t stream);

/* ---- frequency bands of a perturbation (ica_band.hip; DESIGN.md "Band VI") ----
 * The orthonormal 8x8 block DCT-II of every channel plane, blocks aligned to the image origin, fp32, rows then columns
 * (the transform pair of the JPEG round trip).  Coefficient (u, v) belongs to band max(u, v) = 0..7; a band set is a
 * mask 0..255, bit k selecting band k; P_S = IDCT . [band in S] . DCT.  Images are planar NCHW fp32 [B][3][H][W].
 * Status as above: -5 for an unsupported problem (H or W not a positive multiple of 8, B < 1, B > 65535,
 * H * W >= 2^29, V < 1, V > ica_band_max_variants(), a mask outside 0..255) or a missing / misaligned pointer, -7 for
 * an output that overlaps an input or another output; nothing is launched then.  ws: scratch of the *_ws_size floats
 * (0 for an unsupported problem).  Reductions are fixed-order and an image's blocks depend on (H, W) only: a row's
 * numbers are the same bits alone and in a batch, run to run.
 *
 * ica_band_split: n = im_adv - im_s.  energy [B][8]: energy[b][k] = |P_{k} n[b]|^2 / (3 H W), summed over the
 * coefficients.  With out: for the V masks (a host array, read before the call returns) out[v * B + b] =
 * clamp(im_s[b] + P_{masks[v]} n[b], 0, 1) ([V * B][3][H][W], the layout of ica_transfer_apply) and, if asked for,
 * mse_in [V][B] = mean((out[v * B + b] - im_s[b])^2).  out == NULL (then mse_in == NULL, masks unused): the energies
 * only.  The variants go through the kernel ica_band_split_chunk() at a time, the forward DCT once per chunk.
 * ica_band_project: y = P_mask x; mask 0 writes zeros.
 * ica_band_prologue / ica_band_adam: the step kernels of the band-limited L2 attack, ica_attack_prologue_ex and
 * ica_attack_adam_ex at clamp_in = 1 with p = P_mask(clip(noise, +-eps)) in place of clip(noise, +-eps):
 *   prologue  im_in = clamp(im_s + p, 0, 1) -> im_in4 [B][H][W][4] nChw4c (lane 3 = 0);
 *             loss_i [B] = mean((im_s - im_in)^2)
 *   adam      g = loss_i[b] > thr ? -2 fl(invN (im_s - im_in)) : gnet4 (nChw4c; row gpos[b] if gpos, else b; lane 3 is
 *             never used); g = bound-backward at im_s + p against [0, 1]; g = P_mask g; g = bound-backward at the noise
 *             against +-eps; torch's Adam step on noise, m, v in place.  branch[b] = cheap, census[b] += cheap,
 *             im_in_out = im_in: each optional. */
int ica_band_split_chunk(void);
int ica_band_max_variants(void);
size_t ica_band_split_ws_size(int V, int B, int H, int W);
int ica_band_split(const float* im_s, const float* im_adv, const int* masks, int V, int B, int H, int W, float* out,
                   float* energy, float* mse_in, float* ws, hipStream_t stream);
int ica_band_project(const float* x, int mask, int B, int H, int W, float* y, hipStream_t stream);
size_t ica_band_prologue_ws_size(int B, int H, int W);
int ica_band_prologue(const float* noise, const float* im_s, float* im_in4, float* loss_i, int B, int H, int W,
                      float eps, int mask, float* ws, hipStream_t stream);
int ica_band_adam(float* noise, const float* im_s, const float* gnet4, const float* loss_i, float* m, float* v,
                  float* im_in_out, int B, int H, int W, float eps, float thr, float invN, float bc2s, float neg_step,
                  int* branch, const int* gpos, int* census, int mask, hipStream_t stream);

/* ---- iterated re-compression (ica_recompress.hip) ---------------------------
 * The step between two generations of recompression.py (coder.py:21-48), on the device and for a whole batch.
 * Images are B x 3 x H x W; codes are one uint32 per pixel, r | g << 8 | b << 16, [B][H][W] (the top byte is written
 * 0 and ignored on input).  Status: 0, or -5 and nothing launched for B < 1, B > 65535, H < 1, W % 4 != 0,
 * H * W > 2^29 - 1, a missing pointer or an nChw4c pointer that is not 16-byte aligned.  Workspaces are scratch, in
 * floats, sized by the *_ws_size query (0 for an unsupported problem).  Reductions are fixed-order and an image's
 * blocks depend on H * W only: an image's numbers are the same bits alone and in a batch.
 *
 * ica_requant8: x_hat4 [B][1][H][W][4] nChw4c fp32 (unclamped, lane 3 never used), orig [B][3][H][W] planar.
 * With c = clamp(x_hat, 0, 1) and k = (uint)rint(c * 255) (fp32 product, half-to-even) per channel:
 *   q = the packed k;  next4 lanes 0..2 = (float)k / 255.0f (correctly rounded), lane 3 = 0;
 *   out (planar [B][3][H][W], NULL to skip) = c;
 *   sse_orig[b] = sum (c - orig)^2;  sse_gen[b] = sum ((k - k_prev) / 255)^2;
 *   changed[b] = the number of the 3 H W code values that differ from prev_q (exact);
 *   moving[0] (NULL to skip) = the number of images with changed != 0.
 * A NaN in x_hat clamps to 0: code 0, out 0.  next4 may be x_hat4 and q may be prev_q (a pixel is read before it is
 * written, by the same thread).
 * ica_quant8_pack: planar im -> q and next4 by the same clamp, rounding and division (generation 0).
 * ica_floor_bits: bits[b] = sum over c < C, pixels of log(max(lik, floor)) of lik4 [B][ceil(C / 4)][H][W][4] (natural
 * log; floor > 0; a NaN counts as the floor); any W, C * H * W limited to 2^30 quads. */
size_t ica_requant8_ws_size(int B, int H, int W);
int ica_requant8(const float* x_hat4, const float* orig, const uint32_t* prev_q, int B, int H, int W, float* next4,
                 uint32_t* q, float* out, float* sse_orig, float* sse_gen, long long* changed, int* moving, float* ws,
                 hipStream_t stream);
int ica_quant8_pack(const float* im, int B, int H, int W, float* next4, uint32_t* q, hipStream_t stream);
size_t ica_floor_bits_ws_size(int B, int C, int H, int W);
int ica_floor_bits(const float* lik4, int B, int C, int H, int W, float floor, float* bits, float* ws,
                   hipStream_t stream);

/* ---- MS-SSIM (ica_msssim.hip) ---------------------------------------------- */
/* mode 0 = pytorch_msssim (valid, per-channel, relu), mode 1 = utils/torch_msssim (same-pad, global). */
int ica_msssim_blocks(int H, int W, int ws, int mode);
int ica_msssim_level(const float* X, const float* Y, int P, int H, int W, const float* win_host, int ws, int mode,
                     float C1, float C2, float* part, float* out, float* maps, const float* wgt, hipStream_t stream);
int ica_msssim_level_bwd(const float* X, const float* Y, const float* maps, int P, int H, int W, const float* win_host,
                         int ws, int mode, float* gX, float* gY, hipStream_t stream);
int ica_msssim_combine(const float* lvl, int P, int G, int mode, const float* dval, float* val, float* wgt,
                       const float* nout_host, hipStream_t stream);
int ica_avgpool2(const float* X, float* Y, int P, int H, int W, int ph, int pw, hipStream_t stream);
int ica_avgpool2_bwd(const float* gO, float* gX, int P, int H, int W, int ph, int pw, hipStream_t stream);
int ica_scale(float* x, long n, float s, hipStream_t stream);


/* ---- adversarial fine-tune backward (ica_train.hip) ------------------------
 * Replaces the autograd backward of `out_criterion["loss"].backward()` in train.py:358-359 (train.train --adv),
 * adv_train.py:184-186, for the bmshj2018 models; RateDistortionLoss train.py:37-96. */
/* floats of split-K workspace ica_wgrad needs; ica_wgrad_nsplit picks the split count for nchunks pixel rows. */
size_t ica_wgrad_ws_size(int A, int Bc, int KS, int nsplit);
int ica_wgrad_nsplit(int A, int Bc, long nchunks);
/* out[a][b][ky][kx] (+)= sum_{n,p} Sm[n][a][p] * Lg[n][b][S*p + k - P]   (nChw4c operands)
 *   conv   W[o][c]:  Sm = dL/dy (a = o, small grid = output), Lg = x (b = c, big grid = input)
 *   deconv W[c][o]:  Sm = x (a = c, small grid = input),      Lg = dL/dy (b = o, big grid = output)
 * KS,S in {(5,2),(3,1),(1,1),(3,2),(1,2),(5,1)}; deterministic (fixed-order split reduction). */
int ica_wgrad(const float* Sm, const float* Lg, float* ws, float* out, int N, int A, int Bc, int Hs, int Ws, int Hb,
              int Wb, int KS, int S, int P, int nsplit, int accumulate, hipStream_t stream);
/* out[c] (+)= sum over n, pixels of x (nChw4c): bias and GDN beta' gradients. */
int ica_channel_sum(const float* x, float* out, int N, int C, int H, int W, int accumulate, hipStream_t stream);
int ica_relu_bwd(float* g, const float* y, long n, hipStream_t stream);          /* g *= (y > 0) */
int ica_abs_bwd(float* g, const float* x, long n, hipStream_t stream);           /* g *= sign(x) */
int ica_gdn_xsq(const float* y, const float* s, float* out, long n, hipStream_t stream); /* (y/s)^2 */
/* out = g * lrelu'(a) (a: the layer's saved leaky-ReLU output, slope 0.01): the pre-activation gradient of the
 * cheng2020 / mbt2018 leaky-ReLU layers (train.py:358-359 through CompressAI's nn.LeakyReLU). */
int ica_lrelu_bwd(const float* g, const float* a, float* out, long n, hipStream_t stream);
/* t = dL/dn of a GDN (inverse 0: t = -0.5 g y s^2) or IGDN (inverse 1: t = 0.5 g y / s^2) layer from g = dL/dy and
 * its saved (y, s) (utils/ops.py GDN; the GDN parameter gradients of the k3 residual layers, whose backward launch
 * fuses the GDN backward without writing t). */
int ica_gdn_t(const float* g, const float* y, const float* s, float* t, long n, int inverse, hipStream_t stream);
/* NonNegativeParametrizer backward (utils/ops.py:58-81): gout (+)= g' * 2 max(p,bound), LowerBound gate. */
int ica_reparam_bwd(const float* p, const float* gprime, float* gout, long n, float bound, int accumulate,
                    hipStream_t stream);
/* d/dlik of sum log(clamp(lik, 2^-16)) * scale  (train.py:60-64). */
int ica_bpp_grad(const float* lik, float* g, long n, float scale, hipStream_t stream);
/* GaussianConditional backward (train mode, no means): gy = dL/dy_tilde, gs = dL/dscales. */
int ica_gc_bwd(const float* y_tilde, const float* sigma, const float* glik, float* gy, float* gs, int B, int C, int H,
               int W, hipStream_t stream);
/* EntropyBottleneck backward (train mode): gv = dL/dz_tilde; gprm[C][58] = grads of the effective params. */
int ica_eb_bwd(const float* v, const float* glik, const float* prm, float* gv, float* gprm, int N, int C, int H, int W,
               hipStream_t stream);
/* gprm -> raw parameter grads (softplus / tanh chains); raw, graw: host arrays of 14 device pointers
 * (_matrix0..4, _bias0..4, _factor0..3); graw is accumulated into. */
int ica_eb_param_scatter(const float* gprm, const float* const* raw, float* const* graw, int C, hipStream_t stream);
/* g4 += scale * (x_hat - x)   (x_hat nChw4c 3 channels, x NCHW). */
int ica_mse_grad(const float* x_hat4, const float* x, float* g4, int B, int H, int W, float scale,
                 hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ICA_HIP_H */
