// The entropy side of the bitrate attack (attack_rd -r): the train-mode likelihoods of the unrounded latents with
// ZERO noise, their per-image sum of ln lik and the gradient of  L = scale * sum ln lik  with respect to the VALUES
// only (no parameter gradient: the attack freezes the codec).  Tensors are fp32 nChw4c [B][C4][H][W][4].
//
//   rate_gc_kernel   GaussianConditional: the forward of gc_kernel (ica_elem.hip, training, noise 0) and the backward
//                    of bpp_grad_kernel + gc_bwd_kernel + relu_bwd_kernel (ica_train.hip) in one pass, with
//                    g = dL/dlik = scale / max(lraw, 1e-9) formed in registers
//   rate_eb_kernel   EntropyBottleneck at v -/+ 0.5: the forward of eb_kernel (training, noise 0) and dL/dv by carrying
//                    dF/du through the 1-3-3-3-3-1 chain next to F (the input is one scalar, so forward mode needs no
//                    saved activations), element-parallel, the 4 x 58 packed parameters of a channel quad in LDS
//
// Bound rules (utils/ops.py:28-41, LowerBound: g passes where x >= bound or g < 0): scale > 0 makes g > 0, so the
// likelihood bound passes nothing where lraw < 1e-9 (exactly 0 there); the 0.11 scale bound passes dL/dsigma below
// the bound only where it is negative.  h_s ends in a ReLU whose output is sigma: sigma <= 0 gives dL/dsigma = 0.
//
// Reductions: ica_reduce.h.  A thread adds its terms in loop order, block_sum_paired adds the block, the block writes
// one partial, and ica_reduce_rows adds an image's partials.  The partials of an image are a function of (C, H, W)
// alone and no float atomic is used, so an image's numbers are the same bits alone and in a batch, run to run.
#include <math.h>

#include "ica_reduce.h"

namespace {

constexpr int RATE_THREADS = 256;
constexpr int RATE_GC_BLOCKS = 256;     // per image (the rest is grid-strided)
constexpr int RATE_EB_MAX_BLOCKS = 64;  // per (image, channel quad) plane
constexpr float RATE_LIK_BOUND = 1e-9f;
constexpr float RATE_SCALE_BOUND = 0.11f;

// grid (blocks of the image, image); quads = C4 * H * W channel quads per image, HW = H * W
__global__ __launch_bounds__(RATE_THREADS) void rate_gc_kernel(const float* __restrict__ y4,
                                                               const float* __restrict__ sigma4,
                                                               float* __restrict__ gy4, float* __restrict__ gsig4,
                                                               float* __restrict__ part, int C, long quads, long HW,
                                                               float scale) {
  __shared__ float sh[4];
  const int b = blockIdx.y;
  const long base = (long)b * quads * 4;
  const float k2 = -0.70710678118654752f, inv_sqrt2pi = 0.3989422804014327f;
  float acc = 0.f;
  for (long q = (long)blockIdx.x * RATE_THREADS + threadIdx.x; q < quads; q += (long)gridDim.x * RATE_THREADS) {
    const int c0 = (int)(q / HW) * 4;
    const f32x4 yv = ld4(y4 + base + q * 4), sv = ld4(sigma4 + base + q * 4);
    f32x4 gy = {0.f, 0.f, 0.f, 0.f}, gs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c0 + e >= C) continue;   // padding lanes: 0 out, nothing added
      const float v = yv[e], sr = sv[e];
      const float s = fmaxf(sr, RATE_SCALE_BOUND);
      const float av = fabsf(v);
      const float zu = fdiv_rn(fsub_rn(0.5f, av), s), zl = fdiv_rn(fsub_rn(-0.5f, av), s);
      const float up = 0.5f * erfcf(k2 * zu), lo = 0.5f * erfcf(k2 * zl);
      const float lraw = fsub_rn(up, lo);
      const float l = fmaxf(lraw, RATE_LIK_BOUND);
      acc += logf(l);
      float g = fdiv_rn(scale, l);
      g = (lraw >= RATE_LIK_BOUND || g < 0.f) ? g : 0.f;   // likelihood LowerBound
      const float pu = inv_sqrt2pi * expf(-0.5f * zu * zu), pl = inv_sqrt2pi * expf(-0.5f * zl * zl);
      // d lraw / d av = (pl - pu) / s ; d lraw / d s = (pl * zl - pu * zu) / s
      const float dav = g * (pl - pu) / s;
      float dsv = g * (pl * zl - pu * zu) / s;
      gy[e] = v > 0.f ? dav : (v < 0.f ? -dav : 0.f);
      dsv = (sr >= RATE_SCALE_BOUND || dsv < 0.f) ? dsv : 0.f;   // scale LowerBound
      gs[e] = sr > 0.f ? dsv : 0.f;                              // h_s's final ReLU
    }
    st4(gy4 + base + q * 4, gy);
    st4(gsig4 + base + q * 4, gs);
  }
  const float r = block_sum_paired(acc, sh);
  if (threadIdx.x == 0) part[(long)b * gridDim.x + blockIdx.x] = r;
}

// F(u) of eb_logit (ica_elem.hip, the same rounded operations) and dF/du
ICA_DEV void eb_logit_d(const float* q, float u, float& F, float& dF) {
  float a[3], d[3], a1[3], d1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float t = fadd_rn(fmul_rn(q[k], u), q[3 + k]);
    const float th = tanhf(t);
    a[k] = fadd_rn(t, fmul_rn(q[6 + k], th));
    d[k] = q[k] * (1.0f + q[6 + k] * (1.0f - th * th));
  }
  const float* s = q + 9;
#pragma unroll
  for (int layer = 0; layer < 3; ++layer) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float t = fadd_rn(fadd_rn(fmul_rn(s[3 * k], a[0]), fmul_rn(s[3 * k + 1], a[1])), fmul_rn(s[3 * k + 2], a[2]));
      t = fadd_rn(t, s[9 + k]);
      const float dt = s[3 * k] * d[0] + s[3 * k + 1] * d[1] + s[3 * k + 2] * d[2];
      const float th = tanhf(t);
      a1[k] = fadd_rn(t, fmul_rn(s[12 + k], th));
      d1[k] = dt * (1.0f + s[12 + k] * (1.0f - th * th));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[k] = a1[k];
      d[k] = d1[k];
    }
    s += 15;
  }
  F = fadd_rn(fadd_rn(fadd_rn(fmul_rn(s[0], a[0]), fmul_rn(s[1], a[1])), fmul_rn(s[2], a[2])), s[3]);
  dF = s[0] * d[0] + s[1] * d[1] + s[2] * d[2];
}

ICA_DEV float rate_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// grid (blocks of the plane, channel quad, image)
__global__ __launch_bounds__(RATE_THREADS) void rate_eb_kernel(const float* __restrict__ v4,
                                                               const float* __restrict__ prm,
                                                               float* __restrict__ gv4, float* __restrict__ part,
                                                               int C, int C4, int HW, float scale) {
  __shared__ float sh[4];
  __shared__ float s_prm[4 * 58];
  const int nb = gridDim.x, blk = blockIdx.x, cq = blockIdx.y, b = blockIdx.z;
  for (int i = threadIdx.x; i < 4 * 58; i += RATE_THREADS) {
    const int c = cq * 4 + i / 58;
    s_prm[i] = c < C ? prm[(size_t)c * 58 + i % 58] : 0.f;
  }
  __syncthreads();
  const size_t plane = ((size_t)b * C4 + cq) * (size_t)HW * 4;
  const int n = HW * 4;   // one thread per element: lane e = i & 3 of pixel i >> 2 (consecutive lanes, consecutive floats)
  float acc = 0.f;
  for (int i = blk * RATE_THREADS + threadIdx.x; i < n; i += nb * RATE_THREADS) {
    const int e = i & 3;
    float gv = 0.f;
    if (cq * 4 + e < C) {   // padding lanes: 0 out, nothing added
      const float v = v4[plane + i];
      const float* q = s_prm + e * 58;
      float lower, dlower, upper, dupper;
      eb_logit_d(q, fsub_rn(v, 0.5f), lower, dlower);
      eb_logit_d(q, fadd_rn(v, 0.5f), upper, dupper);
      const float sm = fadd_rn(lower, upper);
      const float sg = sm > 0.f ? -1.f : (sm < 0.f ? 1.f : 0.f);   // detached
      const float su = rate_sigmoid(sg * upper), sl = rate_sigmoid(sg * lower);
      const float diff = fsub_rn(su, sl);
      const float lraw = fabsf(diff);
      const float l = fmaxf(lraw, RATE_LIK_BOUND);
      acc += logf(l);
      float g = fdiv_rn(scale, l);
      g = (lraw >= RATE_LIK_BOUND || g < 0.f) ? g : 0.f;   // likelihood LowerBound
      const float gd = diff > 0.f ? g : (diff < 0.f ? -g : 0.f);
      gv = gd * sg * (su * (1.f - su) * dupper - sl * (1.f - sl) * dlower);
    }
    gv4[plane + i] = gv;
  }
  const float r = block_sum_paired(acc, sh);
  if (threadIdx.x == 0) part[((size_t)b * C4 + cq) * nb + blk] = r;
}

int rate_eb_blocks(int H, int W) { return capped_blocks(4L * H * W, RATE_THREADS, RATE_EB_MAX_BLOCKS); }

// 0, or the status of a problem the kernels do not take
int rate_check(int B, int C, int H, int W, float scale) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return -5;
  if (B > 65535 || (C + 3) / 4 > 65535 || (long)H * W > 0x0fffffffL) return -5;   // 4 H W + a grid stride < 2^31
  if ((long)B * ((C + 3) / 4) > 0x7fffffffffffL / (4L * H * W)) return -5;   // elements < 2^47
  if (!(scale > 0.f) || isinf(scale)) return -5;   // the bound rules above are written for scale > 0
  return 0;
}

}  // namespace

extern "C" {

int ica_rate_gc_blocks(void) { return RATE_GC_BLOCKS; }

int ica_rate_eb_blocks(int C, int H, int W) {
  if (C <= 0 || H <= 0 || W <= 0) return 0;
  return ((C + 3) / 4) * rate_eb_blocks(H, W);
}

int ica_rate_gc(const float* y4, const float* sigma4, float* gy4, float* gsig4, float* part, int B, int C, int H,
                int W, float scale, hipStream_t st) {
  if (int rc = rate_check(B, C, H, W, scale)) return rc;
  if (!y4 || !sigma4 || !gy4 || !gsig4 || !part) return -5;
  if (!aligned16(y4) || !aligned16(sigma4) || !aligned16(gy4) || !aligned16(gsig4)) return -5;
  const long HW = (long)H * W, quads = (long)((C + 3) / 4) * HW;
  const size_t bytes = sizeof(float) * 4 * (size_t)quads * B;
  if (overlaps(gy4, bytes, gsig4, bytes) || overlaps(gy4, bytes, y4, bytes) || overlaps(gy4, bytes, sigma4, bytes) ||
      overlaps(gsig4, bytes, y4, bytes) || overlaps(gsig4, bytes, sigma4, bytes))
    return -7;
  ICA_LAUNCH(rate_gc_kernel, dim3(RATE_GC_BLOCKS, B), dim3(RATE_THREADS), 0, st, y4, sigma4, gy4, gsig4, part, C,
             quads, HW, scale);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_rate_eb(const float* v4, const float* prm, float* gv4, float* part, int B, int C, int H, int W, float scale,
                hipStream_t st) {
  if (int rc = rate_check(B, C, H, W, scale)) return rc;
  if (!v4 || !prm || !gv4 || !part) return -5;
  if (!aligned16(v4) || !aligned16(gv4)) return -5;
  const int C4 = (C + 3) / 4;
  const size_t bytes = sizeof(float) * 4 * (size_t)C4 * H * W * B;
  if (overlaps(gv4, bytes, v4, bytes)) return -7;
  ICA_LAUNCH(rate_eb_kernel, dim3(rate_eb_blocks(H, W), C4, B), dim3(RATE_THREADS), 0, st, v4, prm, gv4, part, C, C4,
             H * W, scale);
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
