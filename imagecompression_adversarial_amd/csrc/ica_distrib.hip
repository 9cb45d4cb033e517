// The latent-distribution study of visual_distribution.py on the tensors the eval forward leaves on the device
// (fp32 nChw4c, [B][C/4][H][W][4]): per (image, channel) the histogram of y over unit bins, the distribution the
// entropy model predicts for the channel (the spatial mean of the per-pixel Gaussian bin masses) and the rate the
// codec's own likelihoods give the channel.
//
//   latent_distrib_kernel   torch.histc per channel (:158-159), predicted_distribution (:85-101), sum -log2(lik)
//
// Bins: bin k covers [vmin + k, vmin + k + 1), the last one closed on the right; vmax = vmin + nbins (fp32).
//
// hist restates the CPU torch.histc of a float tensor, every step one rounded fp32 operation:
//   skip unless vmin <= v <= vmax (a NaN fails the test and +-inf lies outside: both are skipped);
//   pos = (int)(((v - vmin) * (float)nbins) / (vmax - vmin));  pos == nbins -> nbins - 1.
// Counts are integers (LDS atomics per block, then one global integer atomic per non-zero bin), so order-free.
//
// pred, per element, in torch.distributions.Normal.cdf's operation order:
//   sigma = scale < floor ? floor : scale;  r = 1 / sigma;  edge_j = vmin + j  (j = 0 .. nbins)
//   cdf_j = 0.5 * (1 + erff(((edge_j - mu) * r) / sqrt(2)));  mass_k = cdf_{k+1} - cdf_k, floored at pred_floor.
// Adjacent bins share cdf_j, so an element costs nbins + 1 erff.  edge_j is one rounded fp32 sum.  The reference forms
// the same abscissae as (vmin + 0.5 + k) -/+ 0.5; the two agree bit for bit whenever those sums are exact in fp32 (an
// integer or half-integer vmin, the default -5.5 among them) and otherwise differ by at most one ulp of the edge,
// far inside the tolerance of pred (tests/test_gpu_distribution.py, case vmin0.1).
//
// A thread keeps 4 x DIST_BINS running sums in registers, so a block covers DIST_BINS bins; nbins > DIST_BINS runs
// ceil(nbins / DIST_BINS) bin chunks as further blocks of the same launch (the default 11 bins are one chunk and one pass over the inputs; 64 bins read the
// inputs four times, the only price of the register budget).  Chunk 0 alone counts hist and sums bits.
//
// Reductions: ica_reduce.h.  A thread adds its pixels p, p + gridDim.x * 256, ... in that order, block_sum adds the
// block, the block writes one partial per (channel, bin) and finish_rows adds the partials of a row.  The blocks of
// a plane are capped_blocks(H * W, DIST_THREADS, DIST_MAX_BLOCKS): a function of the plane size only, so a row's
// pred and bits are the same bits alone and in a batch, run to run.  Both constants are part of that promise.
#include <math.h>

#include "ica_reduce.h"

namespace {

constexpr int DIST_THREADS = 256;
constexpr int DIST_MAX_BLOCKS = 64;   // per (image, channel quad) plane
constexpr int DIST_BINS = 16;         // bins per block: 64 accumulators per thread
constexpr int DIST_MAX_NBINS = 64;
constexpr float DIST_SQRT2 = 1.41421356237309504880f;

// grid (blocks of the plane, channel quad, image * nchunks + chunk)
__global__ __launch_bounds__(DIST_THREADS) void latent_distrib_kernel(
    const float* __restrict__ y4, const float* __restrict__ s4, const float* __restrict__ m4,
    const float* __restrict__ l4, int C4, int HW, float vmin, int nbins, int nchunks, float scale_floor,
    float pred_floor, int* __restrict__ hist, float* __restrict__ part_pred, float* __restrict__ part_bits) {
  __shared__ float red[4];
  __shared__ int s_hist[4 * DIST_MAX_NBINS];
  const int nb = gridDim.x, blk = blockIdx.x, cq = blockIdx.y;
  const int b = blockIdx.z / nchunks, chunk = blockIdx.z - b * nchunks;
  const int k0 = chunk * DIST_BINS;
  const int nk = min(nbins - k0, DIST_BINS);   // 1 .. DIST_BINS, block-uniform
  const bool first = chunk == 0;
  const size_t plane = ((size_t)b * C4 + cq) * (size_t)HW * 4;
  const float vmax = fadd_rn(vmin, (float)nbins), width = fsub_rn(vmax, vmin), fn = (float)nbins;

  if (first) {
    for (int i = threadIdx.x; i < 4 * nbins; i += DIST_THREADS) s_hist[i] = 0;
    __syncthreads();
  }
  float edge[DIST_BINS + 1];
#pragma unroll
  for (int j = 0; j <= DIST_BINS; ++j) edge[j] = fadd_rn(vmin, (float)(k0 + j));

  float acc[4][DIST_BINS];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int k = 0; k < DIST_BINS; ++k) acc[e][k] = 0.f;
  f32x4 bits = {0.f, 0.f, 0.f, 0.f};

  for (int p = blk * DIST_THREADS + threadIdx.x; p < HW; p += nb * DIST_THREADS) {
    const size_t at = plane + (size_t)p * 4;
    const f32x4 s = ld4(s4 + at);
    f32x4 m = {0.f, 0.f, 0.f, 0.f};
    if (m4) m = ld4(m4 + at);
    if (first) {
      const f32x4 v = ld4(y4 + at);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (v[e] >= vmin && v[e] <= vmax) {
          int pos = (int)fdiv_rn(fmul_rn(fsub_rn(v[e], vmin), fn), width);
          pos = pos < 0 ? 0 : (pos > nbins - 1 ? nbins - 1 : pos);
          atomicAdd(&s_hist[e * nbins + pos], 1);
        }
      }
      if (l4) {
        const f32x4 l = ld4(l4 + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) bits[e] = fsub_rn(bits[e], log2f(l[e]));
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float sigma = s[e] < scale_floor ? scale_floor : s[e];   // torch.clamp(min=): a NaN stays
      const float r = fdiv_rn(1.f, sigma);
      float lo = fmul_rn(0.5f, fadd_rn(1.f, erff(fdiv_rn(fmul_rn(fsub_rn(edge[0], m[e]), r), DIST_SQRT2))));
#pragma unroll
      for (int k = 0; k < DIST_BINS; ++k) {
        if (k < nk) {
          const float hi =
              fmul_rn(0.5f, fadd_rn(1.f, erff(fdiv_rn(fmul_rn(fsub_rn(edge[k + 1], m[e]), r), DIST_SQRT2))));
          const float d = fsub_rn(hi, lo);
          acc[e][k] = fadd_rn(acc[e][k], d < pred_floor ? pred_floor : d);
          lo = hi;
        }
      }
    }
  }

  // partials: part_pred[((b * C + c) * nbins + k) * nb + blk], part_bits[(b * C + c) * nb + blk]
  const size_t ch0 = ((size_t)b * C4 + cq) * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int k = 0; k < DIST_BINS; ++k) {
      if (k < nk) {
        const float t = block_sum(acc[e][k], red);
        if (threadIdx.x == 0) part_pred[((ch0 + e) * nbins + k0 + k) * nb + blk] = t;
      }
    }
  }
  if (first) {
    if (l4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = block_sum(bits[e], red);
        if (threadIdx.x == 0) part_bits[(ch0 + e) * nb + blk] = t;
      }
    }
    __syncthreads();   // the LDS counts of every wave (block_sum's barriers do not run without l4)
    for (int i = threadIdx.x; i < 4 * nbins; i += DIST_THREADS) {
      const int n = s_hist[i];
      if (n) atomicAdd(hist + ch0 * nbins + i, n);   // i = e * nbins + k
    }
  }
}

int dist_blocks(int H, int W) { return capped_blocks((long)H * W, DIST_THREADS, DIST_MAX_BLOCKS); }
int dist_chunks(int nbins) { return (nbins + DIST_BINS - 1) / DIST_BINS; }

// 0, or the status of a problem the kernel does not take
int dist_check(int B, int C, int H, int W, int nbins) {
  if (C <= 0 || C % 4 != 0) return -2;
  if (nbins < 1 || nbins > DIST_MAX_NBINS) return -5;
  if (B <= 0 || H <= 0 || W <= 0 || C / 4 > 65535 || (long)H * W > 0x7fffffffL / 4) return -5;
  if ((long)B * dist_chunks(nbins) > 65535) return -5;
  if ((long)B * C > 0x7fffffffL / ((nbins + 1) * DIST_MAX_BLOCKS)) return -5;   // rows and partials fit an int
  if ((long)B * C > 0x7fffffffffffL / ((long)H * W)) return -5;                   // B C H W elements < 2^47
  return 0;
}

}  // namespace

extern "C" {

size_t ica_latent_distrib_ws_size(int B, int C, int H, int W, int nbins) {
  if (dist_check(B, C, H, W, nbins)) return 0;
  return (size_t)B * C * (nbins + 1) * dist_blocks(H, W);
}

int ica_latent_distrib(const float* y4, const float* scales4, const float* means4, const float* lik4, int B, int C,
                       int H, int W, float vmin, int nbins, float scale_floor, float pred_floor, int* hist,
                       float* pred, float* bits, float* work, hipStream_t st) {
  if (int rc = dist_check(B, C, H, W, nbins)) return rc;
  if (!y4 || !scales4 || !hist || !pred || !work || (lik4 && !bits)) return -5;
  if (!(vmin == vmin) || isinf(vmin)) return -5;
  if (!aligned16(y4) || !aligned16(scales4) || !aligned16(means4) || !aligned16(lik4)) return -5;
  const int nb = dist_blocks(H, W), nchunks = dist_chunks(nbins);
  const size_t in_bytes = sizeof(float) * (size_t)B * C * H * W, rows = (size_t)B * C;
  const size_t work_bytes = sizeof(float) * rows * (nbins + 1) * nb;
  const void* ins[4] = {y4, scales4, means4, lik4};
  const void* outs[4] = {hist, pred, bits, work};
  const size_t out_bytes[4] = {sizeof(int) * rows * nbins, sizeof(float) * rows * nbins, sizeof(float) * rows,
                               work_bytes};
  for (int o = 0; o < 4; ++o) {
    if (!outs[o]) continue;
    for (int i = 0; i < 4; ++i)
      if (ins[i] && overlaps(outs[o], out_bytes[o], ins[i], in_bytes)) return -7;
    for (int q = o + 1; q < 4; ++q)
      if (outs[q] && overlaps(outs[o], out_bytes[o], outs[q], out_bytes[q])) return -7;
  }
  hipError_t e = hipMemsetAsync(hist, 0, out_bytes[0], st);
  if (e != hipSuccess) return (int)e;
  float* part_pred = work;
  float* part_bits = work + rows * nbins * nb;
  ICA_LAUNCH(latent_distrib_kernel, dim3(nb, C / 4, B * nchunks), dim3(DIST_THREADS), 0, st, y4, scales4, means4, lik4,
             C / 4, H * W, vmin, nbins, nchunks, scale_floor, pred_floor, hist, part_pred, part_bits);
  ICA_CHECK_LAUNCH();
  finish_rows(st, part_pred, (int)(rows * nbins), nb, (float)((long)H * W), pred);   // the mean over (H, W)
  ICA_CHECK_LAUNCH();
  if (lik4) {
    finish_rows(st, part_bits, (int)rows, nb, 1.f, bits);   // the sum is not divided
    ICA_CHECK_LAUNCH();
  }
  return 0;
}

}  // extern "C"
