// The pair loop of transfer_noise.py for a block of N noises x M target images, pair (i, j) at index i * M + j:
//
//   transfer_apply_kernel   transfer_noise.py:88-89: im_in = clamp(im[j] + noise[i], 0, 1) as planar NCHW fp32
//                           [N * M][3][H][W] (ready for the eval forward) and mean((im_in - im[j])^2)
//   transfer_score_kernel   transfer_noise.py:96, :133: mean over the 3 real channels of (clamp(x_hat4[i * M + j]) -
//                           clamp(x_s4[j]))^2, read from the nChw4c tensors the decoder leaves; no NCHW copy of the
//                           N * M reconstructions and no expanded reference tensor is written
//
// Both kernels stream: grid (blocks, M, ceil(N / TN)).  A thread loads a quad of target j once and reuses it for the
// TN noises (reconstructions) of its tile, so a pair costs one 16-byte load and, for apply, one 16-byte store per
// quad, plus 1 / TN of the target's.  Arithmetic as noise_apply_kernel (ica_degrade.hip): fadd_rn, clamp, fsub_rn,
// one fmaf chain per thread.  Reductions: ica_reduce.h (sequential block order, one row of partials per pair), so a
// pair's numbers do not depend on N, M or the tile remainder.
#include "ica_reduce.h"

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_TN = 4;                  // noises per thread tile (grid.z = ceil(N / TR_TN))
constexpr int TR_MAX_BLOCKS = 1024;       // blocks per pair, as ica_noise_apply

// quads: 3 H W / 4 floats-of-four per image.  part[(i * M + j) * gridDim.x + blockIdx.x]
__global__ __launch_bounds__(TR_THREADS) void transfer_apply_kernel(const float* __restrict__ im,
                                                                    const float* __restrict__ noise,
                                                                    float* __restrict__ out, long quads, int N,
                                                                    float* __restrict__ part) {
  __shared__ float red[4];
  const int j = blockIdx.y, M = gridDim.y, i0 = blockIdx.z * TR_TN;
  const int tn = min(TR_TN, N - i0);   // block-uniform
  const float* a_base = im + (size_t)j * quads * 4;
  float sd[TR_TN];
#pragma unroll
  for (int t = 0; t < TR_TN; ++t) sd[t] = 0.f;
  for (long q = (long)blockIdx.x * TR_THREADS + threadIdx.x; q < quads; q += (long)gridDim.x * TR_THREADS) {
    const f32x4 a = ld4(a_base + q * 4);
    f32x4 n[TR_TN];
#pragma unroll
    for (int t = 0; t < TR_TN; ++t)
      if (t < tn) n[t] = ld4(noise + ((size_t)(i0 + t) * quads + q) * 4);
#pragma unroll
    for (int t = 0; t < TR_TN; ++t) {
      if (t < tn) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = clamp01(fadd_rn(a[e], n[t][e]));
          const float d = fsub_rn(o[e], a[e]);
          sd[t] = fmaf(d, d, sd[t]);
        }
        st4(out + (((size_t)(i0 + t) * M + j) * quads + q) * 4, o);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < TR_TN; ++t) {
    if (t < tn) {
      const float s = block_sum(sd[t], red);
      if (threadIdx.x == 0) part[((size_t)(i0 + t) * M + j) * gridDim.x + blockIdx.x] = s;
    }
  }
}

// pixels: H W quads (the 4 channel lanes of a pixel, lane 3 padding) per image
template <bool CLAMP>
__global__ __launch_bounds__(TR_THREADS) void transfer_score_kernel(const float* __restrict__ x_hat4,
                                                                    const float* __restrict__ x_s4, long pixels,
                                                                    int N, float* __restrict__ part) {
  __shared__ float red[4];
  const int j = blockIdx.y, M = gridDim.y, i0 = blockIdx.z * TR_TN;
  const int tn = min(TR_TN, N - i0);   // block-uniform
  const float* s_base = x_s4 + (size_t)j * pixels * 4;
  float sd[TR_TN];
#pragma unroll
  for (int t = 0; t < TR_TN; ++t) sd[t] = 0.f;
  for (long p = (long)blockIdx.x * TR_THREADS + threadIdx.x; p < pixels; p += (long)gridDim.x * TR_THREADS) {
    f32x4 s = ld4(s_base + p * 4);
    if (CLAMP) {
#pragma unroll
      for (int e = 0; e < 3; ++e) s[e] = clamp01(s[e]);
    }
    f32x4 x[TR_TN];
#pragma unroll
    for (int t = 0; t < TR_TN; ++t)
      if (t < tn) x[t] = ld4(x_hat4 + (((size_t)(i0 + t) * M + j) * pixels + p) * 4);
#pragma unroll
    for (int t = 0; t < TR_TN; ++t) {
      if (t < tn) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {   // lane 3 is padding: it never enters a sum
          const float d = fsub_rn(CLAMP ? clamp01(x[t][e]) : x[t][e], s[e]);
          sd[t] = fmaf(d, d, sd[t]);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < TR_TN; ++t) {
    if (t < tn) {
      const float v = block_sum(sd[t], red);
      if (threadIdx.x == 0) part[((size_t)(i0 + t) * M + j) * gridDim.x + blockIdx.x] = v;
    }
  }
}

// 0 if the grid holds N x M pairs of H x W images (grid.y = M, grid.z = ceil(N / TN), finish grid.x = N M)
int pairs_check(int N, int M, int H, int W) {
  if (N < 1 || M < 1 || M > 65535 || (N + TR_TN - 1) / TR_TN > 65535) return -5;
  if ((long)N * M > 0x7fffffffL / TR_MAX_BLOCKS) return -5;
  if (H < 1 || W < 1 || (long)H * W > 0x7fffffffL / 4) return -5;
  return 0;
}

int stream_blocks(long units) { return capped_blocks(units, TR_THREADS, TR_MAX_BLOCKS); }

}  // namespace

extern "C" {

size_t ica_transfer_apply_ws_size(int N, int M, int H, int W) {
  if (pairs_check(N, M, H, W) || W % 4) return 0;
  return (size_t)N * M * stream_blocks((long)3 * H * W / 4);
}

int ica_transfer_apply(const float* im, const float* noise, float* im_in, int N, int M, int H, int W, float* mse_in,
                       float* ws, hipStream_t st) {
  if (pairs_check(N, M, H, W) || W % 4) return -5;
  if (!im || !noise || !im_in || !mse_in || !ws) return -5;
  if (!aligned16(im) || !aligned16(noise) || !aligned16(im_in)) return -5;
  const size_t img = (size_t)3 * H * W * sizeof(float);
  if (overlaps(im_in, (size_t)N * M * img, im, (size_t)M * img) ||
      overlaps(im_in, (size_t)N * M * img, noise, (size_t)N * img))
    return -7;   // a pair's output would be read as another pair's input
  const long quads = (long)3 * H * W / 4;
  const int nb = stream_blocks(quads);
  ICA_LAUNCH(transfer_apply_kernel, dim3(nb, M, (N + TR_TN - 1) / TR_TN), dim3(TR_THREADS), 0, st, im, noise, im_in,
             quads, N, ws);
  ICA_CHECK_LAUNCH();
  finish_rows(st, ws, N * M, nb, (float)((long)3 * H * W), mse_in);
  ICA_CHECK_LAUNCH();
  return 0;
}

size_t ica_transfer_score_ws_size(int N, int M, int H, int W) {
  if (pairs_check(N, M, H, W)) return 0;
  return (size_t)N * M * stream_blocks((long)H * W);
}

int ica_transfer_score(const float* x_hat4, const float* x_s4, int N, int M, int H, int W, int clamp, float* mse_out,
                       float* ws, hipStream_t st) {
  if (pairs_check(N, M, H, W)) return -5;
  if (!x_hat4 || !x_s4 || !mse_out || !ws) return -5;
  if (!aligned16(x_hat4) || !aligned16(x_s4)) return -5;
  const long pixels = (long)H * W;
  const int nb = stream_blocks(pixels);
  const dim3 grid(nb, M, (N + TR_TN - 1) / TR_TN);
  if (clamp)
    ICA_LAUNCH(transfer_score_kernel<true>, grid, dim3(TR_THREADS), 0, st, x_hat4, x_s4, pixels, N, ws);
  else
    ICA_LAUNCH(transfer_score_kernel<false>, grid, dim3(TR_THREADS), 0, st, x_hat4, x_s4, pixels, N, ws);
  ICA_CHECK_LAUNCH();
  finish_rows(st, ws, N * M, nb, (float)((long)3 * H * W), mse_out);
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
