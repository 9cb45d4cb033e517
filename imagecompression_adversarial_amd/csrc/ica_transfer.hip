// The pair loop of transfer_noise.py for a block of N noises x M target images, pair (i, j) at index i * M + j:
//
//   transfer_apply_kernel   transfer_noise.py:88-89: im_in = clamp(im[j] + noise[i], 0, 1) as planar NCHW fp32
//                           [N * M][3][H][W] (ready for the eval forward) and mean((im_in - im[j])^2)
//   transfer_score_kernel   transfer_noise.py:96, :133: mean over the 3 real channels of (clamp(x_hat4[i * M + j]) -
//                           clamp(x_s4[j]))^2, read from the nChw4c tensors the decoder leaves; no NCHW copy of the
//                           N * M reconstructions and no expanded reference tensor is written
//   pair_finish_kernel      one wave per pair sums the pair's block partials in index order
//
// Both kernels stream: grid (blocks, M, ceil(N / TN)).  A thread loads a quad of target j once and reuses it for the
// TN noises (reconstructions) of its tile, so a pair costs one 16-byte load and, for apply, one 16-byte store per
// quad, plus 1 / TN of the target's.  Arithmetic as noise_apply_kernel (ica_degrade.hip): fadd_rn, clamp, fsub_rn,
// one fmaf chain per thread; the block's 256 threads in a fixed tree; no float atomic.  The blocks of a pair depend
// on (H, W) only, so a pair's numbers are the same bits whatever N, M and the tile remainder are, run to run.
#include "ica_common.h"

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_TN = 4;                  // noises per thread tile (grid.z = ceil(N / TR_TN))
constexpr int TR_MAX_BLOCKS = 1024;       // blocks per pair, as ica_noise_apply

ICA_DEV float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // keeps a NaN, as torch.clamp

// sum over the block in a fixed order (wave butterfly, then the four waves in index order); red: 4 floats of LDS
ICA_DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = fadd_rn(fadd_rn(fadd_rn(red[0], red[1]), red[2]), red[3]);
  __syncthreads();
  return s;
}

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

// out[pair] = (sum of the pair's n partials) / count: lane l adds the partials l, l + 64, ... in that order, then the
// butterfly (what degrade_finish_kernel does for an image)
__global__ __launch_bounds__(64) void pair_finish_kernel(const float* __restrict__ part, int n, float count,
                                                         float* __restrict__ out) {
  const float* p = part + (size_t)blockIdx.x * n;
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) s = fadd_rn(s, p[i]);
  s = wave_sum(s);
  if (threadIdx.x == 0) out[blockIdx.x] = fdiv_rn(s, count);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes) {
  const char* pa = static_cast<const char*>(a);
  const char* pb = static_cast<const char*>(b);
  return pa < pb + bbytes && pb < pa + abytes;
}

// 0 if the grid holds N x M pairs of H x W images (grid.y = M, grid.z = ceil(N / TN), finish grid.x = N M)
int pairs_check(int N, int M, int H, int W) {
  if (N < 1 || M < 1 || M > 65535 || (N + TR_TN - 1) / TR_TN > 65535) return -5;
  if ((long)N * M > 0x7fffffffL / TR_MAX_BLOCKS) return -5;
  if (H < 1 || W < 1 || (long)H * W > 0x7fffffffL / 4) return -5;
  return 0;
}

int stream_blocks(long units) {
  const long g = (units + TR_THREADS - 1) / TR_THREADS;
  return (int)(g > TR_MAX_BLOCKS ? TR_MAX_BLOCKS : g);
}

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
  ICA_LAUNCH(pair_finish_kernel, dim3(N * M), dim3(64), 0, st, (const float*)ws, nb, (float)((long)3 * H * W),
             mse_in);
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
  ICA_LAUNCH(pair_finish_kernel, dim3(N * M), dim3(64), 0, st, (const float*)ws, nb, (float)((long)3 * H * W),
             mse_out);
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
