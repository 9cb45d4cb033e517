// The deterministic per-image reductions and the launch-argument checks the attack and study kernels share.
//
// Reductions (DESIGN.md §3 "Reductions"): a thread adds its terms in one fixed chain; the 64 lanes of a wave meet in
// the xor butterfly of wave_sum; the four waves of a 256-thread block are added in one of the two orders below; a block
// writes one partial; and partials_sum adds the partials of a row (an image, a pair, an (image, candidate)) with one
// wave, lane l taking the partials l, l + 64, ... in that order.  The number of blocks per image depends on the image
// size only (capped_blocks with each study's own thread count and cap) and no float atomic is used, so a row's
// numbers are the same bits alone and in a batch, run to run.  Every order here is part of that promise and is
// pinned by tests/test_gpu_reduce_pinned.py: a change to one changes results and needs its fixture recorded again.
#pragma once
#include "ica_common.h"

ICA_DEV unsigned wave_sum(unsigned v) {   // exact, so order-free; next to the float wave_sum of ica_common.h
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}
ICA_DEV int wave_sum(int v) { return (int)wave_sum((unsigned)v); }

// The sequential block order, ((w0 + w1) + w2) + w3, every thread gets the sum: the study kernels (ica_degrade.hip,
// ica_transfer.hip, ica_recompress.hip).  256 threads; red: 4 floats of LDS, free again on return.
ICA_DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = fadd_rn(fadd_rn(fadd_rn(red[0], red[1]), red[2]), red[3]);
  __syncthreads();
  return s;
}
ICA_DEV unsigned block_sum_u(unsigned v, unsigned* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const unsigned s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}

// The paired block order, (w0 + w1) + (w2 + w3), thread 0 alone gets the sum (the others 0): the attack kernels
// (ica_elem.hip: the step's partials, reduce_rows_kernel; ica_cw.hip: cw_gate_kernel).  256 threads; sh: 4 floats.
ICA_DEV float block_sum_paired(float v, float* sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  return r;
}

ICA_DEV float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // keeps a NaN, as torch.clamp

// One wave sums p[0 .. n): lane adds p[lane], p[lane + 64], ... to 0 in that order, then the butterfly.
ICA_DEV float partials_sum(const float* __restrict__ p, int n, int lane) {
  float s = 0.f;
  for (int i = lane; i < n; i += 64) s = fadd_rn(s, p[i]);
  return wave_sum(s);
}

namespace {

// One wave per row: out[(row / rpi) * ld + off + row % rpi] = partials_sum(row's n partials) / count (count 1 leaves
// the sum as it is: x / 1 is exact).  done (optional): the rows of finished images are left alone.
__global__ __launch_bounds__(64) void finish_rows_kernel(const float* __restrict__ part, int n, float count,
                                                         float* __restrict__ out, int rpi, long ld, long off,
                                                         const int* __restrict__ done) {
  const int row = blockIdx.x, img = row / rpi;
  if (done && done[img]) return;
  const float s = partials_sum(part + (size_t)row * n, n, threadIdx.x);
  if (threadIdx.x == 0) out[(size_t)img * ld + off + (row - img * rpi)] = fdiv_rn(s, count);
}

constexpr int SELECT_THREADS = 256;

// The first-fit step of a budget sweep (ica_degrade.hip's sigma scan, ica_jpeg.hip's quality scan).  One block: per
// unfinished image the first candidate of this chunk with mse <= budget; remaining[0] = images still without an answer
__global__ __launch_bounds__(SELECT_THREADS) void sweep_select_kernel(const float* __restrict__ mse, long ld, int s0,
                                                                      int S, float budget, int B,
                                                                      int* __restrict__ idx, int* __restrict__ done,
                                                                      int* __restrict__ remaining) {
  __shared__ int left;
  if (threadIdx.x == 0) left = 0;
  __syncthreads();
  int mine = 0;
  for (int b = threadIdx.x; b < B; b += SELECT_THREADS) {
    if (done[b]) continue;
    int found = -1;
    for (int s = 0; s < S && found < 0; ++s)
      if (mse[(size_t)b * ld + s0 + s] <= budget) found = s0 + s;
    if (found >= 0) {
      idx[b] = found;
      done[b] = 1;
    } else {
      ++mine;
    }
  }
  if (mine) atomicAdd(&left, mine);
  __syncthreads();
  if (threadIdx.x == 0) remaining[0] = left;
}

inline void finish_rows(hipStream_t st, const float* part, int rows, int n, float count, float* out, int rpi = 1,
                        long ld = 1, long off = 0, const int* done = nullptr) {
  ICA_LAUNCH(finish_rows_kernel, dim3(rows), dim3(64), 0, st, part, n, count, out, rpi, ld, off, done);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes) {
  const char* pa = static_cast<const char*>(a);
  const char* pb = static_cast<const char*>(b);
  return pa < pb + bbytes && pb < pa + abytes;
}

// ceil(units / threads) blocks per image, at most cap (the rest is grid-strided).  Both constants fix the number of
// partials of an image and with it the bits of its sums: each study passes its own.
inline int capped_blocks(long units, int threads, int cap) {
  const long g = (units + threads - 1) / threads;
  return (int)(g > cap ? cap : g);
}

}  // namespace
