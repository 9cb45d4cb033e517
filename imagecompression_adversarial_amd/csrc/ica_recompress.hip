// The step between two generations of recompression.py (coder.py:21-48: clamp -> x 255 -> np.round -> uint8 -> PNG ->
// / 255.0 -> .to(device)) kept on the device:
//
//   requant8_kernel     x_hat4 (the forward's nChw4c reconstruction, 3 channels + a dead lane) -> the 8-bit codes of
//                       clamp(x_hat), the next generation's nChw4c input code / 255, optionally planar clamp(x_hat),
//                       and per image sum((clamp(x_hat) - orig)^2), sum(((q - prev_q) / 255)^2) and the number of
//                       code values that differ from prev_q
//   quant8_pack_kernel  planar fp32 image -> codes + nChw4c input (generation 0 of any source)
//   floor_bits_kernel   per image sum log(max(p, floor)) over the real channels of an nChw4c likelihood tensor
//                       (RateDistortionLoss, train.py:60-64: the floor is 2^-16 there)
//
// Arithmetic (fp32): c = x > 0 ? x : 0, then c < 1 ? c : 1, so a NaN becomes 0 and codes to 0; q = rint(c * 255) with
// the product rounded once and the rounding half-to-even (np.round of the float32 product); code / 255 is the
// correctly rounded IEEE quotient, which equals float32(float64(code) / 255.0) for all 256 codes (multiplying by a
// reciprocal does not).  A pixel is one 16-byte load and one 16-byte store on the nChw4c side; the planar tensors and
// the codes move as 4-byte accesses that a wave makes contiguous.
//
// Reductions: ica_reduce.h (sequential block order, at most RQ_MAX_BLOCKS partials per image).  The change count is
// an exact integer sum (at most 3 H W < 2^32).
#include "ica_reduce.h"

namespace {

constexpr int RQ_THREADS = 256;
constexpr int RQ_MAX_BLOCKS = 512;        // per image
constexpr float RQ_INV255 = 1.0f / 255.0f;   // sse_gen only (a sum with a tolerance); never the next input

ICA_DEV float clamp01z(float v) {          // torch.clamp(v, 0, 1) for numbers; a NaN gives 0
  v = v > 0.f ? v : 0.f;
  return v < 1.f ? v : 1.f;
}
ICA_DEV unsigned code8(float c) { return (unsigned)rintf(fmul_rn(c, 255.f)); }   // c in [0, 1]
ICA_DEV float decode8(unsigned k) { return fdiv_rn((float)k, 255.f); }

__global__ __launch_bounds__(RQ_THREADS) void requant8_kernel(const f32x4* x4, const float* __restrict__ orig,
                                                              const unsigned* prev, f32x4* next4, unsigned* q,
                                                              float* __restrict__ out, int HW,
                                                              float* __restrict__ part_o, float* __restrict__ part_g,
                                                              unsigned* __restrict__ part_c) {
  __shared__ float red[4];
  __shared__ unsigned redc[4];
  const int b = blockIdx.y;
  const size_t pbase = (size_t)b * HW;
  const float* op = orig + 3 * pbase;
  float* outp = out ? out + 3 * pbase : nullptr;
  float so = 0.f, sg = 0.f;
  unsigned cnt = 0;
  for (int p = blockIdx.x * RQ_THREADS + threadIdx.x; p < HW; p += gridDim.x * RQ_THREADS) {
    const f32x4 v = x4[pbase + p];
    const unsigned pq = prev[pbase + p];
    f32x4 nx;
    unsigned code = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float c = clamp01z(v[e]);
      const unsigned k = code8(c);
      nx[e] = decode8(k);
      code |= k << (8 * e);
      const float d = fsub_rn(c, op[(size_t)e * HW + p]);
      so = fmaf(d, d, so);
      const int dq = (int)k - (int)((pq >> (8 * e)) & 255u);
      const float g = fmul_rn((float)dq, RQ_INV255);
      sg = fmaf(g, g, sg);
      cnt += dq != 0;
      if (outp) outp[(size_t)e * HW + p] = c;
    }
    nx[3] = 0.f;
    next4[pbase + p] = nx;
    q[pbase + p] = code;
  }
  const float to = block_sum(so, red), tg = block_sum(sg, red);
  const unsigned tc = block_sum_u(cnt, redc);
  if (threadIdx.x == 0) {
    const size_t at = (size_t)b * gridDim.x + blockIdx.x;
    part_o[at] = to;
    part_g[at] = tg;
    part_c[at] = tc;
  }
}

// one block: wave w finishes the images w, w + 4, ...; moving[0] = images with a changed code
__global__ __launch_bounds__(RQ_THREADS) void requant8_finish_kernel(const float* __restrict__ part_o,
                                                                     const float* __restrict__ part_g,
                                                                     const unsigned* __restrict__ part_c, int B, int nb,
                                                                     float* __restrict__ sse_orig,
                                                                     float* __restrict__ sse_gen,
                                                                     long long* __restrict__ changed,
                                                                     int* __restrict__ moving) {
  __shared__ int mv;
  if (threadIdx.x == 0) mv = 0;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int b = wave; b < B; b += RQ_THREADS / 64) {
    const size_t base = (size_t)b * nb;
    // partials_sum's order for the two float rows, in one loop with the count: three loops one after the other
    // wait for memory three times per 64 partials (measured: 174 against 142 us per ica_requant8 call at B = 32)
    float so = 0.f, sg = 0.f;
    unsigned c = 0;
    for (int i = lane; i < nb; i += 64) {
      so = fadd_rn(so, part_o[base + i]);
      sg = fadd_rn(sg, part_g[base + i]);
      c += part_c[base + i];
    }
    so = wave_sum(so);
    sg = wave_sum(sg);
    c = wave_sum(c);
    if (lane == 0) {
      sse_orig[b] = so;
      sse_gen[b] = sg;
      changed[b] = (long long)c;
      if (c) atomicAdd(&mv, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && moving) moving[0] = mv;
}

__global__ __launch_bounds__(RQ_THREADS) void quant8_pack_kernel(const float* __restrict__ im, f32x4* __restrict__ next4,
                                                                 unsigned* __restrict__ q, int HW) {
  const int p = blockIdx.x * RQ_THREADS + threadIdx.x;
  if (p >= HW) return;
  const size_t pbase = (size_t)blockIdx.y * HW;
  const float* ip = im + 3 * pbase;
  f32x4 nx;
  unsigned code = 0;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const unsigned k = code8(clamp01z(ip[(size_t)e * HW + p]));
    nx[e] = decode8(k);
    code |= k << (8 * e);
  }
  nx[3] = 0.f;
  next4[pbase + p] = nx;
  q[pbase + p] = code;
}

// lik4 [B][ceil(C / 4)][H][W][4]: the lanes of the last channel group past C are loaded and never used
__global__ __launch_bounds__(RQ_THREADS) void floor_bits_kernel(const f32x4* __restrict__ lik4, int C, int HW, int quads,
                                                                float floor, float* __restrict__ part) {
  __shared__ float red[4];
  const int b = blockIdx.y;
  const f32x4* lp = lik4 + (size_t)b * quads;
  float s = 0.f;
  for (int i = blockIdx.x * RQ_THREADS + threadIdx.x; i < quads; i += gridDim.x * RQ_THREADS) {
    const f32x4 v = lp[i];
    const int live = C - 4 * (i / HW);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < live) s = fadd_rn(s, logf(v[e] > floor ? v[e] : floor));   // a NaN counts as the floor
  }
  const float t = block_sum(s, red);
  if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = t;
}

bool image_ok(int B, int H, int W) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 4 && W % 4 == 0 && (long)H * W <= 0x7fffffffL / 4;
}
int blocks_of(long n) { return capped_blocks(n, RQ_THREADS, RQ_MAX_BLOCKS); }
long lik_quads(int C, int H, int W) { return (long)((C + 3) / 4) * H * W; }
bool lik_ok(int B, int C, int H, int W) {
  return B >= 1 && B <= 65535 && C >= 1 && H >= 1 && W >= 1 && (long)H * W <= 0x7fffffffL / 4 &&
         lik_quads(C, H, W) <= 0x7fffffffL / 2;
}

}  // namespace

extern "C" {

size_t ica_requant8_ws_size(int B, int H, int W) {
  if (!image_ok(B, H, W)) return 0;
  return (size_t)3 * B * blocks_of((long)H * W);
}

int ica_requant8(const float* x_hat4, const float* orig, const uint32_t* prev_q, int B, int H, int W, float* next4,
                 uint32_t* q, float* out, float* sse_orig, float* sse_gen, long long* changed, int* moving, float* ws,
                 hipStream_t st) {
  if (!image_ok(B, H, W)) return -5;
  if (!x_hat4 || !orig || !prev_q || !next4 || !q || !sse_orig || !sse_gen || !changed || !ws) return -5;
  if (!aligned16(x_hat4) || !aligned16(next4)) return -5;
  const int HW = H * W, nb = blocks_of(HW);
  float* part_o = ws;
  float* part_g = ws + (size_t)B * nb;
  unsigned* part_c = reinterpret_cast<unsigned*>(ws + (size_t)2 * B * nb);
  ICA_LAUNCH(requant8_kernel, dim3(nb, B), dim3(RQ_THREADS), 0, st, reinterpret_cast<const f32x4*>(x_hat4), orig,
             reinterpret_cast<const unsigned*>(prev_q), reinterpret_cast<f32x4*>(next4),
             reinterpret_cast<unsigned*>(q), out, HW, part_o, part_g, part_c);
  ICA_CHECK_LAUNCH();
  ICA_LAUNCH(requant8_finish_kernel, dim3(1), dim3(RQ_THREADS), 0, st, (const float*)part_o, (const float*)part_g,
             (const unsigned*)part_c, B, nb, sse_orig, sse_gen, changed, moving);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_quant8_pack(const float* im, int B, int H, int W, float* next4, uint32_t* q, hipStream_t st) {
  if (!image_ok(B, H, W)) return -5;
  if (!im || !next4 || !q || !aligned16(next4)) return -5;
  const int HW = H * W;
  ICA_LAUNCH(quant8_pack_kernel, dim3((HW + RQ_THREADS - 1) / RQ_THREADS, B), dim3(RQ_THREADS), 0, st, im,
             reinterpret_cast<f32x4*>(next4), reinterpret_cast<unsigned*>(q), HW);
  ICA_CHECK_LAUNCH();
  return 0;
}

size_t ica_floor_bits_ws_size(int B, int C, int H, int W) {
  if (!lik_ok(B, C, H, W)) return 0;
  return (size_t)B * blocks_of(lik_quads(C, H, W));
}

int ica_floor_bits(const float* lik4, int B, int C, int H, int W, float floor, float* bits, float* ws,
                   hipStream_t st) {
  if (!lik_ok(B, C, H, W) || !(floor > 0.f)) return -5;
  if (!lik4 || !bits || !ws || !aligned16(lik4)) return -5;
  const int quads = (int)lik_quads(C, H, W), nb = blocks_of(quads);
  ICA_LAUNCH(floor_bits_kernel, dim3(nb, B), dim3(RQ_THREADS), 0, st, reinterpret_cast<const f32x4*>(lik4), C, H * W,
             quads, floor, ws);
  ICA_CHECK_LAUNCH();
  finish_rows(st, ws, B, nb, 1.f, bits);   // one wave per image; the sum is not divided
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
