// The per-channel latent range ("safe zone") of the reference: its profile statistic, the clamp defence and the
// detector score, on the latent y = g_a(x) the engine already holds on the device (fp32 nChw4c,
// [B][C/4][H][W][4]).
//
//   latent_range_kernel      feature_range.py:19-21   amax / amin / amax(abs) of y over each (image, channel) plane
//   latent_clamp_kernel      clamp_value_naive (attack_rd.py:66-67, search.py:34-35): two torch.where selects
//   latent_clamp_bwd_kernel  the autograd of those two selects with respect to y
//   latent_detect_kernel     detect (search.py:137-146), one score per image
//
// All four are bandwidth- or launch-bound: 16-byte loads of whole channel quads, no LDS traffic beyond the
// cross-wave step of a reduction, no float atomics (max / min / integer sums are order-free, so every result is
// the same bits whatever the launch shape).  torch's reductions propagate NaN while v_max / v_min drop it, so the
// reductions carry a NaN flag next to the running extreme.
#include <math.h>

#include "ica_reduce.h"

#define LAT_THREADS 256
#define LAT_WAVES (LAT_THREADS / 64)

ICA_DEV float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
ICA_DEV float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
ICA_DEV int wave_or(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}

// One block per (channel quad, image): the threads stride the plane's HW quads, each keeping the running
// max / min of its four channels (started at -inf / +inf) and a 4-bit NaN mask; a wave butterfly, then the
// LAT_WAVES partial results meet in LDS and the first four threads write one channel each.  (The sign of a zero
// extreme in a plane with zeros of both signs is v_max / v_min's choice, not necessarily torch's: ica_hip.h.)
__global__ __launch_bounds__(LAT_THREADS) void latent_range_kernel(const float* __restrict__ y4, int C4, int HW,
                                                                   float* __restrict__ out_max,
                                                                   float* __restrict__ out_min,
                                                                   float* __restrict__ out_absmax) {
  const int cq = blockIdx.x, b = blockIdx.y;
  const float* plane = y4 + ((size_t)b * C4 + cq) * (size_t)HW * 4;
  f32x4 mx = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  f32x4 mn = {INFINITY, INFINITY, INFINITY, INFINITY};
  int nan = 0;
  for (int p = threadIdx.x; p < HW; p += LAT_THREADS) {
    const f32x4 v = ld4(plane + (size_t)p * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      mx[e] = fmaxf(mx[e], v[e]);
      mn[e] = fminf(mn[e], v[e]);
      nan |= (v[e] != v[e]) << e;
    }
  }
  __shared__ float s_mx[LAT_WAVES][4], s_mn[LAT_WAVES][4];
  __shared__ int s_nan[LAT_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  nan = wave_or(nan);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float a = wave_max(mx[e]), i = wave_min(mn[e]);
    if (lane == 0) {
      s_mx[wave][e] = a;
      s_mn[wave][e] = i;
    }
  }
  if (lane == 0) s_nan[wave] = nan;
  __syncthreads();
  if (threadIdx.x < 4) {
    const int e = threadIdx.x;
    float a = s_mx[0][e], i = s_mn[0][e];
    int n = s_nan[0];
#pragma unroll
    for (int w = 1; w < LAT_WAVES; ++w) {
      a = fmaxf(a, s_mx[w][e]);
      i = fminf(i, s_mn[w][e]);
      n |= s_nan[w];
    }
    const bool isnan_ = (n >> e) & 1;
    const size_t o = (size_t)b * C4 * 4 + (size_t)cq * 4 + e;
    out_max[o] = isnan_ ? NAN : a;
    out_min[o] = isnan_ ? NAN : i;
    if (out_absmax) out_absmax[o] = isnan_ ? NAN : fmaxf(fabsf(a), fabsf(i));
  }
}

// t = y > cmax ? cmax : y;  o = t < cmin ? cmin : t   (a NaN fails both tests and passes through; a channel with
// cmin > cmax does what the two lines say).  blockIdx.y is the image, so a block's count of changed elements
// (o != y) belongs to one image: a wave sum, then one integer atomic per wave.  y4 may alias out4 (each thread
// reads its quad before it writes it).
__global__ __launch_bounds__(LAT_THREADS) void latent_clamp_kernel(const float* y4, const float* __restrict__ cmax,
                                                                   const float* __restrict__ cmin, float* out4,
                                                                   int C4, int HW, int* __restrict__ nclamped) {
  const int b = blockIdx.y;
  const long per = (long)C4 * HW;   // quads of one image
  const float* src = y4 + (size_t)b * per * 4;
  float* dst = out4 + (size_t)b * per * 4;
  int cnt = 0;
  for (long q = (long)blockIdx.x * LAT_THREADS + threadIdx.x; q < per; q += (long)gridDim.x * LAT_THREADS) {
    const int cq = (int)(q / HW);
    const f32x4 hi = ld4(cmax + cq * 4), lo = ld4(cmin + cq * 4);
    const f32x4 v = ld4(src + q * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = v[e] > hi[e] ? hi[e] : v[e];
      o[e] = t < lo[e] ? lo[e] : t;
      cnt += o[e] != v[e];
    }
    st4(dst + q * 4, o);
  }
  if (nclamped) {
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(nclamped + b, cnt);
  }
}

// g passes where both selects took y: !(y > cmax) && !(t < cmin); elsewhere the gradient of y is 0.
__global__ __launch_bounds__(LAT_THREADS) void latent_clamp_bwd_kernel(float* __restrict__ g4,
                                                                       const float* __restrict__ y4,
                                                                       const float* __restrict__ cmax,
                                                                       const float* __restrict__ cmin, int C4,
                                                                       int HW) {
  const int b = blockIdx.y;
  const long per = (long)C4 * HW;
  const float* src = y4 + (size_t)b * per * 4;
  float* g = g4 + (size_t)b * per * 4;
  for (long q = (long)blockIdx.x * LAT_THREADS + threadIdx.x; q < per; q += (long)gridDim.x * LAT_THREADS) {
    const int cq = (int)(q / HW);
    const f32x4 hi = ld4(cmax + cq * 4), lo = ld4(cmin + cq * 4);
    const f32x4 v = ld4(src + q * 4);
    f32x4 gv = ld4(g + q * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool over = v[e] > hi[e];
      const float t = over ? hi[e] : v[e];
      gv[e] = (!over && !(t < lo[e])) ? gv[e] : 0.f;
    }
    st4(g + q * 4, gv);
  }
}

// One block per image.  Per channel, each step one correctly rounded fp32 operation as torch computes it:
//   a = clamp(imax - cmax, min=0) / (cmax + 1)        b = |clamp(imin - cmin, max=0) / (cmin + 1)|
// (clamp keeps a NaN), then score = max_c a + max_c b with torch.max's NaN propagation.
__global__ __launch_bounds__(LAT_THREADS) void latent_detect_kernel(const float* __restrict__ imax,
                                                                    const float* __restrict__ imin,
                                                                    const float* __restrict__ cmax,
                                                                    const float* __restrict__ cmin,
                                                                    float* __restrict__ score, int C) {
  const int b = blockIdx.x;
  float ma = -INFINITY, mb = -INFINITY;
  int nan = 0;
  for (int c = threadIdx.x; c < C; c += LAT_THREADS) {
    const float hi = cmax[c], lo = cmin[c];
    float ea = fsub_rn(imax[(size_t)b * C + c], hi);
    ea = ea != ea ? ea : (ea < 0.f ? 0.f : ea);
    float eb = fsub_rn(imin[(size_t)b * C + c], lo);
    eb = eb != eb ? eb : (eb > 0.f ? 0.f : eb);
    const float a = fdiv_rn(ea, fadd_rn(hi, 1.f));
    const float bb = fabsf(fdiv_rn(eb, fadd_rn(lo, 1.f)));
    nan |= (a != a) | ((bb != bb) << 1);
    ma = fmaxf(ma, a);
    mb = fmaxf(mb, bb);
  }
  __shared__ float s_a[LAT_WAVES], s_b[LAT_WAVES];
  __shared__ int s_nan[LAT_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  ma = wave_max(ma);
  mb = wave_max(mb);
  nan = wave_or(nan);
  if (lane == 0) {
    s_a[wave] = ma;
    s_b[wave] = mb;
    s_nan[wave] = nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < LAT_WAVES; ++w) {
      ma = fmaxf(ma, s_a[w]);
      mb = fmaxf(mb, s_b[w]);
      nan |= s_nan[w];
    }
    score[b] = fadd_rn((nan & 1) ? NAN : ma, (nan & 2) ? NAN : mb);
  }
}

static inline int lat_blocks_per_image(long quads) { return max(1, capped_blocks(quads, LAT_THREADS, 1024)); }
static inline int lat_check(int B, int C, int H, int W) {
  if (C <= 0 || C % 4 != 0) return -2;
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || (long)H * W > 0x7fffffffL / 4) return -5;
  return 0;
}

extern "C" {

int ica_latent_range(const float* y4, int B, int C, int H, int W, float* out_max, float* out_min, float* out_absmax,
                     hipStream_t st) {
  if (int rc = lat_check(B, C, H, W)) return rc;
  ICA_LAUNCH(latent_range_kernel, dim3(C / 4, B), dim3(LAT_THREADS), 0, st, y4, C / 4, H * W, out_max, out_min,
             out_absmax);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_latent_clamp(const float* y4, const float* cmax, const float* cmin, float* out4, int B, int C, int H, int W,
                     int* nclamped, hipStream_t st) {
  if (int rc = lat_check(B, C, H, W)) return rc;
  if (nclamped) {
    hipError_t e = hipMemsetAsync(nclamped, 0, sizeof(int) * (size_t)B, st);
    if (e != hipSuccess) return (int)e;
  }
  ICA_LAUNCH(latent_clamp_kernel, dim3(lat_blocks_per_image((long)(C / 4) * H * W), B), dim3(LAT_THREADS), 0, st, y4,
             cmax, cmin, out4, C / 4, H * W, nclamped);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_latent_clamp_bwd(float* g4, const float* y4, const float* cmax, const float* cmin, int B, int C, int H, int W,
                         hipStream_t st) {
  if (int rc = lat_check(B, C, H, W)) return rc;
  ICA_LAUNCH(latent_clamp_bwd_kernel, dim3(lat_blocks_per_image((long)(C / 4) * H * W), B), dim3(LAT_THREADS), 0, st,
             g4, y4, cmax, cmin, C / 4, H * W);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_latent_detect(const float* imax, const float* imin, const float* cmax, const float* cmin, float* score, int B,
                      int C, hipStream_t st) {
  if (C <= 0 || C % 4 != 0) return -2;
  if (B <= 0) return -5;
  ICA_LAUNCH(latent_detect_kernel, dim3(B), dim3(LAT_THREADS), 0, st, imax, imin, cmax, cmin, score, C);
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
