// The loss side of the RD evaluation (batch_test, the reference's test.py) and of the trainer's validation
// (validate.py, the reference's test_epoch): RateDistortionLoss (train.py:50-96) on the tensors the eval forward left
// on the device, one launch per batch.
//
//   rd_metrics_kernel<false>  training=False.  Per image: sse = sum (clamp(x_hat, 0, 1) - target)^2 over 3 H W,
//                       lny / lnz = sum ln max(lik, 2^-16) over the y / z likelihood planes, nclamp = the number of
//                       likelihood elements below 2^-16 (a census: where it is large the clamp, not the codec, set the
//                       bpp), and the clamped reconstruction as NCHW, which the MS-SSIM kernels read as it is
//   rd_metrics_kernel<true>   training=True on an eval forward (ica_val_metrics).  The same sums with the UNCLAMPED
//                       x_hat, no census, and the unclamped NCHW reconstruction only where the caller asks for it (the
//                       ms-ssim metric reads it; a null pointer skips the store)
//
// It stands in for ica_nc4_bound_to_nchw, the torch clamp / log / sum of each likelihood plane and the torch MSE.
// x_hat and the likelihoods are fp32 nChw4c ([B][1][H][W][4], [B][C4][h][w][4]); target and the output are NCHW.
// A block walks the image's pixels, then the y quads, then the z quads: one 16-byte load per thread and iteration.
// Padding lanes (c >= C; lane 3 of x_hat) are read with their quad and add nothing.
//
// Reductions: ica_reduce.h.  A thread adds its terms in loop order, block_sum_paired adds the block, the block writes
// one partial per sum (part[b][k][block], k = sse, lny, lnz) and ica_reduce_rows adds the 3 B rows.  The partials of an
// image are a function of the shapes alone and no float atomic is used, so an image's numbers are the same bits alone
// and in a batch, run to run.  The census is exact: a wave sum, then one integer atomic per wave.
#include <math.h>

#include "ica_reduce.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_BLOCKS = 256;                     // per image (the rest is grid-strided)
constexpr float RD_LIK_MIN = 1.0f / 65536.0f;      // train.py:62 torch.clamp(likelihoods, min=1./65536)

// sum ln max(lik, 2^-16) of this block's quads of one image's plane; cnt: elements below the bound
ICA_DEV float rd_plane(const float* __restrict__ lik4, int C, long quads, long HW, int& cnt) {
  float acc = 0.f;
  for (long q = (long)blockIdx.x * RD_THREADS + threadIdx.x; q < quads; q += (long)gridDim.x * RD_THREADS) {
    const int c0 = (int)(q / HW) * 4;
    const f32x4 v = ld4(lik4 + q * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c0 + e >= C) continue;   // padding lanes add nothing
      const float l = v[e];
      cnt += l < RD_LIK_MIN;
      acc += logf(l < RD_LIK_MIN ? RD_LIK_MIN : l);   // keeps a NaN, as torch.clamp
    }
  }
  return acc;
}

// grid (blocks of the image, image); qy / qz: channel quads of one image's y / z plane (qz = 0 without z)
// VAL: the validation scorer (x_hat unclamped, out optional, nclamp unused)
template <bool VAL>
__global__ __launch_bounds__(RD_THREADS) void rd_metrics_kernel(const float* __restrict__ xhat4,
                                                                const float* __restrict__ target,
                                                                const float* __restrict__ liky4,
                                                                const float* __restrict__ likz4,
                                                                float* __restrict__ out, float* __restrict__ part,
                                                                int* __restrict__ nclamp, long HW, int Cy, long qy,
                                                                long HWy, int Cz, long qz, long HWz) {
  __shared__ float sh[4];
  const int b = blockIdx.y;
  const float* xh = xhat4 + (long)b * HW * 4;
  const float* tg = target + (long)b * HW * 3;
  float* o = (VAL && !out) ? nullptr : out + (long)b * HW * 3;
  float sse = 0.f;
  for (long pix = (long)blockIdx.x * RD_THREADS + threadIdx.x; pix < HW; pix += (long)gridDim.x * RD_THREADS) {
    const f32x4 v = ld4(xh + pix * 4);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float r = VAL ? v[c] : clamp01(v[c]);
      if (!VAL || o) o[c * HW + pix] = r;
      const float d = fsub_rn(r, tg[c * HW + pix]);
      sse += d * d;
    }
  }
  int cnt = 0;
  const float lny = rd_plane(liky4 + (long)b * qy * 4, Cy, qy, HWy, cnt);
  const float lnz = qz ? rd_plane(likz4 + (long)b * qz * 4, Cz, qz, HWz, cnt) : 0.f;
  float* p = part + (long)b * 3 * gridDim.x + blockIdx.x;
  const float r0 = block_sum_paired(sse, sh);
  const float r1 = block_sum_paired(lny, sh);
  const float r2 = block_sum_paired(lnz, sh);
  if (threadIdx.x == 0) {
    p[0] = r0;
    p[gridDim.x] = r1;
    p[2 * gridDim.x] = r2;
  }
  if (VAL) return;
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(nclamp + b, cnt);
}

// 0, or the status of a plane the kernel does not take
int rd_plane_check(int B, int C, int H, int W) {
  if (C <= 0 || H <= 0 || W <= 0) return -5;
  if ((C + 3) / 4 > 65535 || (long)H * W > 0x0fffffffL) return -5;
  if ((long)B * ((C + 3) / 4) > 0x7fffffffffffL / (4L * H * W)) return -5;   // elements < 2^47
  return 0;
}

// The argument checks both entries share: 0, -5 or -7 (include/ica_hip.h).  out may be null where out_optional.
int rd_args_check(const float* xhat4, const float* target, const float* liky4, const float* likz4, const float* out,
                  bool out_optional, const void* part, int B, int H, int W, int Cy, int Hy, int Wy, int Cz, int Hz,
                  int Wz) {
  if (B <= 0 || B > 65535) return -5;
  if (int rc = rd_plane_check(B, 3, H, W)) return rc;
  if (int rc = rd_plane_check(B, Cy, Hy, Wy)) return rc;
  if (likz4) {
    if (int rc = rd_plane_check(B, Cz, Hz, Wz)) return rc;
  } else if (Cz || Hz || Wz) {
    return -5;   // a z shape without a z plane
  }
  if (!xhat4 || !target || !liky4 || (!out && !out_optional) || !part) return -5;
  if (!aligned16(xhat4) || !aligned16(liky4) || !aligned16(likz4)) return -5;
  if (!out) return 0;
  const size_t HW = (size_t)H * W, qy = (size_t)((Cy + 3) / 4) * Hy * Wy;
  const size_t qz = likz4 ? (size_t)((Cz + 3) / 4) * Hz * Wz : 0;
  const size_t f = sizeof(float), ob = f * 3 * HW * B;
  if (overlaps(out, ob, xhat4, f * 4 * HW * B) || overlaps(out, ob, target, ob) ||
      overlaps(out, ob, liky4, f * 4 * qy * B) || (likz4 && overlaps(out, ob, likz4, f * 4 * qz * B)))
    return -7;
  return 0;
}


}  // namespace

extern "C" {

int ica_rd_metrics_blocks(void) { return RD_BLOCKS; }

int ica_rd_metrics(const float* xhat4, const float* target, const float* liky4, const float* likz4, float* out,
                   float* part, int* nclamp, int B, int H, int W, int Cy, int Hy, int Wy, int Cz, int Hz, int Wz,
                   hipStream_t st) {
  if (!nclamp) return -5;
  if (int rc = rd_args_check(xhat4, target, liky4, likz4, out, false, part, B, H, W, Cy, Hy, Wy, Cz, Hz, Wz)) return rc;
  const long HW = (long)H * W, HWy = (long)Hy * Wy, HWz = likz4 ? (long)Hz * Wz : 0;
  const long qy = (long)((Cy + 3) / 4) * HWy, qz = likz4 ? (long)((Cz + 3) / 4) * HWz : 0;
  hipError_t e = hipMemsetAsync(nclamp, 0, sizeof(int) * (size_t)B, st);
  if (e != hipSuccess) return (int)e;
  ICA_LAUNCH(rd_metrics_kernel<false>, dim3(RD_BLOCKS, B), dim3(RD_THREADS), 0, st, xhat4, target, liky4, likz4, out,
             part, nclamp, HW, Cy, qy, HWy, Cz, qz, HWz);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_val_metrics(const float* xhat4, const float* target, const float* liky4, const float* likz4, float* out,
                    float* part, int B, int H, int W, int Cy, int Hy, int Wy, int Cz, int Hz, int Wz,
                    hipStream_t st) {
  if (int rc = rd_args_check(xhat4, target, liky4, likz4, out, true, part, B, H, W, Cy, Hy, Wy, Cz, Hz, Wz)) return rc;
  const long HW = (long)H * W, HWy = (long)Hy * Wy, HWz = likz4 ? (long)Hz * Wz : 0;
  const long qy = (long)((Cy + 3) / 4) * HWy, qz = likz4 ? (long)((Cz + 3) / 4) * HWz : 0;
  ICA_LAUNCH(rd_metrics_kernel<true>, dim3(RD_BLOCKS, B), dim3(RD_THREADS), 0, st, xhat4, target, liky4, likz4, out,
             part, (int*)nullptr, HW, Cy, qy, HWy, Cz, qz, HWz);
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
