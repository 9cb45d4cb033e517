// Patch-wise VI localisation (psnr_partial, attack_patch.py:119-146): for every win x win window at a given
// stride, mse_in = mean((im_s - im_adv)^2) and mse_out = mean((out_s - out_adv)^2) over the 3 * win^2 window
// elements, vi = mse_out / mse_in with a blanked border, the worst window, and the four patches cut there.
// Planar NCHW fp32 inputs [B][3][H][W]; the reference's unfold (win^2 * 3 values per window, in fp16) is
// replaced by box sums over the squared-error plane.
//
// Arithmetic (fp32, DESIGN.md "Patch VI"): with n = win / stride, a window sum factors through
// stride x stride cells,
//   cell[r][x] = sum_{c < 3} sum_{dy < stride} sum_{dx < stride} d^2     (one fma chain, <= 48 terms)
//   hs[r][x]   = sum_{k < n} cell[r][x + k]                              (one chain, <= 128 terms)
//   win[y][x]  = sum_{k < n} hs[y + k][x]                                (one chain, <= 128 terms)
// every term is non-negative, every chain runs in index order whatever the batch or the grid, nothing is
// subtracted and no float atomic is used: an image's maps are the same bits alone and in a batch, run to run.
//
//   patch_rows_kernel    one block per (cell row, image): reads the s pixel rows of the four images once
//                        (16-byte loads), leaves the row's cells in LDS and writes its horizontal sums hs
//   patch_cols_kernel    vertical sums (each thread 8 consecutive windows of one column, so a row of hs is read
//                        once per 8 windows), the means, vi and the argmax: one 64-bit atomicMax per wave on
//                        (float bits of vi >= 0, ~index), which is order-free and breaks ties towards the
//                        smallest row-major index
//   patch_finish_kernel  unpacks the keys into val[B] and pos[B][2]
//   patch_gather_kernel  reads pos on the device and writes the patches [B][4][3][win][win]
#include "ica_common.h"

namespace {

constexpr int ROWS_THREADS = 256;
constexpr int COLS_TX = 64;   // window columns per block (one wave per row group)
constexpr int COLS_TG = 4;    // row groups per block
constexpr int COLS_TY = 8;    // consecutive windows of one column per thread

template <int S>
__global__ __launch_bounds__(ROWS_THREADS) void patch_rows_kernel(
    const float* __restrict__ im_adv, const float* __restrict__ out_adv, const float* __restrict__ im_s,
    const float* __restrict__ out_s, int H, int W, int n, int ch, int nw, float* __restrict__ hs_in,
    float* __restrict__ hs_out) {
  extern __shared__ float cells[];   // [2][W / S]
  const int r = blockIdx.x, b = blockIdx.y;
  const int wc = W / S;
  float* cin = cells;
  float* cout = cells + wc;
  const size_t plane = (size_t)H * W;
  const size_t img = (size_t)b * 3 * plane + (size_t)r * S * W;
  for (int q = threadIdx.x; q < W / 4; q += ROWS_THREADS) {
    float ai[4 / S], ao[4 / S];
#pragma unroll
    for (int j = 0; j < 4 / S; ++j) ai[j] = ao[j] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int dy = 0; dy < S; ++dy) {
        const size_t o = img + c * plane + (size_t)dy * W + 4 * q;
        const f32x4 a = ld4(im_s + o), p = ld4(im_adv + o), u = ld4(out_s + o), v = ld4(out_adv + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float di = fsub_rn(a[e], p[e]), dq = fsub_rn(u[e], v[e]);
          ai[e / S] = fmaf(di, di, ai[e / S]);
          ao[e / S] = fmaf(dq, dq, ao[e / S]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4 / S; ++j) {
      cin[q * (4 / S) + j] = ai[j];
      cout[q * (4 / S) + j] = ao[j];
    }
  }
  __syncthreads();
  const size_t row = ((size_t)b * ch + r) * nw;
  for (int x = threadIdx.x; x < nw; x += ROWS_THREADS) {   // x + n - 1 <= nw + n - 2 < W / S
    float si = 0.f, so = 0.f;
    for (int k = 0; k < n; ++k) {
      si = fadd_rn(si, cin[x + k]);
      so = fadd_rn(so, cout[x + k]);
    }
    hs_in[row + x] = si;
    hs_out[row + x] = so;
  }
}

ICA_DEV unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(COLS_TX* COLS_TG) void patch_cols_kernel(
    const float* __restrict__ hs_in, const float* __restrict__ hs_out, int n, int ch, int nh, int nw, int border,
    float count, float* __restrict__ mse_in, float* __restrict__ mse_out, float* __restrict__ vi,
    unsigned long long* __restrict__ key) {
  const int b = blockIdx.z;
  const int x = blockIdx.x * COLS_TX + (threadIdx.x % COLS_TX);
  const int y0 = (blockIdx.y * COLS_TG + threadIdx.x / COLS_TX) * COLS_TY;
  unsigned long long best = 0;
  if (x < nw && y0 < nh) {
    const size_t base = (size_t)b * ch * nw + x;
    float si[COLS_TY], so[COLS_TY];
#pragma unroll
    for (int j = 0; j < COLS_TY; ++j) si[j] = so[j] = 0.f;
    // window y0 + j sums rows y0 + j .. y0 + j + n - 1 in that order: row y0 + i is its term k = i - j
    for (int i = 0; i < n + COLS_TY - 1; ++i) {
      const int row = y0 + i;
      if (row >= ch) break;
      const float a = hs_in[base + (size_t)row * nw], c = hs_out[base + (size_t)row * nw];
#pragma unroll
      for (int j = 0; j < COLS_TY; ++j)
        if (i >= j && i - j < n) {
          si[j] = fadd_rn(si[j], a);
          so[j] = fadd_rn(so[j], c);
        }
    }
#pragma unroll
    for (int j = 0; j < COLS_TY; ++j) {
      const int y = y0 + j;
      if (y < nh) {
        const float mi = fdiv_rn(si[j], count), mo = fdiv_rn(so[j], count);
        const bool edge = y < border || y >= nh - border || x < border || x >= nw - border;
        const float v = (edge || !(mi > 0.f)) ? 0.f : fdiv_rn(mo, mi);
        const size_t o = ((size_t)b * nh + y) * nw + x;
        mse_in[o] = mi;
        mse_out[o] = mo;
        vi[o] = v;
        const unsigned idx = (unsigned)y * (unsigned)nw + (unsigned)x;
        const unsigned long long k = ((unsigned long long)__float_as_uint(v) << 32) | (0xffffffffu - idx);
        best = k > best ? k : best;
      }
    }
  }
  best = wave_max_u64(best);
  if ((threadIdx.x & 63) == 0 && best != 0) atomicMax(key + b, best);
}

__global__ void patch_finish_kernel(const unsigned long long* __restrict__ key, int B, int nw, float* __restrict__ val,
                                    int* __restrict__ pos) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned long long k = key[b];
  const unsigned idx = k ? 0xffffffffu - (unsigned)k : 0u;   // no window wrote a key: value 0 at (0, 0)
  val[b] = __uint_as_float((unsigned)(k >> 32));
  pos[2 * b] = (int)(idx / (unsigned)nw);
  pos[2 * b + 1] = (int)(idx % (unsigned)nw);
}

__global__ void patch_gather_kernel(const float* __restrict__ im_adv, const float* __restrict__ out_adv,
                                    const float* __restrict__ im_s, const float* __restrict__ out_s,
                                    const int* __restrict__ pos, float* __restrict__ patches, int H, int W, int win,
                                    int stride, int nh, int nw) {
  const int b = blockIdx.y;
  // a position outside the map (a pos buffer the caller filled itself) is pulled inside: no read leaves the image
  const int py = min(max(pos[2 * b], 0), nh - 1) * stride, px = min(max(pos[2 * b + 1], 0), nw - 1) * stride;
  const int per = 3 * win * win;
  const size_t plane = (size_t)H * W;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < 4 * per; t += gridDim.x * blockDim.x) {
    const int which = t / per, e = t - which * per;
    const int c = e / (win * win), rem = e - c * win * win;
    const int y = rem / win, x = rem - y * win;
    const float* src = which == 0 ? im_adv : which == 1 ? out_adv : which == 2 ? im_s : out_s;
    patches[(size_t)b * 4 * per + t] = src[((size_t)b * 3 + c) * plane + (size_t)(py + y) * W + (px + x)];
  }
}

// 0 if (H, W, win, stride, border) is a supported problem
int patch_check(int B, int H, int W, int win, int stride, int border) {
  if (B < 1 || B > 65535) return -5;
  if (stride != 1 && stride != 2 && stride != 4) return -5;
  if (win < stride || win > 128 || win % stride) return -5;
  if (H < win || W < win || W % 4 || border < 0) return -5;
  if ((size_t)2 * (W / stride) * sizeof(float) > 65536) return -5;   // the cell row of one block lives in LDS
  if ((long)((H - win) / stride + 1) * ((W - win) / stride + 1) > 0x7fffffffL) return -5;
  return 0;
}

}  // namespace

extern "C" {

size_t ica_patch_vi_ws_size(int B, int H, int W, int win, int stride) {
  if (patch_check(B, H, W, win, stride, 0)) return 0;
  const size_t n = win / stride, nh = (H - win) / stride + 1, nw = (W - win) / stride + 1;
  return (size_t)2 * B * (nh - 1 + n) * nw;
}

int ica_patch_vi(const float* im_adv, const float* out_adv, const float* im_s, const float* out_s, int B, int H, int W,
                 int win, int stride, int border, float* ws, void* key_ws, float* mse_in, float* mse_out, float* vi,
                 float* val, int* pos, hipStream_t st) {
  const int rc = patch_check(B, H, W, win, stride, border);
  if (rc) return rc;
  const int n = win / stride, nh = (H - win) / stride + 1, nw = (W - win) / stride + 1, ch = nh - 1 + n;
  float* hs_in = ws;
  float* hs_out = ws + (size_t)B * ch * nw;
  unsigned long long* key = static_cast<unsigned long long*>(key_ws);
  if (hipMemsetAsync(key, 0, sizeof(unsigned long long) * B, st) != hipSuccess) return -6;
  const size_t lds = (size_t)2 * (W / stride) * sizeof(float);
  const dim3 grid(ch, B);
  if (stride == 1)
    ICA_LAUNCH(patch_rows_kernel<1>, grid, dim3(ROWS_THREADS), lds, st, im_adv, out_adv, im_s, out_s, H, W, n, ch, nw,
               hs_in, hs_out);
  else if (stride == 2)
    ICA_LAUNCH(patch_rows_kernel<2>, grid, dim3(ROWS_THREADS), lds, st, im_adv, out_adv, im_s, out_s, H, W, n, ch, nw,
               hs_in, hs_out);
  else
    ICA_LAUNCH(patch_rows_kernel<4>, grid, dim3(ROWS_THREADS), lds, st, im_adv, out_adv, im_s, out_s, H, W, n, ch, nw,
               hs_in, hs_out);
  ICA_CHECK_LAUNCH();
  const dim3 cgrid((nw + COLS_TX - 1) / COLS_TX, (nh + COLS_TG * COLS_TY - 1) / (COLS_TG * COLS_TY), B);
  if (cgrid.y > 65535) return -5;
  ICA_LAUNCH(patch_cols_kernel, cgrid, dim3(COLS_TX * COLS_TG), 0, st, hs_in, hs_out, n, ch, nh, nw, border,
             (float)(3 * win * win), mse_in, mse_out, vi, key);
  ICA_CHECK_LAUNCH();
  ICA_LAUNCH(patch_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, st, key, B, nw, val, pos);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_patch_gather(const float* im_adv, const float* out_adv, const float* im_s, const float* out_s, const int* pos,
                     float* patches, int B, int H, int W, int win, int stride, hipStream_t st) {
  const int rc = patch_check(B, H, W, win, stride, 0);
  if (rc) return rc;
  const int nh = (H - win) / stride + 1, nw = (W - win) / stride + 1;
  const int total = 4 * 3 * win * win;
  ICA_LAUNCH(patch_gather_kernel, dim3((total + 255) / 256, B), dim3(256), 0, st, im_adv, out_adv, im_s, out_s, pos,
             patches, H, W, win, stride, nh, nw);
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
