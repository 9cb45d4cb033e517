// Image-space degradations of random_noise.py on planar NCHW fp32 tensors [B][3][H][W]:
//
//   gauss_blur_kernel    torchvision gaussian_blur (random_noise.py:31-33, :55-58): reflect padding without edge
//                        repeat, then a ky x kx correlation of every channel; optional clamp to [0, 1] and the
//                        per-image mean((out - ref)^2)
//   blur_sweep_kernel    the sigma scan of generate_blurimages (random_noise.py:59-63): mean((clamp(blur_s(x)) - x)^2)
//                        of up to SWEEP_CHUNK candidate kernels per launch from one staged tile, no image written
//   sweep_select_kernel  (ica_reduce.h) per image the first candidate of the chunk with mse <= budget, and the done flag
//   noise_apply_kernel   random_noise.py:80: clamp(im + noise, 0, 1), mean(noise^2) and mean((im_in - im)^2)
//
// Arithmetic (fp32, DESIGN.md "Degradations"): the 2-D weight of tap (i, j) is the single rounded product
// wy[i] * wx[j] (what torch.mm of the two tap vectors gives); an output pixel is one fmaf chain over the taps in
// row-major order, started at 0.  A block stages a 64 x 32 tile and its halo in LDS once (16-byte row loads inside
// the image, reflected scalar loads at its edges); each thread then holds the window of its 4 x 2 output pixels in
// registers, so the sweep scores every candidate of the chunk without touching LDS or HBM again.
//
// Reductions: ica_reduce.h (sequential block order; one partial per tile, NOISE_MAX_BLOCKS caps noise_apply's).
#include "ica_reduce.h"

namespace {

constexpr int DG_THREADS = 256;
constexpr int DG_TW = 64;                 // tile width: 16 threads x 4 pixels
constexpr int DG_TH = 32;                 // tile height: 16 threads x 2 rows
constexpr int DG_ROWS = 2;                // output rows per thread
constexpr int DG_PAD = 4;                 // halo columns staged on each side (kx / 2 <= 4), keeps quads aligned
constexpr int DG_KMAX = 9;
constexpr int DG_LW = DG_TW + 2 * DG_PAD;             // 72 floats per LDS row
constexpr int DG_LH = DG_TH + DG_KMAX - 1;            // 40 rows
constexpr int DG_WIN = DG_KMAX + DG_ROWS - 1;         // window rows a thread holds
constexpr int SWEEP_CHUNK = 32;           // candidates per sweep launch (their per-thread sums live in LDS)
constexpr int NOISE_MAX_BLOCKS = 1024;

// index i of a reflect-padded axis of length n (no edge repeat), then pulled inside: the positions of a partial
// tile that lie past the padded image feed no output pixel, they only must not leave the plane
ICA_DEV int reflect_in(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

// rows [y0 - py, y0 + TH + py) x columns [x0 - PAD, x0 + TW + PAD) of one plane -> tile[DG_LH][DG_LW]
ICA_DEV void load_tile(const float* __restrict__ plane, int H, int W, int x0, int y0, int py, float* tile) {
  const int quads = (DG_TH + 2 * py) * (DG_LW / 4);
  for (int q = threadIdx.x; q < quads; q += DG_THREADS) {
    const int r = q / (DG_LW / 4), cq = q - r * (DG_LW / 4);
    const float* row = plane + (size_t)reflect_in(y0 - py + r, H) * W;
    const int gx = x0 - DG_PAD + 4 * cq;
    f32x4 v;
    if (gx >= 0 && gx + 3 < W) {
      v = ld4(row + gx);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = row[reflect_in(gx + e, W)];
    }
    st4(tile + r * DG_LW + 4 * cq, v);
  }
}

// the 12 staged columns under a thread's 4 pixels, for every window row it needs
ICA_DEV void load_window(const float* tile, int tx, int tr, int ky, float (&v)[DG_WIN][12]) {
#pragma unroll
  for (int i = 0; i < DG_WIN; ++i) {
    if (i < ky + DG_ROWS - 1) {
      const float* p = tile + (DG_ROWS * tr + i) * DG_LW + 4 * tx;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const f32x4 q = ld4(p + 4 * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][4 * k + e] = q[e];
      }
    }
  }
}

// acc[r][e] = sum_{i < ky} sum_{j < KX} (wy[i] * wx[j]) * window[i + r][e + j], one fmaf chain in row-major tap order
template <int KX>
ICA_DEV void correlate(const float (&v)[DG_WIN][12], const float* __restrict__ wx, const float* __restrict__ wy, int ky,
                       float (&acc)[DG_ROWS][4]) {
  constexpr int OFF = DG_PAD - KX / 2;
  float wxr[KX];
#pragma unroll
  for (int j = 0; j < KX; ++j) wxr[j] = wx[j];
#pragma unroll
  for (int r = 0; r < DG_ROWS; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = 0.f;
#pragma unroll
  for (int i = 0; i < DG_KMAX; ++i) {
    if (i < ky) {
      const float wyi = wy[i];
#pragma unroll
      for (int j = 0; j < KX; ++j) {
        const float w = fmul_rn(wyi, wxr[j]);
#pragma unroll
        for (int r = 0; r < DG_ROWS; ++r)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[r][e] = fmaf(w, v[i + r][OFF + e + j], acc[r][e]);
      }
    }
  }
}

template <int KX>
__global__ __launch_bounds__(DG_THREADS) void gauss_blur_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ wx,
                                                                const float* __restrict__ wy, int ky, int H, int W,
                                                                int clamp, const float* __restrict__ ref,
                                                                float* __restrict__ out, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float tile[DG_LH * DG_LW];
  __shared__ float red[4];
  const int pl = blockIdx.z, b = pl / 3;
  const int x0 = blockIdx.x * DG_TW, y0 = blockIdx.y * DG_TH;
  const size_t base = (size_t)pl * H * W;
  load_tile(x + base, H, W, x0, y0, ky / 2, tile);
  __syncthreads();
  const int tx = threadIdx.x & 15, tr = threadIdx.x >> 4;
  float v[DG_WIN][12], acc[DG_ROWS][4];
  load_window(tile, tx, tr, ky, v);
  correlate<KX>(v, wx + (size_t)b * KX, wy + (size_t)b * ky, ky, acc);
  const int gx = x0 + 4 * tx;
  float sq = 0.f;
#pragma unroll
  for (int r = 0; r < DG_ROWS; ++r) {
    const int gy = y0 + DG_ROWS * tr + r;
    if (gx < W && gy < H) {   // W % 4 == 0: a quad is inside the row or outside it
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = clamp ? clamp01(acc[r][e]) : acc[r][e];
      const size_t at = base + (size_t)gy * W + gx;
      st4(out + at, o);
      if (ref) {
        const f32x4 t = ld4(ref + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = fsub_rn(o[e], t[e]);
          sq = fmaf(d, d, sq);
        }
      }
    }
  }
  if (part) {
    const float s = block_sum(sq, red);
    if (threadIdx.x == 0) part[(size_t)pl * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

template <int KX>
__global__ __launch_bounds__(DG_THREADS) void blur_sweep_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ wx,
                                                                const float* __restrict__ wy, int S, int ky, int H,
                                                                int W, const int* __restrict__ done,
                                                                float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float tile[DG_LH * DG_LW];
  __shared__ float sums[SWEEP_CHUNK * DG_THREADS];
  const int pl = blockIdx.z, b = pl / 3;
  if (done[b]) return;   // block-uniform: the image has its answer
  const int x0 = blockIdx.x * DG_TW, y0 = blockIdx.y * DG_TH, py = ky / 2;
  load_tile(x + (size_t)pl * H * W, H, W, x0, y0, py, tile);
  __syncthreads();
  const int tx = threadIdx.x & 15, tr = threadIdx.x >> 4;
  float v[DG_WIN][12], acc[DG_ROWS][4];
  load_window(tile, tx, tr, ky, v);
  f32x4 centre[DG_ROWS];
  bool valid[DG_ROWS];
#pragma unroll
  for (int r = 0; r < DG_ROWS; ++r) {
    centre[r] = ld4(tile + (DG_ROWS * tr + r + py) * DG_LW + DG_PAD + 4 * tx);
    valid[r] = x0 + 4 * tx < W && y0 + DG_ROWS * tr + r < H;
  }
  for (int s = 0; s < S; ++s) {
    correlate<KX>(v, wx + (size_t)s * KX, wy + (size_t)s * ky, ky, acc);
    float sq = 0.f;
#pragma unroll
    for (int r = 0; r < DG_ROWS; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = valid[r] ? fsub_rn(clamp01(acc[r][e]), centre[r][e]) : 0.f;
        sq = fmaf(d, d, sq);
      }
    sums[s * DG_THREADS + threadIdx.x] = sq;
  }
  __syncthreads();
  // wave w sums the candidates w, w + 4, ...: each lane four threads' values in index order, then the butterfly
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t nblk = (size_t)gridDim.x * gridDim.y * 3;
  const size_t blk = (size_t)(pl - 3 * b) * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x;
  for (int s = wave; s < S; s += DG_THREADS / 64) {
    const float* p = sums + s * DG_THREADS + lane;
    const float t = wave_sum(fadd_rn(fadd_rn(fadd_rn(p[0], p[64]), p[128]), p[192]));
    if (lane == 0) part[((size_t)b * S + s) * nblk + blk] = t;
  }
}

__global__ __launch_bounds__(DG_THREADS) void noise_apply_kernel(const float* __restrict__ im,
                                                                 const float* __restrict__ noise,
                                                                 float* __restrict__ out, long quads,
                                                                 float* __restrict__ part_noise,
                                                                 float* __restrict__ part_in) {
  __shared__ float red[4];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * quads * 4;
  float sn = 0.f, sd = 0.f;
  for (long q = (long)blockIdx.x * DG_THREADS + threadIdx.x; q < quads; q += (long)gridDim.x * DG_THREADS) {
    const f32x4 a = ld4(im + base + q * 4), n = ld4(noise + base + q * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = clamp01(fadd_rn(a[e], n[e]));
      sn = fmaf(n[e], n[e], sn);
      const float d = fsub_rn(o[e], a[e]);
      sd = fmaf(d, d, sd);
    }
    st4(out + base + q * 4, o);
  }
  const float tn = block_sum(sn, red), td = block_sum(sd, red);
  if (threadIdx.x == 0) {
    part_noise[(size_t)b * gridDim.x + blockIdx.x] = tn;
    part_in[(size_t)b * gridDim.x + blockIdx.x] = td;
  }
}

// 0 if (B, H, W, kx, ky) is a supported blur problem
int blur_check(int B, int H, int W, int kx, int ky) {
  if (B < 1 || B > 21845) return -5;   // 3 B planes on grid.z
  if (kx < 1 || kx > DG_KMAX || !(kx & 1) || ky < 1 || ky > DG_KMAX || !(ky & 1)) return -5;
  if (H < 1 || W < 4 || W % 4 || H <= ky / 2 || W <= kx / 2) return -5;
  if ((long)H * W > 0x7fffffffL / 4 || (H + DG_TH - 1) / DG_TH > 65535) return -5;
  return 0;
}
int tiles_of(int H, int W) { return ((W + DG_TW - 1) / DG_TW) * ((H + DG_TH - 1) / DG_TH); }
int noise_blocks(long quads) { return capped_blocks(quads, DG_THREADS, NOISE_MAX_BLOCKS); }

#define DG_DISPATCH_KX(kern, kx, grid, st, ...)                                                  \
  do {                                                                                           \
    switch (kx) {                                                                                \
      case 1: ICA_LAUNCH(kern<1>, grid, dim3(DG_THREADS), 0, st, __VA_ARGS__); break;           \
      case 3: ICA_LAUNCH(kern<3>, grid, dim3(DG_THREADS), 0, st, __VA_ARGS__); break;           \
      case 5: ICA_LAUNCH(kern<5>, grid, dim3(DG_THREADS), 0, st, __VA_ARGS__); break;           \
      case 7: ICA_LAUNCH(kern<7>, grid, dim3(DG_THREADS), 0, st, __VA_ARGS__); break;           \
      default: ICA_LAUNCH(kern<9>, grid, dim3(DG_THREADS), 0, st, __VA_ARGS__); break;          \
    }                                                                                            \
  } while (0)

}  // namespace

extern "C" {

int ica_blur_sweep_chunk(void) { return SWEEP_CHUNK; }

size_t ica_gauss_blur_ws_size(int B, int H, int W) {
  if (blur_check(B, H, W, 1, 1)) return 0;
  return (size_t)B * 3 * tiles_of(H, W);
}

int ica_gauss_blur(const float* x, const float* wx, const float* wy, int B, int H, int W, int kx, int ky, int clamp,
                   const float* ref, float* out, float* mse, float* ws, hipStream_t st) {
  const int rc = blur_check(B, H, W, kx, ky);
  if (rc) return rc;
  if (!x || !wx || !wy || !out || (ref && (!mse || !ws)) || (!ref && mse)) return -5;
  if (!aligned16(x) || !aligned16(out) || !aligned16(ref)) return -5;
  const size_t bytes = (size_t)B * 3 * H * W * sizeof(float);
  if (overlaps(x, bytes, out, bytes)) return -7;   // a tile's halo is read after its neighbour was written
  const dim3 grid((W + DG_TW - 1) / DG_TW, (H + DG_TH - 1) / DG_TH, 3 * B);
  float* part = ref ? ws : nullptr;
  DG_DISPATCH_KX(gauss_blur_kernel, kx, grid, st, x, wx, wy, ky, H, W, clamp, ref, out, part);
  ICA_CHECK_LAUNCH();
  if (ref) {
    finish_rows(st, ws, B, 3 * tiles_of(H, W), (float)((long)3 * H * W), mse);
    ICA_CHECK_LAUNCH();
  }
  return 0;
}

size_t ica_blur_sweep_ws_size(int B, int H, int W) {
  if (blur_check(B, H, W, 1, 1)) return 0;
  return (size_t)B * SWEEP_CHUNK * 3 * tiles_of(H, W);
}

int ica_blur_sweep(const float* x, const float* wx, const float* wy, int S, int B, int H, int W, int kx, int ky,
                   float budget, int s0, float* mse, long ld, int* idx, int* done, int* remaining, float* ws,
                   hipStream_t st) {
  const int rc = blur_check(B, H, W, kx, ky);
  if (rc) return rc;
  if (S < 1 || S > SWEEP_CHUNK || s0 < 0 || ld < (long)s0 + S) return -5;
  if (!x || !wx || !wy || !mse || !idx || !done || !remaining || !ws || !aligned16(x)) return -5;
  const dim3 grid((W + DG_TW - 1) / DG_TW, (H + DG_TH - 1) / DG_TH, 3 * B);
  DG_DISPATCH_KX(blur_sweep_kernel, kx, grid, st, x, wx, wy, S, ky, H, W, (const int*)done, ws);
  ICA_CHECK_LAUNCH();
  finish_rows(st, ws, B * S, 3 * tiles_of(H, W), (float)((long)3 * H * W), mse, S, ld, s0, done);
  ICA_CHECK_LAUNCH();
  ICA_LAUNCH(sweep_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, st, (const float*)mse, ld, s0, S, budget, B, idx, done,
             remaining);
  ICA_CHECK_LAUNCH();
  return 0;
}

size_t ica_noise_apply_ws_size(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 4 || W % 4 || (long)H * W > 0x7fffffffL / 4) return 0;
  return (size_t)2 * B * noise_blocks((long)3 * H * W / 4);
}

int ica_noise_apply(const float* im, const float* noise, float* out, int B, int H, int W, float* noise_power,
                    float* mse_in, float* ws, hipStream_t st) {
  if (B < 1 || B > 65535 || H < 1 || W < 4 || W % 4 || (long)H * W > 0x7fffffffL / 4) return -5;
  if (!im || !noise || !out || !noise_power || !mse_in || !ws) return -5;
  if (!aligned16(im) || !aligned16(noise) || !aligned16(out)) return -5;
  const long quads = (long)3 * H * W / 4;
  const int nb = noise_blocks(quads);
  float* part_noise = ws;
  float* part_in = ws + (size_t)B * nb;
  ICA_LAUNCH(noise_apply_kernel, dim3(nb, B), dim3(DG_THREADS), 0, st, im, noise, out, quads, part_noise, part_in);
  ICA_CHECK_LAUNCH();
  const float count = (float)((long)3 * H * W);
  finish_rows(st, part_noise, B, nb, count, noise_power);
  ICA_CHECK_LAUNCH();
  finish_rows(st, part_in, B, nb, count, mse_in);
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
