// The baseline-JPEG transform round trip (DESIGN.md "JPEG round trip") on planar NCHW fp32 tensors [B][3][H][W]:
// no entropy coding, only what changes the samples.
//
//   jpeg_blocks_kernel   steps 1-5: 8-bit levels, RGB -> YCbCr, the 2x2 box mean of the chroma (4:2:0), then per 8x8
//                        block  -128, DCT, quantise, dequantise, inverse DCT, +128, round, clamp.  The decoded planes
//                        are integers in 0..255 and go to the workspace as bytes: Y at full size, Cb and Cr at the
//                        chroma size.  With SWEEP the forward DCT is computed once and stays in registers; each
//                        candidate table then costs quantise, dequantise and the inverse DCT.
//   jpeg_colour_kernel   steps 6-7: the triangle upsampling of the chroma (4:2:0), YCbCr -> RGB, rint, clamp,
//                        levels / 255; the image and, fused, the per-image sum of (out - ref)^2.  With SWEEP no image is
//                        written and the sums of all candidates of the chunk come from one read of x.
//
// Two passes through the byte planes (1.5 B per pixel at 4:2:0, 3 B at 4:4:4, written once and read once) are the
// 4:2:0 route: the triangle filter reads the chroma of the neighbouring MCUs, which the second pass finds decoded,
// whatever tile decoded it, so the result does not depend on the tiling.  4:4:4 takes the same two passes.
//
// Arithmetic: fp32.  The 8-point DCT (ica_dct8.h) is the even-odd factorisation with the constants
// 0.5 cos(k pi / 16); rows first, then columns, and the inverse in the opposite order. A decoded chroma sample is an integer, so the triangle filter
// (9 a + 3 b + 3 c + d) / 16 is exact in any order.
//
// A block of jpeg_blocks_kernel stages a 64 x 32 pixel tile (whole MCUs: H and W are multiples of the MCU) as three
// fp32 planes in LDS.  Eight threads share an 8x8 block: one per row in the row passes, one per column in the column
// pass, so the column pass reads 64 consecutive floats per eight blocks and the row passes read 16-byte quads.
//
// Reductions: ica_reduce.h (sequential block order; JP_MAX_BLOCKS caps the partials of an image).
#include "ica_dct8.h"
#include "ica_reduce.h"

namespace {

constexpr int JP_THREADS = 256;
constexpr int JP_TW = 64;                  // tile width: 16 threads x 4 pixels, 8 blocks
constexpr int JP_TH = 32;                  // tile height: 16 threads x 2 rows, 4 blocks
constexpr int JP_CHUNK = 8;                // candidates per sweep launch (their decoded planes live in the workspace)
constexpr int JP_MAX_BLOCKS = 1024;
constexpr int JP_TAB = 128;                // floats per table pair: luminance [64], chrominance [64], row-major
constexpr int JP_STE = 0, JP_CUBIC = 1;    // the surrogates of the backward (include/ica_hip.h)

ICA_DEV float level255(float v) { return fminf(fmaxf(rintf(v), 0.f), 255.f); }

// plane p of the LDS tile: the tasks of a pass over it are k = 0 .. w h / 8 - 1 with w = 8 nbx
template <bool S420>
ICA_DEV constexpr int plane_nbx(int p) { return (S420 && p) ? JP_TW / 16 : JP_TW / 8; }

// round i of a pass: which plane and which task this thread takes; false if none.  Round 0 is the Y plane (256
// tasks); at 4:2:0 round 1 holds both chroma planes (64 tasks each), at 4:4:4 rounds 1 and 2 one chroma plane each.
template <bool S420>
ICA_DEV bool task_of(int i, int tid, int& p, int& k) {
  if (i == 0 || !S420) {
    p = i;
    k = tid;
    return true;
  }
  p = 1 + (tid >> 6);
  k = tid & 63;
  return tid < 128;
}

ICA_DEV void store8(unsigned char* at, const float (&v)[8]) {
  u32x2 w;
  w[0] = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
  w[1] = (unsigned)v[4] | ((unsigned)v[5] << 8) | ((unsigned)v[6] << 16) | ((unsigned)v[7] << 24);
  *reinterpret_cast<u32x2*>(at) = w;
}

ICA_DEV void load8(const unsigned char* at, float (&v)[8]) {
  const u32x2 w = *reinterpret_cast<const u32x2*>(at);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = (float)((w[0] >> (8 * e)) & 255u);
    v[4 + e] = (float)((w[1] >> (8 * e)) & 255u);
  }
}

// tabs: the table pair of image b [B][JP_TAB], or with SWEEP of candidate s [S][JP_TAB].  wsY [B][S][H][W] bytes,
// wsC [B][S][2][Hc][Wc] bytes (S = 1 without SWEEP).
template <bool S420, bool SWEEP>
__global__ __launch_bounds__(JP_THREADS) void jpeg_blocks_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ tabs, int S, int H, int W,
                                                                 const int* __restrict__ done,
                                                                 unsigned char* __restrict__ wsY,
                                                                 unsigned char* __restrict__ wsC) {
  __shared__ __attribute__((aligned(16))) float pl[3][JP_TH][JP_TW];
  constexpr int NR = S420 ? 2 : 3;         // rounds of a pass
  const int b = blockIdx.z, tid = threadIdx.x;
  if (SWEEP && done[b]) return;   // block-uniform: the image has its answer
  const int x0 = blockIdx.x * JP_TW, y0 = blockIdx.y * JP_TH;
  const size_t HW = (size_t)H * W;

  {  // steps 1-3: a thread takes 4 x 2 pixels, that is two chroma samples at 4:2:0
    const int tx = tid & 15, ty = tid >> 4;
    const int gx = x0 + 4 * tx, gy = y0 + 2 * ty;
    const bool in = gx < W && gy < H;      // whole MCUs: a 4 x 2 patch is inside the image or outside it
    float cb[2][4], cr[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      f32x4 c[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        c[ch] = in ? ld4(x + ((size_t)b * 3 + ch) * HW + (size_t)(gy + r) * W + gx) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 yv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float R = rintf(fmul_rn(clamp01(c[0][e]), 255.f)), G = rintf(fmul_rn(clamp01(c[1][e]), 255.f)),
                    Bl = rintf(fmul_rn(clamp01(c[2][e]), 255.f));
        yv[e] = level255(fmaf(0.114f, Bl, fmaf(0.587f, G, 0.299f * R)));
        cb[r][e] = level255(fmaf(0.5f, Bl, fmaf(-0.331264f, G, fmaf(-0.168736f, R, 128.f))));
        cr[r][e] = level255(fmaf(-0.081312f, Bl, fmaf(-0.418688f, G, fmaf(0.5f, R, 128.f))));
      }
      st4(&pl[0][2 * ty + r][4 * tx], yv);
      if (!S420) {
        st4(&pl[1][2 * ty + r][4 * tx], f32x4{cb[r][0], cb[r][1], cb[r][2], cb[r][3]});
        st4(&pl[2][2 * ty + r][4 * tx], f32x4{cr[r][0], cr[r][1], cr[r][2], cr[r][3]});
      }
    }
    if (S420) {   // sums of four integers below 256 and a power-of-two scale: exact
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        pl[1][ty][2 * tx + h] = 0.25f * ((cb[0][2 * h] + cb[0][2 * h + 1]) + (cb[1][2 * h] + cb[1][2 * h + 1]));
        pl[2][ty][2 * tx + h] = 0.25f * ((cr[0][2 * h] + cr[0][2 * h + 1]) + (cr[1][2 * h] + cr[1][2 * h + 1]));
      }
    }
  }
  __syncthreads();

  // forward rows: task k = (row y, block column bx)
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    int p, k;
    if (!task_of<S420>(i, tid, p, k)) continue;
    const int nbx = plane_nbx<S420>(p), y = k / nbx, bx = k - y * nbx;
    float* row = &pl[p][y][8 * bx];
    const f32x4 lo = ld4(row), hi = ld4(row + 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = lo[e] - 128.f;
      v[4 + e] = hi[e] - 128.f;
    }
    dct8(v);
    st4(row, f32x4{v[0], v[1], v[2], v[3]});
    st4(row + 4, f32x4{v[4], v[5], v[6], v[7]});
  }
  __syncthreads();

  // forward columns: task k = (block row by, column xx); the coefficients of the column stay in registers
  float coef[NR][8];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    int p, k;
    if (!task_of<S420>(i, tid, p, k)) continue;
    const int w = 8 * plane_nbx<S420>(p), by = k / w, xx = k - by * w;
#pragma unroll
    for (int u = 0; u < 8; ++u) coef[i][u] = pl[p][8 * by + u][xx];
    dct8(coef[i]);
  }
  // a column task is the only one that touches its column until the barrier below: no barrier needed here

  const int Wc = S420 ? W / 2 : W, Hc = S420 ? H / 2 : H;
  const int cx0 = S420 ? x0 / 2 : x0, cy0 = S420 ? y0 / 2 : y0;
  for (int s = 0; s < S; ++s) {
    const float* tab = tabs + (size_t)(SWEEP ? s : b) * JP_TAB;
    // quantise, dequantise, inverse columns
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      int p, k;
      if (!task_of<S420>(i, tid, p, k)) continue;
      const int w = 8 * plane_nbx<S420>(p), by = k / w, xx = k - by * w;
      const float* tq = tab + (p ? 64 : 0) + (xx & 7);
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float q = tq[8 * u];
        v[u] = fmul_rn(roundf(fdiv_rn(coef[i][u], q)), q);   // roundf: half away from zero
      }
      idct8(v);
#pragma unroll
      for (int u = 0; u < 8; ++u) pl[p][8 * by + u][xx] = v[u];
    }
    __syncthreads();
    // inverse rows, +128, round, clamp, eight bytes to the workspace
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      int p, k;
      if (!task_of<S420>(i, tid, p, k)) continue;
      const int nbx = plane_nbx<S420>(p), y = k / nbx, bx = k - y * nbx;
      const float* row = &pl[p][y][8 * bx];
      const f32x4 lo = ld4(row), hi = ld4(row + 4);
      float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      idct8(v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = level255(v[e] + 128.f);
      const size_t img = (size_t)b * S + s;
      if (p == 0) {
        const int gx = x0 + 8 * bx, gy = y0 + y;
        if (gx < W && gy < H) store8(wsY + img * HW + (size_t)gy * W + gx, v);
      } else {
        const int gx = cx0 + 8 * bx, gy = cy0 + y;
        if (gx < Wc && gy < Hc) store8(wsC + (img * 2 + (p - 1)) * ((size_t)Hc * Wc) + (size_t)gy * Wc + gx, v);
      }
    }
    __syncthreads();   // the next candidate overwrites the planes
  }
}

// The chroma of an 8 x 2 pixel patch (pixel rows 2 py, 2 py + 1, columns 8 px ..) from one decoded plane, minus 128.
// 4:2:0: the triangle filter, 3/4 of the nearest sample and 1/4 of the next one along each axis, edges replicated.
template <bool S420>
ICA_DEV void chroma_patch(const unsigned char* __restrict__ P, int Hc, int Wc, int py, int px, float (&o)[2][8]) {
  if (!S420) {
    load8(P + (size_t)(2 * py) * Wc + 8 * px, o[0]);
    load8(P + (size_t)(2 * py + 1) * Wc + 8 * px, o[1]);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int e = 0; e < 8; ++e) o[r][e] -= 128.f;
    return;
  }
  const int cx = 4 * px, xl = max(cx - 1, 0), xr = min(cx + 4, Wc - 1);
  const int rows[3] = {max(py - 1, 0), py, min(py + 1, Hc - 1)};
  float a[3][6];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const unsigned char* row = P + (size_t)rows[r] * Wc;
    const unsigned w = *reinterpret_cast<const unsigned*>(row + cx);
    a[r][0] = (float)row[xl];
#pragma unroll
    for (int e = 0; e < 4; ++e) a[r][1 + e] = (float)((w >> (8 * e)) & 255u);
    a[r][5] = (float)row[xr];
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    float v[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = 3.f * a[1][j] + a[2 * r][j];   // even row: the row above; odd: the row below
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int near = 1 + (e >> 1), next = (e & 1) ? near + 1 : near - 1;
      o[r][e] = (3.f * v[near] + v[next]) * 0.0625f - 128.f;
    }
  }
}

// ref: what the squared error is taken against (with SWEEP: x itself, required).  out: the image, not with SWEEP.
// part: [B][gridDim.x], with SWEEP [B][S][gridDim.x]; null if no error is asked for.
template <bool S420, bool SWEEP>
__global__ __launch_bounds__(JP_THREADS) void jpeg_colour_kernel(const float* __restrict__ ref,
                                                                 const unsigned char* __restrict__ wsY,
                                                                 const unsigned char* __restrict__ wsC, int S, int H,
                                                                 int W, const int* __restrict__ done,
                                                                 float* __restrict__ out, float* __restrict__ part) {
  constexpr int NS = SWEEP ? JP_CHUNK : 1;
  __shared__ float sums[SWEEP ? JP_CHUNK * JP_THREADS : 4];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (SWEEP && done[b]) return;   // block-uniform
  const int PW = W / 8, Wc = S420 ? W / 2 : W, Hc = S420 ? H / 2 : H;
  const long patches = (long)PW * (H / 2);
  const size_t HW = (size_t)H * W, CHW = (size_t)Hc * Wc;
  float sq[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) sq[s] = 0.f;
  for (long pid = (long)blockIdx.x * JP_THREADS + tid; pid < patches; pid += (long)gridDim.x * JP_THREADS) {
    const int py = (int)(pid / PW), px = (int)(pid - (long)py * PW);
    const size_t at = (size_t)b * 3 * HW + (size_t)(2 * py) * W + 8 * px;   // channel 0, first row of the patch
    f32x4 t[3][2][2];
    if (ref) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          t[ch][r][0] = ld4(ref + at + ch * HW + (size_t)r * W);
          t[ch][r][1] = ld4(ref + at + ch * HW + (size_t)r * W + 4);
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s >= S) break;
      const size_t img = (size_t)b * S + s;
      float cb[2][8], cr[2][8];
      chroma_patch<S420>(wsC + img * 2 * CHW, Hc, Wc, py, px, cb);
      chroma_patch<S420>(wsC + (img * 2 + 1) * CHW, Hc, Wc, py, px, cr);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        float yv[8];
        load8(wsY + img * HW + (size_t)(2 * py + r) * W + 8 * px, yv);
        f32x4 o[3][2];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float R = fmaf(1.402f, cr[r][e], yv[e]);
          const float G = fmaf(-0.714136f, cr[r][e], fmaf(-0.344136f, cb[r][e], yv[e]));
          const float Bl = fmaf(1.772f, cb[r][e], yv[e]);
          o[0][e >> 2][e & 3] = fdiv_rn(level255(R), 255.f);
          o[1][e >> 2][e & 3] = fdiv_rn(level255(G), 255.f);
          o[2][e >> 2][e & 3] = fdiv_rn(level255(Bl), 255.f);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (!SWEEP) st4(out + at + ch * HW + (size_t)r * W + 4 * h, o[ch][h]);
            if (ref) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float d = fsub_rn(o[ch][h][e], t[ch][r][h][e]);
                sq[s] = fmaf(d, d, sq[s]);
              }
            }
          }
      }
    }
  }
  if (!SWEEP) {
    if (part) {
      const float total = block_sum(sq[0], sums);
      if (tid == 0) part[(size_t)b * gridDim.x + blockIdx.x] = total;
    }
    return;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s)
    if (s < S) sums[s * JP_THREADS + tid] = sq[s];
  __syncthreads();
  // wave w sums the candidates w, w + 4, ...: each lane four threads' values in index order, then the butterfly
  const int wave = tid >> 6, lane = tid & 63;
  for (int s = wave; s < S; s += JP_THREADS / 64) {
    const float* p = sums + s * JP_THREADS + lane;
    const float total = wave_sum(fadd_rn(fadd_rn(fadd_rn(p[0], p[64]), p[128]), p[192]));
    if (lane == 0) part[((size_t)b * S + s) * gridDim.x + blockIdx.x] = total;
  }
}

// ---- the backward under a surrogate (DESIGN.md "JPEG round trip", "The attack through it") ----------------------
// Roundings of samples have derivative 1, a clamp passes the gradient iff the rounded value lies in 0 .. 255 (step 1:
// iff 0 <= x <= 1), the coefficient quantiser has derivative d(r), r = c / q - roundf(c / q): 1 (ste) or 3 r^2
// (cubic).  Everything else is linear and gets its transpose.  The masks and d are those of the forward's own values:
// both kernels recompute them with the forward's expressions.

ICA_DEV bool passes255(float v) {   // the inclusive mask of level255, on the rounded value; a NaN does not pass
  const float r = rintf(v);
  return r >= 0.f && r <= 255.f;
}

// sample (y, x) of the triangle-upsampled chroma plane (4:2:0) or of the plane itself, minus 128: chroma_patch's value
template <bool S420>
ICA_DEV float chroma_at(const unsigned char* __restrict__ P, int Hc, int Wc, int y, int x) {
  if (!S420) return (float)P[(size_t)y * Wc + x] - 128.f;
  const int cy = y >> 1, cx = x >> 1;
  const int ny = (y & 1) ? min(cy + 1, Hc - 1) : max(cy - 1, 0), nx = (x & 1) ? min(cx + 1, Wc - 1) : max(cx - 1, 0);
  const unsigned char *near = P + (size_t)cy * Wc, *next = P + (size_t)ny * Wc;
  const float vn = 3.f * (float)near[cx] + (float)next[cx], vx = 3.f * (float)near[nx] + (float)next[nx];
  return (3.f * vn + vx) * 0.0625f - 128.f;   // integers below 2^12: exact, as in chroma_patch
}

// weights with which chroma sample c of n collects the pixels 2 c - 1 .. 2 c + 2 along an axis: the transpose of the
// triangle filter, the replicated edge folded into the edge pixel
ICA_DEV void triangle_t(int c, int n, float (&w)[4]) {
  w[0] = c ? 0.25f : 0.f;
  w[1] = c ? 0.75f : 1.f;
  w[2] = c < n - 1 ? 0.75f : 1.f;
  w[3] = c < n - 1 ? 0.25f : 0.f;
}

// The transpose of steps 6-7 for one 64 x 32 pixel tile: gY [B][H][W], gC [B][2][Hc][Wc].  A thread takes pixels of
// the tile and, at 4:2:0, of the one-pixel ring around it: R, G, B as jpeg_colour_kernel computes them, the step-7
// masks, / 255, the transposed YCbCr -> RGB matrix.  At 4:2:0 the full-size chroma gradients of tile and ring wait in
// LDS and every chroma sample of the tile then gathers its 4 x 4 pixels in a fixed order: no atomics, and a sample's
// sum does not depend on which tile forms it.
template <bool S420>
__global__ __launch_bounds__(JP_THREADS) void jpeg_colour_bwd_kernel(const float* __restrict__ g_out,
                                                                     const unsigned char* __restrict__ wsY,
                                                                     const unsigned char* __restrict__ wsC, int H,
                                                                     int W, float* __restrict__ gY,
                                                                     float* __restrict__ gC) {
  constexpr int RING = S420 ? 1 : 0, LW = JP_TW + 2 * RING, LH = JP_TH + 2 * RING;
  __shared__ float gc[2][S420 ? LH : 1][S420 ? LW : 1];   // 4:2:0 only
  const int b = blockIdx.z, tid = threadIdx.x;
  const int x0 = blockIdx.x * JP_TW, y0 = blockIdx.y * JP_TH;
  const int Wc = S420 ? W / 2 : W, Hc = S420 ? H / 2 : H;
  const size_t HW = (size_t)H * W, CHW = (size_t)Hc * Wc;
  const unsigned char* Pb = wsC + (size_t)b * 2 * CHW;
  const unsigned char* Pr = Pb + CHW;
  for (int i = tid; i < LW * LH; i += JP_THREADS) {
    const int ly = i / LW, lx = i - ly * LW;
    const int y = y0 - RING + ly, x = x0 - RING + lx;
    float gcb = 0.f, gcr = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t at = (size_t)y * W + x;
      const float yv = (float)wsY[(size_t)b * HW + at];
      const float cb = chroma_at<S420>(Pb, Hc, Wc, y, x), cr = chroma_at<S420>(Pr, Hc, Wc, y, x);
      const float R = fmaf(1.402f, cr, yv);
      const float G = fmaf(-0.714136f, cr, fmaf(-0.344136f, cb, yv));
      const float Bl = fmaf(1.772f, cb, yv);
      const float* g = g_out + (size_t)b * 3 * HW + at;
      const float gR = passes255(R) ? fdiv_rn(g[0], 255.f) : 0.f;
      const float gG = passes255(G) ? fdiv_rn(g[HW], 255.f) : 0.f;
      const float gB = passes255(Bl) ? fdiv_rn(g[2 * HW], 255.f) : 0.f;
      gcb = fmaf(1.772f, gB, -0.344136f * gG);
      gcr = fmaf(1.402f, gR, -0.714136f * gG);
      const bool own = ly >= RING && ly < LH - RING && lx >= RING && lx < LW - RING;
      if (own) gY[(size_t)b * HW + at] = (gR + gG) + gB;
      if (!S420) {
        gC[(size_t)b * 2 * CHW + at] = gcb;
        gC[((size_t)b * 2 + 1) * CHW + at] = gcr;
      }
    }
    if constexpr (S420) {
      gc[0][ly][lx] = gcb;
      gc[1][ly][lx] = gcr;
    }
  }
  if constexpr (S420) {
    __syncthreads();
    // chroma sample (cy, cx) of the tile: pixels 2 cy - 1 .. 2 cy + 2, that is LDS rows 2 k .. 2 k + 3 of local row k
    constexpr int TCW = JP_TW / 2, TCH = JP_TH / 2;
    for (int i = tid; i < 2 * TCW * TCH; i += JP_THREADS) {
      const int p = i / (TCW * TCH), k = i - p * (TCW * TCH), ky = k / TCW, kx = k - ky * TCW;
      const int cy = y0 / 2 + ky, cx = x0 / 2 + kx;
      if (cy >= Hc || cx >= Wc) continue;
      float wy[4], wx[4];
      triangle_t(cy, Hc, wy);
      triangle_t(cx, Wc, wx);
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* row = &gc[p][2 * ky + j][2 * kx];
        const float s = (wx[0] * row[0] + wx[1] * row[1]) + (wx[2] * row[2] + wx[3] * row[3]);
        acc = fmaf(wy[j], s, acc);
      }
      gC[((size_t)b * 2 + p) * CHW + (size_t)cy * Wc + cx] = acc;
    }
  }
}

// The transpose of steps 1-5 for one 64 x 32 pixel tile, laid out as jpeg_blocks_kernel's.  The forward is run again up
// to the decoded samples: the thread of a 4 x 2 pixel patch keeps the masks of steps 1 and 2 for the epilogue, a
// column task keeps d(r) of its eight coefficients, a row task the step-4 masks of its eight samples.  The gradient
// tile then takes the planes' place in LDS: mask, forward rows and columns (the transposes of the inverse rows and
// columns), x d, inverse columns and rows.  With d = 1 (ste) the orthonormal pair is the identity and is left out.
template <bool S420, bool CUBIC>
__global__ __launch_bounds__(JP_THREADS) void jpeg_blocks_bwd_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ tabs, int H, int W,
                                                                     const float* __restrict__ gY,
                                                                     const float* __restrict__ gC,
                                                                     float* __restrict__ g_x) {
  __shared__ __attribute__((aligned(16))) float pl[3][JP_TH][JP_TW];
  constexpr int NR = S420 ? 2 : 3;
  const int b = blockIdx.z, tid = threadIdx.x;
  const int x0 = blockIdx.x * JP_TW, y0 = blockIdx.y * JP_TH;
  const size_t HW = (size_t)H * W;
  const int tx = tid & 15, ty = tid >> 4;
  const int px = x0 + 4 * tx, py = y0 + 2 * ty;
  const bool in = px < W && py < H;          // whole MCUs: a 4 x 2 patch is inside the image or outside it
  // bit 8 ch + 4 r + e: step 1 passes channel ch of pixel (r, e); step 2 passes plane ch (Y, Cb, Cr) there
  unsigned m1 = 0u, m2 = 0u;

  {  // steps 1-3, as jpeg_blocks_kernel
    float cb[2][4], cr[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      f32x4 c[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        c[ch] = in ? ld4(x + ((size_t)b * 3 + ch) * HW + (size_t)(py + r) * W + px) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 yv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          if (c[ch][e] >= 0.f && c[ch][e] <= 1.f) m1 |= 1u << (8 * ch + 4 * r + e);
        const float R = rintf(fmul_rn(clamp01(c[0][e]), 255.f)), G = rintf(fmul_rn(clamp01(c[1][e]), 255.f)),
                    Bl = rintf(fmul_rn(clamp01(c[2][e]), 255.f));
        const float fy = fmaf(0.114f, Bl, fmaf(0.587f, G, 0.299f * R));
        const float fb = fmaf(0.5f, Bl, fmaf(-0.331264f, G, fmaf(-0.168736f, R, 128.f)));
        const float fr = fmaf(-0.081312f, Bl, fmaf(-0.418688f, G, fmaf(0.5f, R, 128.f)));
        if (passes255(fy)) m2 |= 1u << (4 * r + e);
        if (passes255(fb)) m2 |= 1u << (8 + 4 * r + e);
        if (passes255(fr)) m2 |= 1u << (16 + 4 * r + e);
        yv[e] = level255(fy);
        cb[r][e] = level255(fb);
        cr[r][e] = level255(fr);
      }
      st4(&pl[0][2 * ty + r][4 * tx], yv);
      if (!S420) {
        st4(&pl[1][2 * ty + r][4 * tx], f32x4{cb[r][0], cb[r][1], cb[r][2], cb[r][3]});
        st4(&pl[2][2 * ty + r][4 * tx], f32x4{cr[r][0], cr[r][1], cr[r][2], cr[r][3]});
      }
    }
    if (S420) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        pl[1][ty][2 * tx + h] = 0.25f * ((cb[0][2 * h] + cb[0][2 * h + 1]) + (cb[1][2 * h] + cb[1][2 * h + 1]));
        pl[2][ty][2 * tx + h] = 0.25f * ((cr[0][2 * h] + cr[0][2 * h + 1]) + (cr[1][2 * h] + cr[1][2 * h + 1]));
      }
    }
  }
  __syncthreads();

  // forward rows
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    int p, k;
    if (!task_of<S420>(i, tid, p, k)) continue;
    const int nbx = plane_nbx<S420>(p), y = k / nbx, bx = k - y * nbx;
    float* row = &pl[p][y][8 * bx];
    const f32x4 lo = ld4(row), hi = ld4(row + 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = lo[e] - 128.f;
      v[4 + e] = hi[e] - 128.f;
    }
    dct8(v);
    st4(row, f32x4{v[0], v[1], v[2], v[3]});
    st4(row + 4, f32x4{v[4], v[5], v[6], v[7]});
  }
  __syncthreads();

  // forward columns, quantise (d(r) stays with the column task), dequantise, inverse columns
  float dq[CUBIC ? NR : 1][8];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    int p, k;
    if (!task_of<S420>(i, tid, p, k)) continue;
    const int w = 8 * plane_nbx<S420>(p), by = k / w, xx = k - by * w;
    const float* tq = tabs + (size_t)b * JP_TAB + (p ? 64 : 0) + (xx & 7);
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = pl[p][8 * by + u][xx];
    dct8(v);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float q = tq[8 * u], t = fdiv_rn(v[u], q), n = roundf(t);
      if constexpr (CUBIC) {
        const float r = fsub_rn(t, n);
        dq[i][u] = 3.f * fmul_rn(r, r);
      }
      v[u] = fmul_rn(n, q);
    }
    idct8(v);
#pragma unroll
    for (int u = 0; u < 8; ++u) pl[p][8 * by + u][xx] = v[u];
  }
  __syncthreads();

  // inverse rows give the decoded samples and so the step-4 masks; the row task then puts the masked gradient of its
  // eight samples in their place (it alone touches them between two barriers), with cubic after the forward row pass
  const int Wc = S420 ? W / 2 : W, Hc = S420 ? H / 2 : H;
  const int cx0 = S420 ? x0 / 2 : x0, cy0 = S420 ? y0 / 2 : y0;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    int p, k;
    if (!task_of<S420>(i, tid, p, k)) continue;
    const int nbx = plane_nbx<S420>(p), y = k / nbx, bx = k - y * nbx;
    float* row = &pl[p][y][8 * bx];
    const f32x4 lo = ld4(row), hi = ld4(row + 4);
    float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    idct8(v);
    const float* src;
    bool have;
    if (p == 0) {
      const int gx = x0 + 8 * bx, gy = y0 + y;
      have = gx < W && gy < H;
      src = gY + (size_t)b * HW + (size_t)gy * W + gx;
    } else {
      const int gx = cx0 + 8 * bx, gy = cy0 + y;
      have = gx < Wc && gy < Hc;
      src = gC + ((size_t)b * 2 + (p - 1)) * ((size_t)Hc * Wc) + (size_t)gy * Wc + gx;
    }
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 glo = have ? ld4(src) : z, ghi = have ? ld4(src + 4) : z;
    float g[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      g[e] = passes255(v[e] + 128.f) ? glo[e] : 0.f;
      g[4 + e] = passes255(v[4 + e] + 128.f) ? ghi[e] : 0.f;
    }
    if constexpr (CUBIC) dct8(g);
    st4(row, f32x4{g[0], g[1], g[2], g[3]});
    st4(row + 4, f32x4{g[4], g[5], g[6], g[7]});
  }
  __syncthreads();

  if constexpr (CUBIC) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      int p, k;
      if (!task_of<S420>(i, tid, p, k)) continue;
      const int w = 8 * plane_nbx<S420>(p), by = k / w, xx = k - by * w;
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = pl[p][8 * by + u][xx];
      dct8(v);
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = fmul_rn(v[u], dq[i][u]);
      idct8(v);
#pragma unroll
      for (int u = 0; u < 8; ++u) pl[p][8 * by + u][xx] = v[u];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      int p, k;
      if (!task_of<S420>(i, tid, p, k)) continue;
      const int nbx = plane_nbx<S420>(p), y = k / nbx, bx = k - y * nbx;
      float* row = &pl[p][y][8 * bx];
      const f32x4 lo = ld4(row), hi = ld4(row + 4);
      float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      idct8(v);
      st4(row, f32x4{v[0], v[1], v[2], v[3]});
      st4(row + 4, f32x4{v[4], v[5], v[6], v[7]});
    }
    __syncthreads();
  }

  // epilogue, the patch of the prologue: box-mean transpose, step-2 masks, transposed RGB -> YCbCr, x 255, step-1 mask
  if (!in) return;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const f32x4 ly = ld4(&pl[0][2 * ty + r][4 * tx]);
    f32x4 lb, lr;
    if (S420) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lb[e] = 0.25f * pl[1][ty][2 * tx + (e >> 1)];
        lr[e] = 0.25f * pl[2][ty][2 * tx + (e >> 1)];
      }
    } else {
      lb = ld4(&pl[1][2 * ty + r][4 * tx]);
      lr = ld4(&pl[2][2 * ty + r][4 * tx]);
    }
    f32x4 o[3];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int bit = 4 * r + e;
      const float a = (m2 >> bit) & 1u ? ly[e] : 0.f, c = (m2 >> (8 + bit)) & 1u ? lb[e] : 0.f,
                  d = (m2 >> (16 + bit)) & 1u ? lr[e] : 0.f;
      const float gR = fmaf(0.5f, d, fmaf(-0.168736f, c, 0.299f * a));
      const float gG = fmaf(-0.418688f, d, fmaf(-0.331264f, c, 0.587f * a));
      const float gB = fmaf(-0.081312f, d, fmaf(0.5f, c, 0.114f * a));
      o[0][e] = (m1 >> bit) & 1u ? fmul_rn(gR, 255.f) : 0.f;
      o[1][e] = (m1 >> (8 + bit)) & 1u ? fmul_rn(gG, 255.f) : 0.f;
      o[2][e] = (m1 >> (16 + bit)) & 1u ? fmul_rn(gB, 255.f) : 0.f;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) st4(g_x + ((size_t)b * 3 + ch) * HW + (size_t)(py + r) * W + px, o[ch]);
  }
}

// 0 if (B, H, W, sub) is a supported problem: sub is 420 or 444, H and W multiples of the MCU (16 or 8)
int jpeg_check(int B, int H, int W, int sub) {
  if (sub != 420 && sub != 444) return -5;
  const int mcu = sub == 420 ? 16 : 8;
  if (B < 1 || B > 65535) return -5;       // B on grid.y / grid.z
  if (H < mcu || W < mcu || H % mcu || W % mcu) return -5;
  if ((long)H * W > 0x7fffffffL / 4 || (H + JP_TH - 1) / JP_TH > 65535) return -5;
  return 0;
}
int jpeg_blocks(int H, int W) { return capped_blocks((long)(W / 8) * (H / 2), JP_THREADS, JP_MAX_BLOCKS); }

// the workspace of `cand` decoded images per input image, in floats: the partials first (a multiple of 4, so the
// byte planes behind them start 16-byte aligned), then Y and the two chroma planes
size_t jpeg_part_floats(int B, int H, int W, int cand) { return ((size_t)B * cand * jpeg_blocks(H, W) + 3) / 4 * 4; }
size_t jpeg_plane_bytes(int H, int W, int sub) { return (size_t)H * W * (sub == 420 ? 3 : 6) / 2; }
size_t jpeg_ws_floats(int B, int H, int W, int sub, int cand) {
  if (jpeg_check(B, H, W, sub)) return 0;
  return jpeg_part_floats(B, H, W, cand) + (size_t)B * cand * jpeg_plane_bytes(H, W, sub) / 4;
}

template <bool SWEEP>
int jpeg_launch(const float* x, const float* tabs, int S, int B, int H, int W, int sub, const int* done,
                const float* ref, float* out, float* part, float* ws, hipStream_t st) {
  unsigned char* wsY = reinterpret_cast<unsigned char*>(ws + jpeg_part_floats(B, H, W, SWEEP ? JP_CHUNK : 1));
  unsigned char* wsC = wsY + (size_t)B * S * H * W;
  const dim3 tiles((W + JP_TW - 1) / JP_TW, (H + JP_TH - 1) / JP_TH, B), strips(jpeg_blocks(H, W), B);
  if (sub == 420) {
    ICA_LAUNCH((jpeg_blocks_kernel<true, SWEEP>), tiles, dim3(JP_THREADS), 0, st, x, tabs, S, H, W, done, wsY, wsC);
    ICA_CHECK_LAUNCH();
    ICA_LAUNCH((jpeg_colour_kernel<true, SWEEP>), strips, dim3(JP_THREADS), 0, st, ref, (const unsigned char*)wsY,
               (const unsigned char*)wsC, S, H, W, done, out, part);
  } else {
    ICA_LAUNCH((jpeg_blocks_kernel<false, SWEEP>), tiles, dim3(JP_THREADS), 0, st, x, tabs, S, H, W, done, wsY, wsC);
    ICA_CHECK_LAUNCH();
    ICA_LAUNCH((jpeg_colour_kernel<false, SWEEP>), strips, dim3(JP_THREADS), 0, st, ref, (const unsigned char*)wsY,
               (const unsigned char*)wsC, S, H, W, done, out, part);
  }
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int ica_jpeg_sweep_chunk(void) { return JP_CHUNK; }

size_t ica_jpeg_roundtrip_ws_size(int B, int H, int W, int sub) { return jpeg_ws_floats(B, H, W, sub, 1); }

int ica_jpeg_roundtrip(const float* x, const float* tabs, int B, int H, int W, int sub, const float* ref, float* out,
                       float* mse, float* ws, hipStream_t st) {
  const int rc = jpeg_check(B, H, W, sub);
  if (rc) return rc;
  if (!x || !tabs || !out || !ws || (ref && !mse) || (!ref && mse)) return -5;
  if (!aligned16(x) || !aligned16(out) || !aligned16(ref) || !aligned16(ws)) return -5;
  const size_t bytes = (size_t)B * 3 * H * W * sizeof(float);
  if (overlaps(x, bytes, out, bytes) || (ref && overlaps(ref, bytes, out, bytes))) return -7;
  const int rc2 = jpeg_launch<false>(x, tabs, 1, B, H, W, sub, nullptr, ref, out, ref ? ws : nullptr, ws, st);
  if (rc2) return rc2;
  if (ref) {
    finish_rows(st, ws, B, jpeg_blocks(H, W), (float)((long)3 * H * W), mse);
    ICA_CHECK_LAUNCH();
  }
  return 0;
}

// workspace of the backward, in floats: gY [B][H][W], gC [B][2][Hc][Wc], then the decoded byte planes
size_t ica_jpeg_roundtrip_bwd_ws_size(int B, int H, int W, int sub) {
  if (jpeg_check(B, H, W, sub)) return 0;
  return (size_t)B * H * W * (sub == 420 ? 3 : 6) / 2 + (size_t)B * jpeg_plane_bytes(H, W, sub) / 4;
}

int ica_jpeg_roundtrip_bwd(const float* x, const float* tabs, const float* g_out, int B, int H, int W, int sub,
                           int surrogate, float* g_x, float* ws, hipStream_t st) {
  const int rc = jpeg_check(B, H, W, sub);
  if (rc) return rc;
  if (surrogate != JP_STE && surrogate != JP_CUBIC) return -5;
  if (!x || !tabs || !g_out || !g_x || !ws) return -5;
  if (!aligned16(x) || !aligned16(g_out) || !aligned16(g_x) || !aligned16(ws)) return -5;
  const size_t bytes = (size_t)B * 3 * H * W * sizeof(float);
  if (overlaps(x, bytes, g_x, bytes) || overlaps(g_out, bytes, g_x, bytes)) return -7;
  const size_t HW = (size_t)H * W, CHW = sub == 420 ? HW / 4 : HW;
  float* gY = ws;
  float* gC = gY + (size_t)B * HW;
  unsigned char* wsY = reinterpret_cast<unsigned char*>(gC + (size_t)B * 2 * CHW);
  unsigned char* wsC = wsY + (size_t)B * HW;
  const dim3 tiles((W + JP_TW - 1) / JP_TW, (H + JP_TH - 1) / JP_TH, B), threads(JP_THREADS);
  const int* none = nullptr;
#define JPEG_BWD(S420, CUBIC)                                                                                    \
  ICA_LAUNCH((jpeg_blocks_kernel<S420, false>), tiles, threads, 0, st, x, tabs, 1, H, W, none, wsY, wsC);          \
  ICA_CHECK_LAUNCH();                                                                                             \
  ICA_LAUNCH((jpeg_colour_bwd_kernel<S420>), tiles, threads, 0, st, g_out, (const unsigned char*)wsY,              \
             (const unsigned char*)wsC, H, W, gY, gC);                                                            \
  ICA_CHECK_LAUNCH();                                                                                             \
  ICA_LAUNCH((jpeg_blocks_bwd_kernel<S420, CUBIC>), tiles, threads, 0, st, x, tabs, H, W, (const float*)gY,        \
             (const float*)gC, g_x);                                                                              \
  ICA_CHECK_LAUNCH()
  if (sub == 420) {
    if (surrogate == JP_CUBIC) { JPEG_BWD(true, true); } else { JPEG_BWD(true, false); }
  } else {
    if (surrogate == JP_CUBIC) { JPEG_BWD(false, true); } else { JPEG_BWD(false, false); }
  }
#undef JPEG_BWD
  return 0;
}

size_t ica_jpeg_sweep_ws_size(int B, int H, int W, int sub) { return jpeg_ws_floats(B, H, W, sub, JP_CHUNK); }

int ica_jpeg_sweep(const float* x, const float* tabs, int S, int B, int H, int W, int sub, float budget, int s0,
                   float* mse, long ld, int* idx, int* done, int* remaining, float* ws, hipStream_t st) {
  const int rc = jpeg_check(B, H, W, sub);
  if (rc) return rc;
  if (S < 1 || S > JP_CHUNK || s0 < 0 || ld < (long)s0 + S) return -5;
  if (!x || !tabs || !mse || !idx || !done || !remaining || !ws || !aligned16(x) || !aligned16(ws)) return -5;
  const int rc2 = jpeg_launch<true>(x, tabs, S, B, H, W, sub, done, x, nullptr, ws, ws, st);
  if (rc2) return rc2;
  finish_rows(st, ws, B * S, jpeg_blocks(H, W), (float)((long)3 * H * W), mse, S, ld, s0, done);
  ICA_CHECK_LAUNCH();
  ICA_LAUNCH(sweep_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, st, (const float*)mse, ld, s0, S, budget, B, idx,
             done, remaining);
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
