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
// Arithmetic: fp32.  The 8-point DCT is the even-odd factorisation with the constants 0.5 cos(k pi / 16); rows first,
// then columns, and the inverse in the opposite order.  A decoded chroma sample is an integer, so the triangle filter
// (9 a + 3 b + 3 c + d) / 16 is exact in any order.
//
// A block of jpeg_blocks_kernel stages a 64 x 32 pixel tile (whole MCUs: H and W are multiples of the MCU) as three
// fp32 planes in LDS.  Eight threads share an 8x8 block: one per row in the row passes, one per column in the column
// pass, so the column pass reads 64 consecutive floats per eight blocks and the row passes read 16-byte quads.
//
// Reductions: ica_reduce.h (sequential block order; JP_MAX_BLOCKS caps the partials of an image).
#include "ica_reduce.h"

namespace {

constexpr int JP_THREADS = 256;
constexpr int JP_TW = 64;                  // tile width: 16 threads x 4 pixels, 8 blocks
constexpr int JP_TH = 32;                  // tile height: 16 threads x 2 rows, 4 blocks
constexpr int JP_CHUNK = 8;                // candidates per sweep launch (their decoded planes live in the workspace)
constexpr int JP_MAX_BLOCKS = 1024;
constexpr int JP_TAB = 128;                // floats per table pair: luminance [64], chrominance [64], row-major

// 0.5 cos(k pi / 16); C4 is also sqrt(1 / 8), the scale of the DC row
constexpr float C1 = 0.49039264020161522f, C2 = 0.46193976625564337f, C3 = 0.41573480615127262f,
                C4 = 0.35355339059327376f, C5 = 0.27778511650980111f, C6 = 0.19134171618254489f,
                C7 = 0.09754516100806413f;

// the orthonormal 8-point DCT-II, in place
ICA_DEV void dct8(float (&v)[8]) {
  const float s0 = v[0] + v[7], s1 = v[1] + v[6], s2 = v[2] + v[5], s3 = v[3] + v[4];
  const float d0 = v[0] - v[7], d1 = v[1] - v[6], d2 = v[2] - v[5], d3 = v[3] - v[4];
  const float a = s0 + s3, b = s1 + s2, c = s0 - s3, d = s1 - s2;
  v[0] = C4 * (a + b);
  v[4] = C4 * (a - b);
  v[2] = C2 * c + C6 * d;
  v[6] = C6 * c - C2 * d;
  v[1] = C1 * d0 + C3 * d1 + C5 * d2 + C7 * d3;
  v[3] = C3 * d0 - C7 * d1 - C1 * d2 - C5 * d3;
  v[5] = C5 * d0 - C1 * d1 + C7 * d2 + C3 * d3;
  v[7] = C7 * d0 - C5 * d1 + C3 * d2 - C1 * d3;
}

// its inverse (the transpose), in place
ICA_DEV void idct8(float (&v)[8]) {
  const float a = C4 * (v[0] + v[4]), b = C4 * (v[0] - v[4]);
  const float c = C2 * v[2] + C6 * v[6], d = C6 * v[2] - C2 * v[6];
  const float e0 = a + c, e1 = b + d, e2 = b - d, e3 = a - c;
  const float o0 = C1 * v[1] + C3 * v[3] + C5 * v[5] + C7 * v[7];
  const float o1 = C3 * v[1] - C7 * v[3] - C1 * v[5] - C5 * v[7];
  const float o2 = C5 * v[1] - C1 * v[3] + C7 * v[5] + C3 * v[7];
  const float o3 = C7 * v[1] - C5 * v[3] + C3 * v[5] - C1 * v[7];
  v[0] = e0 + o0;
  v[7] = e0 - o0;
  v[1] = e1 + o1;
  v[6] = e1 - o1;
  v[2] = e2 + o2;
  v[5] = e2 - o2;
  v[3] = e3 + o3;
  v[4] = e3 - o3;
}

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
