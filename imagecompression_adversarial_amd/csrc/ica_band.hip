// Frequency bands of a perturbation (DESIGN.md "Band VI") on planar NCHW fp32 tensors [B][3][H][W], H and W multiples
// of 8.  The transform is the orthonormal 8x8 block DCT-II of every channel plane (ica_dct8.h), blocks aligned to the
// image origin; coefficient (u, v) of a block belongs to band max(u, v) = 0..7; a band set is an 8-bit mask S and
//
//   P_S = IDCT . [band in S] . DCT          (symmetric, idempotent, block-local; the eight P_{k} sum to I)
//
//   band_split_kernel      n = im_adv - im_s: the band energies |P_{k} n|^2 (from the coefficients) and, per mask of
//                          the chunk, clamp01(im_s + P_S n) with its mean((x - im_s)^2).  The forward DCT is computed
//                          once and stays in registers; a variant costs a mask, the inverse DCT, an add, a clamp, a
//                          store and its squared-error chain.
//   band_project_kernel    y = P_S x
//   band_prologue_kernel   the attack prologue with p = P_S(clip(noise)) in place of clip(noise)
//   band_adam_kernel       the attack's Adam kernel with the transpose: the gradient is projected between the
//                          bound-backward at im_s + p and the one at the noise
//
// All four run the same four device functions (rows_fwd, cols_fwd, cols_inv, rows_inv) on one LDS layout.  They and
// the DCT pair they call are compiled with floating-point contraction off: every operation of the transform is then
// one correctly rounded fp32 operation in source order, and the compiler has no choice left that could depend on the
// kernel the functions are inlined into (with contraction on, the prologue's im_in differed from the composition
// in the last bit of 710 of 58752 values of a 2 x 3 x 72 x 136 case).  So a fused kernel gives the bits of the
// composition of ica_band_project with the per-pixel kernels of ica_elem.hip, whose pinned operation order the
// per-pixel halves copy.
//
// A block takes 64 x 32 pixel tiles of one image (tile t, t + gridDim.x, ...), three fp32 planes in LDS.  Eight threads
// share an 8x8 block.  Thread tid is the row task (row tid / 8 of the tile, block column tid % 8): it loads its eight
// pixels of each plane from memory as two 16-byte quads, runs the row transform in registers and owns those pixels
// again after the inverse, so the per-pixel operands (im_s, the noise) stay in its registers across the transform.
// It is also the column task (block row tid / 64, column tid % 64), which reads 64 consecutive floats per wave.  A
// plane row is padded to 68 floats: the 16-byte row accesses of two tile rows (lanes l and l + 8) then start four
// banks apart instead of on the same bank.  LDS: 3 x 32 x 68 x 4 B = 26112 B, plus 16 B for the block sums.
//
// Reductions: ica_reduce.h (sequential block order, one partial per block and row, finish_rows); the number of
// blocks of an image depends on its size only (BD_MAX_BLOCKS) and no float atomic is used, so a row's numbers are the
// same bits alone and in a batch, run to run.
#pragma clang fp contract(off)   // the transform: up to the matching pragma below
#include "ica_dct8.h"
#include "ica_reduce.h"

namespace {

constexpr int BD_THREADS = 256;
constexpr int BD_TW = 64;                  // tile width: 8 blocks
constexpr int BD_TH = 32;                  // tile height: 4 blocks
constexpr int BD_LD = 68;                  // floats per plane row in LDS (64 + 4 of padding, rows stay 16-byte aligned)
constexpr int BD_CHUNK = 8;                // variants per split launch (the masks travel by value)
constexpr int BD_MAX_V = 256;              // variants per ica_band_split call: every mask once
constexpr int BD_MAX_BLOCKS = 1024;        // blocks per image

struct BandMasks {
  int m[BD_CHUNK];
};

typedef float BandPlanes[3][BD_TH][BD_LD];

// where the row task of thread tid stands in the image for tile t; false if its eight pixels lie outside (H and W are
// multiples of 8: they are all inside or all outside)
ICA_DEV bool row_task_at(int t, int tilesX, int tid, int H, int W, int& gy, int& gx) {
  const int ty = t / tilesX, tx = t - ty * tilesX;
  gy = ty * BD_TH + (tid >> 3);
  gx = tx * BD_TW + 8 * (tid & 7);
  return gy < H && gx < W;
}

ICA_DEV void load8(const float* p, bool in, float (&v)[8]) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const f32x4 lo = in ? ld4(p) : z, hi = in ? ld4(p + 4) : z;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = lo[e];
    v[4 + e] = hi[e];
  }
}

ICA_DEV void store8(float* p, const float (&v)[8]) {
  st4(p, f32x4{v[0], v[1], v[2], v[3]});
  st4(p + 4, f32x4{v[4], v[5], v[6], v[7]});
}

// forward rows: the row task transforms its eight samples of each plane and puts them into the tile
ICA_DEV void rows_fwd(BandPlanes& pl, int tid, float (&v)[3][8]) {
  const int y = tid >> 3, bx = tid & 7;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    dct8(v[p]);
    store8(&pl[p][y][8 * bx], v[p]);
  }
}

// forward columns: the coefficients (u, v = column % 8), u = 0..7, of the column task stay in registers
ICA_DEV void cols_fwd(const BandPlanes& pl, int tid, float (&coef)[3][8]) {
  const int by = tid >> 6, xx = tid & 63;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
#pragma unroll
    for (int u = 0; u < 8; ++u) coef[p][u] = pl[p][8 * by + u][xx];
    dct8(coef[p]);
  }
}

// the band mask and the inverse columns.  A column task is the only one that touches its column between cols_fwd
// and the barrier after this.
ICA_DEV void cols_inv(BandPlanes& pl, int tid, const float (&coef)[3][8], int mask) {
  const int by = tid >> 6, xx = tid & 63, vq = xx & 7;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    float w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) w[u] = ((mask >> max(u, vq)) & 1) ? coef[p][u] : 0.f;
    idct8(w);
#pragma unroll
    for (int u = 0; u < 8; ++u) pl[p][8 * by + u][xx] = w[u];
  }
}

// inverse rows: the row task gets its eight samples of each plane back
ICA_DEV void rows_inv(const BandPlanes& pl, int tid, float (&v)[3][8]) {
  const int y = tid >> 3, bx = tid & 7;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const float* row = &pl[p][y][8 * bx];
    const f32x4 lo = ld4(row), hi = ld4(row + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[p][e] = lo[e];
      v[p][4 + e] = hi[e];
    }
    idct8(v[p]);
  }
}

// v <- P_mask v for the tile whose row-task samples are v.  Ends with the planes free to be written again.
ICA_DEV void project_tile(BandPlanes& pl, int tid, float (&v)[3][8], int mask) {
  float coef[3][8];
  rows_fwd(pl, tid, v);
  __syncthreads();
  cols_fwd(pl, tid, coef);
  cols_inv(pl, tid, coef, mask);
  __syncthreads();
  rows_inv(pl, tid, v);
  __syncthreads();
}

#pragma clang fp contract(fast)   // the per-pixel halves and the reductions: the build's default, as in ica_elem.hip

// epart [B][8][gridDim.x] (null: no energies), mpart [V][B][gridDim.x] with the chunk's variants at v0 .. v0 + S - 1,
// out [V][B][3][H][W]
__global__ __launch_bounds__(BD_THREADS) void band_split_kernel(const float* __restrict__ im_s,
                                                                const float* __restrict__ im_adv, BandMasks masks,
                                                                int S, int v0, int H, int W, int tilesX, int tiles,
                                                                float* __restrict__ out, float* __restrict__ epart,
                                                                float* __restrict__ mpart) {
  __shared__ __attribute__((aligned(16))) BandPlanes pl;
  __shared__ float red[4];
  const int b = blockIdx.y, B = gridDim.y, tid = threadIdx.x;
  const size_t HW = (size_t)H * W;
  float en[8], sd[BD_CHUNK];
#pragma unroll
  for (int k = 0; k < 8; ++k) en[k] = 0.f;
#pragma unroll
  for (int s = 0; s < BD_CHUNK; ++s) sd[s] = 0.f;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    int gy, gx;
    const bool in = row_task_at(t, tilesX, tid, H, W, gy, gx);
    const size_t at = (size_t)b * 3 * HW + (size_t)gy * W + gx;   // plane 0
    float sv[3][8], v[3][8];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      float a[8];
      load8(im_s + at + p * HW, in, sv[p]);
      load8(im_adv + at + p * HW, in, a);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[p][e] = fsub_rn(a[e], sv[p][e]);
    }
    float coef[3][8];
    rows_fwd(pl, tid, v);
    __syncthreads();
    cols_fwd(pl, tid, coef);
    if (epart) {   // block-uniform.  Column v = vq holds bands max(u, vq): u <= vq in band vq, the others in band u
      const int vq = tid & 7;
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        float low = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float c = coef[p][u];
          low = u <= vq ? fmaf(c, c, low) : low;
          en[u] = u > vq ? fmaf(c, c, en[u]) : en[u];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) en[k] = k == vq ? fadd_rn(en[k], low) : en[k];
      }
    }
#pragma unroll
    for (int s = 0; s < BD_CHUNK; ++s) {
      if (s >= S) break;
      cols_inv(pl, tid, coef, masks.m[s]);
      __syncthreads();
      rows_inv(pl, tid, v);
      if (in) {
        float* o = out + ((size_t)(v0 + s) * B + b) * 3 * HW + (size_t)gy * W + gx;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          float x[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            x[e] = clamp01(fadd_rn(sv[p][e], v[p][e]));
            const float d = fsub_rn(x[e], sv[p][e]);
            sd[s] = fmaf(d, d, sd[s]);
          }
          store8(o + p * HW, x);
        }
      }
      __syncthreads();   // the next variant, or the next tile, overwrites the planes
    }
    if (S == 0) __syncthreads();   // block-uniform: the next tile's rows_fwd overwrites what cols_fwd read
  }
  if (epart) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float total = block_sum(en[k], red);
      if (tid == 0) epart[((size_t)b * 8 + k) * gridDim.x + blockIdx.x] = total;
    }
  }
#pragma unroll
  for (int s = 0; s < BD_CHUNK; ++s) {
    if (s >= S) break;
    const float total = block_sum(sd[s], red);
    if (tid == 0) mpart[((size_t)(v0 + s) * B + b) * gridDim.x + blockIdx.x] = total;
  }
}

__global__ __launch_bounds__(BD_THREADS) void band_project_kernel(const float* __restrict__ x, int mask, int H, int W,
                                                                  int tilesX, int tiles, float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) BandPlanes pl;
  const int b = blockIdx.y, tid = threadIdx.x;
  const size_t HW = (size_t)H * W;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    int gy, gx;
    const bool in = row_task_at(t, tilesX, tid, H, W, gy, gx);
    const size_t at = (size_t)b * 3 * HW + (size_t)gy * W + gx;
    float v[3][8];
#pragma unroll
    for (int p = 0; p < 3; ++p) load8(x + at + p * HW, in, v[p]);
    project_tile(pl, tid, v, mask);
    if (in) {
#pragma unroll
      for (int p = 0; p < 3; ++p) store8(y + at + p * HW, v[p]);
    }
  }
}

// nc = Up(Low(noise, -eps), eps); p = P_S(nc); im_in = Up(Low(im_s + p, 0), 1) -> im_in4 (nChw4c, lane 3 = 0) and
// the partial sums of (im_s - im_in)^2: part [B][gridDim.x].  Per pixel as attack_prologue_kernel (ica_elem.hip).
__global__ __launch_bounds__(BD_THREADS) void band_prologue_kernel(const float* __restrict__ noise,
                                                                   const float* __restrict__ im_s, int mask, float eps,
                                                                   int H, int W, int tilesX, int tiles,
                                                                   float* __restrict__ im_in4,
                                                                   float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) BandPlanes pl;
  __shared__ float red[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const size_t HW = (size_t)H * W;
  float acc = 0.f;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    int gy, gx;
    const bool in = row_task_at(t, tilesX, tid, H, W, gy, gx);
    const size_t pix = (size_t)gy * W + gx, at = (size_t)b * 3 * HW + pix;
    float sv[3][8], v[3][8];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      load8(im_s + at + p * HW, in, sv[p]);
      load8(noise + at + p * HW, in, v[p]);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[p][e] = fminf(fmaxf(v[p][e], -eps), eps);
    }
    project_tile(pl, tid, v, mask);
    if (in) {
      float* o4 = im_in4 + ((size_t)b * HW + pix) * 4;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const float s = sv[p][e];
          const float u = fadd_rn(s, v[p][e]);
          const float ii = fminf(fmaxf(u, 0.f), 1.f);
          q[p] = ii;
          const float d = fsub_rn(s, ii);
          acc = fadd_rn(acc, fmul_rn(d, d));
        }
        st4(o4 + 4 * e, q);
      }
    }
  }
  const float total = block_sum(acc, red);
  if (tid == 0) part[(size_t)b * gridDim.x + blockIdx.x] = total;
}

// Branch select, the transpose of the prologue and torch's Adam step on the noise, in place; per pixel as
// attack_adam_kernel (ica_elem.hip) at clamp_in = 1 without a supplied cheap gradient:
//   cheap[b] = loss_i[b] > thr -> g = -2 fl(invN (im_s - im_in)), else g = g_net (nChw4c, lane 3 never read into g)
//   g = bound-bwd at u = im_s + p against [0, 1];  g = P_S g;  g = bound-bwd at the noise against +-eps;  Adam
// gpos, census, branch, im_in_out: as there.
__global__ __launch_bounds__(BD_THREADS) void band_adam_kernel(float* __restrict__ noise,
                                                               const float* __restrict__ im_s,
                                                               const float* __restrict__ gnet4,
                                                               const float* __restrict__ loss_i,
                                                               float* __restrict__ m, float* __restrict__ v,
                                                               float* __restrict__ im_in_out, int mask, int H, int W,
                                                               int tilesX, int tiles, float eps, float thr, float invN,
                                                               float bc2s, float neg_step, int* __restrict__ branch,
                                                               const int* __restrict__ gpos,
                                                               int* __restrict__ census) {
  __shared__ __attribute__((aligned(16))) BandPlanes pl;
  const int b = blockIdx.y, tid = threadIdx.x;
  const bool cheap = loss_i[b] > thr;
  if (blockIdx.x == 0 && tid == 0) {
    if (branch) branch[b] = cheap ? 1 : 0;
    if (census) census[b] += cheap ? 1 : 0;
  }
  const size_t HW = (size_t)H * W;
  const size_t grow = cheap ? 0 : (size_t)(gpos ? gpos[b] : b);   // the network gradient is read only when used
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    int gy, gx;
    const bool in = row_task_at(t, tilesX, tid, H, W, gy, gx);
    const size_t pix = (size_t)gy * W + gx, at = (size_t)b * 3 * HW + pix;
    float nz[3][8], sv[3][8], g[3][8];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      load8(im_s + at + p * HW, in, sv[p]);
      load8(noise + at + p * HW, in, nz[p]);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[p][e] = fminf(fmaxf(nz[p][e], -eps), eps);
    }
    project_tile(pl, tid, g, mask);   // g = p
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f32x4 gn = {0.f, 0.f, 0.f, 0.f};
      if (!cheap && in) gn = ld4(gnet4 + (grow * HW + pix + e) * 4);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const float s = sv[p][e];
        const float u = fadd_rn(s, g[p][e]);
        const float lowU = fmaxf(u, 0.f);
        const float ii = fminf(lowU, 1.f);
        float gg;
        if (cheap) {
          const float tt = fmul_rn(invN, fsub_rn(s, ii));
          gg = -fadd_rn(tt, tt);
        } else {
          gg = gn[p];
        }
        gg = (lowU <= 1.f || gg > 0.f) ? gg : gg * 0.f;
        gg = (u >= 0.f || gg < 0.f) ? gg : gg * 0.f;
        sv[p][e] = ii;          // im_s is not needed again
        g[p][e] = in ? gg : 0.f;
      }
    }
    if (im_in_out && in) {
#pragma unroll
      for (int p = 0; p < 3; ++p) store8(im_in_out + at + p * HW, sv[p]);
    }
    project_tile(pl, tid, g, mask);   // the projection is symmetric: its transpose is itself
    if (in) {
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        float mo[8], vo[8], no[8];
        load8(m + at + p * HW, true, mo);
        load8(v + at + p * HW, true, vo);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float z = nz[p][e];
          const float lowN = fmaxf(z, -eps);
          float gg = g[p][e];
          gg = (lowN <= eps || gg > 0.f) ? gg : gg * 0.f;
          gg = (z >= -eps || gg < 0.f) ? gg : gg * 0.f;
          const float mn = __fmaf_rn(0.1f, fsub_rn(gg, mo[e]), mo[e]);
          const float vn = fadd_rn(fmul_rn(vo[e], 0.999f), fmul_rn(fmul_rn(0.001f, gg), gg));
          const float denom = fadd_rn(fdiv_rn(sqrtf(vn), bc2s), 1e-8f);
          mo[e] = mn;
          vo[e] = vn;
          no[e] = fadd_rn(z, fmul_rn(neg_step, fdiv_rn(mn, denom)));
        }
        store8(m + at + p * HW, mo);
        store8(v + at + p * HW, vo);
        store8(noise + at + p * HW, no);
      }
    }
  }
}

// 0 if B images of H x W are a supported problem
int band_check(int B, int H, int W) {
  if (B < 1 || B > 65535) return -5;       // B on grid.y
  if (H < 8 || W < 8 || H % 8 || W % 8) return -5;
  if ((long)H * W > 0x7fffffffL / 4) return -5;
  return 0;
}
int band_tiles_x(int W) { return (W + BD_TW - 1) / BD_TW; }
int band_tiles(int H, int W) { return band_tiles_x(W) * ((H + BD_TH - 1) / BD_TH); }
int band_blocks(int H, int W) { return capped_blocks(band_tiles(H, W), 1, BD_MAX_BLOCKS); }

}  // namespace

extern "C" {

int ica_band_split_chunk(void) { return BD_CHUNK; }
int ica_band_max_variants(void) { return BD_MAX_V; }

// floats: the energy partials [B][8][blocks], then the mse_in partials [V][B][blocks]
size_t ica_band_split_ws_size(int V, int B, int H, int W) {
  if (band_check(B, H, W) || V < 1 || V > BD_MAX_V) return 0;
  return (size_t)(8 + V) * B * band_blocks(H, W);
}

int ica_band_split(const float* im_s, const float* im_adv, const int* masks, int V, int B, int H, int W, float* out,
                   float* energy, float* mse_in, float* ws, hipStream_t st) {
  const int rc = band_check(B, H, W);
  if (rc) return rc;
  if (V < 1 || V > BD_MAX_V) return -5;
  if (!im_s || !im_adv || !energy || !ws || (out && !masks) || (!out && mse_in)) return -5;
  if (!aligned16(im_s) || !aligned16(im_adv) || !aligned16(out)) return -5;
  if (out) {
    for (int i = 0; i < V; ++i)
      if (masks[i] < 0 || masks[i] > 0xFF) return -5;
    const size_t bytes = (size_t)B * 3 * H * W * sizeof(float);
    if (overlaps(out, (size_t)V * bytes, im_s, bytes) || overlaps(out, (size_t)V * bytes, im_adv, bytes)) return -7;
  }
  const int nb = band_blocks(H, W), tilesX = band_tiles_x(W), tiles = band_tiles(H, W);
  float* epart = ws;
  float* mpart = ws + (size_t)8 * B * nb;
  const dim3 grid(nb, B), threads(BD_THREADS);
  for (int v0 = 0; v0 < (out ? V : 1); v0 += BD_CHUNK) {
    BandMasks mk = {};
    const int S = out ? (V - v0 < BD_CHUNK ? V - v0 : BD_CHUNK) : 0;
    for (int s = 0; s < S; ++s) mk.m[s] = masks[v0 + s];
    ICA_LAUNCH(band_split_kernel, grid, threads, 0, st, im_s, im_adv, mk, S, v0, H, W, tilesX, tiles, out,
               v0 == 0 ? epart : (float*)nullptr, mpart);
    ICA_CHECK_LAUNCH();
  }
  const float count = (float)((long)3 * H * W);
  finish_rows(st, epart, B * 8, nb, count, energy);
  ICA_CHECK_LAUNCH();
  if (out && mse_in) {
    finish_rows(st, mpart, V * B, nb, count, mse_in);
    ICA_CHECK_LAUNCH();
  }
  return 0;
}

int ica_band_project(const float* x, int mask, int B, int H, int W, float* y, hipStream_t st) {
  const int rc = band_check(B, H, W);
  if (rc) return rc;
  if (mask < 0 || mask > 0xFF || !x || !y || !aligned16(x) || !aligned16(y)) return -5;
  const size_t bytes = (size_t)B * 3 * H * W * sizeof(float);
  if (overlaps(x, bytes, y, bytes)) return -7;
  ICA_LAUNCH(band_project_kernel, dim3(band_blocks(H, W), B), dim3(BD_THREADS), 0, st, x, mask, H, W,
             band_tiles_x(W), band_tiles(H, W), y);
  ICA_CHECK_LAUNCH();
  return 0;
}

// floats: the loss_i partials [B][blocks]
size_t ica_band_prologue_ws_size(int B, int H, int W) {
  if (band_check(B, H, W)) return 0;
  return (size_t)B * band_blocks(H, W);
}

int ica_band_prologue(const float* noise, const float* im_s, float* im_in4, float* loss_i, int B, int H, int W,
                      float eps, int mask, float* ws, hipStream_t st) {
  const int rc = band_check(B, H, W);
  if (rc) return rc;
  if (mask < 0 || mask > 0xFF || !noise || !im_s || !im_in4 || !loss_i || !ws) return -5;
  if (!aligned16(noise) || !aligned16(im_s) || !aligned16(im_in4)) return -5;
  const size_t bytes = (size_t)B * 3 * H * W * sizeof(float), bytes4 = (size_t)B * 4 * H * W * sizeof(float);
  if (overlaps(im_in4, bytes4, noise, bytes) || overlaps(im_in4, bytes4, im_s, bytes)) return -7;
  const int nb = band_blocks(H, W);
  ICA_LAUNCH(band_prologue_kernel, dim3(nb, B), dim3(BD_THREADS), 0, st, noise, im_s, mask, eps, H, W,
             band_tiles_x(W), band_tiles(H, W), im_in4, ws);
  ICA_CHECK_LAUNCH();
  finish_rows(st, ws, B, nb, (float)((long)3 * H * W), loss_i);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_band_adam(float* noise, const float* im_s, const float* gnet4, const float* loss_i, float* m, float* v,
                  float* im_in_out, int B, int H, int W, float eps, float thr, float invN, float bc2s, float neg_step,
                  int* branch, const int* gpos, int* census, int mask, hipStream_t st) {
  const int rc = band_check(B, H, W);
  if (rc) return rc;
  if (mask < 0 || mask > 0xFF || !noise || !im_s || !loss_i || !m || !v) return -5;   // gnet4: null if all cheap
  if (!aligned16(noise) || !aligned16(im_s) || !aligned16(gnet4) || !aligned16(m) || !aligned16(v) ||
      !aligned16(im_in_out))
    return -5;
  const size_t bytes = (size_t)B * 3 * H * W * sizeof(float);
  float* outs[4] = {noise, m, v, im_in_out};
  for (int o = 0; o < 4; ++o) {
    if (!outs[o]) continue;
    if (overlaps(outs[o], bytes, im_s, bytes)) return -7;
    if (gnet4 && overlaps(outs[o], bytes, gnet4, (size_t)16)) return -7;   // its extent depends on gpos: its start
    for (int q = o + 1; q < 4; ++q)
      if (outs[q] && overlaps(outs[o], bytes, outs[q], bytes)) return -7;
  }
  ICA_LAUNCH(band_adam_kernel, dim3(band_blocks(H, W), B), dim3(BD_THREADS), 0, st, noise, im_s, gnet4, loss_i, m, v,
             im_in_out, mask, H, W, band_tiles_x(W), band_tiles(H, W), eps, thr, invN, bc2s, neg_step, branch, gpos,
             census);
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
