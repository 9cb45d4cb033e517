// C&W-style binary-search attack (the reference's second attack family), per-image semantics: every image of
// the batch follows the trajectory of its own B == 1 reference run, with the whole search state on the device.
//
// Reference anchors:
//   step loss + gate                  attack_cw.py:115-140      (attack_cw_fast.py:100-125)
//   step loop, Adam, bisection on c   attack_cw.py:142-199      (search_noise; attack_cw_fast.py:127-183)
//   outer search on the level         attack_cw.py:238-259      (attack_; attack_cw_fast.py:222-243)
//   bounds pass-through               utils/ops.py:28-56
//
// Per-image state (device tensors the host allocates; field-major, field f of image b at [f * B + b]):
//   sd   double [6][B]   c_l, c_r, c, level, min, max             (Python floats in the reference)
//   lold float  [B]      loss_i_old                               (fp32 tensor in the reference)
//   si   int    [5][B]   t (Adam steps of the current level), round (rounds done in the level),
//                        levels (levels completed), active, reset
// loss_i and mse_o are fp32 and are compared against the double thresholds rounded to fp32, as torch compares
// a fp32 tensor with a Python scalar.
#include "ica_reduce.h"

enum { CW_CL = 0, CW_CR = 1, CW_C = 2, CW_LEVEL = 3, CW_MIN = 4, CW_MAX = 5 };
enum { CW_T = 0, CW_ROUND = 1, CW_LEVELS = 2, CW_ACTIVE = 3, CW_RESET = 4 };

// mse_o[b] = invN * sum_k part[b][k] in reduce_rows_kernel's order (strided slices, then the paired block_sum of
// ica_reduce.h), then the gate on the loss weight and the image's Adam step count.  One block per image.
__global__ void cw_gate_kernel(const float* __restrict__ part, int nblk, float invN, const double* __restrict__ sd,
                               int* __restrict__ si, float* __restrict__ mse_o, float* __restrict__ c_eff, int B) {
  __shared__ float sh[4];
  const int b = blockIdx.x;
  float v = 0.f;
  for (int k = threadIdx.x; k < nblk; k += 256) v += part[(long)b * nblk + k];
  const float sum = block_sum_paired(v, sh);
  if (threadIdx.x != 0) return;
  const int active = si[CW_ACTIVE * B + b];
  if (!active) {   // a finished image keeps its last mse_o; its Adam launch is skipped
    c_eff[b] = 0.f;
    return;
  }
  const float mse = sum * invN;
  mse_o[b] = mse;
  c_eff[b] = mse > (float)(sd[CW_LEVEL * B + b] * 1.1) ? 0.f : (float)sd[CW_C * B + b];
  si[CW_T * B + b] += 1;
}

// Fused step update of the active images: g = d loss_i / d im_in + c_eff[b] * gnet (gnet: the network's gradient
// of loss_o at unit weight; the backward is linear in it and c >= 0 keeps the sign the bound gates read), the
// [0, 1] and +-eps pass-through gates on the summed gradient, then the torch-Adam update in attack_adam_kernel's
// op order.  (bc2s, neg_step) come from tab[t[b] - 1].  HW % 4 == 0: 16-byte accesses on every plane.
__global__ void cw_adam_kernel(float* __restrict__ noise, const float* __restrict__ im_s,
                               const float* __restrict__ gnet4, const float* __restrict__ c_eff,
                               float* __restrict__ m, float* __restrict__ v, float* __restrict__ im_in_out, long HW,
                               float eps, float invN, const f32x2* __restrict__ tab, int ntab,
                               const int* __restrict__ si, int B, int clamp_in) {
  const int b = blockIdx.y;
  if (!si[CW_ACTIVE * B + b]) return;
  const int ti = min(max(si[CW_T * B + b] - 1, 0), ntab - 1);
  const f32x2 sc = tab[ti];
  const float bc2s = sc[0], neg_step = sc[1];
  const float ce = c_eff[b];
  const long off = (long)b * 3 * HW;
  const long HW4 = HW >> 2;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < HW4; q += (long)gridDim.x * 256) {
    const long pix0 = q * 4;
    f32x4 gn[4] = {};
    if (ce != 0.f) {   // a gated image's network gradient has weight 0: not read
#pragma unroll
      for (int k = 0; k < 4; ++k) gn[k] = ld4(gnet4 + ((long)b * HW + pix0 + k) * 4);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long i0 = off + c * HW + pix0;
      const f32x4 nz4 = ld4(noise + i0), s4 = ld4(im_s + i0), m4 = ld4(m + i0), v4 = ld4(v + i0);
      f32x4 no, mo, vo, io;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float nz = nz4[k], s = s4[k];
        const float lowN = fmaxf(nz, -eps);
        const float nc = fminf(lowN, eps);
        const float u = fadd_rn(s, nc);
        const float lowU = clamp_in ? fmaxf(u, 0.f) : u;
        const float ii = clamp_in ? fminf(lowU, 1.f) : u;
        io[k] = ii;
        const float t = fmul_rn(invN, fsub_rn(s, ii));
        float g = fadd_rn(-fadd_rn(t, t), fmul_rn(ce, gn[k][c]));
        if (clamp_in) {
          g = (lowU <= 1.f || g > 0.f) ? g : g * 0.f;
          g = (u >= 0.f || g < 0.f) ? g : g * 0.f;
        }
        g = (lowN <= eps || g > 0.f) ? g : g * 0.f;
        g = (nz >= -eps || g < 0.f) ? g : g * 0.f;
        const float mn = __fmaf_rn(0.1f, fsub_rn(g, m4[k]), m4[k]);
        const float vn = fadd_rn(fmul_rn(v4[k], 0.999f), fmul_rn(fmul_rn(0.001f, g), g));
        const float denom = fadd_rn(fdiv_rn(sqrtf(vn), bc2s), 1e-8f);
        mo[k] = mn;
        vo[k] = vn;
        no[k] = fadd_rn(nz, fmul_rn(neg_step, fdiv_rn(mn, denom)));
      }
      if (im_in_out) st4(im_in_out + i0, io);
      st4(m + i0, mo);
      st4(v + i0, vo);
      st4(noise + i0, no);
    }
  }
}

// End of a round (every `steps` steps): bisection on c with the last step's mse_o, end of level, outer search
// on the level with the last step's loss_i, break, and the start of the next level.  fast: the level ends by
// attack_cw_fast's width / residual rule instead of after ssteps rounds; max_rounds bounds the rounds of a
// level in both modes (the Adam table has steps * max_rounds entries).  reset[b] is rewritten for every image
// (1 only when it starts a new level); *n_active = images still running.  One block of 64 threads.
__global__ void cw_round_kernel(const float* __restrict__ loss_i, const float* __restrict__ mse_o,
                                double* __restrict__ sd, float* __restrict__ lold, int* __restrict__ si,
                                int* __restrict__ n_active, int B, int fast, int ssteps, int max_rounds, double la,
                                double noise) {
  int cnt = 0;
  for (int b = threadIdx.x; b < B; b += 64) {
    si[CW_RESET * B + b] = 0;
    if (!si[CW_ACTIVE * B + b]) continue;
    const float mo = mse_o[b], li = loss_i[b];
    const double level = sd[CW_LEVEL * B + b];
    double c_l = sd[CW_CL * B + b], c_r = sd[CW_CR * B + b];
    const double c = sd[CW_C * B + b];
    const float target = (float)(0.99 * level);
    if (mo < target) c_l = c; else c_r = c;
    sd[CW_CL * B + b] = c_l;
    sd[CW_CR * B + b] = c_r;
    sd[CW_C * B + b] = (c_r + c_l) / 2;
    const int round = si[CW_ROUND * B + b] + 1;
    si[CW_ROUND * B + b] = round;
    bool more;
    if (fast) {
      const double w = fabs(c_r - c_l);
      more = w > 0.0001 && (w > 0.01 || fabsf(fsub_rn(mo, target)) > (float)(level * 0.01));
    } else {
      more = round < ssteps;
    }
    if (more && round < max_rounds) {
      ++cnt;
      continue;
    }
    // the level is over: attack_'s stop test, then the bisection on the level
    const bool brk = fabsf(fsub_rn(li, lold[b])) < (float)(noise * 0.01) &&
                     fabsf(fsub_rn(li, (float)noise)) < (float)(noise * 0.1);
    if (brk) {
      si[CW_ACTIVE * B + b] = 0;
      continue;
    }
    double mn = sd[CW_MIN * B + b], mx = sd[CW_MAX * B + b];
    if (li > (float)noise) mx = level; else mn = level;
    sd[CW_MIN * B + b] = mn;
    sd[CW_MAX * B + b] = mx;
    sd[CW_LEVEL * B + b] = (mn + mx) / 2;
    const int levels = si[CW_LEVELS * B + b] + 1;
    si[CW_LEVELS * B + b] = levels;
    if (levels >= ssteps) {
      si[CW_ACTIVE * B + b] = 0;
      continue;
    }
    lold[b] = li;
    sd[CW_CL * B + b] = 0.0;
    sd[CW_CR * B + b] = la;
    sd[CW_C * B + b] = la;
    si[CW_ROUND * B + b] = 0;
    si[CW_T * B + b] = 0;
    si[CW_RESET * B + b] = 1;
    ++cnt;
  }
  cnt = wave_sum(cnt);
  if (threadIdx.x == 0) *n_active = cnt;
}

// noise = m = v = 0 for the images that start a new level (reset[b]); the blocks of other images exit at once.
__global__ void cw_reset_kernel(f32x4* __restrict__ noise, f32x4* __restrict__ m, f32x4* __restrict__ v,
                                const int* __restrict__ si, int B, long quads) {
  const int b = blockIdx.y;
  if (!si[CW_RESET * B + b]) return;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
    noise[(long)b * quads + i] = z;
    m[(long)b * quads + i] = z;
    v[(long)b * quads + i] = z;
  }
}

extern "C" {

int ica_cw_gate(const float* part, int nblk, float invN, const double* sd, int* si, float* mse_o, float* c_eff,
                int B, hipStream_t st) {
  if (B <= 0 || nblk <= 0) return -2;
  ICA_LAUNCH(cw_gate_kernel, dim3(B), dim3(256), 0, st, part, nblk, invN, sd, si, mse_o, c_eff, B);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_cw_adam(float* noise, const float* im_s, const float* gnet4, const float* c_eff, float* m, float* v,
                float* im_in_out, int B, int H, int W, float eps, float invN, const float* tab, int ntab,
                const int* si, int clamp_in, hipStream_t st) {
  const long HW = (long)H * W;
  if (B <= 0 || ntab <= 0 || HW <= 0 || (HW & 3)) return -2;
  const long HW4 = HW >> 2;
  const int gx = (int)((HW4 + 255) / 256 < 256 ? (HW4 + 255) / 256 : 256);
  ICA_LAUNCH(cw_adam_kernel, dim3(gx, B), dim3(256), 0, st, noise, im_s, gnet4, c_eff, m, v, im_in_out, HW, eps,
             invN, reinterpret_cast<const f32x2*>(tab), ntab, si, B, clamp_in);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_cw_round(const float* loss_i, const float* mse_o, double* sd, float* lold, int* si, int* n_active, int B,
                 int fast, int ssteps, int max_rounds, const double* cfg, hipStream_t st) {
  if (B <= 0 || ssteps <= 0 || max_rounds <= 0 || !cfg) return -2;
  ICA_LAUNCH(cw_round_kernel, dim3(1), dim3(64), 0, st, loss_i, mse_o, sd, lold, si, n_active, B, fast, ssteps,
             max_rounds, cfg[0], cfg[1]);
  ICA_CHECK_LAUNCH();
  return 0;
}

int ica_cw_reset(float* noise, float* m, float* v, const int* si, int B, long floats_per_image, hipStream_t st) {
  if (B <= 0 || floats_per_image <= 0 || floats_per_image % 4) return -2;
  const long quads = floats_per_image / 4;
  const int gx = (int)((quads + 255) / 256 < 256 ? (quads + 255) / 256 : 256);
  ICA_LAUNCH(cw_reset_kernel, dim3(gx, B), dim3(256), 0, st, reinterpret_cast<f32x4*>(noise),
             reinterpret_cast<f32x4*>(m), reinterpret_cast<f32x4*>(v), si, B, quads);
  ICA_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
