// The universal perturbation's update: one additive noise [1][3][H][W] fitted to B images at once (DESIGN.md §8
// "Universal perturbation").  Its semantics are attack_rd.attack_ with a noise that broadcasts over the batch: the
// batch-coupled branch and losses of train.py:342, and the sum over the batch that autograd forms where the noise was
// broadcast, in front of the noise bounds' backward and torch.optim.Adam.
//
// The prologue is attack_prologue_kernel at noise stride 0 (ica_elem.hip, ica_universal_prologue).  This file holds
// the update.  Per noise element, in this order (the pinned one):
//   for b = 0 .. B-1:   u = s_b + nc, lowU = max(u, 0), ii_b = min(lowU, 1)          (nc = min(max(nz, -eps), eps))
//                       g_b = cheap ? -(t + t), t = gscale * (s_b - ii_b) : gnet4[b]   (cheap = loss_i[0] > thr)
//                       g_b through image b's own Up / Low [0, 1] pass-through
//   G = g_0; G = G + g_b for b = 1 .. B-1 in that order (one thread, no atomics: the same bits for any grid)
//   G through the noise bounds' pass-through, then attack_adam_kernel's Adam, op for op.
// The grid runs over pixels only, so noise, m and v are read and written once per step (9 planes of H W floats each
// way; the per-image kernel moves them B times), next to B x 7 planes of im_s and gnet4.
#include <type_traits>

#include "ica_reduce.h"

namespace {

constexpr int UNI_BLOCKS = 256;   // blocks of 256 threads; the rest is grid-strided
constexpr int UNI_GROUP = 4;      // images whose loads are issued before the first of them is used

// V floats of one plane: one 16-byte access (V == 4) or one float (V == 1, the tail form for H W % 4 != 0)
template <int V>
struct Vec {
  float e[V];
};
// base + i floats with the byte offset formed in 32 bits: the load takes a scalar base and a 32-bit lane offset
ICA_DEV const float* at(const float* base, unsigned i) {
  return reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + (i << 2));
}
ICA_DEV float* at(float* base, unsigned i) {
  return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + (i << 2));
}

template <int V>
ICA_DEV Vec<V> ldv(const float* p) {
  Vec<V> r;
  if constexpr (V == 4) {
    const f32x4 t = ld4(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) r.e[k] = t[k];
  } else {
    r.e[0] = p[0];
  }
  return r;
}
template <int V>
ICA_DEV void stv(float* p, const Vec<V>& v) {
  if constexpr (V == 4) {
    st4(p, f32x4{v.e[0], v.e[1], v.e[2], v.e[3]});
  } else {
    p[0] = v.e[0];
  }
}

template <int V>
__global__ __launch_bounds__(256) void universal_adam_kernel(
    float* __restrict__ noise, const float* __restrict__ im_s, const float* __restrict__ gnet4,
    const float* __restrict__ loss_i, float* __restrict__ m, float* __restrict__ v, float* __restrict__ im_in_out,
    int B, long HW, float eps, float thr, float gscale, float bc2s, float neg_step, int* __restrict__ branch,
    int* __restrict__ census) {
  const bool cheap = loss_i[0] > thr;   // the coupled loop wrote the batch mean into every entry
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int b = 0; b < B; ++b) {
      if (branch) branch[b] = cheap ? 1 : 0;
      if (census) census[b] += cheap ? 1 : 0;
    }
  }
  // 32-bit byte offsets inside an image (the launcher refuses H W >= 2^27), 64-bit only in the block-uniform image
  // bases: a load is a scalar base plus one lane offset, and no 64-bit address is kept per load
  const unsigned hw = (unsigned)HW, n = hw / V;   // V == 4 is launched only for HW % 4 == 0
  for (unsigned q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
    const unsigned pix0 = q * V;
    Vec<V> nz[3], mo[3], vo[3], G[3] = {};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      nz[c] = ldv<V>(at(noise, c * hw + pix0));
      mo[c] = ldv<V>(at(m, c * hw + pix0));
      vo[c] = ldv<V>(at(v, c * hw + pix0));
    }
    // NG images from b0 on: their loads first (NG x 7 16-byte loads in flight at V == 4), then the serial adds
    auto images = [&](int b0, auto ng) {
      constexpr int NG = decltype(ng)::value;
      Vec<V> s[NG][3];
      f32x4 gn[NG][V] = {};
#pragma unroll
      for (int j = 0; j < NG; ++j) {
        const float* sb = im_s + (long)(b0 + j) * 3 * HW;
        const float* gb = gnet4 + (long)(b0 + j) * 4 * HW;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[j][c] = ldv<V>(at(sb, c * hw + pix0));
        if (!cheap) {   // the network gradient is read only when used
#pragma unroll
          for (int k = 0; k < V; ++k) gn[j][k] = ld4(at(gb, (pix0 + k) * 4));
        }
      }
#pragma unroll
      for (int j = 0; j < NG; ++j) {
        const int b = b0 + j;
        float* ib = im_in_out ? im_in_out + (long)b * 3 * HW : nullptr;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          Vec<V> ii;
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const float nc = fminf(fmaxf(nz[c].e[k], -eps), eps);
            const float sv = s[j][c].e[k];
            const float u = fadd_rn(sv, nc);
            const float lowU = fmaxf(u, 0.f);
            ii.e[k] = fminf(lowU, 1.f);
            float g;
            if (cheap) {
              const float t = fmul_rn(gscale, fsub_rn(sv, ii.e[k]));
              g = -fadd_rn(t, t);
            } else {
              g = gn[j][k][c];
            }
            g = (lowU <= 1.f || g > 0.f) ? g : g * 0.f;
            g = (u >= 0.f || g < 0.f) ? g : g * 0.f;
            G[c].e[k] = b == 0 ? g : fadd_rn(G[c].e[k], g);
          }
          if (ib) stv<V>(at(ib, c * hw + pix0), ii);
        }
      }
    };
    int b0 = 0;   // (not unrolled further: a second group in flight would only cost registers)
#pragma unroll 1
    for (; b0 + UNI_GROUP <= B; b0 += UNI_GROUP) images(b0, std::integral_constant<int, UNI_GROUP>{});
#pragma unroll 1
    for (; b0 < B; ++b0) images(b0, std::integral_constant<int, 1>{});
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Vec<V> no;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float z = nz[c].e[k];
        const float lowN = fmaxf(z, -eps);
        float g = G[c].e[k];
        g = (lowN <= eps || g > 0.f) ? g : g * 0.f;
        g = (z >= -eps || g < 0.f) ? g : g * 0.f;
        const float mn = __fmaf_rn(0.1f, fsub_rn(g, mo[c].e[k]), mo[c].e[k]);
        // hipcc contracts a product into the add that follows it, explicit round-to-nearest intrinsics or not, and it
        // does so differently in attack_adam_kernel's two forms.  Those bits are the pinned ones, so the fused
        // operations are spelled out here, per form: v = fma(g, 0.001 g, 0.999 v) in the 16-byte form and
        // fma(0.999, v, (0.001 g) g) in the scalar form; the step is fma(neg_step, m / denom, noise) in both.
        float vn;
        if constexpr (V == 4) {
          vn = __fmaf_rn(g, fmul_rn(0.001f, g), fmul_rn(vo[c].e[k], 0.999f));
        } else {
          vn = __fmaf_rn(0.999f, vo[c].e[k], fmul_rn(fmul_rn(0.001f, g), g));
        }
        const float denom = fadd_rn(fdiv_rn(sqrtf(vn), bc2s), 1e-8f);
        mo[c].e[k] = mn;
        vo[c].e[k] = vn;
        no.e[k] = __fmaf_rn(neg_step, fdiv_rn(mn, denom), z);
      }
      stv<V>(at(m, c * hw + pix0), mo[c]);
      stv<V>(at(v, c * hw + pix0), vo[c]);
      stv<V>(at(noise, c * hw + pix0), no);
    }
  }
}

}  // namespace

extern "C" int ica_universal_adam(float* noise, const float* im_s, const float* gnet4, const float* loss_i, float* m,
                                  float* v, float* im_in_out, int B, int H, int W, float eps, float thr, float gscale,
                                  float bc2s, float neg_step, int* branch, int* census, hipStream_t st) {
  const long HW = (long)H * W;
  if (B < 1 || H < 1 || W < 1 || HW >= (1L << 27) || !noise || !im_s || !loss_i || !m || !v)
    return (int)hipErrorInvalidValue;
  if ((HW & 3) == 0) {
    // four pixels per thread: every plane in 16-byte accesses
    ICA_LAUNCH(universal_adam_kernel<4>, dim3(capped_blocks(HW >> 2, 256, UNI_BLOCKS)), dim3(256), 0, st, noise, im_s,
               gnet4, loss_i, m, v, im_in_out, B, HW, eps, thr, gscale, bc2s, neg_step, branch, census);
  } else {
    ICA_LAUNCH(universal_adam_kernel<1>, dim3(capped_blocks(HW, 256, UNI_BLOCKS)), dim3(256), 0, st, noise, im_s, gnet4,
               loss_i, m, v, im_in_out, B, HW, eps, thr, gscale, bc2s, neg_step, branch, census);
  }
  ICA_CHECK_LAUNCH();
  return 0;
}
