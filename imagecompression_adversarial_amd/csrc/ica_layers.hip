// The reductions of the layer-wise error-propagation study (layer_compare, anchors/utils.py:132-166): per image and
// per layer the sums of squared activation differences between an adversarial and a clean forward, for every layer
// of a side (encoder, latent, decoder) in ONE launch.
//
//   layer_sums_kernel   grid (blocks of the largest layer, image, layer); the layer's descriptor selects the mode
//
// Inputs are fp32 nChw4c activations [B][ceil(C/4)][H][W][4].  The pointers of a descriptor address contiguous views
// of B images each: the halves (thirds) of one batched forward, no gather and no copy.  They share one storage
// layout, row-major or parity-split (ica_conv_args.layout): both keep the channel quad of a pixel together and only
// permute the pixels of a (image, channel quad) plane, the same way in every tensor of the descriptor, and a sum of
// squared differences over a whole plane does not depend on the order of its pixels' storage.  (It does fix the
// order of the additions: the numbers of a parity-split layer are those of that layout.  The host hands over both
// tensors of a descriptor from one launch, so they cannot differ.)
//
// Modes, two sums per (layer, image):
//   PAIR     s0 = sum (a - b)^2                                   s1 = 0
//   QUANT    s0 = sum (a - rne(b))^2                              s1 = sum (rne(a) - rne(b))^2
//   TRIPLE   s0 = sum (a - c)^2                                   s1 = sum (b - c)^2      (c is loaded once)
// rne = round half to even (v_rndne_f32), the bits of torch.round; no rounded plane is written.  Each term is
// d = a - b (one rounded fp32 subtraction), then acc = fma(d, d, acc).  Lanes of the padding channels (c >= C)
// are selected away, not multiplied: they add nothing whatever they hold (NaN, inf).
//
// Reductions: ica_reduce.h.  A thread walks the channel quads q = blk * 256 + tid, + nb * 256, ... of its image in that
// order with one accumulator per lane of the quad, adds the four as ((l0 + l1) + l2) + l3, block_sum adds the block
// and the block writes one partial per sum.  A layer has nb = capped_blocks(quads, LAY_THREADS * LAY_QUADS,
// LAY_MAX_BLOCKS) blocks per image: a function of (C, H, W) alone.  A row of partials always has LAY_MAX_BLOCKS
// slots; block 0 zero-fills the slots nb .. LAY_MAX_BLOCKS - 1, and ica_reduce_rows adds a row with one slot per
// thread (LAY_MAX_BLOCKS = 256 = its block), so adding the zeros is exact and the row's sum does not depend on what
// else the table holds.  No float atomics: an image's numbers are the same bits alone and in a batch, run to run.
// LAY_THREADS, LAY_QUADS and LAY_MAX_BLOCKS are part of that promise.
//
// The descriptor table travels by value in the kernel arguments (16 x 40 bytes): no device-side table, no upload.
#include "ica_reduce.h"

// C-ABI mirror of include/ica_hip.h: the modes, the table limit and ica_layer_desc
enum { ICA_LAYER_PAIR = 0, ICA_LAYER_QUANT = 1, ICA_LAYER_TRIPLE = 2 };
enum { ICA_LAYERS_MAX = 16 };
struct ica_layer_desc {
  const float* a;
  const float* b;
  const float* c;
  int C, H, W, mode;
};
extern "C" int ica_reduce_rows(const float* part, float* out, int B, int nblk, float scale, hipStream_t st);

namespace {

constexpr int LAY_THREADS = 256;
constexpr int LAY_QUADS = 4;          // quads a thread should at least have before a layer gets another block
constexpr int LAY_MAX_BLOCKS = 256;   // per (layer, image); also the slots of a row of partials

struct LayerTable {
  ica_layer_desc l[ICA_LAYERS_MAX];
};

int layer_blocks(long quads) { return capped_blocks(quads, LAY_THREADS * LAY_QUADS, LAY_MAX_BLOCKS); }

ICA_DEV float sq_acc(float a, float b, float acc) {
  const float d = fsub_rn(a, b);
  return __fmaf_rn(d, d, acc);
}

// part[((layer * B + image) * 2 + k) * LAY_MAX_BLOCKS + blk]
__global__ __launch_bounds__(LAY_THREADS) void layer_sums_kernel(const LayerTable tab, float* __restrict__ part) {
  __shared__ float red[4];
  const ica_layer_desc L = tab.l[blockIdx.z];
  const long HW = (long)L.H * L.W;
  const long quads = (long)((L.C + 3) >> 2) * HW;
  const int nb = (int)min((quads + LAY_THREADS * LAY_QUADS - 1) / (LAY_THREADS * LAY_QUADS), (long)LAY_MAX_BLOCKS);
  const int blk = blockIdx.x, b = blockIdx.y, B = gridDim.y;
  if (blk >= nb) return;   // block-uniform: a smaller layer of the table
  const size_t img = (size_t)b * (size_t)quads * 4;
  const float* __restrict__ pa = L.a + img;
  const float* __restrict__ pb = L.b + img;
  const float* __restrict__ pc = L.mode == ICA_LAYER_TRIPLE ? L.c + img : nullptr;
  const int tail = L.C & 3;                       // real lanes of the last channel quad (0: all four)
  const long full = tail ? quads - HW : quads;    // quads before the last channel quad's plane
  const int mode = L.mode;

  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  for (long q = (long)blk * LAY_THREADS + threadIdx.x; q < quads; q += (long)nb * LAY_THREADS) {
    const int lanes = q < full ? 4 : tail;
    const f32x4 va = ld4(pa + q * 4), vb = ld4(pb + q * 4);
    if (mode == ICA_LAYER_PAIR) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = sq_acc(va[e], vb[e], s0[e]);
        s0[e] = e < lanes ? t : s0[e];
      }
    } else if (mode == ICA_LAYER_QUANT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float rb = rintf(vb[e]);
        const float t0 = sq_acc(va[e], rb, s0[e]);
        const float t1 = sq_acc(rintf(va[e]), rb, s1[e]);
        s0[e] = e < lanes ? t0 : s0[e];
        s1[e] = e < lanes ? t1 : s1[e];
      }
    } else {
      const f32x4 vc = ld4(pc + q * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t0 = sq_acc(va[e], vc[e], s0[e]);
        const float t1 = sq_acc(vb[e], vc[e], s1[e]);
        s0[e] = e < lanes ? t0 : s0[e];
        s1[e] = e < lanes ? t1 : s1[e];
      }
    }
  }
  const float t0 = block_sum(fadd_rn(fadd_rn(fadd_rn(s0[0], s0[1]), s0[2]), s0[3]), red);
  const float t1 = block_sum(fadd_rn(fadd_rn(fadd_rn(s1[0], s1[1]), s1[2]), s1[3]), red);
  float* row = part + ((size_t)blockIdx.z * B + b) * 2 * LAY_MAX_BLOCKS;
  if (threadIdx.x == 0) {
    row[blk] = t0;
    row[LAY_MAX_BLOCKS + blk] = t1;
  }
  if (blk == 0) {   // the unused slots of both rows
    for (int i = nb + threadIdx.x; i < LAY_MAX_BLOCKS; i += LAY_THREADS) {
      row[i] = 0.f;
      row[LAY_MAX_BLOCKS + i] = 0.f;
    }
  }
}

// 0, or the status of a table the kernel does not take
int layers_check(const ica_layer_desc* layers, int n, int B) {
  if (!layers || n < 1 || n > ICA_LAYERS_MAX || B < 1 || B > 65535) return -5;
  for (int i = 0; i < n; ++i) {
    const ica_layer_desc& L = layers[i];
    if (L.mode != ICA_LAYER_PAIR && L.mode != ICA_LAYER_QUANT && L.mode != ICA_LAYER_TRIPLE) return -5;
    if (L.C <= 0 || L.H <= 0 || L.W <= 0) return -5;
    if (!L.a || !L.b || (L.mode == ICA_LAYER_TRIPLE && !L.c)) return -5;
    if (!aligned16(L.a) || !aligned16(L.b) || (L.mode == ICA_LAYER_TRIPLE && !aligned16(L.c))) return -5;
    const long c4 = ((long)L.C + 3) / 4;
    if ((long)L.H * L.W > 0x7fffffffL / 4 || c4 > 0x7fffffffL / ((long)L.H * L.W)) return -5;   // quads of an image fit an int
    if ((long)B * c4 * L.H * L.W > 0x7fffffffffffL / 4) return -5;                              // elements < 2^47
  }
  return 0;
}

}  // namespace

extern "C" {

int ica_layer_sums_blocks(int C, int H, int W) {
  if (C <= 0 || H <= 0 || W <= 0) return 0;
  return layer_blocks(((long)C + 3) / 4 * H * W);
}

size_t ica_layer_sums_ws_size(int n, int B) {
  if (n < 1 || n > ICA_LAYERS_MAX || B < 1 || B > 65535) return 0;
  return (size_t)n * B * 2 * LAY_MAX_BLOCKS;
}

int ica_layer_sums(const ica_layer_desc* layers, int n, int B, float* sums, float* work, hipStream_t st) {
  if (int rc = layers_check(layers, n, B)) return rc;
  if (!sums || !work) return -5;
  const size_t sums_bytes = sizeof(float) * (size_t)n * B * 2, work_bytes = sizeof(float) * ica_layer_sums_ws_size(n, B);
  if (overlaps(sums, sums_bytes, work, work_bytes)) return -7;
  LayerTable tab = {};
  int nbmax = 1;
  for (int i = 0; i < n; ++i) {
    const ica_layer_desc& L = layers[i];
    const size_t bytes = sizeof(float) * (size_t)B * ((L.C + 3) / 4) * L.H * L.W * 4;
    const void* ins[3] = {L.a, L.b, L.mode == ICA_LAYER_TRIPLE ? L.c : nullptr};
    for (const void* p : ins)
      if (p && (overlaps(sums, sums_bytes, p, bytes) || overlaps(work, work_bytes, p, bytes))) return -7;
    tab.l[i] = L;
    if (L.mode != ICA_LAYER_TRIPLE) tab.l[i].c = nullptr;
    nbmax = max(nbmax, ica_layer_sums_blocks(L.C, L.H, L.W));
  }
  ICA_LAUNCH(layer_sums_kernel, dim3(nbmax, B, n), dim3(LAY_THREADS), 0, st, tab, work);
  ICA_CHECK_LAUNCH();
  return ica_reduce_rows(work, sums, n * B * 2, LAY_MAX_BLOCKS, 1.f, st);
}

}  // extern "C"
