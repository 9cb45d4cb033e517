// The orthonormal 8-point DCT-II pair the block transforms share (ica_jpeg.hip: the JPEG round trip; ica_band.hip:
// the frequency-band projection).  fp32, the even-odd factorisation with the constants 0.5 cos(k pi / 16).  A 2-D
// transform runs rows first, then columns, and its inverse in the opposite order.  The operation order of both
// functions is part of the results of every kernel that includes this file.
#pragma once
#include "ica_common.h"

namespace {

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

}  // namespace
