// Device helpers the mask files share (hugs_staticmask.hip, hugs_samamg.hip): SAM's postprocess_masks as a function of the output
// pixel, and a union-find whose roots are the smallest index of their set.
#pragma once
#include "hugs_common.h"

namespace {

constexpr int LR = 256, LR_UP = 1024;
struct LrAxis { int i[4]; float w[4]; };     // crop tap a = 0, 1: low-res taps i[2a], i[2a+1] with lambda w[2a+1]; w[0]: the crop taps' lambda

// torch's area_pixel_compute_source_index + the index / lambda of upsample_bilinear2d, fp32
__device__ __forceinline__ void lr_tap(int dst, float scale, int in, int& i0, int& i1, float& lam) {
  const float s = fmaxf(((float)dst + 0.5f) * scale - 0.5f, 0.f);
  i0 = min((int)s, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

__device__ __forceinline__ LrAxis lr_axis(int dst, float scale, int in) {
  LrAxis a;
  int c0, c1;
  lr_tap(dst, scale, in, c0, c1, a.w[0]);
  lr_tap(c0, (float)LR / (float)LR_UP, LR, a.i[0], a.i[1], a.w[1]);
  lr_tap(c1, (float)LR / (float)LR_UP, LR, a.i[2], a.i[3], a.w[3]);
  a.w[2] = 0.f;
  return a;
}

__device__ __forceinline__ float lr_bilerp(float p00, float p01, float p10, float p11, float ly, float lx) {
  return (1.f - ly) * ((1.f - lx) * p00 + lx * p01) + ly * ((1.f - lx) * p10 + lx * p11);
}

__device__ __forceinline__ float lr_logit(const float* __restrict__ L, const LrAxis& y, const LrAxis& x) {
  float mid[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const float* r0 = L + y.i[2 * a] * LR;
      const float* r1 = L + y.i[2 * a + 1] * LR;
      mid[a][b] = lr_bilerp(r0[x.i[2 * b]], r0[x.i[2 * b + 1]], r1[x.i[2 * b]], r1[x.i[2 * b + 1]], y.w[2 * a + 1], x.w[2 * b + 1]);
    }
  return lr_bilerp(mid[0][0], mid[0][1], mid[1][0], mid[1][1], y.w[0], x.w[0]);
}

__device__ __forceinline__ int uf_find(volatile int* P, int x) {
  int p;
  while ((p = P[x]) != x) x = p;
  return x;
}
// parents only ever decrease, so the root of a set is its smallest index
__device__ __forceinline__ void uf_unite(int* P, int a, int b) {
  bool done = false;
  while (!done) {
    a = uf_find(P, a);
    b = uf_find(P, b);
    if (a == b) break;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&P[b], a);
    done = old == b;
    b = old;
  }
}

}  // namespace
