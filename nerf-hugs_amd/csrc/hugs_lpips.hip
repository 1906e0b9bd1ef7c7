// LPIPS (AlexNet) on the device, fp32 throughout: the third column of the eval tables (the reference's metrics.py:30-34,61,
// nerfacto/eval.py:58-60, nerfacto/train.py:70-74: LearnedPerceptualImagePatchSimilarity(normalize=True, net_type='alex')).
//   input   (2x - 1 - shift) / scale per channel; both images run as a batch of 2, activations NHWC fp32
//   conv1   3->64 11x11 s4 p2 | pool 3x3 s2 | conv2 64->192 5x5 p2 | pool | conv3 192->384 | conv4 384->256 | conv5 256->256 (3x3 p1)
//   taps    the five post-ReLU maps: unit-normalise over channels, squared difference, `lin` weights, channel sum, spatial mean
// Convolutions are implicit GEMMs on v_mfma_f32_32x32x2_f32 (M = 2*Ho*Wo pixels, N = Cout, K = taps x Cin), a 4-wave workgroup
// owning 64 pixels x 64 channels (32x32 per wave):
//   * k_lpips_conv (conv2..5): the K loop runs over taps x 32-channel chunks.  Per stage the 64x32 A tile is gathered from
//     global memory (row coordinates computed once per tile, out-of-image taps and rows >= M are zeros) and the 32x64 B
//     tile is read from the repacked [K][Cout] weights, both prefetched into registers during the previous stage's MFMAs
//     and double-buffered through LDS.  The MFMA's two k-slots take k and k+16 of the chunk, so a lane reads its 16 A
//     values of a stage as four 128-bit LDS reads of one row (pitch 36 floats: conflict-free).
//   * k_lpips_conv1: Cin = 3 does not fill a chunk, so a block stages the (39 x 39 x 3->4) transformed input patch of its
//     8x8 output pixels in LDS once and builds A from it: one 128-bit LDS read is one tap's channels, the two k-slots take taps
//     2p and 2p+1 of a kernel row (11 taps + 1 zero tap), channel 3 is never multiplied.  One kernel row of weights per stage.
//   * every stage (K = 32 / 36) accumulates into a fresh accumulator that is then added to the running one: blocked
//     summation, so the rounding error grows with the number of stages, not with K (up to 3456).
//   * the epilogue adds the bias, applies ReLU and stores NHWC (a wave's store instruction is 2 pixels x 32 channels: 128 B rows).
// Max-pooling is a kernel of its own: a pooled value is used by 25 (conv2) or 9 (conv3) taps of Cout/64 column tiles;
// folded into the gather, each of those uses would redo the 9-way max over 9x the bytes.
// k_lpips_dist: one wave per tap pixel, the channels of both images in registers (<= 6 per lane), two butterfly sums for the
// norms, one for the weighted squared difference.  k_lpips_means: one block per tap sums its per-pixel map in a fixed order (double)
// -- no float atomics anywhere: results are bit-reproducible, and lpips(a, b) == lpips(b, a) bit for bit because a row of
// the GEMM is computed by the same operations in the same order whichever batch slot it sits in.
#include "hugs_common.h"

namespace {

typedef float f32x16_t __attribute__((ext_vector_type(16)));

constexpr int NL = 5;
constexpr int L_CIN[NL] = {3, 64, 192, 384, 256}, L_COUT[NL] = {64, 192, 384, 256, 256}, L_KS[NL] = {11, 5, 3, 3, 3};
constexpr int C1_TAPS = 12;                          // 11 taps of a kernel row + one zero tap (the k-slots go in pairs)
constexpr int C1_ROWS = 11 * C1_TAPS * 3;            // packed conv1 weight rows: [ky][12][3]
constexpr int T1 = 8, P1 = (T1 - 1) * 4 + 11, P1W = 40;      // conv1: 8x8 output pixels <- 39x39 input pixels, LDS pitch 40
constexpr int BM = 64, BN = 64, BK = 32, LDA = BK + 4;       // conv2..5 tile; A pitch 36 floats

struct Geom { int h[NL], w[NL], hp[2], wp[2]; };             // spatial size of the five taps and of the two pooled maps

__host__ bool geom_of(int H, int W, Geom& g) {
  if (H < 31 || W < 31) return false;
  g.h[0] = (H + 4 - 11) / 4 + 1; g.w[0] = (W + 4 - 11) / 4 + 1;
  g.hp[0] = (g.h[0] - 3) / 2 + 1; g.wp[0] = (g.w[0] - 3) / 2 + 1;
  g.h[1] = g.hp[0]; g.w[1] = g.wp[0];
  g.hp[1] = (g.h[1] - 3) / 2 + 1; g.wp[1] = (g.w[1] - 3) / 2 + 1;
  for (int l = 2; l < NL; ++l) { g.h[l] = g.hp[1]; g.w[l] = g.wp[1]; }
  return true;
}

__host__ long long krows_of(int l) { return l == 0 ? C1_ROWS : (long long)L_KS[l] * L_KS[l] * L_CIN[l]; }
// packed weights, per layer: W [krows][Cout], bias [Cout], lin [Cout]
__host__ long long packed_floats_total() {
  long long n = 0;
  for (int l = 0; l < NL; ++l) n += (krows_of(l) + 2) * L_COUT[l];
  return n;
}

// D (32x32) of one wave: register v of lane l is row 8*(v/4) + 4*(l/32) + v%4, column l%32.  out rows have pitch Cout.
__device__ __forceinline__ int acc_row(int v, int g) { return 8 * (v >> 2) + 4 * g + (v & 3); }

__global__ void __launch_bounds__(256)
k_lpips_conv1(int H, int W, int Ho, int Wo, const float* __restrict__ a, const float* __restrict__ b,
              const float* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ out) {
  __shared__ float4 patch[P1 * P1W];
  __shared__ __align__(16) float wbuf[2][C1_TAPS * 3 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1, g = lane >> 5, l32 = lane & 31;
  const int img = blockIdx.z, oy0 = blockIdx.y * T1, ox0 = blockIdx.x * T1;
  const float* __restrict__ src = img ? b : a;
  // a weight stage (one kernel row) is 576 float4: two per thread and a third for the first 64 threads
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 w0, w1, w2 = z4;
#define LPIPS_LOAD_W(ky_)                                                         \
  {                                                                               \
    const float4* wsrc = (const float4*)(wp + (size_t)(ky_) * C1_TAPS * 3 * 64);   \
    w0 = wsrc[tid]; w1 = wsrc[tid + 256];                                         \
    if (tid < 64) w2 = wsrc[tid + 512];                                           \
  }
#define LPIPS_STORE_W(buf_)                                                       \
  {                                                                               \
    float4* wdst = (float4*)wbuf[buf_];                                           \
    wdst[tid] = w0; wdst[tid + 256] = w1;                                         \
    if (tid < 64) wdst[tid + 512] = w2;                                           \
  }
  LPIPS_LOAD_W(0)
  for (int i = tid; i < P1 * P1W; i += 256) {
    const int r = i / P1W, c = i - r * P1W, iy = oy0 * 4 - 2 + r, ix = ox0 * 4 - 2 + c;
    float4 v = z4;
    if (c < P1 && iy >= 0 && iy < H && ix >= 0 && ix < W) {
      const float* p = src + ((size_t)iy * W + ix) * 3;
      v.x = (2.f * p[0] - 1.f - (-.030f)) / .458f;
      v.y = (2.f * p[1] - 1.f - (-.088f)) / .448f;
      v.z = (2.f * p[2] - 1.f - (-.188f)) / .450f;
    }
    patch[i] = v;
  }
  LPIPS_STORE_W(0)
  __syncthreads();
  const int m = wm * 32 + l32, prow = (m >> 3) * 4, pcol = (m & 7) * 4;
  f32x16_t acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  for (int ky = 0; ky < 11; ++ky) {
    if (ky + 1 < 11) LPIPS_LOAD_W(ky + 1)
    const float* wb = &wbuf[ky & 1][wn * 32 + l32];
    f32x16_t c;
#pragma unroll
    for (int v = 0; v < 16; ++v) c[v] = 0.f;
#pragma unroll
    for (int pr = 0; pr < C1_TAPS / 2; ++pr) {
      const int tap = 2 * pr + g;
      const float4 av = patch[(prow + ky) * P1W + pcol + tap];
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wb[(tap * 3 + 0) * 64], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wb[(tap * 3 + 1) * 64], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wb[(tap * 3 + 2) * 64], c, 0, 0, 0);
    }
    acc += c;
    if (ky + 1 < 11) LPIPS_STORE_W((ky + 1) & 1)
    __syncthreads();
  }
  const int n = wn * 32 + l32;
  const float bn = bias[n];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int r = wm * 32 + acc_row(v, g), oy = oy0 + (r >> 3), ox = ox0 + (r & 7);
    if (oy < Ho && ox < Wo) out[(((size_t)img * Ho + oy) * Wo + ox) * 64 + n] = fmaxf(acc[v] + bn, 0.f);
  }
}

// stride-1 'same' convolution + bias + ReLU: in [2, Hs, Ws, Cin] -> out [2, Hs, Ws, Cout]; Cin % 32 == 0, Cout % 64 == 0
__global__ void __launch_bounds__(256)
k_lpips_conv(int Hs, int Ws, int Cin, int Cout, int KS, const float* __restrict__ in, const float* __restrict__ wp,
             const float* __restrict__ bias, float* __restrict__ out) {
  __shared__ __align__(16) float As[2][BM * LDA];
  __shared__ __align__(16) float Bs[2][BK * BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1, g = lane >> 5, l32 = lane & 31;
  const int M = 2 * Hs * Ws, m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, pad = KS >> 1;
  // the two A rows (of 4 channels) and B rows (of 4 columns) this thread moves per stage
  const int lr = tid >> 3, kq = tid & 7, br = tid >> 4, bq = tid & 15;
  int oy0, ox0, oy1, ox1;
  const float *rb0, *rb1;
#define LPIPS_ROW(j_, oy_, ox_, rb_)                                                              \
  {                                                                                               \
    const int mm = m0 + lr + 32 * (j_);                                                           \
    const int im = mm / (Hs * Ws), rem = mm - im * (Hs * Ws);                                     \
    oy_ = mm < M ? rem / Ws : -(1 << 20); /* rows past M never pass the bounds test below */      \
    ox_ = rem % Ws;                                                                               \
    rb_ = in + (size_t)(mm < M ? im : 0) * Hs * Ws * Cin + kq * 4;                                \
  }
  LPIPS_ROW(0, oy0, ox0, rb0)
  LPIPS_ROW(1, oy1, ox1, rb1)
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 a0, a1, b0, b1;
  int ky = 0, kx = 0, c0 = 0;                        // the stage being loaded: tap (ky, kx), channels c0 .. c0+31
  const float* wrow = wp + (size_t)br * Cout + n0 + bq * 4;
#define LPIPS_GATHER(oy_, ox_, rb_, dst_)                                                         \
  {                                                                                               \
    const int iy = oy_ + ky - pad, ix = ox_ + kx - pad;                                           \
    const bool ok = iy >= 0 && iy < Hs && ix >= 0 && ix < Ws;                                     \
    dst_ = z4;                                                                                    \
    if (ok) dst_ = *(const float4*)(rb_ + ((size_t)iy * Ws + ix) * Cin + c0);                     \
  }
#define LPIPS_LOAD_STAGE                                                                          \
  {                                                                                               \
    LPIPS_GATHER(oy0, ox0, rb0, a0)                                                               \
    LPIPS_GATHER(oy1, ox1, rb1, a1)                                                               \
    b0 = *(const float4*)wrow;                                                                    \
    b1 = *(const float4*)(wrow + (size_t)16 * Cout);                                              \
    wrow += (size_t)BK * Cout; c0 += BK;                                                          \
    if (c0 == Cin) { c0 = 0; if (++kx == KS) { kx = 0; ++ky; } }                                  \
  }
#define LPIPS_STORE_STAGE(buf_)                                                                   \
  {                                                                                               \
    *(float4*)(&As[buf_][lr * LDA + kq * 4]) = a0;                                                \
    *(float4*)(&As[buf_][(lr + 32) * LDA + kq * 4]) = a1;                                         \
    *(float4*)(&Bs[buf_][br * BN + bq * 4]) = b0;                                                 \
    *(float4*)(&Bs[buf_][(br + 16) * BN + bq * 4]) = b1;                                          \
  }
  const int ns = KS * KS * (Cin / BK);
  LPIPS_LOAD_STAGE
  LPIPS_STORE_STAGE(0)
  __syncthreads();
  f32x16_t acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  for (int s = 0; s < ns; ++s) {
    if (s + 1 < ns) LPIPS_LOAD_STAGE
    const float* la = &As[s & 1][(wm * 32 + l32) * LDA + g * 16];
    const float* lb = &Bs[s & 1][(g * 16) * BN + wn * 32 + l32];
    float4 af[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) af[q] = *(const float4*)(la + q * 4);
    f32x16_t c;
#pragma unroll
    for (int v = 0; v < 16; ++v) c[v] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q].x, lb[(q * 4 + 0) * BN], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q].y, lb[(q * 4 + 1) * BN], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q].z, lb[(q * 4 + 2) * BN], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q].w, lb[(q * 4 + 3) * BN], c, 0, 0, 0);
    }
    acc += c;
    if (s + 1 < ns) LPIPS_STORE_STAGE((s + 1) & 1)
    __syncthreads();
  }
  const int n = n0 + wn * 32 + l32;
  const float bn = bias[n];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int mm = m0 + wm * 32 + acc_row(v, g);
    if (mm < M) out[(size_t)mm * Cout + n] = fmaxf(acc[v] + bn, 0.f);
  }
}

// 3x3 stride-2 max-pool without padding, NHWC, 4 channels per thread
__global__ void __launch_bounds__(256)
k_lpips_maxpool(int Hi, int Wi, int Ho, int Wo, int C, const float* __restrict__ in, float* __restrict__ out) {
  const int cq = C >> 2;
  const long long n = 2ll * Ho * Wo * cq, i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % cq);
  long long p = i / cq;
  const int x = (int)(p % Wo); p /= Wo;
  const int y = (int)(p % Ho), im = (int)(p / Ho);
  const float* src = in + (((size_t)im * Hi + 2 * y) * Wi + 2 * x) * C + c * 4;
  float4 m = *(const float4*)src;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float4 v = *(const float4*)(src + ((size_t)dy * Wi + dx) * C);
      m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
  *(float4*)(out + (size_t)i * 4) = m;
}

// feat [2, P, C] (C <= 384) -> map [P]: sum_c lin[c] * (f0/(|f0| + 1e-10) - f1/(|f1| + 1e-10))^2, one wave per pixel
__global__ void __launch_bounds__(256)
k_lpips_dist(int P, int C, const float* __restrict__ feat, const float* __restrict__ lin, float* __restrict__ map) {
  const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;
  const float* f0 = feat + (size_t)p * C;
  const float* f1 = feat + ((size_t)P + p) * C;
  float x0[6], x1[6], s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int c = j * 64 + lane;
    x0[j] = c < C ? f0[c] : 0.f;
    x1[j] = c < C ? f1[c] : 0.f;
    s0 += x0[j] * x0[j];
    s1 += x1[j] * x1[j];
  }
  const float d0 = sqrtf(wave_sum_f(s0)) + 1e-10f, d1 = sqrtf(wave_sum_f(s1)) + 1e-10f;
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int c = j * 64 + lane;
    const float t = x0[j] / d0 - x1[j] / d1;
    if (c < C) d += (t * t) * lin[c];
  }
  d = wave_sum_f(d);
  if (lane == 0) map[p] = d;
}

struct MapSet { long long off[NL]; int n[NL]; };

// block l: means[l] = mean(map_l) summed in a fixed order in double, out[1 + l] its float
__global__ void __launch_bounds__(1024) k_lpips_means(MapSet ms, const float* __restrict__ maps, double* __restrict__ means,
                                                       float* __restrict__ out) {
  __shared__ double sm[1024];
  const int l = blockIdx.x, n = ms.n[l];
  const float* m = maps + ms.off[l];
  double s = 0.;
  for (int i = threadIdx.x; i < n; i += 1024) s += (double)m[i];
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int d = 512; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) sm[threadIdx.x] += sm[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    means[l] = sm[0] / (double)n;
    out[1 + l] = (float)means[l];
  }
}

// out[0] = the sum of the five layer means
__global__ void k_lpips_total(const double* __restrict__ means, float* __restrict__ out) {
  if (threadIdx.x == 0) out[0] = (float)((((means[0] + means[1]) + means[2]) + means[3]) + means[4]);
}

// workspace, in floats: the five taps, the two pooled maps, the five layer means (doubles), then the five per-pixel distance maps
struct WsLayout { long long feat[NL], pool[2], means, maps, total; MapSet ms; };

__host__ WsLayout ws_layout(const Geom& g) {
  WsLayout w;
  long long o = 0;
  for (int l = 0; l < NL; ++l) { w.feat[l] = o; o += 2ll * g.h[l] * g.w[l] * L_COUT[l]; }
  for (int l = 0; l < 2; ++l) { w.pool[l] = o; o += 2ll * g.hp[l] * g.wp[l] * L_COUT[l]; }
  w.means = o; o += 2 * NL;          // (every size above is a multiple of 64 floats: 8-byte aligned)
  w.maps = o;
  long long mo = 0;
  for (int l = 0; l < NL; ++l) { w.ms.off[l] = mo; w.ms.n[l] = g.h[l] * g.w[l]; mo += w.ms.n[l]; }
  w.total = o + mo;
  return w;
}

}  // namespace

extern "C" long long hugs_lpips_alex_ws_bytes(int H, int W) {
  Geom g;
  if (!geom_of(H, W, g) || H > 16384 || W > 16384) return 0;
  return ws_layout(g).total * (long long)sizeof(float);
}

extern "C" int hugs_lpips_alex(int H, int W, const float* a, const float* b, const float* packed, long long packed_floats,
                               float* ws, float* out, float* maps, void* stream) {
  HUGS_REQUIRE(a && b && packed && ws && out, -2, "hugs_lpips_alex: null pointer");
  Geom g;
  HUGS_REQUIRE(geom_of(H, W, g), -2, "hugs_lpips_alex: image %dx%d smaller than 31x31 (the second max-pool has no output)", H, W);
  HUGS_REQUIRE(H <= 16384 && W <= 16384, -2, "hugs_lpips_alex: image %dx%d larger than 16384", H, W);
  HUGS_REQUIRE(packed_floats == packed_floats_total(), -2, "hugs_lpips_alex: %lld packed weight floats, expected %lld",
               packed_floats, packed_floats_total());
  HUGS_REQUIRE((((uintptr_t)packed | (uintptr_t)ws) & 15) == 0, -2, "hugs_lpips_alex: packed weights / workspace not 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const WsLayout w = ws_layout(g);
  float* dmap = maps ? maps : ws + w.maps;
  const float* in = nullptr;
  const float* wl = packed;
  for (int l = 0; l < NL; ++l) {
    const int co = L_COUT[l];
    const float *bias = wl + krows_of(l) * co, *lin = bias + co;
    float* f = ws + w.feat[l];
    if (l == 0) {
      k_lpips_conv1<<<dim3((g.w[0] + T1 - 1) / T1, (g.h[0] + T1 - 1) / T1, 2), 256, 0, st>>>(H, W, g.h[0], g.w[0], a, b, wl, bias, f);
      HUGS_CHECK_LAUNCH("k_lpips_conv1");
    } else {
      const int M = 2 * g.h[l] * g.w[l];
      k_lpips_conv<<<dim3((M + BM - 1) / BM, co / BN), 256, 0, st>>>(g.h[l], g.w[l], L_CIN[l], co, L_KS[l], in, wl, bias, f);
      HUGS_CHECK_LAUNCH("k_lpips_conv");
    }
    const int P = g.h[l] * g.w[l];
    k_lpips_dist<<<(P + 3) / 4, 256, 0, st>>>(P, co, f, lin, dmap + w.ms.off[l]);
    HUGS_CHECK_LAUNCH("k_lpips_dist");
    in = f;
    if (l < 2) {
      float* p = ws + w.pool[l];
      const long long n = 2ll * g.hp[l] * g.wp[l] * (co / 4);
      k_lpips_maxpool<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(g.h[l], g.w[l], g.hp[l], g.wp[l], co, f, p);
      HUGS_CHECK_LAUNCH("k_lpips_maxpool");
      in = p;
    }
    wl = lin + co;
  }
  double* means = (double*)(ws + w.means);
  k_lpips_means<<<NL, 1024, 0, st>>>(w.ms, dmap, means, out);
  HUGS_CHECK_LAUNCH("k_lpips_means");
  k_lpips_total<<<1, 64, 0, st>>>(means, out);
  HUGS_CHECK_LAUNCH("k_lpips_total");
  return 0;
}
