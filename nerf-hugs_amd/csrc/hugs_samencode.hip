// SAM's ViT image encoder on the device, fp32 throughout: Sam.preprocess + ImageEncoderViT, the predictor.set_image(sam_image)
// of HuGS/generate_static_mask.py:338 (the model built at :192), from the resized RGB image [h_in,w_in,3] to the embedding
// [256,64,64] that hugs_sam_set_image takes.  Every matrix product runs on v_mfma_f32_32x32x2_f32.
//
//   * k_enc_gemm<LOADER, EPI>: C[M,N] = A[M,K] @ Wt[K,N] (+ bias).  A workgroup of four waves owns a 128 x 128 tile of C, a wave
//     a 64 x 64 quarter (2 x 2 MFMA blocks, 64 accumulator registers).  K advances in stages of 16: the A [128][16] and B
//     [16][128] slabs of stage s + 1 are fetched from global memory into registers before the 32 MFMAs of stage s are issued
//     and written to the other half of the LDS ring after them, so the loads fly under the matrix pipe and one barrier per
//     stage suffices.  37 KB of LDS and < 256 registers: two to four workgroups share a CU.  Each stage sums its 16 products
//     into a fresh accumulator that is then added to the running one (rounding grows with K / 16, not K).  A rows live in LDS
//     at pitch 20 (a lane's two 128-bit reads of its row are conflict-free), B rows at pitch 132 (the half-waves' k rows are 8
//     apart: 8 * 132 = 32 banks apart).  The MFMA's two k-slots take k and k + 8 of the stage.
//     Loaders: plain rows (row tail masked); the patch embedding (reads the uint8 / float image, normalises, zero-pads: the
//     16 x 16 x 3 patch is the K axis, ordered (py, px, c) like the image row); the neck's 3 x 3 convolution (K = tap * 256 +
//     channel, shifted zero-padded rows).  Epilogues: plain, GELU, residual add, residual add through the window -> grid row
//     map (pad rows dropped).  blockIdx.z batches the per-head rel-pos products.
//   * k_enc_ln<NV, MODE>: one wave per row, the row in registers, two-pass mean / variance.  MODE 1 writes the rows in window
//     order (25 windows of 14 x 14 cut from the 70 x 70 zero-padded grid; pad rows are written as zeros, after the norm);
//     MODE 2 writes the neck's result channel-major.
//   * k_enc_attn<HD, G>: flash attention with the decomposed relative-position bias, for the windows (G = 14, 196 keys) and
//     the global blocks (G = 64, 4096 keys).  A workgroup holds 128 queries of one (window, head), a wave 32 of them, and
//     streams tiles of 64 keys and values through LDS.  It computes S^T = K Q^T, so a lane owns one query column: the softmax
//     statistics are per-lane scalars (one cross-half shuffle), and the probabilities leave the MFMA in exactly the register
//     layout the B operand of O^T = V^T P^T wants -- they never touch LDS.  Q^T (HD / 2 registers) stays in registers for the
//     whole kernel.  The bias comes from P = Q @ [rel_pos_h ; rel_pos_w]^T, a product of k_enc_gemm: for G = 64 a key tile is
//     one key row kh, so the rel_h term is one scalar per lane and tile and the 32 rel_w terms of a lane are loaded once and
//     kept in registers; for G = 14 both are gathered per tile from the (L2-resident) 64-float strip of the query.  HD = 80 is
//     forty k-steps of S and three 32-channel blocks of O (the last one half used); nothing is padded to 128.
// No atomics: results are bit-reproducible.  Nothing is allocated: activations ping-pong in the caller's workspace.
#include "hugs_common.h"

namespace {

typedef float f32x16_t __attribute__((ext_vector_type(16)));

constexpr int EG = 64, ENT = 4096, EWIN = 14, ENW = 25, EWT = 196, EROWS_W = ENW * EWT, ENECK = 256, EMAXD = 1280;
constexpr int PW_G = 256, PO_G = 128, PW_W = 64, PO_W = 32;      // rel-pos product row: [h terms | w terms at PO], width PW

__device__ __forceinline__ int acc_row(int v, int g) { return 8 * (v >> 2) + 4 * g + (v & 3); }
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
// window-order row -> grid row, -1 for a pad row
__device__ __forceinline__ int win_to_grid(int r) {
  const int w = r / EWT, i = r - w * EWT, gy = (w / 5) * EWIN + i / EWIN, gx = (w % 5) * EWIN + i % EWIN;
  return (gy < EG && gx < EG) ? gy * EG + gx : -1;
}

// ---------------------------------------------------------------- GEMM
enum { LD_PLAIN = 0, LD_PATCH = 1, LD_CONV3 = 2 };
enum { EPI_PLAIN = 0, EPI_GELU = 1, EPI_RES = 2, EPI_RESWIN = 3 };
constexpr int BM = 128, BN = 128, BK = 16, LDA_S = BK + 4, LDB_S = BN + 4;

struct GemmArgs {
  int M, N, K;
  const float* A; int lda; long long az;      // az: A offset per blockIdx.z
  const float* Wt;                            // [K][N]
  const float* bias;                          // [N] or NULL
  const float* res; float* out; int ldo; long long oz;      // res may alias out (in-place residual)
  const void* img; int img_u8, h_in, w_in;    // LD_PATCH
};

template <int LOADER>
__device__ __forceinline__ float4 load_a(const GemmArgs& g, const float* A, int row, int k) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (LOADER == LD_PLAIN) {
    if (row < g.M) v = *(const float4*)(A + (size_t)row * g.lda + k);
  } else if (LOADER == LD_PATCH) {
    // row = token (ty, tx); k = (py * 16 + px) * 3 + c; (x - mean) / std, zero outside [h_in, w_in]
    const int y = (row >> 6) * 16 + k / 48, r = k % 48;
    float e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int px = (r + i) / 3, c = (r + i) - 3 * px, x = (row & 63) * 16 + px;
      e[i] = 0.f;
      if (y < g.h_in && x < g.w_in) {
        const size_t at = ((size_t)y * g.w_in + x) * 3 + c;
        const float raw = g.img_u8 ? (float)((const unsigned char*)g.img)[at] : ((const float*)g.img)[at];
        e[i] = (raw - (c == 0 ? 123.675f : c == 1 ? 116.28f : 103.53f)) / (c == 0 ? 58.395f : c == 1 ? 57.12f : 57.375f);
      }
    }
    v = make_float4(e[0], e[1], e[2], e[3]);
  } else {
    // row = (y, x) of the 64 x 64 grid; k = (ky * 3 + kx) * 256 + channel
    const int tap = k >> 8, sy = (row >> 6) + tap / 3 - 1, sx = (row & 63) + tap % 3 - 1;
    if (sy >= 0 && sy < EG && sx >= 0 && sx < EG) v = *(const float4*)(A + (size_t)(sy * EG + sx) * ENECK + (k & 255));
  }
  return v;
}

template <int LOADER, int EPI>
__global__ void __launch_bounds__(256, 2) k_enc_gemm(const GemmArgs g) {
  __shared__ __align__(16) float As[2][BM * LDA_S];
  __shared__ __align__(16) float Bs[2][BK * LDB_S];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5, l32 = lane & 31;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN, wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const float* A = g.A + blockIdx.z * g.az;
  float* out = g.out + blockIdx.z * g.oz;
  // a thread's share of a stage: two float4 of A (rows ar, ar + 64; k offset ak) and two of B (k rows bk, bk + 8; column bc)
  const int ar = tid >> 2, ak = (tid & 3) * 4, bk = tid >> 5, bc = (tid & 31) * 4;
  const bool bok = n0 + bc < g.N;
  float4 pa[2], pb[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      pa[i] = load_a<LOADER>(g, A, m0 + ar + 64 * i, k0 + ak);
      pb[i] = bok ? *(const float4*)(g.Wt + (size_t)(k0 + bk + 8 * i) * g.N + n0 + bc) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *(float4*)(&As[buf][(ar + 64 * i) * LDA_S + ak]) = pa[i];
      *(float4*)(&Bs[buf][(bk + 8 * i) * LDB_S + bc]) = pb[i];
    }
  };
  f32x16_t acc[2][2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[rb][cb][v] = 0.f;
  const int nk = g.K / BK;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s < nk; ++s) {
    const int buf = s & 1;
    if (s + 1 < nk) fetch((s + 1) * BK);
    float a[2][8], b[2][8];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float4 t = *(const float4*)(&As[buf][(wm + rb * 32 + l32) * LDA_S + hf * 8 + q * 4]);
        a[rb][4 * q] = t.x; a[rb][4 * q + 1] = t.y; a[rb][4 * q + 2] = t.z; a[rb][4 * q + 3] = t.w;
      }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int j = 0; j < 8; ++j) b[cb][j] = Bs[buf][(hf * 8 + j) * LDB_S + wn + cb * 32 + l32];
    f32x16_t c[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int v = 0; v < 16; ++v) c[rb][cb][v] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) c[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[rb][j], b[cb][j], c[rb][cb], 0, 0, 0);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) acc[rb][cb] += c[rb][cb];
    if (s + 1 < nk) stash(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int col = n0 + wn + cb * 32 + l32;
    if (col >= g.N) continue;
    const float bb = g.bias ? g.bias[col] : 0.f;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        int row = m0 + wm + rb * 32 + acc_row(v, hf);
        if (row >= g.M) continue;
        float o = acc[rb][cb][v] + bb;
        if (EPI == EPI_GELU) o = gelu_erf(o);
        if (EPI == EPI_RESWIN) {
          row = win_to_grid(row);
          if (row < 0) continue;
        }
        const size_t at = (size_t)row * g.ldo + col;
        if (EPI == EPI_RES || EPI == EPI_RESWIN) o += g.res[at];
        out[at] = o;
      }
  }
}

// ---------------------------------------------------------------- LayerNorm
// out row r = LN(x[src(r)]) over D <= 64 NV channels.  MODE 0: src = r; 1: window order, pad rows zero; 2: src = r, out[c][r]
template <int NV, int MODE>
__global__ void __launch_bounds__(256) k_enc_ln(int rows, int D, const float* __restrict__ x, const float* __restrict__ lng,
                                                const float* __restrict__ lnb, float eps, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int src = MODE == 1 ? win_to_grid(r) : r;
  float v[NV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    v[i] = (src >= 0 && c < D) ? x[(size_t)src * D + c] : 0.f;
    s += v[i];
  }
  const float mean = wave_sum_f(s) / (float)D;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < D ? v[i] - mean : 0.f;
    ss += v[i] * v[i];
  }
  const float rs = 1.f / sqrtf(wave_sum_f(ss) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c >= D) continue;
    const float y = src >= 0 ? v[i] * rs * lng[c] + lnb[c] : 0.f;
    if (MODE == 2) out[(size_t)c * rows + r] = y;
    else out[(size_t)r * D + c] = y;
  }
}

// ---------------------------------------------------------------- attention
// qkv [windows * G^2][3 D] (q | k | v, each [heads][HD]); P [heads][windows * G^2][PW]; out [windows * G^2][D].
// grid: (ceil(G^2 / 128), heads, windows)
template <int HD, int G>
__global__ void __launch_bounds__(256, 2) k_enc_attn(int D, const float* __restrict__ qkv, const float* __restrict__ P,
                                                     float* __restrict__ out) {
  constexpr int NK = G * G, NT = (NK + 63) / 64, LK = HD + 4, LV = HD + 8, NCB = (HD + 31) / 32, H2 = HD / 2;
  constexpr int PW = G == 64 ? PW_G : PW_W, PO = G == 64 ? PO_G : PO_W;
  __shared__ __align__(16) float Ks[64 * LK];
  __shared__ __align__(16) float Vs[64 * LV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5, l32 = lane & 31;
  const int head = blockIdx.y, rows = gridDim.z * NK;
  const size_t row0 = (size_t)blockIdx.z * NK, ld = 3 * (size_t)D;
  const int qi_raw = blockIdx.x * 128 + wave * 32 + l32, qi = qi_raw < NK ? qi_raw : NK - 1;      // a tail lane repeats the last query
  const int qh = qi / G, qw = qi - qh * G;
  const float* Pq = P + ((size_t)head * rows + row0 + qi) * PW;
  float q[H2];
  {
    const float* qp = qkv + (row0 + qi) * ld + head * HD + hf * H2;
#pragma unroll
    for (int j4 = 0; j4 < H2 / 4; ++j4) {
      const float4 t = *(const float4*)(qp + j4 * 4);
      q[4 * j4] = t.x; q[4 * j4 + 1] = t.y; q[4 * j4 + 2] = t.z; q[4 * j4 + 3] = t.w;
    }
  }
  float pw[2][16];      // G = 64: the rel_w terms of this lane's 32 keys of every tile
  if (G == 64) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int v = 0; v < 16; ++v) pw[kb][v] = Pq[PO + qw - (kb * 32 + acc_row(v, hf)) + G - 1];
  }
  const float scale = 1.f / sqrtf((float)HD);
  f32x16_t o[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int v = 0; v < 16; ++v) o[cb][v] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int t = 0; t < NT; ++t) {
    __syncthreads();                                         // every wave is done with the previous tile
    for (int i = tid; i < 64 * (HD / 4); i += 256) {
      const int r = i / (HD / 4), c4 = i - r * (HD / 4), key = t * 64 + r;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (key < NK) {
        const float* kp = qkv + (row0 + key) * ld + D + head * HD + c4 * 4;
        kv = *(const float4*)kp;
        vv = *(const float4*)(kp + D);
      }
      *(float4*)(Ks + r * LK + c4 * 4) = kv;
      *(float4*)(Vs + r * LV + c4 * 4) = vv;
    }
    __syncthreads();
    // S^T [64 keys][32 queries]: block kb holds key kb * 32 + acc_row(v, hf) of query l32 in register v
    f32x16_t s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int v = 0; v < 16; ++v) s[kb][v] = 0.f;
      const float* kp = Ks + (kb * 32 + l32) * LK + hf * H2;
#pragma unroll
      for (int j4 = 0; j4 < H2 / 4; ++j4) {
        const float4 a = *(const float4*)(kp + j4 * 4);
        s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, q[4 * j4], s[kb], 0, 0, 0);
        s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, q[4 * j4 + 1], s[kb], 0, 0, 0);
        s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, q[4 * j4 + 2], s[kb], 0, 0, 0);
        s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, q[4 * j4 + 3], s[kb], 0, 0, 0);
      }
    }
    float ph = 0.f;
    if (G == 64) ph = Pq[qh - t + G - 1];                    // the tile is the key row kh = t
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        float bias;
        bool ok = true;
        if (G == 64) {
          bias = ph + pw[kb][v];
        } else {
          const int key = t * 64 + kb * 32 + acc_row(v, hf);
          ok = key < NK;
          const int kc = ok ? key : NK - 1, kh = kc / G, kw = kc - kh * G;
          bias = Pq[qh - kh + G - 1] + Pq[PO + qw - kw + G - 1];
        }
        s[kb][v] = ok ? s[kb][v] * scale + bias : -INFINITY;
        mx = fmaxf(mx, s[kb][v]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx), al = expf(m - mn);        // (every tile has a valid key: mn is finite)
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        s[kb][v] = expf(s[kb][v] - mn);
        sum += s[kb][v];
      }
    sum += __shfl_xor(sum, 32);
    l = l * al + sum;
    m = mn;
    // O^T [channels][32 queries] += V^T P^T: MFMA j of block kb takes key kb * 32 + acc_row(j, hf) in this half-wave's k slot
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int ch = cb * 32 + l32 < HD ? cb * 32 + l32 : HD - 1;      // (HD = 80: the rows past 80 of the third block are not stored)
      f32x16_t c;
#pragma unroll
      for (int v = 0; v < 16; ++v) c[v] = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int j = 0; j < 16; ++j)
          c = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[(kb * 32 + acc_row(j, hf)) * LV + ch], s[kb][j], c, 0, 0, 0);
#pragma unroll
      for (int v = 0; v < 16; ++v) o[cb][v] = o[cb][v] * al + c[v];
    }
  }
  if (qi_raw >= NK) return;
  const float inv = 1.f / l;
  float* op = out + (row0 + qi) * (size_t)D + head * HD;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int v4 = 0; v4 < 4; ++v4) {
      const int ch = cb * 32 + acc_row(4 * v4, hf);
      if (ch < HD) *(float4*)(op + ch) = make_float4(o[cb][4 * v4] * inv, o[cb][4 * v4 + 1] * inv, o[cb][4 * v4 + 2] * inv, o[cb][4 * v4 + 3] * inv);
    }
}

// ---------------------------------------------------------------- host side
struct BlockW { const float *n1g, *n1b, *Wqkv, *bqkv, *rel, *Wproj, *bproj, *n2g, *n2b, *W1, *b1, *W2, *b2; };
struct EncW {
  const float *Wpatch, *bpatch, *pos;
  const float *Wn1, *l1g, *l1b, *Wn2, *l2g, *l2b;
  long long total;
};

// the order nerf_hugs_amd.hugs.SamImageEncoder packs in; every matrix is [in][out]; rel: [hd][PW] = [rel_pos_h^T | rel_pos_w^T at PO]
static EncW enc_weights(const float* p, int D, int depth, int hd, const int* global_flags, BlockW* blocks) {
  EncW w;
  long long o = 0;
  auto take = [&](long long n) { const float* r = p + o; o += n; return r; };
  const long long d = D;
  w.Wpatch = take(768 * d); w.bpatch = take(d); w.pos = take(ENT * d);
  for (int i = 0; i < depth; ++i) {
    BlockW b;
    b.n1g = take(d); b.n1b = take(d); b.Wqkv = take(3 * d * d); b.bqkv = take(3 * d);
    b.rel = take((long long)hd * (global_flags[i] ? PW_G : PW_W));
    b.Wproj = take(d * d); b.bproj = take(d); b.n2g = take(d); b.n2b = take(d);
    b.W1 = take(4 * d * d); b.b1 = take(4 * d); b.W2 = take(4 * d * d); b.b2 = take(d);
    if (blocks) blocks[i] = b;
  }
  w.Wn1 = take(d * ENECK); w.l1g = take(ENECK); w.l1b = take(ENECK);
  w.Wn2 = take(9ll * ENECK * ENECK); w.l2g = take(ENECK); w.l2b = take(ENECK);
  w.total = o;
  return w;
}

// workspace, in floats
struct EncWs { long long x, y, big, p, n1, n2, total; };
static EncWs enc_ws(long long D, long long heads) {
  EncWs w;
  long long o = 0;
  auto take = [&](long long n) { const long long r = o; o += (n + 3) / 4 * 4; return r; };
  w.x = take(ENT * D);                       // the residual stream, grid order
  w.y = take(EROWS_W * D);                   // LayerNorm output, then the attention output (window order)
  w.big = take(ENT * 4 * D);                 // qkv [4900][3 D], then the MLP's hidden [4096][4 D]
  const long long pg = (long long)ENT * PW_G, pwin = (long long)EROWS_W * PW_W;
  w.p = take(heads * (pg > pwin ? pg : pwin));
  w.n1 = take((long long)ENT * ENECK);
  w.n2 = take((long long)ENT * ENECK);
  w.total = o;
  return w;
}

template <int LOADER, int EPI>
static int enc_gemm(hipStream_t s, int M, int N, int K, const float* A, int lda, const float* Wt, const float* bias, const float* res,
                    float* out, int ldo, int Z = 1, long long az = 0, long long oz = 0, const void* img = nullptr, int u8 = 0,
                    int h_in = 0, int w_in = 0) {
  HUGS_REQUIRE(K % BK == 0 && N % 4 == 0 && lda % 4 == 0, -3, "k_enc_gemm: K %d, N %d, lda %d", K, N, lda);
  const GemmArgs g = {M, N, K, A, lda, az, Wt, bias, res, out, ldo, oz, img, u8, h_in, w_in};
  k_enc_gemm<LOADER, EPI><<<dim3((N + BN - 1) / BN, (M + BM - 1) / BM, Z), 256, 0, s>>>(g);
  HUGS_CHECK_LAUNCH("k_enc_gemm");
  return 0;
}

template <int MODE>
static int enc_ln(hipStream_t s, int rows, int D, const float* x, const float* g, const float* b, float* out) {
  if (D <= 256) k_enc_ln<4, MODE><<<(rows + 3) / 4, 256, 0, s>>>(rows, D, x, g, b, 1e-6f, out);
  else k_enc_ln<EMAXD / 64, MODE><<<(rows + 3) / 4, 256, 0, s>>>(rows, D, x, g, b, 1e-6f, out);
  HUGS_CHECK_LAUNCH("k_enc_ln");
  return 0;
}

template <int G>
static int enc_attn(hipStream_t s, int D, int heads, int hd, const float* qkv, const float* P, float* out) {
  const dim3 grid((G * G + 127) / 128, heads, G == 64 ? 1 : ENW);
  if (hd == 64) k_enc_attn<64, G><<<grid, 256, 0, s>>>(D, qkv, P, out);
  else k_enc_attn<80, G><<<grid, 256, 0, s>>>(D, qkv, P, out);
  HUGS_CHECK_LAUNCH("k_enc_attn");
  return 0;
}

static int enc_check(const char* who, int D, int depth, int heads) {
  HUGS_REQUIRE(D >= 32 && D % 32 == 0 && D <= EMAXD && depth >= 1 && depth <= 64 && heads >= 1 && D % heads == 0 &&
                   (D / heads == 64 || D / heads == 80),
               -2, "%s: D %d, depth %d, heads %d (D a multiple of 32 up to %d, 1 <= depth <= 64, D / heads 64 or 80)", who, D, depth, heads,
               EMAXD);
  return 0;
}

#define ENC_TRY(call) do { if (int rc_ = (call)) return rc_; } while (0)

}  // namespace

extern "C" long long hugs_sam_enc_ws_bytes(int D, int depth, int heads) {
  ENC_TRY(enc_check("hugs_sam_enc_ws_bytes", D, depth, heads));
  return enc_ws(D, heads).total * 4;
}

extern "C" int hugs_sam_enc_encode(int D, int depth, int heads, const float* packed, long long packed_floats, const int* global_flags,
                                   const void* image, int image_u8, int h_in, int w_in, float* ws, float* out, void* stream) {
  ENC_TRY(enc_check("hugs_sam_enc_encode", D, depth, heads));
  HUGS_REQUIRE(packed && global_flags && image && ws && out, -2, "hugs_sam_enc_encode: null pointer");
  HUGS_REQUIRE(h_in >= 1 && w_in >= 1 && h_in <= 1024 && w_in <= 1024, -2, "hugs_sam_enc_encode: image %d x %d (1..1024 each)", h_in, w_in);
  const int hd = D / heads;
  BlockW blk[64];
  const EncW w = enc_weights(packed, D, depth, hd, global_flags, blk);
  HUGS_REQUIRE(packed_floats == w.total, -2, "hugs_sam_enc_encode: %lld packed weight floats, expected %lld", packed_floats, w.total);
  HUGS_REQUIRE((((uintptr_t)packed | (uintptr_t)ws | (uintptr_t)out) & 15) == 0 && (image_u8 || ((uintptr_t)image & 3) == 0), -2,
               "hugs_sam_enc_encode: pointers not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const EncWs L = enc_ws(D, heads);
  float *x = ws + L.x, *y = ws + L.y, *big = ws + L.big, *P = ws + L.p, *n1 = ws + L.n1, *n2 = ws + L.n2;
  // tokens = patch_embed(preprocess(image)) + pos_embed
  ENC_TRY((enc_gemm<LD_PATCH, EPI_RES>(s, ENT, D, 768, nullptr, 4, w.Wpatch, w.bpatch, w.pos, x, D, 1, 0, 0, image, image_u8, h_in, w_in)));
  for (int i = 0; i < depth; ++i) {
    const BlockW& b = blk[i];
    const bool glob = global_flags[i] != 0;
    const int R = glob ? ENT : EROWS_W, pw = glob ? PW_G : PW_W;
    if (glob) ENC_TRY(enc_ln<0>(s, R, D, x, b.n1g, b.n1b, y));
    else ENC_TRY(enc_ln<1>(s, R, D, x, b.n1g, b.n1b, y));
    ENC_TRY((enc_gemm<LD_PLAIN, EPI_PLAIN>(s, R, 3 * D, D, y, D, b.Wqkv, b.bqkv, nullptr, big, 3 * D)));
    // P[head] = q[head] @ [rel_pos_h ; rel_pos_w]^T  (the unscaled q)
    ENC_TRY((enc_gemm<LD_PLAIN, EPI_PLAIN>(s, R, pw, hd, big, 3 * D, b.rel, nullptr, nullptr, P, pw, heads, hd, (long long)R * pw)));
    if (glob) ENC_TRY(enc_attn<EG>(s, D, heads, hd, big, P, y));
    else ENC_TRY(enc_attn<EWIN>(s, D, heads, hd, big, P, y));
    if (glob) ENC_TRY((enc_gemm<LD_PLAIN, EPI_RES>(s, R, D, D, y, D, b.Wproj, b.bproj, x, x, D)));
    else ENC_TRY((enc_gemm<LD_PLAIN, EPI_RESWIN>(s, R, D, D, y, D, b.Wproj, b.bproj, x, x, D)));
    ENC_TRY(enc_ln<0>(s, ENT, D, x, b.n2g, b.n2b, y));
    ENC_TRY((enc_gemm<LD_PLAIN, EPI_GELU>(s, ENT, 4 * D, D, y, D, b.W1, b.b1, nullptr, big, 4 * D)));
    ENC_TRY((enc_gemm<LD_PLAIN, EPI_RES>(s, ENT, D, 4 * D, big, 4 * D, b.W2, b.b2, x, x, D)));
  }
  // neck: 1x1 conv, LayerNorm2d, 3x3 conv, LayerNorm2d -> [256][64 * 64]
  ENC_TRY((enc_gemm<LD_PLAIN, EPI_PLAIN>(s, ENT, ENECK, D, x, D, w.Wn1, nullptr, nullptr, n1, ENECK)));
  ENC_TRY(enc_ln<0>(s, ENT, ENECK, n1, w.l1g, w.l1b, n2));
  ENC_TRY((enc_gemm<LD_CONV3, EPI_PLAIN>(s, ENT, ENECK, 9 * ENECK, n2, ENECK, w.Wn2, nullptr, nullptr, n1, ENECK)));
  ENC_TRY(enc_ln<2>(s, ENT, ENECK, n1, w.l2g, w.l2b, out));
  return 0;
}
