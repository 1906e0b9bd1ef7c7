// SAM's point prompt encoder and mask decoder on the device, fp32 throughout: the per-prompt loop of HuGS/generate_static_mask.py
// :344-351 (predictor.predict_torch for batches of SfM feature points, multimask output), from the image embedding [256,64,64]
// to the low-resolution logits [N,3,256,256] and predicted IoUs.  Matrix products run on v_mfma_f32_32x32x2_f32 (image side)
// and v_mfma_f32_16x16x4_f32 (token side); every K loop sums 32 (128 on the token side) products into a fresh accumulator that
// is then added to the running one, so the rounding error grows with the number of chunks, not with K.
//
// The image side (4096 tokens x 256 channels per prompt, ~3 GFLOP per prompt) is three kernels, each owning 64 image rows of
// one prompt as a complete [64][256] tile in LDS (pitch 260: a lane's 128-bit reads of its own row are conflict-free):
//   * tile_gemm: a wave multiplies the whole 64-row tile by its own 32 or 64 columns of a [K][N] weight.  Every weight element
//     is used by exactly one wave of the workgroup, so weights go from L2 straight into the B operand (a half-wave reads 128
//     contiguous bytes of a weight row); staging them in LDS would add traffic without adding reuse.  Reuse comes from the A
//     tile: one LDS read feeds two (64-column slab) MFMAs and one B register feeds both 32-row blocks.
//   * k_sam_proj: [K | V] = k @ [Wk | Wv] + table.  The positional term of the keys, (k + pos) @ Wk = k @ Wk + pos @ Wk, is a
//     per-image table (pos @ Wk + bk | bv) computed once in hugs_sam_set_image, so the hot kernel never adds pos.
//   * k_sam_i2t: cross_attn_image_to_token + residual + LN4 in one pass.  q = tile @ Wq + table (layer 0: precomputed once per
//     image, the image tokens are still shared by all prompts); softmax over the T <= 16 token keys in registers (one thread per
//     (row, head), online maximum, token K/V in LDS, the result overwrites q in place); out_proj on the MFMA; + residual into
//     the tile; LayerNorm by one wave per row; the new image tokens are stored once.
//   * k_sam_upscale: one row of the 64 x 64 grid.  ConvTranspose2d(k2,s2) is four 1x1 GEMMs, one per sub-pixel: wave s computes
//     sub-pixel s of conv1 (256 -> 64) for the 64 pixels, LayerNorm + GELU run on the tile in LDS, conv2 (64 -> 32) runs per
//     second-level sub-pixel, and after the GELU each lane takes one output pixel's 32 channels and dots them with the three
//     hypernetwork vectors.  The [32,256,256] tensor never leaves the CU.
// The token side (T = P + 6 rows per prompt) is small: the tokens of a chunk of prompts form one flat [nb*T][256] matrix, so
// k_sam_lin pads to the 16-row MFMA tile only at the end of the chunk; the attentions with T queries are VALU kernels
// (k_sam_selfattn; k_sam_t2i_part / _merge split the 4096 keys 32 ways and merge the partial softmaxes).
// Prompts are processed in chunks of SAM_CHUNK so the workspace is bounded.  No atomics: results are bit-reproducible.
#include "hugs_common.h"

namespace {

typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int SC = 256, SNT = 4096, SHID = 128, SMLP = 2048, SAM_CHUNK = 8, SAM_MAXT = 16, SSPLIT = 32;
constexpr int LDX = SC + 4, LDQ = SHID + 4, PART = 18;
constexpr long long MEG = 1 << 20;
// per-image state, in floats
constexpr long long ST_SRC = 0, ST_POS = MEG, ST_PT = 2 * MEG, ST_PQ = 5 * MEG, ST_KV0 = 6 * MEG, ST_Q0 = 7 * MEG, ST_TOTAL = 7 * MEG + MEG / 2;

__device__ __forceinline__ int acc_row(int v, int g) { return 8 * (v >> 2) + 4 * g + (v & 3); }
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

// acc[rb][cb] = As[64][K] (LDS, pitch lda) @ Wt[K][ldw] (global) for the wave's columns col0 + 32 cb + (0..31)
template <int K, int CB>
__device__ __forceinline__ void tile_gemm(const float* As, int lda, const float* __restrict__ Wt, int ldw, int col0, int lane,
                                          f32x16_t (&acc)[2][CB]) {
  const int g = lane >> 5, l32 = lane & 31;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[rb][cb][v] = 0.f;
  for (int kc = 0; kc < K; kc += 32) {
    // the MFMA's two k-slots take k and k + 16 of the chunk: a lane's 16 A values of a row are four 128-bit LDS reads
    float a[2][16];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 t = *(const float4*)(As + (rb * 32 + l32) * lda + kc + g * 16 + q * 4);
        a[rb][4 * q] = t.x; a[rb][4 * q + 1] = t.y; a[rb][4 * q + 2] = t.z; a[rb][4 * q + 3] = t.w;
      }
    const float* wp = Wt + (size_t)(kc + g * 16) * ldw + col0 + l32;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      float b[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) b[j] = wp[(size_t)j * ldw + cb * 32];
      f32x16_t c0, c1;
#pragma unroll
      for (int v = 0; v < 16; ++v) c0[v] = c1[v] = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0][j], b[j], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1][j], b[j], c1, 0, 0, 0);
      }
      acc[0][cb] += c0;
      acc[1][cb] += c1;
    }
  }
}

__device__ __forceinline__ void load_tile(float* Xs, const float* __restrict__ X, int tid) {      // 64 rows x 256 floats
  for (int i = tid; i < 64 * 64; i += 256) {
    const int r = i >> 6, c4 = i & 63;
    *(float4*)(Xs + r * LDX + c4 * 4) = *(const float4*)(X + (size_t)r * SC + c4 * 4);
  }
}

// out[b][row][0 .. 128 CB) = X[b][row][:] @ Wt[256][128 CB] + add[row * ld_add + col]   (ld_add 0: a bias)
template <int CB>
__global__ void __launch_bounds__(256) k_sam_proj(const float* __restrict__ X, long long sx, const float* __restrict__ Wt,
                                                  const float* __restrict__ add, int ld_add, float* __restrict__ out) {
  __shared__ __align__(16) float Xs[64 * LDX];
  constexpr int NOUT = 128 * CB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5, l32 = lane & 31;
  const int r0 = blockIdx.x * 64, b = blockIdx.y;
  load_tile(Xs, X + (size_t)b * sx + (size_t)r0 * SC, tid);
  __syncthreads();
  f32x16_t acc[2][CB];
  tile_gemm<SC, CB>(Xs, LDX, Wt, NOUT, wave * 32 * CB, lane, acc);
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = r0 + rb * 32 + acc_row(v, g), col = wave * 32 * CB + cb * 32 + l32;
        out[((size_t)b * SNT + row) * NOUT + col] = acc[rb][cb][v] + add[(size_t)row * ld_add + col];
      }
}

// kout[b] = LN(kin[b] + out_proj(softmax(q tokK^T / 4) tokV)), q = QPRE ? qpre rows : kin[b] @ Wq + pq; tokKV [b][T][K 128 | V 128]
template <bool QPRE>
__global__ void __launch_bounds__(256) k_sam_i2t(const float* __restrict__ kin, long long sk, float* __restrict__ kout,
                                                 const float* __restrict__ qpre, const float* __restrict__ Wq,
                                                 const float* __restrict__ pq, const float* __restrict__ tokKV, int T,
                                                 const float* __restrict__ Wo, const float* __restrict__ bo,
                                                 const float* __restrict__ lng, const float* __restrict__ lnb, float eps) {
  __shared__ __align__(16) float Xs[64 * LDX];
  __shared__ __align__(16) float Qs[64 * LDQ];
  __shared__ __align__(16) float TK[SAM_MAXT * SC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5, l32 = lane & 31;
  const int r0 = blockIdx.x * 64, b = blockIdx.y;
  load_tile(Xs, kin + (size_t)b * sk + (size_t)r0 * SC, tid);
  for (int i = tid; i < T * 64; i += 256) *(float4*)(TK + i * 4) = *(const float4*)(tokKV + (size_t)b * T * SC + i * 4);
  if (QPRE)
    for (int i = tid; i < 64 * 32; i += 256) {
      const int r = i >> 5, c4 = i & 31;
      *(float4*)(Qs + r * LDQ + c4 * 4) = *(const float4*)(qpre + (size_t)(r0 + r) * SHID + c4 * 4);
    }
  __syncthreads();
  if (!QPRE) {
    f32x16_t qa[2][1];
    tile_gemm<SC, 1>(Xs, LDX, Wq, SHID, wave * 32, lane, qa);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int r = rb * 32 + acc_row(v, g), col = wave * 32 + l32;
        Qs[r * LDQ + col] = qa[rb][0][v] + pq[(size_t)(r0 + r) * SHID + col];
      }
    __syncthreads();
  }
  // attention: one thread per (row, head); the head is wave-uniform, so the token reads are LDS broadcasts
#pragma unroll 1
  for (int p = tid; p < 512; p += 256) {
    const int r = p & 63, h = p >> 6;
    float* qp = Qs + r * LDQ + h * 16;
    float q[16], o[16], m = -INFINITY, l = 0.f;
#pragma unroll
    for (int d4 = 0; d4 < 4; ++d4) {
      const float4 t = *(const float4*)(qp + d4 * 4);
      q[4 * d4] = t.x; q[4 * d4 + 1] = t.y; q[4 * d4 + 2] = t.z; q[4 * d4 + 3] = t.w;
    }
#pragma unroll
    for (int d = 0; d < 16; ++d) o[d] = 0.f;
    for (int t = 0; t < T; ++t) {
      const float* kp = TK + t * SC + h * 16;
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) s += q[d] * kp[d];
      s *= 0.25f;
      const float mn = fmaxf(m, s), al = expf(m - mn), pr = expf(s - mn);
      l = l * al + pr;
#pragma unroll
      for (int d = 0; d < 16; ++d) o[d] = o[d] * al + pr * kp[SHID + d];
      m = mn;
    }
    const float inv = 1.f / l;
#pragma unroll
    for (int d = 0; d < 16; ++d) qp[d] = o[d] * inv;
  }
  __syncthreads();
  f32x16_t acc[2][2];
  tile_gemm<SHID, 2>(Qs, LDQ, Wo, SC, wave * 64, lane, acc);
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int r = rb * 32 + acc_row(v, g), col = wave * 64 + cb * 32 + l32;
        Xs[r * LDX + col] += acc[rb][cb][v] + bo[col];      // (each tile element is owned by one lane)
      }
  __syncthreads();
  const float4 g4 = *(const float4*)(lng + lane * 4), b4 = *(const float4*)(lnb + lane * 4);
  for (int rr = 0; rr < 16; ++rr) {
    const int r = wave * 16 + rr;
    float4 x = *(const float4*)(Xs + r * LDX + lane * 4);
    const float mean = wave_sum_f((x.x + x.y) + (x.z + x.w)) * (1.f / SC);
    x.x -= mean; x.y -= mean; x.z -= mean; x.w -= mean;
    const float var = wave_sum_f((x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w)) * (1.f / SC);
    const float rs = 1.f / sqrtf(var + eps);
    const float4 y = make_float4(x.x * rs * g4.x + b4.x, x.y * rs * g4.y + b4.y, x.z * rs * g4.z + b4.z, x.w * rs * g4.w + b4.w);
    *(float4*)(kout + ((size_t)b * SNT + r0 + r) * SC + lane * 4) = y;
  }
}

// lowres[b][m][4y + 2sy + ty][4x + 2sx + tx] for the grid row y = blockIdx.x; W1 [256][s 4][64], W2 [64][t 4][32], hyper [4][nb][32]
__global__ void __launch_bounds__(256) k_sam_upscale(const float* __restrict__ k, const float* __restrict__ W1,
                                                     const float* __restrict__ b1, const float* __restrict__ lng,
                                                     const float* __restrict__ lnb, const float* __restrict__ W2,
                                                     const float* __restrict__ b2, const float* __restrict__ hyper, int nb,
                                                     float* __restrict__ lowres) {
  __shared__ __align__(16) float Xs[64 * LDX];
  __shared__ float Gs[4][64 * 33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5, l32 = lane & 31;
  const int y = blockIdx.x, b = blockIdx.y;
  load_tile(Xs, k + ((size_t)b * SNT + y * 64) * SC, tid);
  __syncthreads();
  {
    f32x16_t acc[2][2];
    tile_gemm<SC, 2>(Xs, LDX, W1, SC, wave * 64, lane, acc);
    __syncthreads();                                         // every wave has read the input tile: it becomes [px][s][64]
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int v = 0; v < 16; ++v)
          Xs[(rb * 32 + acc_row(v, g)) * LDX + wave * 64 + cb * 32 + l32] = acc[rb][cb][v] + b1[cb * 32 + l32];
  }
  __syncthreads();
  {                                                          // LayerNorm over the 64 channels (eps 1e-6) + GELU: thread = (px, s)
    float* up = Xs + lane * LDX + wave * 64;
    float s = 0.f, ss = 0.f;
    for (int c4 = 0; c4 < 16; ++c4) {
      const float4 t = *(const float4*)(up + c4 * 4);
      s += (t.x + t.y) + (t.z + t.w);
    }
    const float mean = s * (1.f / 64.f);
    for (int c4 = 0; c4 < 16; ++c4) {
      const float4 t = *(const float4*)(up + c4 * 4);
      ss += ((t.x - mean) * (t.x - mean) + (t.y - mean) * (t.y - mean)) + ((t.z - mean) * (t.z - mean) + (t.w - mean) * (t.w - mean));
    }
    const float rs = 1.f / sqrtf(ss * (1.f / 64.f) + 1e-6f);
    for (int c4 = 0; c4 < 16; ++c4) {
      float4 t = *(const float4*)(up + c4 * 4);
      const float4 g4 = *(const float4*)(lng + c4 * 4), b4 = *(const float4*)(lnb + c4 * 4);
      t.x = gelu_erf((t.x - mean) * rs * g4.x + b4.x); t.y = gelu_erf((t.y - mean) * rs * g4.y + b4.y);
      t.z = gelu_erf((t.z - mean) * rs * g4.z + b4.z); t.w = gelu_erf((t.w - mean) * rs * g4.w + b4.w);
      *(float4*)(up + c4 * 4) = t;
    }
  }
  __syncthreads();
  const int sy = wave >> 1, sx = wave & 1;
  const float* hy = hyper + (size_t)b * 32;
  for (int t = 0; t < 4; ++t) {
    f32x16_t acc[2][1];
    tile_gemm<64, 1>(Xs + wave * 64, LDX, W2, 128, t * 32, lane, acc);
    const float bb = b2[l32];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int v = 0; v < 16; ++v) Gs[wave][(rb * 32 + acc_row(v, g)) * 33 + l32] = gelu_erf(acc[rb][0][v] + bb);
    __syncthreads();
    float d[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < 32; ++c) {
      const float gv = Gs[wave][lane * 33 + c];
#pragma unroll
      for (int m = 0; m < 3; ++m) d[m] += gv * hy[(size_t)(m + 1) * nb * 32 + c];
    }
    const int Y = 4 * y + 2 * sy + (t >> 1), X = 4 * lane + 2 * sx + (t & 1);
#pragma unroll
    for (int m = 0; m < 3; ++m) lowres[(((size_t)b * 3 + m) * 256 + Y) * 256 + X] = d[m];
    __syncthreads();
  }
}

// ---------------------------------------------------------------- token side
// out[z][M][N] = act((X [+ X2])[M][K] @ Wt[z][K][N] + bias[z][N]); K % 128 == 0; rows have pitch ldx / ldo
__global__ void __launch_bounds__(256) k_sam_lin(int M, int N, int K, const float* __restrict__ X, int ldx, const float* __restrict__ X2,
                                                 const float* __restrict__ Wt, const float* __restrict__ bias, float* __restrict__ out,
                                                 int ldo, int relu, long long xz, long long wz, long long bz, long long oz) {
  __shared__ __align__(16) float As[16 * LDQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4, z = blockIdx.z;
  X += z * xz; Wt += z * wz; bias += z * bz; out += z * oz;
  if (X2) X2 += z * xz;
  const int m0 = blockIdx.x * 16, c0 = blockIdx.y * 64 + wave * 16, col = c0 + l16;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < K; kc += 128) {
    __syncthreads();
    for (int i = tid; i < 16 * 32; i += 256) {
      const int r = i >> 5, c4 = i & 31;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m0 + r < M) {
        v = *(const float4*)(X + (size_t)(m0 + r) * ldx + kc + c4 * 4);
        if (X2) {
          const float4 u = *(const float4*)(X2 + (size_t)(m0 + r) * ldx + kc + c4 * 4);
          v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
        }
      }
      *(float4*)(As + r * LDQ + c4 * 4) = v;
    }
    __syncthreads();
    if (c0 < N) {                                            // (wave-uniform)
      f32x4_t c = {0.f, 0.f, 0.f, 0.f};
      const float* wp = Wt + (size_t)(kc + kq) * N + (col < N ? col : 0);
#pragma unroll 8
      for (int kk = 0; kk < 128; kk += 4) {
        const float bv = col < N ? wp[(size_t)kk * N] : 0.f;
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(As[l16 * LDQ + kk + kq], bv, c, 0, 0, 0);
      }
      acc += c;
    }
  }
  if (col < N) {
    const float bb = bias[col];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = m0 + 4 * kq + v;
      const float o = acc[v] + bb;
      if (row < M) out[(size_t)row * ldo + col] = relu ? fmaxf(o, 0.f) : o;
    }
  }
}

// out[row] = LN(a[row] + b[row]) over 256 channels (a may be NULL); one wave per row
__global__ void __launch_bounds__(256) k_sam_addln(int rows, const float* a, const float* __restrict__ b, const float* __restrict__ lng,
                                                   const float* __restrict__ lnb, float eps, float* out) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float4 x = *(const float4*)(b + (size_t)r * SC + lane * 4);
  if (a) {
    const float4 u = *(const float4*)(a + (size_t)r * SC + lane * 4);
    x.x += u.x; x.y += u.y; x.z += u.z; x.w += u.w;
  }
  const float mean = wave_sum_f((x.x + x.y) + (x.z + x.w)) * (1.f / SC);
  x.x -= mean; x.y -= mean; x.z -= mean; x.w -= mean;
  const float var = wave_sum_f((x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w)) * (1.f / SC);
  const float rs = 1.f / sqrtf(var + eps);
  const float4 g4 = *(const float4*)(lng + lane * 4), b4 = *(const float4*)(lnb + lane * 4);
  *(float4*)(out + (size_t)r * SC + lane * 4) =
      make_float4(x.x * rs * g4.x + b4.x, x.y * rs * g4.y + b4.y, x.z * rs * g4.z + b4.z, x.w * rs * g4.w + b4.w);
}

// pe(c) for c in [0,1]^2: v = ((2c - 1) @ G) * 2 pi, [sin v | cos v]; thread j of 128 writes channels j and 128 + j
__device__ __forceinline__ void pos_enc(const float* __restrict__ G, float cx, float cy, int j, float& s, float& c) {
  float v = (2.f * cx - 1.f) * G[j] + (2.f * cy - 1.f) * G[128 + j];
  v *= 6.283185307179586f;
  s = sinf(v);
  c = cosf(v);
}

// tokens [b][T][256] = [iou_token; mask_tokens 4; P points; pad]; emb = G 256 | point0 | point1 | not_a_point | no_mask | iou | mask 4
__global__ void __launch_bounds__(128) k_sam_tokens(int P, const float* __restrict__ coords, const int* __restrict__ labels,
                                                    const float* __restrict__ emb, float* __restrict__ tok) {
  const int j = threadIdx.x, b = blockIdx.x, T = P + 6;
  float* o = tok + (size_t)b * T * SC;
  for (int t = 0; t < T; ++t) {
    float lo, hi;
    if (t < 5) {
      const float* e = emb + 256 * (5 + t);
      lo = e[j]; hi = e[128 + j];
    } else if (t == T - 1) {
      lo = emb[768 + j]; hi = emb[768 + 128 + j];
    } else {
      const int i = b * P + t - 5;
      const float* e = emb + (labels[i] > 0 ? 512 : 256);
      pos_enc(emb, (coords[2 * i] + 0.5f) / 1024.f, (coords[2 * i + 1] + 0.5f) / 1024.f, j, lo, hi);
      lo += e[j]; hi += e[128 + j];
    }
    o[t * SC + j] = lo;
    o[t * SC + 128 + j] = hi;
  }
}

// pos[p][256] of grid cell p = 64 i + j: pe(((j + 0.5) / 64, (i + 0.5) / 64)); src[p][c] = embedding[c][p] + no_mask[c]
__global__ void __launch_bounds__(128) k_sam_image(const float* __restrict__ emb, const float* __restrict__ embedding,
                                                   float* __restrict__ pos, float* __restrict__ src) {
  const int j = threadIdx.x, p = blockIdx.x;
  float s, c;
  pos_enc(emb, ((float)(p & 63) + 0.5f) / 64.f, ((float)(p >> 6) + 0.5f) / 64.f, j, s, c);
  pos[(size_t)p * SC + j] = s;
  pos[(size_t)p * SC + 128 + j] = c;
  src[(size_t)p * SC + j] = embedding[(size_t)j * SNT + p] + emb[1024 + j];
  src[(size_t)p * SC + 128 + j] = embedding[(size_t)(128 + j) * SNT + p] + emb[1024 + 128 + j];
}

// self-attention of the tokens: QK [R][q 256 | k 256], V [R][256], 8 heads of 32; thread = (query t, head)
__global__ void __launch_bounds__(128) k_sam_selfattn(int T, const float* __restrict__ QK, const float* __restrict__ V, float* __restrict__ out) {
  const int t = threadIdx.x >> 3, h = threadIdx.x & 7, b = blockIdx.x;
  if (t >= T) return;
  const float* qp = QK + (size_t)(b * T + t) * 512 + h * 32;
  float q[32], o[32], m = -INFINITY, l = 0.f;
#pragma unroll
  for (int d = 0; d < 32; ++d) { q[d] = qp[d]; o[d] = 0.f; }
  for (int u = 0; u < T; ++u) {
    const float* kp = QK + (size_t)(b * T + u) * 512 + 256 + h * 32;
    const float* vp = V + (size_t)(b * T + u) * SC + h * 32;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 32; ++d) s += q[d] * kp[d];
    s *= 0.17677669529663687f;
    const float mn = fmaxf(m, s), al = expf(m - mn), pr = expf(s - mn);
    l = l * al + pr;
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = o[d] * al + pr * vp[d];
    m = mn;
  }
  float* op = out + (size_t)(b * T + t) * SC + h * 32;
#pragma unroll
  for (int d = 0; d < 32; ++d) op[d] = o[d] / l;
}

// token-to-image attention, keys 128 split .. 128 split + 127: part[b][split][(t, head)][max, sum, acc 16]; KV [4096][K 128 | V 128]
__global__ void __launch_bounds__(128) k_sam_t2i_part(int T, const float* __restrict__ Q, const float* __restrict__ KV, long long skv,
                                                      float* __restrict__ part) {
  const int tid = threadIdx.x, t = tid >> 3, h = tid & 7, split = blockIdx.x, b = blockIdx.y;
  if (t >= T) return;
  const float* qp = Q + (size_t)(b * T + t) * SHID + h * 16;
  float q[16], o[16], m = -INFINITY, l = 0.f;
#pragma unroll
  for (int d = 0; d < 16; ++d) { q[d] = qp[d]; o[d] = 0.f; }
  const float* kv = KV + (size_t)b * skv + (size_t)split * (SNT / SSPLIT) * SC + h * 16;
  for (int key = 0; key < SNT / SSPLIT; ++key) {
    const float4* kp = (const float4*)(kv + (size_t)key * SC);
    float s = 0.f;
#pragma unroll
    for (int d4 = 0; d4 < 4; ++d4) {
      const float4 k4 = kp[d4];
      s += q[4 * d4] * k4.x + q[4 * d4 + 1] * k4.y + q[4 * d4 + 2] * k4.z + q[4 * d4 + 3] * k4.w;
    }
    s *= 0.25f;
    const float mn = fmaxf(m, s), al = expf(m - mn), pr = expf(s - mn);
    l = l * al + pr;
#pragma unroll
    for (int d4 = 0; d4 < 4; ++d4) {
      const float4 v4 = kp[32 + d4];
      o[4 * d4] = o[4 * d4] * al + pr * v4.x; o[4 * d4 + 1] = o[4 * d4 + 1] * al + pr * v4.y;
      o[4 * d4 + 2] = o[4 * d4 + 2] * al + pr * v4.z; o[4 * d4 + 3] = o[4 * d4 + 3] * al + pr * v4.w;
    }
    m = mn;
  }
  float* pp = part + (((size_t)b * SSPLIT + split) * 128 + tid) * PART;
  pp[0] = m; pp[1] = l;
#pragma unroll
  for (int d = 0; d < 16; ++d) pp[2 + d] = o[d];
}

__global__ void __launch_bounds__(128) k_sam_t2i_merge(int T, const float* __restrict__ part, float* __restrict__ out) {
  const int tid = threadIdx.x, t = tid >> 3, h = tid & 7, b = blockIdx.x;
  if (t >= T) return;
  const float* pp = part + ((size_t)b * SSPLIT * 128 + tid) * PART;
  float m = -INFINITY;
  for (int s = 0; s < SSPLIT; ++s) m = fmaxf(m, pp[(size_t)s * 128 * PART]);
  float l = 0.f, o[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) o[d] = 0.f;
  for (int s = 0; s < SSPLIT; ++s) {
    const float* ps = pp + (size_t)s * 128 * PART;
    const float w = expf(ps[0] - m);
    l += w * ps[1];
#pragma unroll
    for (int d = 0; d < 16; ++d) o[d] += w * ps[2 + d];
  }
  float* op = out + (size_t)(b * T + t) * SHID + h * 16;
#pragma unroll
  for (int d = 0; d < 16; ++d) op[d] = o[d] / l;
}

// ---------------------------------------------------------------- host side
struct AttnW { const float *Wq, *bq, *Wkv, *bkv, *Wk0, *Wo, *bo, *ng, *nb; };      // a token-to-image attention and its norm
struct LayerW {
  const float *saWqk, *sabqk, *saWv, *sabv, *saWo, *sabo, *n1g, *n1b;
  AttnW t2i;
  const float *W1, *b1, *W2, *b2, *n3g, *n3b;
  const float *iWq, *ibq, *iWk, *ibk, *iWv, *ibv, *iWo, *ibo, *n4g, *n4b;
};
struct SamW {
  const float* emb;                  // G [2][128] | point 0 | point 1 | not_a_point | no_mask | iou token | mask tokens [4][256]
  LayerW L[2];
  AttnW fin;
  const float *uW1, *ub1, *ulg, *ulb, *uW2, *ub2;
  const float *hW[3], *hb[3], *iW[3], *ib[3];
  long long total;
};

// the order nerf_hugs_amd.hugs.SamPointDecoder packs in; every matrix is [in][out]
static SamW sam_weights(const float* p) {
  SamW w;
  long long o = 0;
  auto take = [&](long long n) { const float* r = p + o; o += n; return r; };
  auto attn = [&](AttnW& a) {
    a.Wq = take(SC * SHID); a.bq = take(SHID); a.Wkv = take(SC * SC); a.bkv = take(SC); a.Wk0 = take(SC * SC);
    a.Wo = take(SHID * SC); a.bo = take(SC); a.ng = take(SC); a.nb = take(SC);
  };
  w.emb = take(10 * 256);
  for (int i = 0; i < 2; ++i) {
    LayerW& l = w.L[i];
    l.saWqk = take(SC * 512); l.sabqk = take(512); l.saWv = take(SC * SC); l.sabv = take(SC); l.saWo = take(SC * SC); l.sabo = take(SC);
    l.n1g = take(SC); l.n1b = take(SC);
    attn(l.t2i);
    l.W1 = take(SC * SMLP); l.b1 = take(SMLP); l.W2 = take(SMLP * SC); l.b2 = take(SC); l.n3g = take(SC); l.n3b = take(SC);
    l.iWq = take(SC * SHID); l.ibq = take(SHID); l.iWk = take(SC * SHID); l.ibk = take(SHID); l.iWv = take(SC * SHID); l.ibv = take(SHID);
    l.iWo = take(SHID * SC); l.ibo = take(SC); l.n4g = take(SC); l.n4b = take(SC);
  }
  attn(w.fin);
  w.uW1 = take(SC * SC); w.ub1 = take(64); w.ulg = take(64); w.ulb = take(64); w.uW2 = take(64 * 128); w.ub2 = take(32);
  for (int j = 0; j < 3; ++j) { const int n = j < 2 ? SC : 32; w.hW[j] = take(4ll * SC * n); w.hb[j] = take(4 * n); }
  for (int j = 0; j < 3; ++j) { const int n = j < 2 ? SC : 4; w.iW[j] = take((long long)SC * n); w.ib[j] = take(n); }
  w.total = o;
  return w;
}

// chunk workspace, in floats, for nb prompts of T tokens
struct SamWs { long long tokpe, q, qk, v, att, tmp, h, qt, att128, tokkv, part, k0, k1, kv, hy0, hy1, hyper, io0, io1, total; };
static SamWs sam_ws(long long nb, long long T) {
  SamWs w;
  long long o = 0;
  const long long R = nb * T;
  auto take = [&](long long n) { const long long r = o; o += (n + 3) / 4 * 4; return r; };
  w.tokpe = take(R * SC); w.q = take(R * SC); w.qk = take(R * 512); w.v = take(R * SC); w.att = take(R * SC); w.tmp = take(R * SC);
  w.h = take(R * SMLP); w.qt = take(R * SHID); w.att128 = take(R * SHID); w.tokkv = take(R * SC);
  w.part = take(nb * SSPLIT * 128 * PART);
  w.k0 = take(nb * SNT * SC); w.k1 = take(nb * SNT * SC); w.kv = take(nb * SNT * SC);
  w.hy0 = take(4 * nb * SC); w.hy1 = take(4 * nb * SC); w.hyper = take(4 * nb * 32); w.io0 = take(nb * SC); w.io1 = take(nb * SC);
  w.total = o;
  return w;
}

static int sam_lin(hipStream_t s, int M, int N, int K, const float* X, int ldx, const float* X2, const float* Wt, const float* b,
                   float* out, int ldo, int relu, int Z = 1, long long xz = 0, long long wz = 0, long long bz = 0, long long oz = 0) {
  k_sam_lin<<<dim3((M + 15) / 16, (N + 63) / 64, Z), 256, 0, s>>>(M, N, K, X, ldx, X2, Wt, b, out, ldo, relu, xz, wz, bz, oz);
  HUGS_CHECK_LAUNCH("k_sam_lin");
  return 0;
}

#define SAM_TRY(call) do { if (int rc_ = (call)) return rc_; } while (0)

// q = LN(q + out_proj(attention(q + tokpe over the image keys)))
static int sam_t2i(hipStream_t s, int nb, int T, const AttnW& a, const float* kv, long long skv, float* ws, const SamWs& L, float eps) {
  const int R = nb * T;
  SAM_TRY(sam_lin(s, R, SHID, SC, ws + L.q, SC, ws + L.tokpe, a.Wq, a.bq, ws + L.qt, SHID, 0));
  k_sam_t2i_part<<<dim3(SSPLIT, nb), 128, 0, s>>>(T, ws + L.qt, kv, skv, ws + L.part);
  HUGS_CHECK_LAUNCH("k_sam_t2i_part");
  k_sam_t2i_merge<<<nb, 128, 0, s>>>(T, ws + L.part, ws + L.att128);
  HUGS_CHECK_LAUNCH("k_sam_t2i_merge");
  SAM_TRY(sam_lin(s, R, SC, SHID, ws + L.att128, SHID, nullptr, a.Wo, a.bo, ws + L.tmp, SC, 0));
  k_sam_addln<<<(R + 3) / 4, 256, 0, s>>>(R, ws + L.q, ws + L.tmp, a.ng, a.nb, eps, ws + L.q);
  HUGS_CHECK_LAUNCH("k_sam_addln");
  return 0;
}

}  // namespace

extern "C" long long hugs_sam_ws_bytes(int N, int P) {
  HUGS_REQUIRE(N >= 0 && P >= 1 && P + 6 <= SAM_MAXT, -2, "hugs_sam_ws_bytes: %d prompts of %d points (N >= 0, 1 <= P <= %d)", N, P,
               SAM_MAXT - 6);
  if (N == 0) return ST_TOTAL * 4;
  return sam_ws(N < SAM_CHUNK ? N : SAM_CHUNK, P + 6).total * 4;
}

extern "C" int hugs_sam_set_image(const float* packed, long long packed_floats, const float* embedding, float* state, void* stream) {
  HUGS_REQUIRE(packed && embedding && state, -2, "hugs_sam_set_image: null pointer");
  const SamW w = sam_weights(packed);
  HUGS_REQUIRE(packed_floats == w.total, -2, "hugs_sam_set_image: %lld packed weight floats, expected %lld", packed_floats, w.total);
  HUGS_REQUIRE((((uintptr_t)packed | (uintptr_t)embedding | (uintptr_t)state) & 15) == 0, -2, "hugs_sam_set_image: pointers not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float *src = state + ST_SRC, *pos = state + ST_POS;
  k_sam_image<<<SNT, 128, 0, s>>>(w.emb, embedding, pos, src);
  HUGS_CHECK_LAUNCH("k_sam_image");
  const dim3 grid(SNT / 64, 1);
  const AttnW* t2i[3] = {&w.L[0].t2i, &w.L[1].t2i, &w.fin};
  for (int j = 0; j < 3; ++j) {       // key / value tables: pos @ Wk + bk | bv
    k_sam_proj<2><<<grid, 256, 0, s>>>(pos, 0, t2i[j]->Wk0, t2i[j]->bkv, 0, state + ST_PT + j * MEG);
    HUGS_CHECK_LAUNCH("k_sam_proj");
  }
  for (int j = 0; j < 2; ++j) {       // image-to-token query tables: pos @ Wq + bq
    k_sam_proj<1><<<grid, 256, 0, s>>>(pos, 0, w.L[j].iWq, w.L[j].ibq, 0, state + ST_PQ + j * (MEG / 2));
    HUGS_CHECK_LAUNCH("k_sam_proj");
  }
  k_sam_proj<2><<<grid, 256, 0, s>>>(src, 0, w.L[0].t2i.Wkv, state + ST_PT, SC, state + ST_KV0);
  HUGS_CHECK_LAUNCH("k_sam_proj");
  k_sam_proj<1><<<grid, 256, 0, s>>>(src, 0, w.L[0].iWq, state + ST_PQ, SHID, state + ST_Q0);
  HUGS_CHECK_LAUNCH("k_sam_proj");
  return 0;
}

extern "C" int hugs_sam_predict(int N, int P, const float* coords, const int* labels, const float* packed, long long packed_floats,
                                float ln_eps, const float* state, float* ws, float* lowres, float* iou4, void* stream) {
  HUGS_REQUIRE(N >= 1 && P >= 1 && P + 6 <= SAM_MAXT, -2, "hugs_sam_predict: %d prompts of %d points (N >= 1, 1 <= P <= %d)", N, P,
               SAM_MAXT - 6);
  HUGS_REQUIRE(coords && labels && packed && state && ws && lowres && iou4, -2, "hugs_sam_predict: null pointer");
  const SamW w = sam_weights(packed);
  HUGS_REQUIRE(packed_floats == w.total, -2, "hugs_sam_predict: %lld packed weight floats, expected %lld", packed_floats, w.total);
  HUGS_REQUIRE((((uintptr_t)packed | (uintptr_t)state | (uintptr_t)ws | (uintptr_t)lowres) & 15) == 0, -2,
               "hugs_sam_predict: pointers not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int T = P + 6;
  const SamWs L = sam_ws(N < SAM_CHUNK ? N : SAM_CHUNK, T);
  const long long KS = (long long)SNT * SC;
  for (int n0 = 0; n0 < N; n0 += SAM_CHUNK) {
    const int nb = N - n0 < SAM_CHUNK ? N - n0 : SAM_CHUNK, R = nb * T;
    const dim3 gimg(SNT / 64, nb);
    float *tokpe = ws + L.tokpe, *q = ws + L.q, *tmp = ws + L.tmp, *kbuf[2] = {ws + L.k0, ws + L.k1};
    k_sam_tokens<<<nb, 128, 0, s>>>(P, coords + (size_t)n0 * P * 2, labels + (size_t)n0 * P, w.emb, tokpe);
    HUGS_CHECK_LAUNCH("k_sam_tokens");
    for (int i = 0; i < 2; ++i) {
      const LayerW& l = w.L[i];
      // 1. self-attention (layer 0: on the bare tokens, replacing them)
      SAM_TRY(sam_lin(s, R, 512, SC, i ? q : tokpe, SC, i ? tokpe : nullptr, l.saWqk, l.sabqk, ws + L.qk, 512, 0));
      SAM_TRY(sam_lin(s, R, SC, SC, i ? q : tokpe, SC, nullptr, l.saWv, l.sabv, ws + L.v, SC, 0));
      k_sam_selfattn<<<nb, 128, 0, s>>>(T, ws + L.qk, ws + L.v, ws + L.att);
      HUGS_CHECK_LAUNCH("k_sam_selfattn");
      SAM_TRY(sam_lin(s, R, SC, SC, ws + L.att, SC, nullptr, l.saWo, l.sabo, tmp, SC, 0));
      k_sam_addln<<<(R + 3) / 4, 256, 0, s>>>(R, i ? q : nullptr, tmp, l.n1g, l.n1b, ln_eps, q);
      HUGS_CHECK_LAUNCH("k_sam_addln");
      // 2. tokens attend to the image (layer 0: the image tokens are still the shared ones)
      SAM_TRY(sam_t2i(s, nb, T, l.t2i, i ? ws + L.kv : state + ST_KV0, i ? KS : 0, ws, L, ln_eps));
      // 3. MLP
      SAM_TRY(sam_lin(s, R, SMLP, SC, q, SC, nullptr, l.W1, l.b1, ws + L.h, SMLP, 1));
      SAM_TRY(sam_lin(s, R, SC, SMLP, ws + L.h, SMLP, nullptr, l.W2, l.b2, tmp, SC, 0));
      k_sam_addln<<<(R + 3) / 4, 256, 0, s>>>(R, q, tmp, l.n3g, l.n3b, ln_eps, q);
      HUGS_CHECK_LAUNCH("k_sam_addln");
      // 4. the image attends to the tokens; from here the image tokens are per prompt
      SAM_TRY(sam_lin(s, R, SHID, SC, q, SC, tokpe, l.iWk, l.ibk, ws + L.tokkv, SC, 0));
      SAM_TRY(sam_lin(s, R, SHID, SC, q, SC, nullptr, l.iWv, l.ibv, ws + L.tokkv + SHID, SC, 0));
      if (i == 0)
        k_sam_i2t<true><<<gimg, 256, 0, s>>>(state + ST_SRC, 0, kbuf[0], state + ST_Q0, nullptr, nullptr, ws + L.tokkv, T, l.iWo, l.ibo,
                                             l.n4g, l.n4b, ln_eps);
      else
        k_sam_i2t<false><<<gimg, 256, 0, s>>>(kbuf[0], KS, kbuf[1], nullptr, l.iWq, state + ST_PQ + MEG / 2, ws + L.tokkv, T, l.iWo,
                                              l.ibo, l.n4g, l.n4b, ln_eps);
      HUGS_CHECK_LAUNCH("k_sam_i2t");
      const AttnW& nx = i == 0 ? w.L[1].t2i : w.fin;         // keys / values of the next token-to-image attention
      k_sam_proj<2><<<gimg, 256, 0, s>>>(kbuf[i], KS, nx.Wkv, state + ST_PT + (i + 1) * MEG, SC, ws + L.kv);
      HUGS_CHECK_LAUNCH("k_sam_proj");
    }
    SAM_TRY(sam_t2i(s, nb, T, w.fin, ws + L.kv, KS, ws, L, ln_eps));
    // heads: hyper[m] = MLP_m(mask token m), iou = MLP(iou token); rows have pitch T * 256 in q
    float *h0 = ws + L.hy0, *h1 = ws + L.hy1, *hyper = ws + L.hyper;
    SAM_TRY(sam_lin(s, nb, SC, SC, q + SC, T * SC, nullptr, w.hW[0], w.hb[0], h0, SC, 1, 4, SC, SC * SC, SC, (long long)nb * SC));
    SAM_TRY(sam_lin(s, nb, SC, SC, h0, SC, nullptr, w.hW[1], w.hb[1], h1, SC, 1, 4, (long long)nb * SC, SC * SC, SC, (long long)nb * SC));
    SAM_TRY(sam_lin(s, nb, 32, SC, h1, SC, nullptr, w.hW[2], w.hb[2], hyper, 32, 0, 4, (long long)nb * SC, SC * 32, 32, (long long)nb * 32));
    SAM_TRY(sam_lin(s, nb, SC, SC, q, T * SC, nullptr, w.iW[0], w.ib[0], ws + L.io0, SC, 1));
    SAM_TRY(sam_lin(s, nb, SC, SC, ws + L.io0, SC, nullptr, w.iW[1], w.ib[1], ws + L.io1, SC, 1));
    SAM_TRY(sam_lin(s, nb, 4, SC, ws + L.io1, SC, nullptr, w.iW[2], w.ib[2], iou4 + (size_t)n0 * 4, 4, 0));
    k_sam_upscale<<<dim3(64, nb), 256, 0, s>>>(kbuf[1], w.uW1, w.ub1, w.ulg, w.ulb, w.uW2, w.ub2, hyper, nb,
                                               lowres + (size_t)n0 * 3 * 65536);
    HUGS_CHECK_LAUNCH("k_sam_upscale");
  }
  return 0;
}
