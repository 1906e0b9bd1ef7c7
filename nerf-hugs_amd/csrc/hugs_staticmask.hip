// HuGS static masks on the device: everything HuGS/generate_static_mask.py does after SAM has run (lines 110-145, 239-275,
// 344-407).  All masks are [H,W] fp32 0/1 planes (the reference's own representation; a pixel is set when its value is >= 0.5);
// every decision is made on integers, so the results do not depend on launch geometry or on the order atomics land in.
//
//   1. residual + thresholds (:269-275).  k_rs_residual writes mean_c |pred - gt| and one fp64 partial sum per workgroup (fixed
//      grid, fixed order).  The two order statistics of torch.quantile are found by a radix select over the monotone key of the
//      fp32 bit pattern: three passes of (k_rs_hist: LDS-privatised 2048-bin histogram of the current digit of the keys that share
//      the prefix found so far, one histogram per wanted rank, flushed with integer atomics; k_rs_scan: one wave per rank walks
//      the bins, fixes the digit, and clears the bins for the next pass).  The last scan sums the partials in block order and
//      lerps in fp32 in torch's form; k_rs_masks compares.
//   2. SfM masks (:344-377).  k_sfm_bits streams the [N,H*W] logits once with 16-byte loads: lane l of a wave holds pixels
//      256c + 4l + j (j = 0..3) of chunk c, so ballot j is a 64-bit word whose bit l is pixel 256c + 4l + j -- plane word 4c + j
//      of mask n.  The same loads give the popcounts of (> thr + off) and (> thr - off); a workgroup adds them into two int32
//      counters per mask.  k_sfm_keep takes the IoU / stability decisions (int counts, the quotient rounded once to fp32: a
//      double quotient of two integers below 2^24 rounds to the correctly rounded fp32 one).  k_sfm_accum reads only the planes
//      of kept masks (wave-uniform 8-byte loads) and adds them to the caller's int32 count map, one lane per four pixels.
//   3. labels of the uncovered pixels (:243-259): connected components of seg < 0 under {up, left, up-left} and their
//      mirrors.  k_lab_local runs a union-find (atomicMin on the parent, roots are the smallest index) on a 64x16 tile in LDS and
//      writes parents as global pixel indices; k_lab_border unites across the tiles' top rows and left columns in the global
//      parent array; k_lab_flatten points every pixel at its root; k_lab_final writes S + root (or seg where covered).  The parent
//      array is the output array.
//   4. fill_gap / combine + smooth / erode (:110-125, :386-407): one tile kernel, k_sm_box<SRC>.  A workgroup owns 64x32 pixels,
//      ballots the source predicate of the tile and its halo (<= 7) into LDS as three 64-bit words per row (left / own / right
//      64 columns), and a lane gets the box count of its pixel from k popcounts of a k-bit window funnel-shifted out of those
//      words.  pad: 0 zeros (conv2d 'same'), 1 reflect (fill_gap), 2 ones (cv2.erode's border).  rule 0: m | 2 count >= k^2
//      (= (box(m) + m >= 0.5): the margin to the nearest other count is 0.5 / k^2 >= 1/450, far above fp32 rounding); rule 1:
//      count == k^2 (erode).  SRC 0: an fp32 mask; 1: count map >= 1; 2: (sfm | base) & upper, also written out; 3: the
//      intersect_masks selection of the pixel's label, so the selected mask is never stored.
//   5. intersect_masks for a partition (:128-145): k_lab_hist counts area[l] and inter[l] = #(coarse & l).  A wave takes 64
//      consecutive pixels, finds the runs of equal labels with two ballots and lets the head lane of a run add (length, popcount
//      of the coarse ballot under the run) -- to LDS counters for labels < 2048, to the global table (indexed by the label, i.e. by
//      S + root pixel for new components) otherwise.  selected(l) = inter * den >= num * area in 64-bit integers.
#include "hugs_common.h"
#include "hugs_maskops.h"

namespace {

constexpr int SM_T = 256;
constexpr int SM_MAXPIX = 1 << 24;     // every count is exact in fp32 and int32
constexpr int SM_MAXK = 15;

// ---------------------------------------------------------------- 1. residual, mean, quantile
constexpr int RS_MAXB = 1024;          // workgroups of the residual pass: the summation order is a function of H*W alone
constexpr int RS_BINS = 2048;
struct RsWs {
  double part[RS_MAXB];
  uint32_t hist[2][RS_BINS];
  uint32_t prefix[2], rank[2];
};

static int rs_blocks(int n) {
  const int b = (n + SM_T - 1) / SM_T;
  return b < RS_MAXB ? b : RS_MAXB;
}

// monotone map of the fp32 order onto uint32 (residuals are >= 0; the map is total anyway)
__device__ __forceinline__ uint32_t rs_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rs_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ void __launch_bounds__(SM_T) k_rs_residual(int n, const float* __restrict__ pred, const float* __restrict__ gt,
                                                      float* __restrict__ res, RsWs* ws, uint32_t k0, uint32_t k1) {
  __shared__ double red[SM_T / HUGS_WAVE];
  const int tid = threadIdx.x;
  double s = 0.;
  for (int i = blockIdx.x * SM_T + tid; i < n; i += gridDim.x * SM_T) {
    const size_t o = (size_t)i * 3;
    const float r = (fabsf(pred[o] - gt[o]) + fabsf(pred[o + 1] - gt[o + 1]) + fabsf(pred[o + 2] - gt[o + 2])) / 3.f;
    res[i] = r;
    s += (double)r;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) ws->part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  if (blockIdx.x == 0) {                       // the select's state; the histogram passes are later launches
    for (int b = tid; b < 2 * RS_BINS; b += SM_T) ws->hist[0][b] = 0;
    if (tid == 0) {
      ws->prefix[0] = ws->prefix[1] = 0;
      ws->rank[0] = k0;
      ws->rank[1] = k1;
    }
  }
}

// pass p looks at digit (key >> shift) & (bins - 1) of the keys whose bits above the digit equal the rank's prefix
__global__ void __launch_bounds__(SM_T) k_rs_hist(int n, const float* __restrict__ res, RsWs* ws, int pass, int shift, int bins) {
  __shared__ uint32_t h[2][RS_BINS];
  const int tid = threadIdx.x;
  for (int b = tid; b < 2 * RS_BINS; b += SM_T) h[0][b] = 0;
  __syncthreads();
  const uint32_t p0 = ws->prefix[0], p1 = ws->prefix[1];
  const int mshift = shift + (bins == 1024 ? 10 : 11);      // (only read when pass > 0: then it is < 32)
  for (int i = blockIdx.x * SM_T + tid; i < n; i += gridDim.x * SM_T) {
    const uint32_t key = rs_key(res[i]);
    const uint32_t d = (key >> shift) & (uint32_t)(bins - 1);
    if (pass == 0 || ((key ^ p0) >> mshift) == 0) atomicAdd(&h[0][d], 1u);
    if (pass == 0 || ((key ^ p1) >> mshift) == 0) atomicAdd(&h[1][d], 1u);
  }
  __syncthreads();
  for (int b = tid; b < 2 * RS_BINS; b += SM_T) {
    const uint32_t v = h[0][b];
    if (v) atomicAdd(&ws->hist[0][b], v);
  }
}

// torch's lerp (aten/native/Lerp.h): the form is chosen by the weight
__device__ __forceinline__ float rs_lerp(float a, float b, float w) {
  const float d = __fsub_rn(b, a);
  return w < 0.5f ? __fadd_rn(a, __fmul_rn(w, d)) : __fsub_rn(b, __fmul_rn(d, __fsub_rn(1.f, w)));
}

__global__ void __launch_bounds__(128) k_rs_scan(int n, int nblk, RsWs* ws, int shift, int last, float w, float* __restrict__ thr) {
  const int tid = threadIdx.x, lane = tid & 63, r = tid >> 6;      // wave r owns rank r
  const uint32_t* h = ws->hist[r];
  uint32_t sum = 0;
  for (int b = 0; b < 32; ++b) sum += h[lane * 32 + b];
  uint32_t incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  const uint32_t excl = incl - sum, rank = ws->rank[r];
  uint32_t digit = 0, left = 0;
  const bool mine = rank >= excl && rank < incl;       // exactly one lane: the bins of a rank's prefix hold more keys than the rank
  if (mine) {
    uint32_t cum = excl;
    for (int b = 0; b < 32; ++b) {
      const uint32_t c = h[lane * 32 + b];
      if (rank < cum + c) { digit = lane * 32 + b; left = rank - cum; break; }
      cum += c;
    }
  }
  __syncthreads();                                      // every read of the bins is done
  if (mine) {
    ws->prefix[r] |= digit << shift;
    ws->rank[r] = left;
  }
  for (int b = tid; b < 2 * RS_BINS; b += 128) ws->hist[0][b] = 0;
  if (!last) return;
  __syncthreads();
  if (r == 0) {
    double s = 0.;
    for (int b = lane; b < nblk; b += 64) s += ws->part[b];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
    if (lane == 0) {
      thr[0] = (float)(s / (double)n);
      thr[1] = rs_lerp(rs_unkey(ws->prefix[0]), rs_unkey(ws->prefix[1]), w);
    }
  }
}

__global__ void __launch_bounds__(SM_T) k_rs_masks(int n, const float* __restrict__ res, const float* __restrict__ thr,
                                                   float* __restrict__ base, float* __restrict__ upper) {
  const float tb = thr[0], tu = thr[1];
  for (int i = blockIdx.x * SM_T + threadIdx.x; i < n; i += gridDim.x * SM_T) {
    const float r = res[i];
    const bool b = r <= tb;
    base[i] = b ? 1.f : 0.f;
    upper[i] = (b || r <= tu) ? 1.f : 0.f;
  }
}

// ---------------------------------------------------------------- 2. SfM masks
constexpr int SFM_CPB = 16;            // 256-pixel chunks per workgroup (four per wave)
typedef float sm_f4 __attribute__((ext_vector_type(4)));

static inline int sfm_chunks(int npix) { return (npix + 255) / 256; }

__global__ void __launch_bounds__(SM_T) k_sm_zero_i32(long long n, int* __restrict__ p) {
  for (long long i = (long long)blockIdx.x * SM_T + threadIdx.x; i < n; i += (long long)gridDim.x * SM_T) p[i] = 0;
}

template <bool VEC>
__global__ void __launch_bounds__(SM_T) k_sfm_bits(int npix, int nchunk, const float* __restrict__ logits, float thr, float thi,
                                                   float tlo, unsigned long long* __restrict__ bits, int* __restrict__ cnt) {
  __shared__ int red[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = blockIdx.y;
  if (tid < 2) red[tid] = 0;
  __syncthreads();
  const float* L = logits + (size_t)m * npix;
  unsigned long long* B = bits + (size_t)m * nchunk * 4;
  const int c1 = min((blockIdx.x + 1) * SFM_CPB, nchunk);
  int ci = 0, cu = 0;
  for (int c = blockIdx.x * SFM_CPB + wave; c < c1; c += SM_T / HUGS_WAVE) {
    const int p = c * 256 + 4 * lane;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    bool ok[4];
    if (VEC) {                                            // npix % 4 == 0: a lane's four pixels are all inside or all outside
      const bool in = p < npix;
      if (in) {
        const sm_f4 q = __builtin_nontemporal_load((const sm_f4*)(L + p));
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) ok[j] = in;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ok[j] = p + j < npix;
        if (ok[j]) v[j] = L[p + j];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long b = __ballot(ok[j] && v[j] > thr);
      ci += __popcll(__ballot(ok[j] && v[j] > thi));
      cu += __popcll(__ballot(ok[j] && v[j] > tlo));
      if (lane == 0) B[4 * c + j] = b;
    }
  }
  if (lane == 0) {
    atomicAdd(&red[0], ci);
    atomicAdd(&red[1], cu);
  }
  __syncthreads();
  if (tid < 2 && red[tid]) atomicAdd(&cnt[2 * m + tid], red[tid]);
}

__global__ void __launch_bounds__(SM_T) k_sfm_keep(int N, const float* __restrict__ iou, float iou_thresh, float stab_thresh,
                                                   const int* __restrict__ cnt, int* __restrict__ keep) {
  const int m = blockIdx.x * SM_T + threadIdx.x;
  if (m >= N) return;
  bool k = true;
  if (iou_thresh > 0.f) k = iou[m] > iou_thresh;
  if (stab_thresh > 0.f) {
    const float s = (float)((double)cnt[2 * m] / (double)cnt[2 * m + 1]);      // 0/0 = NaN: dropped
    k = k && s >= stab_thresh;
  }
  keep[m] = k ? 1 : 0;
}

__global__ void __launch_bounds__(SM_T) k_sfm_accum(int npix, int nchunk, int N, const unsigned long long* __restrict__ bits,
                                                    const int* __restrict__ keep, int* __restrict__ count) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * (SM_T / HUGS_WAVE) + (threadIdx.x >> 6);
  if (c >= nchunk) return;
  int a[4] = {0, 0, 0, 0};
  for (int m = 0; m < N; ++m) {
    if (!keep[m]) continue;
    const unsigned long long* B = bits + ((size_t)m * nchunk + c) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] += (int)((B[j] >> lane) & 1ull);
  }
  const int p = c * 256 + 4 * lane;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (p + j < npix && a[j]) count[p + j] += a[j];
}

// ---------------------------------------------------------------- 2b. SfM masks from the decoder's 256 x 256 logits
// SAM's postprocess_masks (bilinear 256 -> 1024, crop [:h_in, :w_in], bilinear -> H x W; align_corners = False) evaluated per
// output pixel: each axis composes to two crop-grid taps of two low-res taps each.  The full-resolution logit is never stored:
// k_lr_count recomputes it for the stability counts, k_lr_accum for the kept masks -- by the same function, so both passes see
// the same bits.
// mask j of the batch: the prompt's first highest-IoU mask (torch.argmax), or all 3 N in order; clears the counters
__global__ void __launch_bounds__(SM_T) k_lr_select(int M, int highest, const float* __restrict__ iou, int* __restrict__ sel,
                                                    float* __restrict__ iou_sel, int* __restrict__ cnt) {
  const int j = blockIdx.x * SM_T + threadIdx.x;
  if (j >= M) return;
  int s = j;
  if (highest) {
    const float a = iou[3 * j], b = iou[3 * j + 1], c = iou[3 * j + 2];
    s = 3 * j + (a >= b ? (a >= c ? 0 : 2) : (b >= c ? 1 : 2));
  }
  sel[j] = s;
  iou_sel[j] = iou[s];
  cnt[2 * j] = cnt[2 * j + 1] = 0;
}

__global__ void __launch_bounds__(SM_T) k_lr_count(int H, int W, float sy, float sx, int h_in, int w_in, const float* __restrict__ lowres,
                                                   const int* __restrict__ sel, float thi, float tlo, int* __restrict__ cnt) {
  __shared__ int red[2];
  const int tid = threadIdx.x, j = blockIdx.y, npix = H * W;
  if (tid < 2) red[tid] = 0;
  __syncthreads();
  const float* L = lowres + (size_t)sel[j] * LR * LR;
  int ci = 0, cu = 0;
  for (int p = blockIdx.x * SM_T + tid; p < npix; p += gridDim.x * SM_T) {
    const int py = p / W, px = p - py * W;
    const float v = lr_logit(L, lr_axis(py, sy, h_in), lr_axis(px, sx, w_in));
    ci += v > thi;
    cu += v > tlo;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { ci += __shfl_xor(ci, d); cu += __shfl_xor(cu, d); }
  if ((tid & 63) == 0) {
    atomicAdd(&red[0], ci);
    atomicAdd(&red[1], cu);
  }
  __syncthreads();
  if (tid < 2 && red[tid]) atomicAdd(&cnt[2 * j + tid], red[tid]);
}

__global__ void __launch_bounds__(SM_T) k_lr_accum(int H, int W, float sy, float sx, int h_in, int w_in, int M, const float* __restrict__ lowres,
                                                   const int* __restrict__ sel, const int* __restrict__ keep, float thr, int* __restrict__ count) {
  const int p = blockIdx.x * SM_T + threadIdx.x;
  if (p >= H * W) return;
  const int py = p / W, px = p - py * W;
  const LrAxis ay = lr_axis(py, sy, h_in), ax = lr_axis(px, sx, w_in);
  int a = 0;
  for (int j = 0; j < M; ++j)
    if (keep[j]) a += lr_logit(lowres + (size_t)sel[j] * LR * LR, ay, ax) > thr;
  if (a) count[p] += a;
}

// ---------------------------------------------------------------- 3. labels of the uncovered pixels
constexpr int LB_W = 64, LB_H = 16;

__global__ void __launch_bounds__(SM_T) k_lab_local(int H, int W, int tx, const int* __restrict__ seg, int* __restrict__ P) {
  __shared__ int L[LB_W * LB_H];
  const int x0 = (blockIdx.x % tx) * LB_W, y0 = (blockIdx.x / tx) * LB_H, tid = threadIdx.x;
  for (int e = tid; e < LB_W * LB_H; e += SM_T) {
    const int gx = x0 + (e & 63), gy = y0 + (e >> 6);
    L[e] = (gx < W && gy < H && seg[(size_t)gy * W + gx] < 0) ? e : -1;
  }
  __syncthreads();
  volatile int* V = L;
  for (int e = tid; e < LB_W * LB_H; e += SM_T) {
    if (V[e] < 0) continue;
    const int lx = e & 63, ly = e >> 6;
    if (lx > 0 && V[e - 1] >= 0) uf_unite(L, e, e - 1);
    if (ly > 0 && V[e - LB_W] >= 0) uf_unite(L, e, e - LB_W);
    if (lx > 0 && ly > 0 && V[e - LB_W - 1] >= 0) uf_unite(L, e, e - LB_W - 1);
  }
  __syncthreads();
  for (int e = tid; e < LB_W * LB_H; e += SM_T) {
    const int gx = x0 + (e & 63), gy = y0 + (e >> 6);
    if (gx >= W || gy >= H) continue;
    int out = -1;
    if (V[e] >= 0) {
      const int r = uf_find(V, e);                      // local row-major order agrees with the global one inside a tile
      out = (y0 + (r >> 6)) * W + x0 + (r & 63);
    }
    P[(size_t)gy * W + gx] = out;
  }
}

// the 64 pixels of a tile's top row and the 15 below its corner in the left column: their up / left / up-left neighbours
// lie in another tile
__global__ void __launch_bounds__(128) k_lab_border(int H, int W, int tx, int* __restrict__ P) {
  const int tid = threadIdx.x;
  if (tid >= LB_W + LB_H - 1) return;
  const int lx = tid < LB_W ? tid : 0, ly = tid < LB_W ? 0 : tid - LB_W + 1;
  const int x = (blockIdx.x % tx) * LB_W + lx, y = (blockIdx.x / tx) * LB_H + ly;
  if (x >= W || y >= H) return;
  volatile int* V = P;
  const int p = y * W + x;
  if (V[p] < 0) return;
  if (x > 0 && V[p - 1] >= 0) uf_unite(P, p, p - 1);
  if (y > 0 && V[p - W] >= 0) uf_unite(P, p, p - W);
  if (x > 0 && y > 0 && V[p - W - 1] >= 0) uf_unite(P, p, p - W - 1);
}

__global__ void __launch_bounds__(SM_T) k_lab_flatten(int n, int* __restrict__ P) {
  const int p = blockIdx.x * SM_T + threadIdx.x;
  if (p >= n) return;
  volatile int* V = P;
  if (V[p] >= 0) V[p] = uf_find(V, p);          // concurrent readers see a parent or the root: both are ancestors
}

__global__ void __launch_bounds__(SM_T) k_lab_final(int n, int S, const int* __restrict__ seg, int* __restrict__ P) {
  const int p = blockIdx.x * SM_T + threadIdx.x;
  if (p >= n) return;
  const int s = seg[p];
  P[p] = s >= 0 ? s : S + P[p];
}

// ---------------------------------------------------------------- 5. per-label histograms
constexpr int LH_CAP = 2048;           // labels below this count in LDS
constexpr int LH_CPB = 16;             // 64-pixel chunks per workgroup

__global__ void __launch_bounds__(SM_T) k_lab_hist(int npix, int S, int ntab, const int* __restrict__ labels,
                                                   const float* __restrict__ coarse, int* __restrict__ tab) {
  __shared__ int sa[LH_CAP], si[LH_CAP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = S < LH_CAP ? S : LH_CAP;
  for (int l = tid; l < nl; l += SM_T) sa[l] = si[l] = 0;
  __syncthreads();
  const int nchunk = (npix + 63) / 64, c1 = min((blockIdx.x + 1) * LH_CPB, nchunk);
  for (int c = blockIdx.x * LH_CPB + wave; c < c1; c += SM_T / HUGS_WAVE) {
    const int p = c * 64 + lane;
    const bool in = p < npix;
    const int l = in ? labels[p] : -1;
    const bool valid = in && (unsigned)l < (unsigned)ntab;
    const unsigned long long cm = __ballot(valid && coarse[in ? p : 0] >= 0.5f);
    const int prev = __shfl_up(l, 1);
    const unsigned long long bm = __ballot(lane == 0 || prev != l);        // run boundaries, the invalid lanes' included
    if (valid && ((bm >> lane) & 1ull)) {
      const unsigned long long rest = lane < 63 ? bm >> (lane + 1) : 0ull;
      const int end = rest ? lane + 1 + __builtin_ctzll(rest) : 64;
      const unsigned long long upto = end == 64 ? ~0ull : (1ull << end) - 1ull;
      const int len = end - lane, ic = __popcll(cm & upto & ~((1ull << lane) - 1ull));
      if (l < nl) {
        atomicAdd(&sa[l], len);
        if (ic) atomicAdd(&si[l], ic);
      } else {
        atomicAdd(&tab[l], len);
        if (ic) atomicAdd(&tab[ntab + l], ic);
      }
    }
  }
  __syncthreads();
  for (int l = tid; l < nl; l += SM_T) {
    if (sa[l]) atomicAdd(&tab[l], sa[l]);
    if (si[l]) atomicAdd(&tab[ntab + l], si[l]);
  }
}

// ---------------------------------------------------------------- 4 + 6. box counts on bit-packed tiles
constexpr int BX_W = 64, BX_H = 32, BX_HALO = SM_MAXK / 2;

struct BoxSrc {
  const void* a;
  const float *b, *c;
  const int* tab;
  int ntab, num, den;
};

template <int SRC>
__device__ __forceinline__ bool box_pred(const BoxSrc& s, size_t i) {
  if (SRC == 0) return ((const float*)s.a)[i] >= 0.5f;
  if (SRC == 1) return ((const int*)s.a)[i] >= 1;
  if (SRC == 2) return (((const float*)s.a)[i] >= 0.5f || s.b[i] >= 0.5f) && s.c[i] >= 0.5f;
  const int l = ((const int*)s.a)[i];
  if ((unsigned)l >= (unsigned)s.ntab) return false;
  return (long long)s.tab[s.ntab + l] * s.den >= (long long)s.tab[l] * s.num;
}

template <int SRC>
__global__ void __launch_bounds__(SM_T) k_sm_box(int H, int W, int tx, BoxSrc src, int k, int pad, int rule, float* __restrict__ combined,
                                                 float* __restrict__ out) {
  __shared__ unsigned long long rows[BX_H + 2 * BX_HALO][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = k >> 1;
  const int x0 = (blockIdx.x % tx) * BX_W, y0 = (blockIdx.x / tx) * BX_H, nrows = BX_H + 2 * h;
  for (int r = wave; r < nrows; r += SM_T / HUGS_WAVE) {
    int gy = y0 - h + r;
    bool yin = gy >= 0 && gy < H;
    if (!yin && pad == 1) {
      gy = gy < 0 ? -gy : 2 * (H - 1) - gy;
      yin = gy >= 0 && gy < H;                  // (rows of a ragged tile further out than the halo feed no stored pixel)
    }
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      int gx = x0 - 64 + 64 * w + lane;
      const bool need = gx >= x0 - h && gx < x0 + BX_W + h;
      bool xin = gx >= 0 && gx < W;
      if (!xin && pad == 1) {
        gx = gx < 0 ? -gx : 2 * (W - 1) - gx;
        xin = gx >= 0 && gx < W;
      }
      bool v = false;
      if (need) {
        if (xin && yin) v = box_pred<SRC>(src, (size_t)gy * W + gx);
        else v = pad == 2;                      // (pad 2 reflects nothing: xin && yin is "inside the image")
      }
      const unsigned long long bal = __ballot(v);
      if (lane == 0) rows[r][w] = bal;
    }
  }
  __syncthreads();
  const int pos = 64 + lane - h, wi = pos >> 6, sh = pos & 63, gx = x0 + lane;
  const unsigned long long kmask = (1ull << k) - 1ull;
  for (int ly = wave * (BX_H / 4); ly < (wave + 1) * (BX_H / 4); ++ly) {
    const int gy = y0 + ly;
    if (gy >= H) break;
    int cnt = 0;
    for (int dy = 0; dy < k; ++dy) {
      const unsigned long long w0 = rows[ly + dy][0], w1 = rows[ly + dy][1], w2 = rows[ly + dy][2];
      const unsigned long long lo = wi ? w1 : w0, hi = wi ? w2 : w1;
      const unsigned long long v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
      cnt += __popcll(v & kmask);
    }
    const bool m = (rows[ly + h][1] >> lane) & 1ull;
    const bool res = rule == 0 ? (m || 2 * cnt >= k * k) : cnt == k * k;
    if (gx < W) {
      out[(size_t)gy * W + gx] = res ? 1.f : 0.f;
      if (SRC == 2 && combined) combined[(size_t)gy * W + gx] = m ? 1.f : 0.f;
    }
  }
}

template <int SRC>
int box_launch(int H, int W, const BoxSrc& src, int k, int pad, int rule, float* combined, float* out, hipStream_t s) {
  const int tx = (W + BX_W - 1) / BX_W, ty = (H + BX_H - 1) / BX_H;
  k_sm_box<SRC><<<tx * ty, SM_T, 0, s>>>(H, W, tx, src, k, pad, rule, combined, out);
  HUGS_CHECK_LAUNCH("k_sm_box");
  return 0;
}

}  // namespace

#define SM_REQUIRE_HW(name)                                                                                                      \
  HUGS_REQUIRE(H >= 3 && W >= 3 && (long long)H * W <= SM_MAXPIX, -2, name ": image %d x %d outside 3 <= H, W and H * W <= 2^24", \
               H, W)

static int sm_grid(long long n) {
  const long long b = (n + SM_T - 1) / SM_T;
  return (int)(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

extern "C" long long hugs_sm_ws_bytes(int what, int H, int W, int n) {
  SM_REQUIRE_HW("hugs_sm_ws_bytes");
  HUGS_REQUIRE(what >= 0 && what <= 2 && n >= 0 && n <= (1 << 30), -2, "hugs_sm_ws_bytes: bad arguments (what=%d, n=%d)", what, n);
  const long long npix = (long long)H * W;
  if (what == 0) return (long long)sizeof(RsWs);
  if (what == 1) return (long long)n * sfm_chunks((int)npix) * 4 * 8 + (long long)n * 2 * 4;
  return 2 * (npix + n) * 4;
}

extern "C" int hugs_sm_residual(int H, int W, const float* pred, const float* gt, float q, float* residual, float* mask_base,
                                float* mask_upper, float* thr, void* ws, void* stream) {
  SM_REQUIRE_HW("hugs_sm_residual");
  HUGS_REQUIRE(pred && gt && residual && mask_base && mask_upper && thr && ws, -2, "hugs_sm_residual: null pointer");
  HUGS_REQUIRE(q >= 0.f && q <= 1.f, -2, "hugs_sm_residual: quantile %g outside [0, 1]", (double)q);
  hipStream_t s = (hipStream_t)stream;
  const int n = H * W, nblk = rs_blocks(n);
  // torch.quantile: rank = q * (n - 1) in the input's precision, below = floor, weight = rank - below
  volatile float posv = q * (float)(n - 1);
  const float pos = posv;
  int k0 = (int)floorf(pos);
  k0 = k0 < 0 ? 0 : (k0 > n - 1 ? n - 1 : k0);
  const int k1 = k0 + 1 < n ? k0 + 1 : n - 1;
  const float w = pos - (float)k0;
  RsWs* W_ = (RsWs*)ws;
  k_rs_residual<<<nblk, SM_T, 0, s>>>(n, pred, gt, residual, W_, (uint32_t)k0, (uint32_t)k1);
  HUGS_CHECK_LAUNCH("k_rs_residual");
  const int shift[3] = {21, 10, 0}, bins[3] = {2048, 2048, 1024};
  for (int p = 0; p < 3; ++p) {
    k_rs_hist<<<nblk, SM_T, 0, s>>>(n, residual, W_, p, shift[p], bins[p]);
    HUGS_CHECK_LAUNCH("k_rs_hist");
    k_rs_scan<<<1, 128, 0, s>>>(n, nblk, W_, shift[p], p == 2, w, thr);
    HUGS_CHECK_LAUNCH("k_rs_scan");
  }
  k_rs_masks<<<sm_grid(n), SM_T, 0, s>>>(n, residual, thr, mask_base, mask_upper);
  HUGS_CHECK_LAUNCH("k_rs_masks");
  return 0;
}

extern "C" int hugs_sm_sfm_add(int N, int H, int W, const float* logits, const float* iou, float iou_thresh, float mask_thr,
                               float stab_off, float stab_thresh, int* count, int* keep, void* ws, void* stream) {
  SM_REQUIRE_HW("hugs_sm_sfm_add");
  HUGS_REQUIRE(N >= 1 && N <= 65535, -2, "hugs_sm_sfm_add: %d masks in one batch (1..65535)", N);
  HUGS_REQUIRE(logits && iou && count && keep && ws, -2, "hugs_sm_sfm_add: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int npix = H * W, nchunk = sfm_chunks(npix);
  unsigned long long* bits = (unsigned long long*)ws;
  int* cnt = (int*)(bits + (size_t)N * nchunk * 4);
  // torch compares the fp32 logits with the Python sum rounded to fp32
  const float thi = (float)((double)mask_thr + (double)stab_off), tlo = (float)((double)mask_thr - (double)stab_off);
  k_sm_zero_i32<<<sm_grid(2 * N), SM_T, 0, s>>>(2 * N, cnt);
  HUGS_CHECK_LAUNCH("k_sm_zero_i32");
  const dim3 grid((nchunk + SFM_CPB - 1) / SFM_CPB, N);
  if (npix % 4 == 0 && ((uintptr_t)logits & 15) == 0)
    k_sfm_bits<true><<<grid, SM_T, 0, s>>>(npix, nchunk, logits, mask_thr, thi, tlo, bits, cnt);
  else
    k_sfm_bits<false><<<grid, SM_T, 0, s>>>(npix, nchunk, logits, mask_thr, thi, tlo, bits, cnt);
  HUGS_CHECK_LAUNCH("k_sfm_bits");
  k_sfm_keep<<<(N + SM_T - 1) / SM_T, SM_T, 0, s>>>(N, iou, iou_thresh, stab_thresh, cnt, keep);
  HUGS_CHECK_LAUNCH("k_sfm_keep");
  k_sfm_accum<<<(nchunk + 3) / 4, SM_T, 0, s>>>(npix, nchunk, N, bits, keep, count);
  HUGS_CHECK_LAUNCH("k_sfm_accum");
  return 0;
}

extern "C" int hugs_sm_sfm_add_lowres(int N, int H, int W, int h_in, int w_in, const float* lowres, const float* iou, float iou_thresh,
                                      float mask_thr, float stab_off, float stab_thresh, int use_highest, int* count, int* keep, void* ws,
                                      void* stream) {
  SM_REQUIRE_HW("hugs_sm_sfm_add_lowres");
  HUGS_REQUIRE(N >= 1 && N <= 16384, -2, "hugs_sm_sfm_add_lowres: %d prompts in one batch (1..16384)", N);
  HUGS_REQUIRE(h_in >= 1 && h_in <= LR_UP && w_in >= 1 && w_in <= LR_UP, -2, "hugs_sm_sfm_add_lowres: input size %d x %d outside 1..%d",
               h_in, w_in, LR_UP);
  HUGS_REQUIRE(lowres && iou && count && keep && ws, -2, "hugs_sm_sfm_add_lowres: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int M = use_highest ? N : 3 * N, npix = H * W;
  int* cnt = (int*)ws;
  int* sel = cnt + 2 * M;
  float* iou_sel = (float*)(sel + M);
  const float thi = (float)((double)mask_thr + (double)stab_off), tlo = (float)((double)mask_thr - (double)stab_off);
  const float sy = (float)h_in / (float)H, sx = (float)w_in / (float)W;
  k_lr_select<<<(M + SM_T - 1) / SM_T, SM_T, 0, s>>>(M, use_highest, iou, sel, iou_sel, cnt);
  HUGS_CHECK_LAUNCH("k_lr_select");
  const int gx = (npix + SM_T * 8 - 1) / (SM_T * 8);
  k_lr_count<<<dim3(gx, M), SM_T, 0, s>>>(H, W, sy, sx, h_in, w_in, lowres, sel, thi, tlo, cnt);
  HUGS_CHECK_LAUNCH("k_lr_count");
  k_sfm_keep<<<(M + SM_T - 1) / SM_T, SM_T, 0, s>>>(M, iou_sel, iou_thresh, stab_thresh, cnt, keep);
  HUGS_CHECK_LAUNCH("k_sfm_keep");
  k_lr_accum<<<(npix + SM_T - 1) / SM_T, SM_T, 0, s>>>(H, W, sy, sx, h_in, w_in, M, lowres, sel, keep, mask_thr, count);
  HUGS_CHECK_LAUNCH("k_lr_accum");
  return 0;
}

extern "C" int hugs_sm_label(int H, int W, int S, const int* seg, int* labels, void* stream) {
  SM_REQUIRE_HW("hugs_sm_label");
  HUGS_REQUIRE(S >= 0 && S <= (1 << 30), -2, "hugs_sm_label: %d segments (0..2^30)", S);
  HUGS_REQUIRE(seg && labels && seg != labels, -2, "hugs_sm_label: null or aliased pointer");
  hipStream_t s = (hipStream_t)stream;
  const int n = H * W, tx = (W + LB_W - 1) / LB_W, ty = (H + LB_H - 1) / LB_H;
  k_lab_local<<<tx * ty, SM_T, 0, s>>>(H, W, tx, seg, labels);
  HUGS_CHECK_LAUNCH("k_lab_local");
  k_lab_border<<<tx * ty, 128, 0, s>>>(H, W, tx, labels);
  HUGS_CHECK_LAUNCH("k_lab_border");
  k_lab_flatten<<<(n + SM_T - 1) / SM_T, SM_T, 0, s>>>(n, labels);
  HUGS_CHECK_LAUNCH("k_lab_flatten");
  k_lab_final<<<(n + SM_T - 1) / SM_T, SM_T, 0, s>>>(n, S, seg, labels);
  HUGS_CHECK_LAUNCH("k_lab_final");
  return 0;
}

extern "C" int hugs_sm_label_hist(int H, int W, int S, const int* labels, const float* coarse, int* tab, void* stream) {
  SM_REQUIRE_HW("hugs_sm_label_hist");
  HUGS_REQUIRE(S >= 0 && S <= (1 << 30), -2, "hugs_sm_label_hist: %d segments (0..2^30)", S);
  HUGS_REQUIRE(labels && coarse && tab, -2, "hugs_sm_label_hist: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int n = H * W, ntab = S + n, nchunk = (n + 63) / 64;
  k_sm_zero_i32<<<sm_grid(2ll * ntab), SM_T, 0, s>>>(2ll * ntab, tab);
  HUGS_CHECK_LAUNCH("k_sm_zero_i32");
  k_lab_hist<<<(nchunk + LH_CPB - 1) / LH_CPB, SM_T, 0, s>>>(n, S, ntab, labels, coarse, tab);
  HUGS_CHECK_LAUNCH("k_lab_hist");
  return 0;
}

static int sm_box_args(const char* name, int H, int W, int k, int pad, int rule) {
  HUGS_REQUIRE(k >= 1 && k <= SM_MAXK && (k & 1), -2, "%s: kernel size %d (odd, 1..%d)", name, k, SM_MAXK);
  HUGS_REQUIRE(pad >= 0 && pad <= 2 && (rule == 0 || rule == 1), -2, "%s: bad pad / rule (%d, %d)", name, pad, rule);
  HUGS_REQUIRE(pad != 1 || (k / 2 < H && k / 2 < W), -2, "%s: reflect padding %d needs a larger image than %d x %d", name, k / 2, H, W);
  return 0;
}

extern "C" int hugs_sm_box(int H, int W, int src, const void* a, const float* b, const float* c, int k, int pad, int rule,
                           float* combined, float* out, void* stream) {
  SM_REQUIRE_HW("hugs_sm_box");
  if (int rc = sm_box_args("hugs_sm_box", H, W, k, pad, rule)) return rc;
  HUGS_REQUIRE(src >= 0 && src <= 2 && a && out && (src != 2 || (b && c)), -2, "hugs_sm_box: bad source %d or null pointer", src);
  const BoxSrc bs{a, b, c, nullptr, 0, 0, 1};
  hipStream_t s = (hipStream_t)stream;
  if (src == 0) return box_launch<0>(H, W, bs, k, pad, rule, nullptr, out, s);
  if (src == 1) return box_launch<1>(H, W, bs, k, pad, rule, nullptr, out, s);
  return box_launch<2>(H, W, bs, k, pad, rule, combined, out, s);
}

extern "C" int hugs_sm_select_erode(int H, int W, const int* labels, const int* tab, int ntab, int num, int den, int k, float* out,
                                    void* stream) {
  SM_REQUIRE_HW("hugs_sm_select_erode");
  if (int rc = sm_box_args("hugs_sm_select_erode", H, W, k, 2, 1)) return rc;
  HUGS_REQUIRE(labels && tab && out && ntab >= 1, -2, "hugs_sm_select_erode: null pointer or empty table");
  HUGS_REQUIRE(num >= 0 && den >= 1 && num <= den && den <= (1 << 20), -2, "hugs_sm_select_erode: threshold %d/%d (0 <= num <= den <= 2^20)",
               num, den);
  const BoxSrc bs{labels, nullptr, nullptr, tab, ntab, num, den};
  return box_launch<3>(H, W, bs, k, 2, 1, nullptr, out, (hipStream_t)stream);
}
