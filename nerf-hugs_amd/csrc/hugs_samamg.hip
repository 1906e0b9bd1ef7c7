// SAM's automatic mask generator around the encoder and the decoder: what segment_anything's SamAutomaticMaskGenerator.generate does
// with the decoder's outputs, and the painting of HuGS/generate_static_mask.py:237-242.  Masks live bit-packed, [K, H, WC] 64-bit
// words with WC = ceil(W / 64); bit l of word c of a row is pixel 64 c + l (the ballot layout of k_sfm_bits).  Every decision is
// integer arithmetic or one correctly rounded fp32 quotient; atomics are integer add / min / max / or, so no result depends on the
// launch geometry or on the order they land in, and every order that matters (slots, ranks, keep lists) is defined by index.
//
//   1. candidates (_process_batch).  k_cd_scan: a workgroup takes CD_ROWS output rows of one candidate.  It stages, for each of its
//      rows, the four low-res rows that row's two crop taps read (lr_axis) in LDS -- [CD_ROWS][4][256] floats, one column per
//      thread -- and a wave then owns 64 consecutive pixels of a row: lr_logit on the staged rows, three ballots (> thr + off,
//      > thr - off, > thr).  The popcounts and the box of the > thr word (ctz / clz of the ballot) are wave-uniform integers,
//      reduced in LDS and added to the candidate's record; the > thr ballot is the candidate's plane word in crop coordinates.
//      Candidates under the IoU threshold return before the staging.  k_cd_keep (one workgroup) takes the three decisions and
//      gives the kept ones consecutive slots by a ballot prefix scan in candidate order; k_cd_place funnel-shifts the crop words
//      to the crop's offset in the image plane and writes zero words elsewhere (uncrop_masks).
//   2. stable rank.  k_rank: thread i counts the keys that precede key i in the stable descending order, against tiles of 256 keys
//      in LDS.
//   3. box NMS.  k_nms_matrix: workgroup (tr, tc), tc >= tr, compares the 64 boxes of rank tile tr with the 64 of tile tc: lane l
//      holds box 64 tc + l, a wave walks 16 rows, one ballot per row is word tc of that row of the suppression matrix.
//      k_nms_reduce: one wave walks the rows in rank order with the removed set in LDS and ORs the rows of the survivors into it.
//      k_gather_rows compacts any per-mask array by the keep list.
//   4. small regions (remove_small_regions, holes then islands).  Union-find per mask on 64 x 16 tiles (one plane word per row)
//      of the mask's box grown by one pixel: k_sr_label unites inside a tile in LDS (left, up, up-left, up-right), k_sr_merge
//      across tile edges in the global parent array, k_sr_count flattens and counts the area at the root.  For the holes the
//      background outside the window is four virtual nodes (the strips above, below, left and right of the window, with their
//      pixel counts) united with the window's edge pixels and with each other where they touch: the outside is labelled without
//      touching a pixel of it, and its area is exact.  k_sr_best finds, for the islands, whether a component reaches min_area and
//      the largest small one (ties: the smallest root, i.e. the first pixel in raster order) with a 64-bit atomicMax.
//      k_sr_apply writes the cleaned words.
//   5. paint.  k_paint: one wave per plane word, one lane per pixel; the masks are walked from the last rank down with
//      wave-uniform 8-byte loads until every lane has its label; masks whose box misses the word are skipped.
#include "hugs_common.h"
#include "hugs_maskops.h"
#include <limits.h>

namespace {

typedef unsigned long long u64;
constexpr int AG_T = 256;
constexpr int AG_MAXSIDE = 4096;       // box areas and intersections stay exact in fp32
constexpr int AG_MAXK = 65535;         // masks in one set: a grid's y extent; the removed set of k_nms_reduce is 1024 words of LDS

// ---------------------------------------------------------------- 1. candidates
constexpr int CD_ROWS = 8;
struct CdStat { int hi, lo, area, x0, y0, x1, y1, slot; };

__global__ void __launch_bounds__(AG_T) k_cd_init(int M, CdStat* __restrict__ st) {
  const int m = blockIdx.x * AG_T + threadIdx.x;
  if (m < M) st[m] = CdStat{0, 0, 0, INT_MAX, INT_MAX, -1, -1, -1};
}

__global__ void __launch_bounds__(AG_T) k_cd_scan(int ch, int cw, int wcc, float sy, float sx, int h_in, int w_in,
                                                  const float* __restrict__ lowres, const float* __restrict__ iou, float iou_thresh,
                                                  float thr, float thi, float tlo, u64* __restrict__ tmp, CdStat* __restrict__ st) {
  __shared__ float rows[CD_ROWS][4][LR];
  __shared__ int red[7];
  const int m = blockIdx.y;
  if (iou_thresh > 0.f && !(iou[m] > iou_thresh)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, y0 = blockIdx.x * CD_ROWS, nr = min(CD_ROWS, ch - y0);
  if (tid < 7) red[tid] = tid < 3 ? 0 : (tid < 5 ? INT_MAX : -1);
  const float* L = lowres + (size_t)m * LR * LR;
  for (int b = 0; b < nr; ++b) {
    const LrAxis ay = lr_axis(y0 + b, sy, h_in);
#pragma unroll
    for (int t = 0; t < 4; ++t) rows[b][t][tid] = L[ay.i[t] * LR + tid];
  }
  __syncthreads();
  int chi = 0, clo = 0, car = 0, mnx = INT_MAX, mny = INT_MAX, mxx = -1, mxy = -1;
  for (int u = wave; u < nr * wcc; u += AG_T / HUGS_WAVE) {
    const int b = u / wcc, c = u - b * wcc, py = y0 + b, px = 64 * c + lane;
    const bool valid = px < cw;
    LrAxis ay = lr_axis(py, sy, h_in);
#pragma unroll
    for (int t = 0; t < 4; ++t) ay.i[t] = t;                      // the staged copies of this row's four low-res rows
    const float v = lr_logit(&rows[b][0][0], ay, lr_axis(valid ? px : 0, sx, w_in));
    const u64 bal = __ballot(valid && v > thr);
    chi += __popcll(__ballot(valid && v > thi));
    clo += __popcll(__ballot(valid && v > tlo));
    if (bal) {
      car += __popcll(bal);
      mnx = min(mnx, 64 * c + __builtin_ctzll(bal));
      mxx = max(mxx, 64 * c + 63 - __builtin_clzll(bal));
      mny = min(mny, py);
      mxy = max(mxy, py);
    }
    if (lane == 0) tmp[((size_t)m * ch + py) * wcc + c] = bal;
  }
  if (lane == 0) {
    atomicAdd(&red[0], chi);
    atomicAdd(&red[1], clo);
    atomicAdd(&red[2], car);
    atomicMin(&red[3], mnx);
    atomicMin(&red[4], mny);
    atomicMax(&red[5], mxx);
    atomicMax(&red[6], mxy);
  }
  __syncthreads();
  int* g = &st[m].hi;
  if (tid < 3) { if (red[tid]) atomicAdd(&g[tid], red[tid]); }
  else if (tid < 5) atomicMin(&g[tid], red[tid]);
  else if (tid < 7) atomicMax(&g[tid], red[tid]);
}

struct CdOut {
  int* boxes;
  float *iou, *stab;
  int* area;
  float* points;
  int *crop, *nkept;
};

// is_box_near_crop_edge's isclose(a, b, atol = 20, rtol = 0) on integers
__device__ __forceinline__ bool cd_near(int a, int b) { return abs(a - b) <= 20; }

__global__ void __launch_bounds__(AG_T) k_cd_keep(int M, const float* __restrict__ iou, const float* __restrict__ points, float iou_thresh,
                                                  float stab_thresh, int cx0, int cy0, int cx1, int cy1, int H, int W, int base, int cap,
                                                  CdStat* __restrict__ st, CdOut o) {
  __shared__ int wsum[AG_T / HUGS_WAVE], carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int m0 = 0; m0 < M; m0 += AG_T) {
    const int m = m0 + tid;
    bool keep = false;
    int bx[4] = {0, 0, 0, 0};
    float stab = 0.f;
    CdStat s{};
    if (m < M) {
      s = st[m];
      keep = !(iou_thresh > 0.f) || iou[m] > iou_thresh;
      stab = (float)((double)s.hi / (double)s.lo);                // 0/0 = NaN: dropped by the comparison below
      if (stab_thresh > 0.f) keep = keep && stab >= stab_thresh;
      if (s.area > 0) { bx[0] = s.x0; bx[1] = s.y0; bx[2] = s.x1; bx[3] = s.y1; }      // batched_mask_to_box: zeros when empty
      bx[0] += cx0; bx[1] += cy0; bx[2] += cx0; bx[3] += cy0;     // uncrop_boxes_xyxy
      const int cb[4] = {cx0, cy0, cx1, cy1}, ib[4] = {0, 0, W, H};
      bool near = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) near = near || (cd_near(bx[e], cb[e]) && !cd_near(bx[e], ib[e]));
      keep = keep && !near;
    }
    const u64 bal = __ballot(keep);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int off = carry + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) off += wsum[w];
    const int slot = base + off;
    if (keep && slot < cap) {
      st[m].slot = slot;
#pragma unroll
      for (int e = 0; e < 4; ++e) o.boxes[4 * slot + e] = bx[e];
      o.crop[4 * slot] = cx0; o.crop[4 * slot + 1] = cy0; o.crop[4 * slot + 2] = cx1; o.crop[4 * slot + 3] = cy1;
      o.iou[slot] = iou[m];
      o.stab[slot] = stab;
      o.area[slot] = s.area;
      o.points[2 * slot] = __fadd_rn(points[2 * (m / 3)], (float)cx0);              // uncrop_points
      o.points[2 * slot + 1] = __fadd_rn(points[2 * (m / 3) + 1], (float)cy0);
    }
    __syncthreads();
    if (tid == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (tid == 0) *o.nkept = min(carry, cap - base);
}

__global__ void __launch_bounds__(AG_T) k_cd_place(int H, int WC, int ch, int wcc, int cx0, int cy0, const u64* __restrict__ tmp,
                                                   const CdStat* __restrict__ st, u64* __restrict__ masks) {
  const int m = blockIdx.y, slot = st[m].slot, idx = blockIdx.x * AG_T + threadIdx.x;
  if (slot < 0 || idx >= H * WC) return;
  const int y = idx / WC, c = idx - y * WC, r = y - cy0;
  u64 out = 0;
  if (r >= 0 && r < ch) {
    const u64* T = tmp + ((size_t)m * ch + r) * wcc;
    const int s = cx0 & 63, a = c - (cx0 >> 6);
    const u64 lo = (a >= 0 && a < wcc) ? T[a] : 0ull, hi = (a >= 1 && a - 1 < wcc) ? T[a - 1] : 0ull;
    out = s ? (lo << s) | (hi >> (64 - s)) : lo;
  }
  masks[((size_t)slot * H + y) * WC + c] = out;
}

// ---------------------------------------------------------------- bool planes <-> bit planes, box and area of a bit plane
__global__ void __launch_bounds__(AG_T) k_pack(long long nwords, int W, int WC, const uint8_t* __restrict__ in, u64* __restrict__ bits) {
  const long long w = (long long)blockIdx.x * (AG_T / HUGS_WAVE) + (threadIdx.x >> 6);
  if (w >= nwords) return;
  const int lane = threadIdx.x & 63, c = (int)(w % WC), x = 64 * c + lane;
  const u64 bal = __ballot(x < W && in[(w / WC) * W + x] != 0);
  if (lane == 0) bits[w] = bal;
}

__global__ void __launch_bounds__(AG_T) k_unpack(long long nwords, int W, int WC, const u64* __restrict__ bits, uint8_t* __restrict__ out) {
  const long long w = (long long)blockIdx.x * (AG_T / HUGS_WAVE) + (threadIdx.x >> 6);
  if (w >= nwords) return;
  const int lane = threadIdx.x & 63, c = (int)(w % WC), x = 64 * c + lane;
  if (x < W) out[(w / WC) * W + x] = (uint8_t)((bits[w] >> lane) & 1ull);
}

// one workgroup per mask: batched_mask_to_box (zeros for an empty mask) and the popcount
__global__ void __launch_bounds__(AG_T) k_bits_stats(int H, int WC, const u64* __restrict__ masks, int* __restrict__ boxes,
                                                     int* __restrict__ area) {
  __shared__ int red[5];
  const int tid = threadIdx.x, k = blockIdx.x;
  if (tid < 5) red[tid] = tid == 0 ? 0 : (tid < 3 ? INT_MAX : -1);
  __syncthreads();
  const u64* B = masks + (size_t)k * H * WC;
  int ar = 0, mnx = INT_MAX, mny = INT_MAX, mxx = -1, mxy = -1;
  for (int i = tid; i < H * WC; i += AG_T) {
    const u64 w = B[i];
    if (!w) continue;
    const int y = i / WC, c = i - y * WC;
    ar += __popcll(w);
    mnx = min(mnx, 64 * c + __builtin_ctzll(w));
    mxx = max(mxx, 64 * c + 63 - __builtin_clzll(w));
    mny = min(mny, y);
    mxy = max(mxy, y);
  }
  if (ar) {
    atomicAdd(&red[0], ar);
    atomicMin(&red[1], mnx);
    atomicMin(&red[2], mny);
    atomicMax(&red[3], mxx);
    atomicMax(&red[4], mxy);
  }
  __syncthreads();
  if (tid == 0) area[k] = red[0];
  if (tid >= 1 && tid < 5) boxes[4 * k + tid - 1] = red[0] ? red[tid] : 0;
}

// ---------------------------------------------------------------- 2. stable descending rank
template <typename T> __device__ __forceinline__ T rank_low() { return T(INT_MIN); }
template <> __device__ __forceinline__ float rank_low<float>() { return -INFINITY; }

template <typename T>
__global__ void __launch_bounds__(AG_T) k_rank(int K, const T* __restrict__ keys, int* __restrict__ rank, int* __restrict__ order) {
  __shared__ T tile[AG_T];
  const int tid = threadIdx.x, i = blockIdx.x * AG_T + tid;
  T si = i < K ? keys[i] : T(0);
  if (!(si == si)) si = rank_low<T>();                              // a NaN key ranks with -inf: the order stays total
  int r = 0;
  for (int j0 = 0; j0 < K; j0 += AG_T) {
    __syncthreads();
    if (j0 + tid < K) {
      const T kj = keys[j0 + tid];
      tile[tid] = kj == kj ? kj : rank_low<T>();
    }
    __syncthreads();
    const int n = min(AG_T, K - j0);
    for (int j = 0; j < n; ++j) {
      const T sj = tile[j];
      r += (sj > si || (sj == si && j0 + j < i)) ? 1 : 0;
    }
  }
  if (i < K) {
    rank[i] = r;
    order[r] = i;
  }
}

// ---------------------------------------------------------------- 3. box NMS
// torchvision's nms on integer boxes: areas and the intersection are exact, the union and the quotient are rounded as fp32 does
__device__ __forceinline__ bool nms_over(const int* a, const int* b, float thr) {
  const float aa = (float)((a[2] - a[0]) * (a[3] - a[1])), ab = (float)((b[2] - b[0]) * (b[3] - b[1]));
  const int iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0), ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0);
  const float inter = (float)(iw * ih);
  return __fdiv_rn(inter, __fsub_rn(__fadd_rn(aa, ab), inter)) > thr;      // 0 / 0 = NaN: not suppressed
}

__global__ void __launch_bounds__(AG_T) k_nms_matrix(int K, int T, const int* __restrict__ boxes, const int* __restrict__ order, float thr,
                                                     u64* __restrict__ S) {
  const int tr = blockIdx.y, tc = blockIdx.x;
  if (tc < tr) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = 64 * tc + lane;
  int bj[4] = {0, 0, 0, 0};
  if (j < K) {
    const int* p = boxes + 4 * order[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) bj[e] = p[e];
  }
  for (int rr = 0; rr < 16; ++rr) {
    const int i = 64 * tr + 16 * wave + rr;
    if (i >= K) break;
    const int* p = boxes + 4 * order[i];
    const int bi[4] = {p[0], p[1], p[2], p[3]};
    const u64 bal = __ballot(j < K && j > i && nms_over(bi, bj, thr));
    if (lane == 0) S[(size_t)i * T + tc] = bal;
  }
}

__global__ void __launch_bounds__(HUGS_WAVE) k_nms_reduce(int K, int T, const u64* __restrict__ S, const int* __restrict__ order,
                                                          int* __restrict__ keep, int* __restrict__ nkeep) {
  __shared__ u64 rem[(AG_MAXK + 63) / 64];
  const int lane = threadIdx.x;
  for (int w = lane; w < T; w += 64) rem[w] = 0;
  __syncthreads();
  int n = 0;
  for (int i = 0; i < K; ++i) {
    if ((rem[i >> 6] >> (i & 63)) & 1ull) continue;       // (wave-uniform)
    if (lane == 0) keep[n] = order[i];
    ++n;
    for (int w = (i >> 6) + lane; w < T; w += 64) rem[w] |= S[(size_t)i * T + w];
    __syncthreads();
  }
  if (lane == 0) *nkeep = n;
}

// dst row j = row keep[j] of src, or of alt where sel[keep[j]] is set; rows are `row` 4-byte words
__global__ void __launch_bounds__(AG_T) k_gather_rows(long long row, const int* __restrict__ keep, const int* __restrict__ nkeep,
                                                      const int* __restrict__ sel, const int* __restrict__ src,
                                                      const int* __restrict__ alt, int* __restrict__ dst) {
  const int j = blockIdx.y;
  if (j >= *nkeep) return;
  const int i = keep[j];
  const int* s = ((alt && sel[i]) ? alt : src) + (size_t)i * row;
  for (long long e = (long long)blockIdx.x * AG_T + threadIdx.x; e < row; e += (long long)gridDim.x * AG_T) dst[(size_t)j * row + e] = s[e];
}

// ---------------------------------------------------------------- 4. small regions
constexpr int SR_H = 16;               // tile: one plane word x 16 rows
struct SrWin { int x0, y0, x1, y1; };
struct SrWs {
  int *P, *A;                          // parents / areas: one slab of H * W + 4 ints per mask of the chunk
  u64* best;
  int* flag;
  long long slab;
};

__device__ __forceinline__ SrWin sr_win(const int* b, int H, int W) {
  return SrWin{max(b[0] - 1, 0), max(b[1] - 1, 0), min(b[2] + 1, W - 1), min(b[3] + 1, H - 1)};
}
__device__ __forceinline__ bool sr_in(const SrWin& w, int x, int y) { return x >= w.x0 && x <= w.x1 && y >= w.y0 && y <= w.y1; }
__device__ __forceinline__ bool sr_tile_out(const SrWin& w, int c, int y0) {
  return 64 * c > w.x1 || 64 * c + 63 < w.x0 || y0 > w.y1 || y0 + SR_H - 1 < w.y0;
}

__global__ void __launch_bounds__(AG_T) k_sr_init(int n, int k0, SrWs ws, int* __restrict__ changed) {
  const int i = blockIdx.x * AG_T + threadIdx.x;
  if (i >= n) return;
  ws.best[i] = 0;
  ws.flag[i] = 0;
  changed[k0 + i] = 0;
}

// mode 0: the background inside the window (holes); 1: the foreground (islands)
__global__ void __launch_bounds__(AG_T) k_sr_label(int mode, int H, int W, int WC, int k0, const u64* __restrict__ bits,
                                                   const int* __restrict__ boxes, SrWs ws) {
  __shared__ int L[64 * SR_H];
  const int tid = threadIdx.x, k = k0 + blockIdx.y, n = H * W, c = blockIdx.x % WC, y0 = (blockIdx.x / WC) * SR_H;
  int* P = ws.P + blockIdx.y * ws.slab;
  int* A = ws.A + blockIdx.y * ws.slab;
  const SrWin win = sr_win(boxes + 4 * k, H, W);
  if (blockIdx.x == 0 && tid < 4) {
    P[n + tid] = n + tid;
    A[n + tid] = 0;
  }
  if (sr_tile_out(win, c, y0)) return;
  for (int e = tid; e < 64 * SR_H; e += AG_T) {
    const int lx = e & 63, gx = 64 * c + lx, gy = y0 + (e >> 6);
    const bool in = sr_in(win, gx, gy);
    bool t = false;
    if (in) {
      t = (int)((bits[((size_t)k * H + gy) * WC + c] >> lx) & 1ull) == mode;
      A[gy * W + gx] = 0;
    }
    L[e] = t ? e : -1;
  }
  __syncthreads();
  volatile int* V = L;
  for (int e = tid; e < 64 * SR_H; e += AG_T) {
    if (V[e] < 0) continue;
    const int lx = e & 63, ly = e >> 6;
    if (lx > 0 && V[e - 1] >= 0) uf_unite(L, e, e - 1);
    if (ly > 0 && V[e - 64] >= 0) uf_unite(L, e, e - 64);
    if (lx > 0 && ly > 0 && V[e - 65] >= 0) uf_unite(L, e, e - 65);
    if (lx < 63 && ly > 0 && V[e - 63] >= 0) uf_unite(L, e, e - 63);
  }
  __syncthreads();
  for (int e = tid; e < 64 * SR_H; e += AG_T) {
    const int gx = 64 * c + (e & 63), gy = y0 + (e >> 6);
    if (!sr_in(win, gx, gy)) continue;
    int out = -1;
    if (V[e] >= 0) {
      const int r = uf_find(V, e);
      out = (y0 + (r >> 6)) * W + 64 * c + (r & 63);
    }
    P[gy * W + gx] = out;
  }
}

__global__ void __launch_bounds__(AG_T) k_sr_merge(int mode, int H, int W, int WC, int k0, const int* __restrict__ boxes, SrWs ws) {
  const int tid = threadIdx.x, k = k0 + blockIdx.y, n = H * W, c = blockIdx.x % WC, y0 = (blockIdx.x / WC) * SR_H;
  int* P = ws.P + blockIdx.y * ws.slab;
  volatile int* V = P;
  const SrWin win = sr_win(boxes + 4 * k, H, W);
  const bool vt = win.y0 > 0, vb = win.y1 < H - 1, vl = win.x0 > 0, vr = win.x1 < W - 1;      // the outside strips that exist
  if (mode == 0 && blockIdx.x == 0 && tid == 0) {
    if (vt && vl) uf_unite(P, n, n + 2);
    if (vt && vr) uf_unite(P, n, n + 3);
    if (vb && vl) uf_unite(P, n + 1, n + 2);
    if (vb && vr) uf_unite(P, n + 1, n + 3);
  }
  if (sr_tile_out(win, c, y0)) return;
  for (int e = tid; e < 64 * SR_H; e += AG_T) {
    const int lx = e & 63, ly = e >> 6, gx = 64 * c + lx, gy = y0 + ly, p = gy * W + gx;
    if (!sr_in(win, gx, gy) || V[p] < 0) continue;
    if (lx == 0 || ly == 0) {
      if (lx == 0 && sr_in(win, gx - 1, gy) && V[p - 1] >= 0) uf_unite(P, p, p - 1);
      if (ly == 0 && sr_in(win, gx, gy - 1) && V[p - W] >= 0) uf_unite(P, p, p - W);
      if (sr_in(win, gx - 1, gy - 1) && V[p - W - 1] >= 0) uf_unite(P, p, p - W - 1);
    }
    if ((ly == 0 || lx == 63) && sr_in(win, gx + 1, gy - 1) && V[p - W + 1] >= 0) uf_unite(P, p, p - W + 1);
    if (mode == 0) {
      if (vt && gy == win.y0) uf_unite(P, p, n);
      if (vb && gy == win.y1) uf_unite(P, p, n + 1);
      if (vl && gx == win.x0) uf_unite(P, p, n + 2);
      if (vr && gx == win.x1) uf_unite(P, p, n + 3);
    }
  }
}

__global__ void __launch_bounds__(AG_T) k_sr_count(int mode, int H, int W, int WC, int k0, const int* __restrict__ boxes, SrWs ws) {
  const int tid = threadIdx.x, k = k0 + blockIdx.y, n = H * W, c = blockIdx.x % WC, y0 = (blockIdx.x / WC) * SR_H;
  int* P = ws.P + blockIdx.y * ws.slab;
  int* A = ws.A + blockIdx.y * ws.slab;
  volatile int* V = P;
  const SrWin win = sr_win(boxes + 4 * k, H, W);
  if (mode == 0 && blockIdx.x == 0 && tid < 4) {
    const int wh = win.y1 - win.y0 + 1;
    const int va = tid == 0 ? win.y0 * W : (tid == 1 ? (H - 1 - win.y1) * W : (tid == 2 ? wh * win.x0 : wh * (W - 1 - win.x1)));
    if (va > 0) atomicAdd(&A[uf_find(V, n + tid)], va);
  }
  if (sr_tile_out(win, c, y0)) return;
  for (int e = tid; e < 64 * SR_H; e += AG_T) {
    const int gx = 64 * c + (e & 63), gy = y0 + (e >> 6), p = gy * W + gx;
    if (!sr_in(win, gx, gy) || V[p] < 0) continue;
    const int r = uf_find(V, p);
    V[p] = r;                                       // concurrent readers see a parent or the root: both are ancestors
    atomicAdd(&A[r], 1);
  }
}

__global__ void __launch_bounds__(AG_T) k_sr_best(int H, int W, int WC, int k0, int min_area, const int* __restrict__ boxes, SrWs ws) {
  const int tid = threadIdx.x, k = k0 + blockIdx.y, c = blockIdx.x % WC, y0 = (blockIdx.x / WC) * SR_H;
  const int* P = ws.P + blockIdx.y * ws.slab;
  const int* A = ws.A + blockIdx.y * ws.slab;
  const SrWin win = sr_win(boxes + 4 * k, H, W);
  if (sr_tile_out(win, c, y0)) return;
  for (int e = tid; e < 64 * SR_H; e += AG_T) {
    const int gx = 64 * c + (e & 63), gy = y0 + (e >> 6), p = gy * W + gx;
    if (!sr_in(win, gx, gy) || P[p] != p) continue;
    const int a = A[p];
    atomicOr(&ws.flag[blockIdx.y], a >= min_area ? 1 : 2);
    if (a < min_area) atomicMax(&ws.best[blockIdx.y], ((u64)a << 32) | (u64)(0xffffffffu - (unsigned)p));
  }
}

// mode 0: out = src with the small holes set; 1: out (= src) loses its small islands.  changed[k] = a pass found a small region.
__global__ void __launch_bounds__(AG_T) k_sr_apply(int mode, int H, int W, int WC, int k0, int min_area, const u64* src,
                                                   const int* __restrict__ boxes, SrWs ws, u64* out, int* __restrict__ changed) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = k0 + blockIdx.y, c = blockIdx.x % WC, y0 = (blockIdx.x / WC) * SR_H;
  const int* P = ws.P + blockIdx.y * ws.slab;
  const int* A = ws.A + blockIdx.y * ws.slab;
  const SrWin win = sr_win(boxes + 4 * k, H, W);
  if (sr_tile_out(win, c, y0)) {
    if (mode == 0 && tid < SR_H && y0 + tid < H) out[((size_t)k * H + y0 + tid) * WC + c] = src[((size_t)k * H + y0 + tid) * WC + c];
    return;
  }
  const int fl = mode ? ws.flag[blockIdx.y] : 0;
  const int best = mode ? (int)(0xffffffffu - (unsigned)(ws.best[blockIdx.y] & 0xffffffffull)) : -1;
  if (mode && (fl & 2) && tid == 0) atomicOr(&changed[k], 1);
  for (int ly = wave * (SR_H / 4); ly < (wave + 1) * (SR_H / 4); ++ly) {
    const int gy = y0 + ly, gx = 64 * c + lane;
    if (gy >= H) break;
    const size_t wi = ((size_t)k * H + gy) * WC + c;
    const u64 w = src[wi];
    bool bit = (w >> lane) & 1ull;
    if (sr_in(win, gx, gy) && (int)bit == mode) {
      const int r = P[gy * W + gx], a = A[r];
      if (mode == 0) bit = a < min_area;
      else bit = a >= min_area || (!(fl & 1) && r == best);
    }
    const u64 nw = __ballot(bit);
    if (lane == 0) {
      out[wi] = nw;
      if (mode == 0 && nw != w) atomicOr(&changed[k], 1);
    }
  }
}

// ---------------------------------------------------------------- 5. paint
__global__ void __launch_bounds__(AG_T) k_paint(int S, int H, int W, int WC, const u64* __restrict__ masks, const int* __restrict__ boxes,
                                                const int* __restrict__ order, int* __restrict__ seg) {
  const int lane = threadIdx.x & 63, idx = blockIdx.x * (AG_T / HUGS_WAVE) + (threadIdx.x >> 6);
  if (idx >= H * WC) return;
  const int y = idx / WC, c = idx - y * WC, x = 64 * c + lane;
  u64 need = __ballot(x < W);
  int label = -1;
  for (int r = S - 1; r >= 0 && need; --r) {
    const int i = order[r];
    const int* b = boxes + 4 * i;
    if (y < b[1] || y > b[3] || b[2] < 64 * c || b[0] > 64 * c + 63) continue;
    const u64 w = masks[((size_t)i * H + y) * WC + c];
    if (((w & need) >> lane) & 1ull) label = r;
    need &= ~w;
  }
  if (x < W) seg[(size_t)y * W + x] = label;
}

static SrWs sr_ws(void* ws, int H, int W, int chunk) {
  SrWs s;
  s.slab = (long long)H * W + 4;
  s.best = (u64*)ws;
  s.P = (int*)(s.best + chunk);
  s.A = s.P + s.slab * chunk;
  s.flag = s.A + s.slab * chunk;
  return s;
}

}  // namespace

#define AG_REQUIRE_HW(name)                                                                                                       \
  HUGS_REQUIRE(H >= 3 && W >= 3 && H <= AG_MAXSIDE && W <= AG_MAXSIDE && (long long)H * W <= (1 << 24), -2,                        \
               name ": image %d x %d outside 3 <= H, W <= %d and H * W <= 2^24", H, W, AG_MAXSIDE)
#define AG_REQUIRE_K(name, K) HUGS_REQUIRE((K) >= 1 && (K) <= AG_MAXK, -2, name ": %d masks (1..%d)", (K), AG_MAXK)

extern "C" long long hugs_amg_ws_bytes(int what, int H, int W, int n) {
  AG_REQUIRE_HW("hugs_amg_ws_bytes");
  HUGS_REQUIRE(what >= 0 && what <= 2 && n >= 1 && n <= AG_MAXK, -2, "hugs_amg_ws_bytes: bad arguments (what=%d, n=%d)", what, n);
  if (what == 0) return 3ll * n * ((long long)H * ((W + 63) / 64) * 8 + (long long)sizeof(CdStat));
  if (what == 1) return (long long)n * ((n + 63) / 64) * 8;
  return (long long)n * (8 + 2 * ((long long)H * W + 4) * 4 + 4);
}

extern "C" int hugs_amg_candidates(int N, int H, int W, int cx0, int cy0, int cx1, int cy1, int h_in, int w_in, const float* lowres,
                                   const float* iou, const float* points, float iou_thresh, float stab_thresh, float stab_off,
                                   float mask_thr, int base, int cap, void* masks, int* boxes, float* iou_out, float* stab_out, int* area,
                                   float* points_out, int* crop_out, int* nkept, void* ws, void* stream) {
  AG_REQUIRE_HW("hugs_amg_candidates");
  HUGS_REQUIRE(N >= 1 && N <= 16384, -2, "hugs_amg_candidates: %d prompts in one batch (1..16384)", N);
  HUGS_REQUIRE(cx0 >= 0 && cy0 >= 0 && cx1 <= W && cy1 <= H && cx1 - cx0 >= 3 && cy1 - cy0 >= 3, -2,
               "hugs_amg_candidates: crop box (%d, %d, %d, %d) outside the %d x %d image or under 3 pixels", cx0, cy0, cx1, cy1, H, W);
  HUGS_REQUIRE(h_in >= 1 && h_in <= LR_UP && w_in >= 1 && w_in <= LR_UP, -2, "hugs_amg_candidates: input size %d x %d outside 1..%d", h_in,
               w_in, LR_UP);
  HUGS_REQUIRE(base >= 0 && cap <= AG_MAXK && base + 3 * N <= cap, -2, "hugs_amg_candidates: %d slots from %d do not hold 3 x %d candidates",
               cap, base, N);
  HUGS_REQUIRE(lowres && iou && points && masks && boxes && iou_out && stab_out && area && points_out && crop_out && nkept && ws, -2,
               "hugs_amg_candidates: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int M = 3 * N, ch = cy1 - cy0, cw = cx1 - cx0, wcc = (cw + 63) / 64, WC = (W + 63) / 64;
  u64* tmp = (u64*)ws;
  CdStat* st = (CdStat*)(tmp + (size_t)M * ch * wcc);
  // torch compares the fp32 logits with the Python sum rounded to fp32
  const float thi = (float)((double)mask_thr + (double)stab_off), tlo = (float)((double)mask_thr - (double)stab_off);
  k_cd_init<<<(M + AG_T - 1) / AG_T, AG_T, 0, s>>>(M, st);
  HUGS_CHECK_LAUNCH("k_cd_init");
  k_cd_scan<<<dim3((ch + CD_ROWS - 1) / CD_ROWS, M), AG_T, 0, s>>>(ch, cw, wcc, (float)h_in / (float)ch, (float)w_in / (float)cw, h_in, w_in,
                                                                   lowres, iou, iou_thresh, mask_thr, thi, tlo, tmp, st);
  HUGS_CHECK_LAUNCH("k_cd_scan");
  const CdOut o{boxes, iou_out, stab_out, area, points_out, crop_out, nkept};
  k_cd_keep<<<1, AG_T, 0, s>>>(M, iou, points, iou_thresh, stab_thresh, cx0, cy0, cx1, cy1, H, W, base, cap, st, o);
  HUGS_CHECK_LAUNCH("k_cd_keep");
  k_cd_place<<<dim3((H * WC + AG_T - 1) / AG_T, M), AG_T, 0, s>>>(H, WC, ch, wcc, cx0, cy0, tmp, st, (u64*)masks);
  HUGS_CHECK_LAUNCH("k_cd_place");
  return 0;
}

extern "C" int hugs_amg_pack(int K, int H, int W, int unpack, void* planes, void* masks, void* stream) {
  AG_REQUIRE_HW("hugs_amg_pack");
  AG_REQUIRE_K("hugs_amg_pack", K);
  HUGS_REQUIRE(planes && masks, -2, "hugs_amg_pack: null pointer");
  const int WC = (W + 63) / 64;
  const long long nwords = (long long)K * H * WC;
  HUGS_REQUIRE(nwords < (1ll << 32), -2, "hugs_amg_pack: %lld plane words (under 2^32)", nwords);
  const int grid = (int)((nwords + 3) / 4);
  if (unpack) k_unpack<<<grid, AG_T, 0, (hipStream_t)stream>>>(nwords, W, WC, (const u64*)masks, (uint8_t*)planes);
  else k_pack<<<grid, AG_T, 0, (hipStream_t)stream>>>(nwords, W, WC, (const uint8_t*)planes, (u64*)masks);
  HUGS_CHECK_LAUNCH("k_pack");
  return 0;
}

extern "C" int hugs_amg_mask_stats(int K, int H, int W, const void* masks, int* boxes, int* area, void* stream) {
  AG_REQUIRE_HW("hugs_amg_mask_stats");
  AG_REQUIRE_K("hugs_amg_mask_stats", K);
  HUGS_REQUIRE(masks && boxes && area, -2, "hugs_amg_mask_stats: null pointer");
  k_bits_stats<<<K, AG_T, 0, (hipStream_t)stream>>>(H, (W + 63) / 64, (const u64*)masks, boxes, area);
  HUGS_CHECK_LAUNCH("k_bits_stats");
  return 0;
}

extern "C" int hugs_amg_rank(int K, const void* keys, int keys_int, int* rank, int* order, void* stream) {
  AG_REQUIRE_K("hugs_amg_rank", K);
  HUGS_REQUIRE(keys && rank && order, -2, "hugs_amg_rank: null pointer");
  if (keys_int) k_rank<int><<<(K + AG_T - 1) / AG_T, AG_T, 0, (hipStream_t)stream>>>(K, (const int*)keys, rank, order);
  else k_rank<float><<<(K + AG_T - 1) / AG_T, AG_T, 0, (hipStream_t)stream>>>(K, (const float*)keys, rank, order);
  HUGS_CHECK_LAUNCH("k_rank");
  return 0;
}

extern "C" int hugs_amg_nms(int K, const int* boxes, const int* order, float iou_threshold, int* keep, int* nkeep, void* ws, void* stream) {
  AG_REQUIRE_K("hugs_amg_nms", K);
  HUGS_REQUIRE(boxes && order && keep && nkeep && ws, -2, "hugs_amg_nms: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int T = (K + 63) / 64;
  k_nms_matrix<<<dim3(T, T), AG_T, 0, s>>>(K, T, boxes, order, iou_threshold, (u64*)ws);
  HUGS_CHECK_LAUNCH("k_nms_matrix");
  k_nms_reduce<<<1, HUGS_WAVE, 0, s>>>(K, T, (const u64*)ws, order, keep, nkeep);
  HUGS_CHECK_LAUNCH("k_nms_reduce");
  return 0;
}

extern "C" int hugs_amg_gather(int K, long long row, const int* keep, const int* nkeep, const int* sel, const void* src, const void* alt,
                               void* dst, void* stream) {
  AG_REQUIRE_K("hugs_amg_gather", K);
  HUGS_REQUIRE(row >= 1 && row <= (1ll << 24), -2, "hugs_amg_gather: rows of %lld words (1..2^24)", row);
  HUGS_REQUIRE(keep && nkeep && src && dst && dst != src && (!alt || sel), -2, "hugs_amg_gather: null or aliased pointer");
  const int gx = (int)((row + AG_T - 1) / AG_T < 64 ? (row + AG_T - 1) / AG_T : 64);
  k_gather_rows<<<dim3(gx, K), AG_T, 0, (hipStream_t)stream>>>(row, keep, nkeep, sel, (const int*)src, (const int*)alt, (int*)dst);
  HUGS_CHECK_LAUNCH("k_gather_rows");
  return 0;
}

extern "C" int hugs_amg_small_regions(int K, int H, int W, int min_area, const void* masks, const int* boxes, void* clean, int* changed,
                                      int chunk, void* ws, void* stream) {
  AG_REQUIRE_HW("hugs_amg_small_regions");
  AG_REQUIRE_K("hugs_amg_small_regions", K);
  HUGS_REQUIRE(min_area >= 1 && chunk >= 1 && chunk <= AG_MAXK, -2, "hugs_amg_small_regions: min_area %d, chunk %d (both >= 1)", min_area, chunk);
  HUGS_REQUIRE(masks && boxes && clean && clean != masks && changed && ws, -2, "hugs_amg_small_regions: null or aliased pointer");
  hipStream_t s = (hipStream_t)stream;
  const int WC = (W + 63) / 64, tiles = WC * ((H + SR_H - 1) / SR_H);
  const SrWs w = sr_ws(ws, H, W, chunk);
  const u64* src = (const u64*)masks;
  u64* out = (u64*)clean;
  for (int k0 = 0; k0 < K; k0 += chunk) {
    const int n = K - k0 < chunk ? K - k0 : chunk;
    const dim3 grid(tiles, n);
    k_sr_init<<<(n + AG_T - 1) / AG_T, AG_T, 0, s>>>(n, k0, w, changed);
    HUGS_CHECK_LAUNCH("k_sr_init");
    for (int mode = 0; mode < 2; ++mode) {
      const u64* in = mode ? out : src;
      k_sr_label<<<grid, AG_T, 0, s>>>(mode, H, W, WC, k0, in, boxes, w);
      HUGS_CHECK_LAUNCH("k_sr_label");
      k_sr_merge<<<grid, AG_T, 0, s>>>(mode, H, W, WC, k0, boxes, w);
      HUGS_CHECK_LAUNCH("k_sr_merge");
      k_sr_count<<<grid, AG_T, 0, s>>>(mode, H, W, WC, k0, boxes, w);
      HUGS_CHECK_LAUNCH("k_sr_count");
      if (mode) {
        k_sr_best<<<grid, AG_T, 0, s>>>(H, W, WC, k0, min_area, boxes, w);
        HUGS_CHECK_LAUNCH("k_sr_best");
      }
      k_sr_apply<<<grid, AG_T, 0, s>>>(mode, H, W, WC, k0, min_area, in, boxes, w, out, changed);
      HUGS_CHECK_LAUNCH("k_sr_apply");
    }
  }
  return 0;
}

extern "C" int hugs_amg_paint(int S, int H, int W, const void* masks, const int* boxes, const int* order, int* seg, void* stream) {
  AG_REQUIRE_HW("hugs_amg_paint");
  HUGS_REQUIRE(S >= 0 && S <= AG_MAXK, -2, "hugs_amg_paint: %d masks (0..%d)", S, AG_MAXK);
  HUGS_REQUIRE(seg && (S == 0 || (masks && boxes && order)), -2, "hugs_amg_paint: null pointer");
  const int WC = (W + 63) / 64;
  k_paint<<<(H * WC + 3) / 4, AG_T, 0, (hipStream_t)stream>>>(S, H, W, WC, (const u64*)masks, boxes, order, seg);
  HUGS_CHECK_LAUNCH("k_paint");
  return 0;
}
