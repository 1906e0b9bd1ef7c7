// The SfM point prompts of HuGS/generate_static_mask.py:293-336 on the device: COLMAP's 2-D observations of one image ->
// the [N,P,2] prompts SAM's decoder takes.  Built with -ffp-contract=off and correctly rounded sqrt (build.sh): a distance is
// sqrt(dx*dx + dy*dy) with every operation rounded to fp32 on its own, what torch.linalg.norm computes for two components.
//
// One family, "for every point i reduce something over all points j", for the three stages that are not element-wise:
//   sp_stream: a workgroup is ONE wave; lane l owns point i = 64 b + l in registers.  The j points go through LDS in tiles of
//   256 (x, y[, state]): while the wave works on one buffer, the next tile's four points per lane are already in flight from
//   global memory and are stored to the other buffer afterwards -- one barrier per tile.  The inner loop reads tile[jj] at a
//   wave-uniform address (an LDS broadcast), so it is pure VALU.  The body tells the skeleton whether its lane still needs
//   tiles; when no lane does, the sweep ends.
//
//   1. delete_same_points (:81-94), greedy in index order.  State per point {0 unknown, 1 kept, 2 dropped}; a round
//      (k_dd_round) lets every unknown i look at the j < i (the tiles at or below its own): a kept j closer than the threshold
//      drops it, no kept or unknown j closer keeps it, else it waits.  d < thr is decided as s < t2 on the squared distance s,
//      with t2 = the smallest fp32 whose correctly rounded root reaches thr (sp_sq_threshold): the same decision, no sqrt.
//      States only ever move from unknown to a final value, so a round may read states other workgroups write in the same
//      launch: a stale "unknown" only postpones a decision.  Round r reads the number of unknowns left in cnt[r] and adds its
//      own to cnt[r + 1]; with cnt[r] == 0 the launch exits at once, and a workgroup without an unknown point exits before its
//      first tile.  The lowest unknown index is decided in every round.  What is left after the caller's last round is walked
//      in index order by one workgroup (k_dd_walk: 1024 lanes share the j < i of one point) -- the greedy loop itself.
//   2. delete_outlier_points (:97-107).  k_ol_sweep, grid (i tiles, j splits): row minimum (fp32) and fp64 sums of d and d*d
//      of the fp32 d over j != i; a wave writes one partial pair and a split's row minima.  k_ol_flag sums the partials in
//      index order (every workgroup does, identically), forms mean and unbiased std over the n (n - 1) distances and flags
//      min < mean + c std in fp64.  No floating atomics: bit-identical from run to run.
//   3. nearest_points (:331-333).  k_nn<K>: a sorted (distance, index) list of K entries per lane in registers, inserted into
//      by a fully unrolled compare-and-shift (static indices only).  j ascends, and only a strictly smaller distance moves an
//      entry: equal distances stay lower index first.  s > bound (bound >= the K-th distance squared) skips the sqrt.
// Order-preserving compaction (k_cp_count, k_cp_scatter): per-256 counts, then each workgroup sums the counts before it and
// places its survivors by ballot ranks.  The filter (:296-309) is element-wise fp64 (k_fp_filter) + that compaction.
#include "hugs_common.h"
#include <math.h>

namespace {

constexpr int SP_T = HUGS_WAVE;        // lanes = i points of a sweep workgroup
constexpr int SP_TJ = 256;             // j points of an LDS tile
constexpr int SP_PER = SP_TJ / SP_T;
constexpr int SP_MAXN = 65536;         // points of the all-pairs stages
constexpr int SP_MAXM = 1 << 20;       // observations of the filter
constexpr int SP_CT = 256;             // element-wise / compaction workgroup
constexpr int SP_CNT = 64;             // int32 counters at the head of the dedupe workspace: cnt[r] = unknowns before round r
constexpr int SP_WALK_T = 1024;
constexpr int SP_MAXSPLIT = 16;
constexpr int SP_MAXK = 32;

__device__ __forceinline__ float sp_d2(float2 p, float2 q) {
  const float dx = __fsub_rn(p.x, q.x), dy = __fsub_rn(p.y, q.y);
  return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}

// Streams the j tiles jt0 .. jt1 - 1 through LDS; body(j0, jn, tile, states) handles the jn points from j0 on and returns
// whether its lane wants further tiles.  Every lane of the workgroup must call it with the same range.
template <bool STATE, class F>
__device__ __forceinline__ void sp_stream(int n, const float2* pts, const int* state, int jt0, int jt1, F&& body) {
  __shared__ float2 sp[2][SP_TJ];
  __shared__ int ss[2][STATE ? SP_TJ : 1];
  if (jt0 >= jt1) return;
  const int lane = threadIdx.x;
  float2 rp[SP_PER];
  int rs[SP_PER];
#pragma unroll
  for (int c = 0; c < SP_PER; ++c) {
    const int j = jt0 * SP_TJ + c * SP_T + lane;
    sp[0][c * SP_T + lane] = j < n ? pts[j] : make_float2(0.f, 0.f);
    if (STATE) ss[0][c * SP_T + lane] = j < n ? state[j] : 2;
  }
  __syncthreads();
  for (int jt = jt0; jt < jt1; ++jt) {
    const int buf = (jt - jt0) & 1;
    const bool more = jt + 1 < jt1;
    if (more) {
#pragma unroll
      for (int c = 0; c < SP_PER; ++c) {
        const int j = (jt + 1) * SP_TJ + c * SP_T + lane;
        rp[c] = j < n ? pts[j] : make_float2(0.f, 0.f);
        if (STATE) rs[c] = j < n ? state[j] : 2;
      }
    }
    const int j0 = jt * SP_TJ;
    const bool want = body(j0, min(SP_TJ, n - j0), sp[buf], ss[STATE ? buf : 0]);
    if (more) {
#pragma unroll
      for (int c = 0; c < SP_PER; ++c) {
        sp[buf ^ 1][c * SP_T + lane] = rp[c];
        if (STATE) ss[buf ^ 1][c * SP_T + lane] = rs[c];
      }
    }
    if (!__syncthreads_or(want)) break;
  }
}

// ---------------------------------------------------------------- filter (:296-309)
__global__ void __launch_bounds__(SP_CT) k_fp_filter(int m, const double* __restrict__ xys, const int* __restrict__ track_len, int thr,
                                                     double fw, double fh, double W, double H, float2* __restrict__ tmp,
                                                     int* __restrict__ keep) {
  const int i = blockIdx.x * SP_CT + threadIdx.x;
  if (i >= m) return;
  const int t = track_len[i];
  keep[i] = (thr == 0 || (t >= 0 && t >= thr)) ? 1 : 0;
  double x = xys[2 * (size_t)i] * fw, y = xys[2 * (size_t)i + 1] * fh;      // np.clip: NaN passes through
  x = x < 0. ? 0. : x;
  x = x > W ? W : x;
  y = y < 0. ? 0. : y;
  y = y > H ? H : y;
  tmp[i] = make_float2((float)x, (float)y);
}

// ---------------------------------------------------------------- order-preserving compaction of the entries with keep == 1
__global__ void __launch_bounds__(SP_CT) k_cp_count(int n, const int* __restrict__ keep, int* __restrict__ bcount) {
  const int i = blockIdx.x * SP_CT + threadIdx.x;
  const int c = __syncthreads_count(i < n && keep[i] == 1);
  if (threadIdx.x == 0) bcount[blockIdx.x] = c;
}

__global__ void __launch_bounds__(SP_CT) k_cp_scatter(int n, const int* __restrict__ keep, const int* __restrict__ bcount,
                                                      const float2* __restrict__ src, float2* __restrict__ out, int* __restrict__ index,
                                                      int* __restrict__ count) {
  __shared__ int red[SP_CT / HUGS_WAVE], wcnt[SP_CT / HUGS_WAVE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, i = b * SP_CT + tid;
  int before = 0;
  for (int c = tid; c < b; c += SP_CT) before += bcount[c];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) before += __shfl_xor(before, d);
  const bool flag = i < n && keep[i] == 1;
  const unsigned long long bal = __ballot(flag);
  if (lane == 0) {
    red[wave] = before;
    wcnt[wave] = __popcll(bal);
  }
  __syncthreads();
  int pos = red[0] + red[1] + red[2] + red[3];
  for (int w = 0; w < wave; ++w) pos += wcnt[w];
  pos += __popcll(bal & ((1ull << lane) - 1ull));
  if (flag) {
    out[pos] = src[i];
    if (index) index[pos] = i;
  }
  if (b == gridDim.x - 1 && tid == 0) *count = red[0] + red[1] + red[2] + red[3] + wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// ---------------------------------------------------------------- 1. delete_same_points
__global__ void __launch_bounds__(SP_CT) k_dd_init(int n, int* __restrict__ state, int* __restrict__ cnt) {
  const int i = blockIdx.x * SP_CT + threadIdx.x;
  if (i < n) state[i] = 0;
  if (i < SP_CNT) cnt[i] = i == 0 ? n : 0;
}

__global__ void __launch_bounds__(SP_T) k_dd_round(int n, const float2* pts, int* state, float t2, const int* cnt_in, int* cnt_out) {
  if (*cnt_in == 0) return;
  const int lane = threadIdx.x, i = blockIdx.x * SP_T + lane;
  const bool unk = i < n && state[i] == 0;
  if (!__syncthreads_or(unk)) return;
  const float2 p = i < n ? pts[i] : make_float2(0.f, 0.f);
  bool hitk = false, hitu = false;
  const int last = min(n, (blockIdx.x + 1) * SP_T) - 1;          // the block's highest i: tiles beyond last - 1 hold no j < i
  sp_stream<true>(n, pts, state, 0, (last + SP_TJ - 1) / SP_TJ, [&](int j0, int jn, const float2* tp, const int* ts) {
    if (unk && !hitk) {
      for (int jj = 0; jj < jn; ++jj) {
        const bool close = sp_d2(p, tp[jj]) < t2 && j0 + jj < i;
        const int s = ts[jj];
        hitk |= close && s == 1;
        hitu |= close && s == 0;
      }
    }
    return unk && !hitk;
  });
  const bool left = unk && !hitk && hitu;
  if (unk && !left) state[i] = hitk ? 2 : 1;
  const int c = __popcll(__ballot(left));
  if (lane == 0 && c) atomicAdd(cnt_out, c);
}

// the greedy loop on what the rounds left: by the time i is reached every j < i is decided, so only the kept ones count
__global__ void __launch_bounds__(SP_WALK_T) k_dd_walk(int n, const float2* __restrict__ pts, int* state, float t2, const int* cnt) {
  if (*cnt == 0) return;
  volatile int* vs = state;
  for (int i = 0; i < n; ++i) {
    if (vs[i] != 0) continue;              // the same word for every lane, last written before the barrier below
    const float2 p = pts[i];
    bool hit = false;
    for (int j = threadIdx.x; j < i; j += SP_WALK_T) hit |= vs[j] == 1 && sp_d2(p, pts[j]) < t2;
    const int any = __syncthreads_or(hit);
    if (threadIdx.x == 0) vs[i] = any ? 2 : 1;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- 2. delete_outlier_points
struct OlStats {
  double mean, std, thr, pad;
};

__global__ void __launch_bounds__(SP_T) k_ol_sweep(int n, int split, int per, const float2* __restrict__ pts, float* __restrict__ minpart,
                                                   double* __restrict__ part) {
  const int lane = threadIdx.x, i = blockIdx.x * SP_T + lane, s = blockIdx.y;
  const int njt = (n + SP_TJ - 1) / SP_TJ, jt0 = s * per, jt1 = min(njt, jt0 + per);
  const float2 p = i < n ? pts[i] : make_float2(0.f, 0.f);
  float mn = INFINITY;
  double s1 = 0., s2 = 0.;
  sp_stream<false>(n, pts, nullptr, jt0, jt1, [&](int j0, int jn, const float2* tp, const int*) {
    for (int jj = 0; jj < jn; ++jj) {
      const float d = sqrtf(sp_d2(p, tp[jj]));
      if (j0 + jj != i) {
        const double dd = (double)d;
        mn = fminf(mn, d);
        s1 += dd;
        s2 += dd * dd;
      }
    }
    return true;
  });
  if (i < n) minpart[(size_t)s * n + i] = mn;
  else s1 = s2 = 0.;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    s1 += __shfl_xor(s1, d);
    s2 += __shfl_xor(s2, d);
  }
  if (lane == 0) {
    part[2 * ((size_t)blockIdx.x * split + s)] = s1;
    part[2 * ((size_t)blockIdx.x * split + s) + 1] = s2;
  }
}

__global__ void __launch_bounds__(SP_CT) k_ol_flag(int n, int split, int nparts, const float* __restrict__ minpart,
                                                   const double* __restrict__ part, float coef, int* __restrict__ keep,
                                                   int* __restrict__ bcount, OlStats* __restrict__ stats) {
  __shared__ double r1[SP_CT / HUGS_WAVE], r2[SP_CT / HUGS_WAVE];
  const int tid = threadIdx.x, i = blockIdx.x * SP_CT + tid;
  double s1 = 0., s2 = 0.;
  for (int c = tid; c < nparts; c += SP_CT) {
    s1 += part[2 * c];
    s2 += part[2 * c + 1];
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    s1 += __shfl_xor(s1, d);
    s2 += __shfl_xor(s2, d);
  }
  if ((tid & 63) == 0) {
    r1[tid >> 6] = s1;
    r2[tid >> 6] = s2;
  }
  __syncthreads();
  s1 = (r1[0] + r1[1]) + (r1[2] + r1[3]);
  s2 = (r2[0] + r2[1]) + (r2[2] + r2[3]);
  const double N = (double)n * (double)(n - 1), mean = s1 / N;
  double var = (s2 - s1 * s1 / N) / (N - 1.);
  var = var > 0. ? var : 0.;
  const double sd = sqrt(var), thr = mean + (double)coef * sd;
  bool flag = false;
  if (i < n) {
    float mn = minpart[i];
    for (int s = 1; s < split; ++s) mn = fminf(mn, minpart[(size_t)s * n + i]);
    flag = (double)mn < thr;
    keep[i] = flag ? 1 : 0;
  }
  const int c = __syncthreads_count(flag);
  if (tid == 0) bcount[blockIdx.x] = c;
  if (blockIdx.x == 0 && tid == 0) {
    stats->mean = mean;
    stats->std = sd;
    stats->thr = thr;
    stats->pad = 0.;
  }
}

// ---------------------------------------------------------------- 3. nearest_points
template <int K>
__global__ void __launch_bounds__(SP_T) k_nn(int n, int kk, const float2* __restrict__ pts, float2* __restrict__ out, int* __restrict__ index) {
  const int lane = threadIdx.x, i = blockIdx.x * SP_T + lane;
  const float2 p = i < n ? pts[i] : make_float2(0.f, 0.f);
  float dk[K];
  int ik[K];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    dk[t] = INFINITY;
    ik[t] = -1;
  }
  float bound = INFINITY;                  // >= dk[K-1]^2 as a real number: s > bound means sqrt(s) >= dk[K-1], never inserted
  sp_stream<false>(n, pts, nullptr, 0, (n + SP_TJ - 1) / SP_TJ, [&](int j0, int jn, const float2* tp, const int*) {
    for (int jj = 0; jj < jn; ++jj) {
      const float s = sp_d2(p, tp[jj]);
      if (s > bound) continue;
      const float d = sqrtf(s);
      if (!(d < dk[K - 1])) continue;
      const int j = j0 + jj;
#pragma unroll
      for (int t = K - 1; t > 0; --t) {
        const bool up = d < dk[t - 1], here = !up && d < dk[t];
        ik[t] = up ? ik[t - 1] : (here ? j : ik[t]);
        dk[t] = up ? dk[t - 1] : (here ? d : dk[t]);
      }
      if (d < dk[0]) {
        dk[0] = d;
        ik[0] = j;
      }
      bound = __fmul_rn(__fmul_rn(dk[K - 1], dk[K - 1]), 1.00000048f);      // (1 + 2^-21: above the rounding of the square)
    }
    return true;
  });
  if (i >= n) return;
#pragma unroll
  for (int t = 0; t < K; ++t) {
    if (t < kk) {
      const int j = ik[t];
      index[(size_t)i * kk + t] = j;
      out[(size_t)i * kk + t] = j >= 0 ? pts[j] : make_float2(NAN, NAN);      // (only NaN / inf coordinates leave a slot empty)
    }
  }
}

// the smallest fp32 s with sqrt(s) >= thr (correctly rounded): d < thr  <=>  d^2-sum < this
float sp_sq_threshold(float thr) {
  if (!(thr > 0.f)) return 0.f;
  volatile float s = thr * thr;
  while (s > 0.f && sqrtf(s) >= thr) s = nextafterf(s, 0.f);
  while (sqrtf(s) < thr) s = nextafterf(s, INFINITY);
  return s;
}

int sp_blocks(int n) { return n > 0 ? (n + SP_CT - 1) / SP_CT : 1; }

// j splits of the outlier sweep: enough workgroups for the device at small n; a function of n alone (the summation order)
int ol_split(int n) {
  const int nbi = (n + SP_T - 1) / SP_T, njt = (n + SP_TJ - 1) / SP_TJ;
  int split = (1024 + nbi - 1) / nbi;
  split = split < njt ? split : njt;
  return split < SP_MAXSPLIT ? (split > 0 ? split : 1) : SP_MAXSPLIT;
}

struct OlLayout {
  int split, per, nparts;
  size_t part, minpart, keep, bcount, bytes;      // byte offsets behind the OlStats head
};

OlLayout ol_layout(int n) {
  OlLayout L;
  const int njt = (n + SP_TJ - 1) / SP_TJ;
  L.split = ol_split(n);
  L.per = (njt + L.split - 1) / L.split;
  L.nparts = ((n + SP_T - 1) / SP_T) * L.split;
  L.part = sizeof(OlStats);
  L.minpart = L.part + (size_t)L.nparts * 2 * sizeof(double);
  L.keep = L.minpart + (size_t)L.split * n * sizeof(float);
  L.bcount = L.keep + (size_t)n * sizeof(int);
  L.bytes = L.bcount + (size_t)sp_blocks(n) * sizeof(int);
  return L;
}

int sp_compact(int n, const int* keep, int* bcount, bool counted, const float2* src, float* out, int* index, int* count, hipStream_t s) {
  if (!counted) {
    k_cp_count<<<sp_blocks(n), SP_CT, 0, s>>>(n, keep, bcount);
    HUGS_CHECK_LAUNCH("k_cp_count");
  }
  k_cp_scatter<<<sp_blocks(n), SP_CT, 0, s>>>(n, keep, bcount, src, (float2*)out, index, count);
  HUGS_CHECK_LAUNCH("k_cp_scatter");
  return 0;
}

}  // namespace

#define SP_REQUIRE_N(name)                                                                                                     \
  HUGS_REQUIRE(n >= 1 && n <= SP_MAXN, -2, name ": %d points (1..%d: the all-pairs stages keep O(n) state and O(n^2) time)", n, \
               SP_MAXN)
#define SP_ALIGNED8(p) (((uintptr_t)(p) & 7) == 0)

extern "C" long long hugs_sfp_ws_bytes(int what, int n) {
  HUGS_REQUIRE(what >= 0 && what <= 2, -2, "hugs_sfp_ws_bytes: what = %d (0 filter, 1 same points, 2 outliers)", what);
  if (what == 0) {
    HUGS_REQUIRE(n >= 1 && n <= SP_MAXM, -2, "hugs_sfp_ws_bytes: %d observations (1..%d)", n, SP_MAXM);
    return (long long)n * 12 + (long long)sp_blocks(n) * 4;
  }
  SP_REQUIRE_N("hugs_sfp_ws_bytes");
  if (what == 1) return 4ll * (SP_CNT + n + sp_blocks(n));
  return (long long)ol_layout(n).bytes;
}

extern "C" int hugs_sfp_filter(int m, const void* xys, const int* track_len, int threshold, int cam_h, int cam_w, int H, int W,
                               float* out, int* count, void* ws, void* stream) {
  HUGS_REQUIRE(m >= 1 && m <= SP_MAXM, -2, "hugs_sfp_filter: %d observations (1..%d)", m, SP_MAXM);
  HUGS_REQUIRE(cam_h >= 1 && cam_w >= 1 && H >= 1 && W >= 1 && threshold >= 0, -2,
               "hugs_sfp_filter: camera %d x %d, image %d x %d, threshold %d", cam_h, cam_w, H, W, threshold);
  HUGS_REQUIRE(xys && track_len && out && count && ws && SP_ALIGNED8(xys) && SP_ALIGNED8(out) && SP_ALIGNED8(ws), -2,
               "hugs_sfp_filter: null or misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  float2* tmp = (float2*)ws;
  int* keep = (int*)(tmp + m);
  k_fp_filter<<<sp_blocks(m), SP_CT, 0, s>>>(m, (const double*)xys, track_len, threshold, (double)W / (double)cam_w,
                                            (double)H / (double)cam_h, (double)W, (double)H, tmp, keep);
  HUGS_CHECK_LAUNCH("k_fp_filter");
  return sp_compact(m, keep, keep + m, false, tmp, out, nullptr, count, s);
}

extern "C" int hugs_sfp_same_rounds(int n, const float* points, float threshold, int first_round, int rounds, void* ws, void* stream) {
  SP_REQUIRE_N("hugs_sfp_same_rounds");
  HUGS_REQUIRE(points && ws && SP_ALIGNED8(points), -2, "hugs_sfp_same_rounds: null or misaligned pointer");
  HUGS_REQUIRE(first_round >= 0 && rounds >= 1 && first_round + rounds < SP_CNT, -2, "hugs_sfp_same_rounds: rounds %d + %d outside 0..%d",
               first_round, rounds, SP_CNT - 1);
  HUGS_REQUIRE(threshold >= 0.f && threshold < INFINITY, -2, "hugs_sfp_same_rounds: threshold %g", (double)threshold);
  hipStream_t s = (hipStream_t)stream;
  int* cnt = (int*)ws;
  int* state = cnt + SP_CNT;
  if (first_round == 0) {
    k_dd_init<<<sp_blocks(n), SP_CT, 0, s>>>(n, state, cnt);
    HUGS_CHECK_LAUNCH("k_dd_init");
  }
  const float t2 = sp_sq_threshold(threshold);
  for (int r = first_round; r < first_round + rounds; ++r) {
    k_dd_round<<<(n + SP_T - 1) / SP_T, SP_T, 0, s>>>(n, (const float2*)points, state, t2, cnt + r, cnt + r + 1);
    HUGS_CHECK_LAUNCH("k_dd_round");
  }
  return 0;
}

extern "C" int hugs_sfp_same_finish(int n, const float* points, float threshold, int last_round, float* out, int* index, int* count,
                                    void* ws, void* stream) {
  SP_REQUIRE_N("hugs_sfp_same_finish");
  HUGS_REQUIRE(points && out && index && count && ws && SP_ALIGNED8(points) && SP_ALIGNED8(out), -2,
               "hugs_sfp_same_finish: null or misaligned pointer");
  HUGS_REQUIRE(last_round >= 1 && last_round < SP_CNT, -2, "hugs_sfp_same_finish: %d rounds were run (1..%d)", last_round, SP_CNT - 1);
  HUGS_REQUIRE(threshold >= 0.f && threshold < INFINITY, -2, "hugs_sfp_same_finish: threshold %g", (double)threshold);
  hipStream_t s = (hipStream_t)stream;
  int* cnt = (int*)ws;
  int* state = cnt + SP_CNT;
  k_dd_walk<<<1, SP_WALK_T, 0, s>>>(n, (const float2*)points, state, sp_sq_threshold(threshold), cnt + last_round);
  HUGS_CHECK_LAUNCH("k_dd_walk");
  return sp_compact(n, state, state + n, false, (const float2*)points, out, index, count, s);
}

extern "C" int hugs_sfp_outliers(int n, const float* points, float std_coefficient, float* out, int* index, int* count, void* ws,
                                 void* stream) {
  HUGS_REQUIRE(n >= 2 && n <= SP_MAXN, -2, "hugs_sfp_outliers: %d points (2..%d)", n, SP_MAXN);
  HUGS_REQUIRE(points && out && index && count && ws && SP_ALIGNED8(points) && SP_ALIGNED8(out) && SP_ALIGNED8(ws), -2,
               "hugs_sfp_outliers: null or misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  const OlLayout L = ol_layout(n);
  char* base = (char*)ws;
  double* part = (double*)(base + L.part);
  float* minpart = (float*)(base + L.minpart);
  int* keep = (int*)(base + L.keep);
  int* bcount = (int*)(base + L.bcount);
  k_ol_sweep<<<dim3((n + SP_T - 1) / SP_T, L.split), SP_T, 0, s>>>(n, L.split, L.per, (const float2*)points, minpart, part);
  HUGS_CHECK_LAUNCH("k_ol_sweep");
  k_ol_flag<<<sp_blocks(n), SP_CT, 0, s>>>(n, L.split, L.nparts, minpart, part, std_coefficient, keep, bcount, (OlStats*)base);
  HUGS_CHECK_LAUNCH("k_ol_flag");
  return sp_compact(n, keep, bcount, true, (const float2*)points, out, index, count, s);
}

extern "C" int hugs_sfp_nearest(int n, int k, const float* points, float* out, int* index, void* stream) {
  SP_REQUIRE_N("hugs_sfp_nearest");
  HUGS_REQUIRE(k >= 1 && k <= SP_MAXK && k <= n, -2, "hugs_sfp_nearest: k = %d (1..min(%d, n = %d))", k, SP_MAXK, n);
  HUGS_REQUIRE(points && out && index && SP_ALIGNED8(points) && SP_ALIGNED8(out), -2, "hugs_sfp_nearest: null or misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  const int grid = (n + SP_T - 1) / SP_T;
  const float2* p = (const float2*)points;
  if (k <= 4) k_nn<4><<<grid, SP_T, 0, s>>>(n, k, p, (float2*)out, index);
  else if (k <= 8) k_nn<8><<<grid, SP_T, 0, s>>>(n, k, p, (float2*)out, index);
  else if (k <= 16) k_nn<16><<<grid, SP_T, 0, s>>>(n, k, p, (float2*)out, index);
  else k_nn<32><<<grid, SP_T, 0, s>>>(n, k, p, (float2*)out, index);
  HUGS_CHECK_LAUNCH("k_nn");
  return 0;
}
