// Colour correction of an eval render on the device (reference MipNeRF360/internal/image.py:82-124 color_correct), fp64 throughout.
//   features a(x) = [x_c x_d (c <= d)] ++ [x_c] ++ [1]  (F = nc(nc+1)/2 + nc + 1; 10 for RGB), per channel c the mask
//   m_c = ok(x0_c) & ok(x_c) & ok(r_c), ok(z) = eps <= z <= 1-eps, w_c = minimum-norm least-squares fit of r_c on a(x) over
//   the masked pixels, x <- clip(a(x) W, 0, 1), num_iters times.
// The least squares is solved through its normal equations.  One pass kernel per iteration streams the image once:
//   * lane l of a wave owns pixel 64*chunk + l: it loads x_{k-1}, applies the previous warp (x_k = clip(a(x_{k-1}) W_{k-1})),
//     stores x_k, takes the masks and stages [x | 1 | 0 | r | m] of its pixel in the wave's LDS rows;
//   * then 16 steps of v_mfma_f64_16x16x4_f64 eat the 64 staged pixels 4 at a time.  Operand layout (CDNA3 ISA 7.1.4, f64
//     16x16x4): A[i][k] and B[k][j] live in lane 16*k + i (resp. + j), so lane l = 16*g + t builds ONE value -- feature t of
//     pixel g of the step -- from two LDS reads (the factor slots of feature t are lane constants; "1" and "0" are slots, so
//     the linear, bias and padding rows need no branch).  A = m_c * feature (rows >= F zero), B = feature, except column F
//     = r_c and column F+1 = 1: one MFMA per channel accumulates A^T M A, the right-hand side A^T M r_c (column F) and the
//     masked count (column F+1, when it fits) in one 16x16 tile, nc tiles of 4 doubles per lane in all.
//     Result layout: D[i][j] is register i/4 of lane 16*(i%4) + j.
//   * the waves of a block add their tiles in LDS in wave order and the block writes one nc x 16 x 16 partial; a one-block
//     solve kernel sums the partials in block order (no floating-point atomics: run-to-run deterministic), diagonalises each
//     F x F Gram matrix with a fixed number of cyclic Jacobi sweeps (one wave per channel, lane k owns row/column k), and
//     forms w = V diag(1/lambda, lambda > 1e-12 lambda_max) V^T b: the pseudo-inverse, i.e. lstsq's minimum-norm solution
//     (w = 0 for an empty mask).  800x1000x3, 5 iterations: 1.96 ms, of which the five solves 1.7 ms (profiles/colorcc_eval.txt).
#include "hugs_common.h"

namespace {

typedef double cc_d4 __attribute__((ext_vector_type(4)));

constexpr int CC_THREADS = 256, CC_WAVES = CC_THREADS / HUGS_WAVE;
constexpr int CC_MAX_BLOCKS = 512;     // two workgroups per CU of a 256-CU part; a constant, so the summation order is a function of npix alone
constexpr int CC_W_SLOTS = 64;         // doubles reserved for W (F * nc <= 60) at the head of the workspace
constexpr int CC_SWEEPS = 12;          // cyclic Jacobi converges quadratically: 15x15 PSD matrices are diagonal to rounding after 7-8
constexpr double CC_CUT = 1e-12;       // eigenvalues <= CC_CUT * lambda_max are treated as zero

__host__ __device__ constexpr int cc_features(int nc) { return nc * (nc + 1) / 2 + nc + 1; }

static int cc_blocks(long long npix) {
  long long b = (npix + CC_THREADS - 1) / CC_THREADS;
  return (int)(b < CC_MAX_BLOCKS ? b : CC_MAX_BLOCKS);
}

// y = a(x) W for one pixel, W [F][NC] in LDS; everything static so x, y stay in registers
template <int NC>
__device__ __forceinline__ void cc_warp(const double* x, const double* sW, double* y) {
#pragma unroll
  for (int e = 0; e < NC; ++e) y[e] = 0.;
  int t = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int d = c; d < NC; ++d, ++t) {
      const double f = x[c] * x[d];
#pragma unroll
      for (int e = 0; e < NC; ++e) y[e] += f * sW[t * NC + e];
    }
#pragma unroll
  for (int c = 0; c < NC; ++c, ++t)
#pragma unroll
    for (int e = 0; e < NC; ++e) y[e] += x[c] * sW[t * NC + e];
#pragma unroll
  for (int e = 0; e < NC; ++e) y[e] = fmin(fmax(y[e] + sW[t * NC + e], 0.), 1.);
}

// xin: the iterate to read (img itself in the first pass).  W != null: warp it first and store the result to xout.
// accum != 0: accumulate the normal equations of the (warped) iterate into part[blockIdx.x].
template <int NC>
__global__ void __launch_bounds__(CC_THREADS)
k_cc_pass(long long npix, const double* img, const double* ref, const double* xin, double* xout, const double* W, double eps,
          int accum, double* __restrict__ part) {
  constexpr int F = cc_features(NC);
  constexpr int ONE = NC, ZERO = NC + 1, RS = NC + 2, MS = 2 * NC + 2, ROW = 3 * NC + 2;
  __shared__ double sW[F * NC];
  __shared__ double stage[CC_WAVES][HUGS_WAVE * ROW];
  __shared__ double red[NC * 256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = lane & 15, g = lane >> 4;
  if (W) {
    for (int i = tid; i < F * NC; i += CC_THREADS) sW[i] = W[i];
    __syncthreads();
  }
  // the two factor slots of this lane's feature (row t of A, column t of B)
  int p = ZERO, q = ZERO;
  {
    int u = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int d = c; d < NC; ++d, ++u)
        if (u == t) { p = c; q = d; }
#pragma unroll
    for (int c = 0; c < NC; ++c, ++u)
      if (u == t) { p = c; q = ONE; }
    if (t == F - 1 || t == F + 1) p = q = ONE;       // bias feature; count column
  }
  const bool is_feat = t < F, is_rhs = t == F;
  const int sel0 = is_feat ? MS : (is_rhs ? RS : ZERO), selstep = (is_feat || is_rhs) ? 1 : 0;
  const double hi = 1. - eps;
  double* st = stage[wave];
  cc_d4 acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = cc_d4{0., 0., 0., 0.};

  const long long nchunk = (npix + 63) / 64;
  for (long long base = (long long)blockIdx.x * CC_WAVES; base < nchunk; base += (long long)gridDim.x * CC_WAVES) {
    const long long pix = (base + wave) * 64 + lane;      // a wave past the last chunk runs masked, so barriers stay uniform
    const bool in = pix < npix;
    double x[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) x[c] = in ? xin[pix * NC + c] : 0.;
    if (W) {
      double y[NC];
      cc_warp<NC>(x, sW, y);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        x[c] = y[c];
        if (in) xout[pix * NC + c] = y[c];
      }
    }
    if (!accum) continue;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double x0 = in ? img[pix * NC + c] : 0., r = in ? ref[pix * NC + c] : 0.;
      const bool m = in && x0 >= eps && x0 <= hi && x[c] >= eps && x[c] <= hi && r >= eps && r <= hi;
      st[lane * ROW + c] = in ? x[c] : 0.;
      st[lane * ROW + RS + c] = r;
      st[lane * ROW + MS + c] = m ? 1. : 0.;
    }
    st[lane * ROW + ONE] = 1.;
    st[lane * ROW + ZERO] = 0.;
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const double* row = st + (4 * s + g) * ROW;
      const double f = row[p] * row[q];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const double v = row[sel0 + selstep * c];          // m_c (feature rows), r_c (column F) or 0
        const double a = is_feat ? f * v : 0.;
        const double b = is_rhs ? v : f;
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!accum) return;
  // D[i][j] = register i/4 of lane 16*(i%4) + j  ->  this lane's register v is D[4v + g][t]
  for (int w = 0; w < CC_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int e = c * 256 + (4 * v + g) * 16 + t;
          red[e] = w == 0 ? acc[c][v] : red[e] + acc[c][v];
        }
    }
    __syncthreads();
  }
  for (int e = tid; e < NC * 256; e += CC_THREADS) part[(size_t)blockIdx.x * (NC * 256) + e] = red[e];
}

// One block.  Sums the partials in block order, then one wave per channel: cyclic Jacobi on G = A^T M A, w = G^+ b.
__global__ void __launch_bounds__(CC_THREADS)
k_cc_solve(int nc, int nblk, const double* __restrict__ part, double* __restrict__ W) {
  __shared__ double G[4][16][16], V[4][16][16], B[4][16], D[4][16];
  const int F = cc_features(nc);
  const int tid = threadIdx.x, k = tid & 63, ch = tid >> 6;
  for (int e = tid; e < nc * 256; e += CC_THREADS) {
    const int c = e >> 8, i = (e >> 4) & 15, j = e & 15;
    if (i >= F || j > F || (j < i)) continue;            // the upper triangle and the right-hand side are all the solve needs
    const double* pe = part + e;
    const size_t stride = (size_t)nc * 256;
    double s = 0.;
    int b = 0;
    for (; b + 16 <= nblk; b += 16) {                   // 16 loads in flight, added in block order
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = pe[(b + u) * stride];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; b < nblk; ++b) s += pe[b * stride];
    if (j == F) B[c][i] = s;
    else G[c][i][j] = G[c][j][i] = s;
  }
  const bool act = ch < nc && k < F;
  if (act)
    for (int j = 0; j < F; ++j) V[ch][k][j] = j == k ? 1. : 0.;
  __syncthreads();
  for (int sweep = 0; sweep < CC_SWEEPS; ++sweep)
    for (int p = 0; p < F - 1; ++p)
      for (int q = p + 1; q < F; ++q) {                  // the loop bounds depend on nc alone: every barrier is uniform
        double c = 1., s = 0., tt = 0., gkp = 0., gkq = 0., vkp = 0., vkq = 0., app = 0., aqq = 0., apq = 0.;
        if (act) {
          app = G[ch][p][p]; aqq = G[ch][q][q]; apq = G[ch][p][q];
          if (apq != 0.) {
            const double th = (aqq - app) / (2. * apq);
            tt = (th >= 0. ? 1. : -1.) / (fabs(th) + sqrt(th * th + 1.));
            c = rsqrt(tt * tt + 1.);
            s = tt * c;
          }
          gkp = G[ch][k][p]; gkq = G[ch][k][q]; vkp = V[ch][k][p]; vkq = V[ch][k][q];
        }
        __syncthreads();
        if (act) {
          if (k == p) {
            G[ch][p][p] = app - tt * apq;
            G[ch][p][q] = 0.;
          } else if (k == q) {
            G[ch][q][q] = aqq + tt * apq;
            G[ch][q][p] = 0.;
          } else {
            const double np_ = c * gkp - s * gkq, nq_ = s * gkp + c * gkq;
            G[ch][k][p] = G[ch][p][k] = np_;
            G[ch][k][q] = G[ch][q][k] = nq_;
          }
          V[ch][k][p] = c * vkp - s * vkq;
          V[ch][k][q] = s * vkp + c * vkq;
        }
        __syncthreads();
      }
  if (act) {                                             // lane k: eigenpair (G[k][k], V[:, k])
    double lmax = 0.;
    for (int i = 0; i < F; ++i) lmax = fmax(lmax, G[ch][i][i]);
    const double lam = G[ch][k][k];
    double d = 0.;
    if (lmax > 0. && lam > CC_CUT * lmax) {
      for (int i = 0; i < F; ++i) d += V[ch][i][k] * B[ch][i];
      d /= lam;
    }
    D[ch][k] = d;
  }
  __syncthreads();
  if (act) {
    double w = 0.;
    for (int j = 0; j < F; ++j) w += V[ch][k][j] * D[ch][j];
    W[k * nc + ch] = w;
  }
}

__global__ void __launch_bounds__(CC_THREADS) k_cc_copy(long long n, const double* __restrict__ a, double* __restrict__ o) {
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * CC_THREADS) o[i] = a[i];
}

template <int NC>
int cc_run(long long npix, int num_iters, double eps, const double* img, const double* ref, double* out, double* ws,
           hipStream_t stream) {
  double* W = ws;
  double* part = ws + CC_W_SLOTS;
  double* xbuf = part + (size_t)CC_MAX_BLOCKS * NC * 256;
  const int blocks = cc_blocks(npix);
  // iterate k (1..num_iters) lands in out when num_iters - k is even, so the last one is out
  auto buf = [&](int k) { return k == 0 ? const_cast<double*>(img) : ((num_iters - k) % 2 == 0 ? out : xbuf); };
  for (int k = 0; k <= num_iters; ++k) {
    const int accum = k < num_iters;
    k_cc_pass<NC><<<blocks, CC_THREADS, 0, stream>>>(npix, img, ref, buf(k > 0 ? k - 1 : 0), buf(k), k > 0 ? W : nullptr, eps,
                                                     accum, part);
    HUGS_CHECK_LAUNCH("k_cc_pass");
    if (accum) {
      k_cc_solve<<<1, CC_THREADS, 0, stream>>>(NC, blocks, part, W);
      HUGS_CHECK_LAUNCH("k_cc_solve");
    }
  }
  return 0;
}

}  // namespace

extern "C" long long hugs_color_correct_ws_bytes(long long npix, int nc) {
  if (npix <= 0 || nc < 1 || nc > 4) return 0;
  return (long long)sizeof(double) * (CC_W_SLOTS + (long long)CC_MAX_BLOCKS * nc * 256 + npix * nc);
}

extern "C" int hugs_color_correct(long long npix, int nc, int num_iters, double eps, const double* img, const double* ref,
                                  double* out, void* ws, void* stream) {
  HUGS_REQUIRE(img && ref && out && ws, -2, "hugs_color_correct: null pointer");
  HUGS_REQUIRE(out != img, -2, "hugs_color_correct: out may not alias img");
  HUGS_REQUIRE(npix > 0 && nc >= 1 && nc <= 4 && num_iters >= 0, -2,
               "hugs_color_correct: bad arguments (npix=%lld, nc=%d (1..4), num_iters=%d)", npix, nc, num_iters);
  hipStream_t s = (hipStream_t)stream;
  if (num_iters == 0) {
    const long long n = npix * nc;
    const long long b = (n + CC_THREADS - 1) / CC_THREADS;
    k_cc_copy<<<(int)(b < 1024 ? b : 1024), CC_THREADS, 0, s>>>(n, img, out);
    HUGS_CHECK_LAUNCH("k_cc_copy");
    return 0;
  }
  switch (nc) {
    case 1: return cc_run<1>(npix, num_iters, eps, img, ref, out, (double*)ws, s);
    case 2: return cc_run<2>(npix, num_iters, eps, img, ref, out, (double*)ws, s);
    case 3: return cc_run<3>(npix, num_iters, eps, img, ref, out, (double*)ws, s);
    default: return cc_run<4>(npix, num_iters, eps, img, ref, out, (double*)ws, s);
  }
}
