// K logistic regressions on embedding vectors (mkws_logreg_fit / mkws_logreg_score, include/mkws.h): what the DataPerf selection harness
// does per split with sklearn.linear_model.LogisticRegression, for P problems in one launch.  multilingual_kws_amd/logreg.py (objective,
// logreg_host) is the specification: f = C * sum_i [logsumexp(z_i) - z_{i,y_i}] + (kappa / 2) * sum W^2, z_i = W x~_i + b.
//
// Fit: one workgroup of 16 waves per problem owns the whole optimisation.  The solver is non-linear conjugate gradients (Polak-Ribiere+,
// the intercepts preconditioned by their own curvature) with an exact one-dimensional Newton line search: the logits Z and the
// direction's image ZD = X~ D^T live in LDS, Z(W + tD) = Z + t ZD, so the line search costs no pass over X.  An iteration is two gathered
// passes over the problem's rows of the bank (which stay in global memory / L2 and are never copied):
//   G  = C (P - Y)^T X~ + kappa W     a thread per column, the rows in list order, K accumulators in registers;
//   ZD = X~ D^T + db                  four rows per wave and turn, lanes across the columns, D read from LDS.
// W, D and the previous gradient live in the workspace; Z is formed again from W every kRefresh iterations so that float32 drift does not
// accumulate.  Every scalar reduction (line-search sums, beta, norms, the objective) is float64 in a fixed butterfly order, there are no
// floating-point atomics: two calls on the same input write the same bytes.  Every loop is bounded by max_iter, kLineSearchCap, K, dim or
// the row count; no workgroup waits for another.
#include "mkws_common.h"

#include <cmath>
#include <cstdint>
#include <mutex>
#include <set>

using mkws::fail;

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRows = MKWS_LOGREG_MAX_ROWS;
constexpr int kMaxK = MKWS_LOGREG_MAX_CLASSES;
constexpr int kMaxDim = MKWS_LOGREG_MAX_DIM;
constexpr int kRefresh = 10;            // Z = X~ W^T + b instead of Z += t ZD every so many iterations
constexpr int kLineSearchCap = 10;      // evaluations of phi'(t), phi''(t) per line search
constexpr double kLineSearchTol = 1e-4; // |phi'(t)| <= this * |phi'(0)| ends it
constexpr int kRowsPerTurn = 4;         // rows a wave multiplies at once in the product pass
constexpr int kRedValues = 2 * kMaxK + 1;
constexpr int kLdsCap = 160 * 1024;
static_assert(kMaxRows == kThreads && kMaxDim == kThreads, "a row per thread in the row phases, a column per thread in the gradient pass");
static_assert(kMaxK == 8, "the class loops are unrolled over 8 accumulators");

// header: reduction scratch [kWaves, kRedValues] doubles, then b, db, gb, gb_prev, 1 / curvature of b: [kMaxK] doubles each
constexpr int kHeaderBytes = (kWaves * kRedValues + 5 * kMaxK) * 8;
static_assert(kHeaderBytes % 16 == 0, "header");

// Z and R / ZD [kMaxRows, K], V = D or W [K, dim], mu and 1 / sigma [dim], the row list and the labels
size_t fit_lds_bytes(int dim, int K) {
  return kHeaderBytes + ((size_t)2 * kMaxRows * K + (size_t)K * dim + 2 * (size_t)dim) * sizeof(float) + 2 * (size_t)kMaxRows * sizeof(int32_t);
}
static_assert(kHeaderBytes + ((size_t)2 * kMaxRows * kMaxK + (size_t)kMaxK * kMaxDim + 2 * (size_t)kMaxDim) * 4 + 2 * (size_t)kMaxRows * 4 <= (size_t)kLdsCap - 4096, "LDS");

struct FitArgs {
  const float* x;
  const int32_t* rows;
  const int32_t* labels;
  const int32_t* offsets;
  const double* C;
  float* coef;
  float* intercept;
  int32_t* info;
  double* stats;
  float* work;
  int n_rows, dim, standardize, max_iter;
  double gtol;
};

// every lane gets the same value: a + b and b + a are the same bits
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// v[0 .. NV) summed over the block, every thread gets the same sums (wave sums added in wave order); two barriers
template <int NV>
__device__ inline void block_sum(double (&v)[NV], double* s_red) {
  static_assert(NV <= kRedValues, "scratch");
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = wave_sum(v[j]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) s_red[(threadIdx.x >> 6) * NV + j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double t = 0.0;
#pragma unroll 4
    for (int w = 0; w < kWaves; ++w) t += s_red[w * NV + j];
    v[j] = t;
  }
  __syncthreads();
}

__device__ inline double block_max(double v, double* s_red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = s_red[0];
  for (int w = 1; w < kWaves; ++w) t = fmax(t, s_red[w]);
  __syncthreads();
  return t;
}

// out[i, k] = sum_c x~[row i, c] * V[k, c] + bias[k] for the problem's n rows: four rows per wave and turn, lanes across the columns.
// K is a template parameter here and in the kernel: the class loops unroll without a branch per class and hold no register for a
// class that is not there
template <int K>
__device__ inline void product_pass(const float* __restrict__ x, const int32_t* s_rows, int n, int dim, const float* s_mu, const float* s_sc,
                                    const float* s_V, const double* s_bias, float* s_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i0 = wave * kRowsPerTurn; i0 < n; i0 += kWaves * kRowsPerTurn) {
    const float* __restrict__ xr[kRowsPerTurn];
#pragma unroll
    for (int r = 0; r < kRowsPerTurn; ++r) xr[r] = x + (size_t)s_rows[min(i0 + r, n - 1)] * dim;     // (a row past the end: read again, not written)
    float acc[kRowsPerTurn][kMaxK];
#pragma unroll
    for (int r = 0; r < kRowsPerTurn; ++r)
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) acc[r][k] = 0.0f;
#pragma unroll 2
    for (int c = lane; c < dim; c += 64) {
      const float m = s_mu[c], s = s_sc[c];
      float xv[kRowsPerTurn];
#pragma unroll
      for (int r = 0; r < kRowsPerTurn; ++r) xv[r] = (xr[r][c] - m) * s;
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
          const float v = s_V[k * dim + c];
#pragma unroll
          for (int r = 0; r < kRowsPerTurn; ++r) acc[r][k] = fmaf(xv[r], v, acc[r][k]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kRowsPerTurn; ++r) {
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
          const float t = wave_sum(acc[r][k]);
          if (lane == 0 && i0 + r < n) s_out[(i0 + r) * K + k] = t + (float)s_bias[k];
        }
      }
    }
  }
}

template <int K>
__global__ __launch_bounds__(kThreads) void logreg_fit_kernel(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char s_raw[];
  const int dim = a.dim;
  double* s_red = reinterpret_cast<double*>(s_raw);
  double* s_b = s_red + kWaves * kRedValues;
  double* s_db = s_b + kMaxK;
  double* s_gb = s_db + kMaxK;
  double* s_gbp = s_gb + kMaxK;
  double* s_mb = s_gbp + kMaxK;
  float* s_Z = reinterpret_cast<float*>(s_raw + kHeaderBytes);       // [n, K] the logits at (W, b)
  float* s_B = s_Z + (size_t)kMaxRows * K;                           // [n, K] C (P - Y) during the gradient pass, ZD during the line search
  float* s_V = s_B + (size_t)kMaxRows * K;                           // [K, dim] the matrix the product pass multiplies by: D, or W
  float* s_mu = s_V + (size_t)K * dim;                               // [dim]
  float* s_sc = s_mu + dim;                                          // [dim] 1 / sigma
  int32_t* s_rows = reinterpret_cast<int32_t*>(s_sc + dim);          // [n]
  int32_t* s_label = s_rows + kMaxRows;                              // [n]

  const int p = blockIdx.x, tid = threadIdx.x;
  const int begin = a.offsets[p];
  const int n = a.offsets[p + 1] - begin;
  int32_t* __restrict__ info = a.info + (size_t)p * 4;
  if (n < 1 || n > kMaxRows) {                                       // nothing of the problem is touched
    if (tid < 4) info[tid] = tid == 0 ? 2 : tid == 3 ? n : 0;
    return;
  }
  int bad = 0;
  if (tid < n) {
    const int r = a.rows[(size_t)begin + tid], y = a.labels[(size_t)begin + tid];
    bad = (unsigned)r >= (unsigned)a.n_rows || (unsigned)y >= (unsigned)K;
    s_rows[tid] = r;
    s_label[tid] = y;
  }
  if (__syncthreads_or(bad)) {                                       // (the barrier also publishes the lists)
    if (tid < 4) info[tid] = tid == 0 ? 2 : tid == 3 ? n : 0;
    return;
  }
  const float* __restrict__ x = a.x;
  const double C = a.C[p];
  const float Cf = (float)C;
  const double kap = K == 2 ? 2.0 : 1.0;
  const size_t kd = (size_t)K * dim;
  float* __restrict__ wW = a.work + (size_t)p * 3 * kd;              // [K, dim] each: the coefficients, the direction, the previous gradient
  float* __restrict__ wD = wW + kd;
  float* __restrict__ wG = wD + kd;

  // the scaler of the problem's own rows: a thread per column, the rows added in list order in float64
  float mu_c = 0.0f, sc_c = 1.0f;
  if (tid < dim) {
    if (a.standardize) {
      double s = 0.0;
      for (int i = 0; i < n; ++i) s += (double)x[(size_t)s_rows[i] * dim + tid];
      const double m = s / (double)n;
      double v = 0.0;
      for (int i = 0; i < n; ++i) {
        const double d = (double)x[(size_t)s_rows[i] * dim + tid] - m;
        v += d * d;
      }
      const double sigma = sqrt(v / (double)n);
      mu_c = (float)m;
      sc_c = sigma == 0.0 ? 1.0f : (float)(1.0 / sigma);
    }
    s_mu[tid] = mu_c;
    s_sc[tid] = sc_c;
    for (int k = 0; k < K; ++k) {
      wW[(size_t)k * dim + tid] = 0.0f;
      wD[(size_t)k * dim + tid] = 0.0f;
      wG[(size_t)k * dim + tid] = 0.0f;
    }
  }
  if (tid < kMaxK) {
    s_b[tid] = 0.0;
    s_db[tid] = 0.0;
    s_gb[tid] = 0.0;
    s_gbp[tid] = 0.0;
    s_mb[tid] = 1.0;
  }
  if (tid < n)
    for (int k = 0; k < K; ++k) s_Z[tid * K + k] = 0.0f;
  __syncthreads();

  int n_iter = 0, reason = 1;
  double f = 0.0, gnorm = 0.0, gg_prev = 1.0;
  for (int it = 0;; ++it) {
    // ---- the objective and C (P - Y) at the cached logits: a thread per row ----
    double red[2 * K + 1];                                           // the loss, then C (p - y) and C p (1 - p) per class
#pragma unroll
    for (int j = 0; j < 2 * K + 1; ++j) red[j] = 0.0;
    if (tid < n) {
      float z[kMaxK], zmax = -INFINITY;
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        z[k] = k < K ? s_Z[tid * K + k] : -INFINITY;
        zmax = fmaxf(zmax, z[k]);
      }
      float e[kMaxK], sum = 0.0f;
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        e[k] = k < K ? expf(z[k] - zmax) : 0.0f;
        sum += e[k];
      }
      const int y = s_label[tid];
      const float inv = 1.0f / sum;
      float zy = 0.0f;
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
          const float pk = e[k] * inv;
          const float r = Cf * (pk - (k == y ? 1.0f : 0.0f));
          s_B[tid * K + k] = r;
          red[1 + k] = (double)r;
          red[1 + K + k] = (double)(Cf * (pk * (1.0f - pk)));
          if (k == y) zy = z[k];
        }
      }
      red[0] = (double)((zmax - zy) + logf(sum));
    }
    block_sum(red, s_red);                                           // (its barriers publish s_B)
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {                                // (no dynamic index into the register array)
      if (tid == k && k < K) {
        s_gb[k] = red[1 + k];
        s_mb[k] = red[1 + K + k] > 1e-30 ? 1.0 / red[1 + K + k] : 1.0;
      }
    }
    const double loss = C * red[0];

    // ---- G = C (P - Y)^T X~ + kappa W: a thread per column, the rows in list order ----
    float g[kMaxK];
    double ww = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) g[k] = 0.0f;
    if (tid < dim) {
#pragma unroll 8
      for (int i = 0; i < n; ++i) {
        const float xv = (x[(size_t)s_rows[i] * dim + tid] - mu_c) * sc_c;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
          if (k < K) g[k] = fmaf(s_B[i * K + k], xv, g[k]);
      }
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
          const float wk = wW[(size_t)k * dim + tid];
          g[k] = fmaf((float)kap, wk, g[k]);
          ww += (double)wk * (double)wk;
        }
      }
    }
    __syncthreads();                                                 // s_gb and s_mb are published; s_B has been read
    // |g|_inf, sum W^2, and for beta: g.Mg, Mg.(g - g_prev), g.D
    double r5[5] = {ww, 0.0, 0.0, 0.0, 0.0}, gmax = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k < K && tid < dim) {
        const double gk = (double)g[k], gp = (double)wG[(size_t)k * dim + tid];
        gmax = fmax(gmax, fabs(gk));
        r5[1] += gk * gk;
        r5[2] += gk * (gk - gp);
        r5[3] += gk * (double)wD[(size_t)k * dim + tid];
      }
    }
    if (tid < K) {
      const double gb = s_gb[tid], yb = s_mb[tid] * gb;
      gmax = fmax(gmax, fabs(gb));
      r5[1] += gb * yb;
      r5[2] += yb * (gb - s_gbp[tid]);
      r5[3] += gb * s_db[tid];
    }
    block_sum(r5, s_red);
    gnorm = block_max(gmax, s_red);
    f = loss + 0.5 * kap * r5[0];
    n_iter = it;
    if (gnorm <= a.gtol) {
      reason = 0;
      break;
    }
    if (it >= a.max_iter) break;                                     // reason 1

    // ---- the direction: D = -M g + beta D, beta = max(0, Mg.(g - g_prev) / g_prev.M g_prev), steepest descent when that is not downhill ----
    double beta = 0.0;
    if (it > 0) {
      beta = fmax(0.0, r5[2] / gg_prev);
      if (!(-r5[1] + beta * r5[3] < -1e-3 * r5[1])) beta = 0.0;
    }
    gg_prev = r5[1];
    double r2[2] = {0.0, 0.0};
    if (tid < dim) {
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
          const float d = fmaf((float)beta, wD[(size_t)k * dim + tid], -g[k]);
          wD[(size_t)k * dim + tid] = d;
          wG[(size_t)k * dim + tid] = g[k];
          s_V[k * dim + tid] = d;
          r2[0] += (double)wW[(size_t)k * dim + tid] * (double)d;
          r2[1] += (double)d * (double)d;
        }
      }
    }
    if (tid < K) {
      s_db[tid] = -s_mb[tid] * s_gb[tid] + beta * s_db[tid];
      s_gbp[tid] = s_gb[tid];
    }
    block_sum(r2, s_red);                                            // (its barriers publish s_V and s_db)
    const double wd = r2[0], dd = r2[1];

    // ---- ZD = X~ D^T + db ----
    product_pass<K>(x, s_rows, n, dim, s_mu, s_sc, s_V, s_db, s_B);
    __syncthreads();

    // ---- the line search on phi(t) = f(W + tD, b + t db): Newton on phi', bracketed (phi is convex); a thread per row ----
    float z[kMaxK], zd[kMaxK], zdy = 0.0f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) z[k] = zd[k] = 0.0f;
    if (tid < n) {
      const int y = s_label[tid];
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
          z[k] = s_Z[tid * K + k];
          zd[k] = s_B[tid * K + k];
          if (k == y) zdy = zd[k];
        }
      }
    }
    double t = 0.0, lo = 0.0, hi = INFINITY, slope0 = 0.0;
    bool settled = false;
    for (int e = 0; e < kLineSearchCap; ++e) {
      double d12[2] = {0.0, 0.0};
      if (tid < n) {
        const float tf = (float)t;
        float u[kMaxK], umax = -INFINITY;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
          u[k] = k < K ? fmaf(tf, zd[k], z[k]) : -INFINITY;
          umax = fmaxf(umax, u[k]);
        }
        float sum = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
          const float ek = k < K ? expf(u[k] - umax) : 0.0f;
          sum += ek;
          s1 = fmaf(ek, zd[k], s1);
          s2 = fmaf(ek * zd[k], zd[k], s2);
        }
        const float inv = 1.0f / sum, m1 = s1 * inv;
        d12[0] = (double)(m1 - zdy);
        d12[1] = (double)fmaxf(fmaf(-m1, m1, s2 * inv), 0.0f);
      }
      block_sum(d12, s_red);
      const double d1 = C * d12[0] + kap * (wd + t * dd), d2 = C * d12[1] + kap * dd;
      if (e == 0) {
        slope0 = d1;
        if (!(d1 < 0.0)) {                                           // not downhill (rounding at the floor): no step
          settled = true;
          break;
        }
      } else if (fabs(d1) <= kLineSearchTol * fabs(slope0)) {
        settled = true;
        break;
      }
      if (d1 < 0.0)
        lo = t;
      else
        hi = t;
      double tn = t - d1 / d2;
      if (!(tn > lo && tn < hi)) tn = hi < INFINITY ? 0.5 * (lo + hi) : 2.0 * lo;
      t = tn;
    }
    if (!settled && lo > 0.0) t = lo;                                // the cap: the furthest point known to be downhill of the start
    if (!(t >= 0.0) || !(t < INFINITY)) t = 0.0;

    // ---- the step ----
    const float tf = (float)t;
    if (tid < dim) {
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        if (k < K) {
          wW[(size_t)k * dim + tid] = fmaf(tf, s_V[k * dim + tid], wW[(size_t)k * dim + tid]);
        }
      }
    }
    if (tid < K) s_b[tid] += t * s_db[tid];
    if ((it + 1) % kRefresh == 0) {
      __syncthreads();                                               // every thread has read s_V (= D)
      if (tid < dim) {
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
          if (k < K) s_V[k * dim + tid] = wW[(size_t)k * dim + tid];
      }
      __syncthreads();
      product_pass<K>(x, s_rows, n, dim, s_mu, s_sc, s_V, s_b, s_Z);
    } else if (tid < n) {
#pragma unroll
      for (int k = 0; k < kMaxK; ++k)
        if (k < K) s_Z[tid * K + k] = fmaf(tf, zd[k], z[k]);
    }
    __syncthreads();
  }

  // ---- the outputs, in raw space: W = W~ / sigma, b = b~ - W~ . (mu / sigma), with sum_k b~_k = 0 ----
  double rb[kMaxK];
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) rb[k] = 0.0;
  if (tid < dim) {
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k < K) {
        const float c = wW[(size_t)k * dim + tid] * sc_c;
        a.coef[(size_t)p * kd + (size_t)k * dim + tid] = c;
        rb[k] = (double)c * (double)mu_c;
      }
    }
  }
  block_sum(rb, s_red);
  double mean_b = 0.0;
  for (int k = 0; k < K; ++k) mean_b += s_b[k];
  mean_b /= (double)K;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k)
    if (tid == k && k < K) a.intercept[(size_t)p * K + k] = (float)(s_b[k] - mean_b - rb[k]);
  if (tid == 0) {
    a.stats[(size_t)p * 2] = f;
    a.stats[(size_t)p * 2 + 1] = gnorm;
    info[0] = 0;
    info[1] = n_iter;
    info[2] = reason;
    info[3] = n;
  }
}

constexpr int kScoreThreads = 256;
constexpr int kScoreRows = kScoreThreads / 64;      // a wave per list entry

__global__ __launch_bounds__(kScoreThreads) void logreg_score_kernel(const float* __restrict__ x, int n_rows, int dim, const int32_t* __restrict__ rows,
                                                                    const int32_t* __restrict__ truth, const int32_t* __restrict__ offsets, int P, int K,
                                                                    const float* __restrict__ coef, const float* __restrict__ intercept, int total,
                                                                    int32_t* __restrict__ pred, float* __restrict__ probs, float* __restrict__ logits,
                                                                    int32_t* correct) {
  const int lane = threadIdx.x & 63;
  const long long e = (long long)blockIdx.x * kScoreRows + (threadIdx.x >> 6);
  if (e >= total) return;
  // the problem whose list holds entry e: the last p with offsets[p] <= e (at most 32 halvings)
  int lo = 0, hi = P + 1;
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int mid = (lo + hi) >> 1;
    if ((long long)offsets[mid] <= e)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int p = lo - 1;
  const int r = rows[e];
  if (p < 0 || p >= P || (unsigned)r >= (unsigned)n_rows) {          // outside every list, or outside the bank: never dereferenced
    if (lane == 0) pred[e] = -1;
    if (lane < K) {
      if (probs) probs[(size_t)e * K + lane] = __builtin_nanf("");
      if (logits) logits[(size_t)e * K + lane] = __builtin_nanf("");
    }
    return;
  }
  const float* __restrict__ xr = x + (size_t)r * dim;
  const float* __restrict__ wp = coef + (size_t)p * K * dim;
  float acc[kMaxK];
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) acc[k] = 0.0f;
  for (int c = lane; c < dim; c += 64) {
    const float v = xr[c];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) acc[k] = fmaf(wp[(size_t)k * dim + c], v, acc[k]);
  }
  float z[kMaxK], zmax = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    z[k] = -INFINITY;
    if (k < K) {
      z[k] = wave_sum(acc[k]) + intercept[(size_t)p * K + k];
      if (z[k] > zmax) {                                             // first argmax
        zmax = z[k];
        arg = k;
      }
    }
  }
  float ex[kMaxK], sum = 0.0f;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    ex[k] = k < K ? expf(z[k] - zmax) : 0.0f;
    sum += ex[k];
  }
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    if (k < K && lane == k) {
      if (probs) probs[(size_t)e * K + k] = ex[k] / sum;
      if (logits) logits[(size_t)e * K + k] = z[k];
    }
  }
  if (lane == 0) {
    pred[e] = arg;
    if (arg == truth[e]) atomicAdd(correct + p, 1);                  // an integer count
  }
}

// more than 64 KB of dynamic LDS: the limit is raised once per device and class count
template <int K>
int launch_fit(const FitArgs& a, int n_problems, hipStream_t stream) {
  static std::mutex mu;
  static std::set<int> done;
  int dev = 0;
  MKWS_HIP(hipGetDevice(&dev));
  {
    std::lock_guard<std::mutex> lk(mu);
    if (!done.count(dev)) {
      // (what the largest shape asks for, not the whole 160 KB: the kernel also has a little static LDS of the compiler's)
      MKWS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(logreg_fit_kernel<K>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)fit_lds_bytes(kMaxDim, K)));
      done.insert(dev);
    }
  }
  hipLaunchKernelGGL(logreg_fit_kernel<K>, dim3(n_problems), dim3(kThreads), fit_lds_bytes(a.dim, K), stream, a);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

int check_shape(int n_rows, int dim, int n_problems, int n_classes) {
  if (n_rows < 0 || n_problems < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (dim < 1) return fail(MKWS_ERR_INVALID_ARG, "dim = %d: at least one column", dim);
  if (n_classes < 2) return fail(MKWS_ERR_INVALID_ARG, "n_classes = %d: at least two classes", n_classes);
  if (n_classes > kMaxK) return fail(MKWS_ERR_UNSUPPORTED, "%d classes: at most %d", n_classes, kMaxK);
  if (dim > kMaxDim) return fail(MKWS_ERR_UNSUPPORTED, "dim = %d: at most %d", dim, kMaxDim);
  return MKWS_OK;
}

}  // namespace

extern "C" size_t mkws_logreg_work_floats(int dim, int n_problems, int n_classes) {
  if (dim < 1 || n_problems < 0 || n_classes < 1) return 0;
  return (size_t)3 * (size_t)n_problems * (size_t)n_classes * (size_t)dim;
}

extern "C" int mkws_logreg_fit(const float* d_x, int n_rows, int dim, const int32_t* d_rows, const int32_t* d_labels, const int32_t* d_offsets,
                               int n_problems, int n_classes, const double* d_C, int standardize, int max_iter, double gtol, float* d_coef,
                               float* d_intercept, int32_t* d_info, double* d_stats, float* d_work, size_t work_floats, void* stream) {
  if (int rc = check_shape(n_rows, dim, n_problems, n_classes)) return rc;
  if (max_iter < 1) return fail(MKWS_ERR_INVALID_ARG, "max_iter = %d: at least one iteration", max_iter);
  if (!(gtol >= 0.0)) return fail(MKWS_ERR_INVALID_ARG, "gtol is NaN or negative");
  if (standardize != 0 && standardize != 1) return fail(MKWS_ERR_INVALID_ARG, "standardize = %d: 0 or 1", standardize);
  if (n_problems == 0) return MKWS_OK;   // nothing to read or write: the buffers may be NULL
  if (!d_x || !d_rows || !d_labels || !d_offsets || !d_C || !d_coef || !d_intercept || !d_info || !d_stats || !d_work)
    return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (work_floats < mkws_logreg_work_floats(dim, n_problems, n_classes))
    return fail(MKWS_ERR_INVALID_ARG, "workspace of %zu floats: mkws_logreg_work_floats asks for %zu", work_floats,
                mkws_logreg_work_floats(dim, n_problems, n_classes));
  FitArgs a;
  a.x = d_x;
  a.rows = d_rows;
  a.labels = d_labels;
  a.offsets = d_offsets;
  a.C = d_C;
  a.coef = d_coef;
  a.intercept = d_intercept;
  a.info = d_info;
  a.stats = d_stats;
  a.work = d_work;
  a.n_rows = n_rows;
  a.dim = dim;
  a.standardize = standardize;
  a.max_iter = max_iter;
  a.gtol = gtol;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (n_classes) {
    case 2: return launch_fit<2>(a, n_problems, s);
    case 3: return launch_fit<3>(a, n_problems, s);
    case 4: return launch_fit<4>(a, n_problems, s);
    case 5: return launch_fit<5>(a, n_problems, s);
    case 6: return launch_fit<6>(a, n_problems, s);
    case 7: return launch_fit<7>(a, n_problems, s);
    default: return launch_fit<8>(a, n_problems, s);
  }
}

extern "C" int mkws_logreg_score(const float* d_x, int n_rows, int dim, const int32_t* d_rows, const int32_t* d_true, const int32_t* d_offsets,
                                 int n_problems, int n_classes, const float* d_coef, const float* d_intercept, int total, int32_t* d_pred,
                                 float* d_probs, float* d_logits, int32_t* d_correct, void* stream) {
  if (int rc = check_shape(n_rows, dim, n_problems, n_classes)) return rc;
  if (total < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (!d_offsets) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (n_problems > 0 && (!d_coef || !d_intercept || !d_correct)) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (total > 0 && (!d_x || !d_rows || !d_true || !d_pred)) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_problems > 0) MKWS_HIP(hipMemsetAsync(d_correct, 0, (size_t)n_problems * sizeof(int32_t), s));
  if (total == 0) return MKWS_OK;
  const unsigned blocks = (unsigned)(((long long)total + kScoreRows - 1) / kScoreRows);
  hipLaunchKernelGGL(logreg_score_kernel, dim3(blocks), dim3(kScoreThreads), 0, s, d_x, n_rows, dim, d_rows, d_true, d_offsets, n_problems, n_classes,
                     d_coef, d_intercept, total, d_pred, d_probs, d_logits, d_correct);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}
