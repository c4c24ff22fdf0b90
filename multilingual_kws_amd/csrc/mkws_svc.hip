// K RBF support-vector classifiers on embedding vectors (mkws_svc_prepare / mkws_svc_kernel / mkws_svc_fit / mkws_svc_score, and for
// probability=True mkws_svc_fit_cv / mkws_svc_platt / mkws_svc_couple, with mkws_soft_vote; include/mkws.h): what the DataPerf selection
// harness does per split with sklearn.svm.SVC(), for P problems side by side.  multilingual_kws_amd/svc.py (svc_host, decision_host,
// predict_host; cv_decision_host, platt_host, couple_host, soft_vote_host) is the specification.
//
// prepare  one workgroup per problem: the lists are checked, the column mean and 1 / sigma of the problem's own rows and sklearn's
//          gamma = 1 / (dim * Var) are formed with float64 accumulation, a thread per column, the rows in list order.
// kernel   out[a, b] = float32(exp(-gamma * max(0, s_a + s_b - 2 a~.b~))) for two gathered row lists: a 64 x 64 tile per workgroup, a~.b~
//          on the 16x16x4 fp32 matrix instruction (16 columns per float32 chain, the chains added in float64), the operands staged
//          through LDS from the gathered rows with centring and scaling applied in the load, the squared norms s summed from the same
//          loaded values.  rbf_tile is the one piece of device code behind the Gram matrices (A = B = a problem's rows) and the
//          scorer (A = training rows, B = evaluation rows).
// fit      one workgroup per (problem, pair of classes): libsvm's SMO (second-order working-set selection, no shrinking) on the pair's
//          rows of the problem's Gram matrix, its sub-matrix in LDS up to kCacheRows rows and read from the (L2-resident) workspace
//          above.  The gradient and alpha are float64 as in libsvm; the kernel values are float32 as in libsvm's cache.  Both selections
//          are wave butterflies plus one LDS exchange; an iteration is three barriers.
// score    a workgroup per 64 evaluation rows walks the model's training rows tile by tile, sums coef * k per (class, other class) in
//          list order and votes.
// fit_cv   one workgroup per (problem, pair, fold): the fit's solver with that fold's entries of the pair held out (the box [0, 0]);
//          their decision values are what is written.  fit and fit_cv are the two instantiations of one solver, smo_pair<HELD>: without
//          held-out entries no flag is read.
// platt    one wave per (problem, pair): Newton's iteration with backtracking on the sigmoid's (A, B) over the pair's fit_cv values,
//          float64, every pass's sums by one butterfly.
// couple   a thread per evaluation entry: pairwise probabilities from the sigmoids, coupled by a Cholesky solve in registers (templated
//          on the class count), the first argmax.
// soft_vote  a thread per evaluation entry: the mean of two probability rows and its first argmax.
// No floating-point atomics (the integer ones count, or take a maximum): two calls on the same input write the same bytes.  Every loop is
// bounded by max_iter, the row count, dim or the class count; no workgroup waits for another.
#include "mkws_common.h"

#include <cmath>
#include <cstdint>
#include <mutex>
#include <set>

using mkws::fail;

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kMaxRows = MKWS_SVC_MAX_ROWS;
constexpr int kMaxK = MKWS_SVC_MAX_CLASSES;
constexpr int kMaxDim = MKWS_SVC_MAX_DIM;
constexpr int kTile = 64;               // rows of either list in one kernel tile
constexpr int kTileThreads = 256;       // 2 x 2 waves, each 2 x 2 matrix-instruction tiles
constexpr int kPrepThreads = 1024;
constexpr int kFitThreads = 256;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kCacheRows = 128;         // a pair of up to this many rows keeps its sub-matrix in LDS (64 KB)
constexpr double kTau = 1e-12;
static_assert(kMaxDim == kPrepThreads, "a column per thread in mkws_svc_prepare");
static_assert(kMaxK == 8, "the class loops are unrolled over 8");

// ------------------------------------------------------------------------------------------------ the kernel tile

struct TileLds {
  float a[2][kTile][17];                // two stages of [row][k], padded
  float b[2][kTile][17];
  double na[kTile], nb[kTile];          // squared norms of the centred and scaled rows
  int32_t ra[kTile], rb[kTile];         // bank rows, -1 = no row (past the list or outside the bank): its operand is zero
};

// acc = A~ B~^T for the 64 + 64 rows named in s.ra / s.rb (filled by the caller; this function makes them visible), s.na / s.nb their
// squared norms.  Wave (wm, wn) holds rows wm * 32 + i * 16 + 4 * (lane >> 4) + r of A against rows wn * 32 + j * 16 + (lane & 15) of
// B in acc[i][j][r].  The matrix instruction's float32 chain runs over 16 columns at a time and its result is added to a float64 total,
// the norms are float64 sums of the exact squares: where the classifier it replaces is exact (every alpha at its bound, or a handful
// of rows) the device is held to the float32 storage of the optimum, and a 1024-term float32 chain alone would spend that.
// Ends with a barrier: the caller may read s.na / s.nb at once.
__device__ inline void rbf_tile(const float* __restrict__ x, int dim, const float* __restrict__ centre, const float* __restrict__ inv, TileLds& s,
                                double (&acc)[2][2][4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = tid >> 4, kk = tid & 15;             // this thread loads rows lr + 16 i, column k0 + kk
  __syncthreads();
  const float* pa[4];
  const float* pb[4];
  float va[4], vb[4];
  double sa[4], sb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ra = s.ra[lr + 16 * i], rb = s.rb[lr + 16 * i];
    pa[i] = ra >= 0 ? x + (size_t)ra * dim : nullptr;
    pb[i] = rb >= 0 ? x + (size_t)rb * dim : nullptr;
    sa[i] = sb[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
  auto fetch = [&](int k0) {
    const int k = k0 + kk;
    const bool in = k < dim;
    const float c = in ? centre[k] : 0.0f, sc = in ? inv[k] : 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      va[i] = (in && pa[i]) ? (pa[i][k] - c) * sc : 0.0f;
      vb[i] = (in && pb[i]) ? (pb[i][k] - c) * sc : 0.0f;
      sa[i] += (double)va[i] * (double)va[i];
      sb[i] += (double)vb[i] * (double)vb[i];
    }
  };
  auto stash = [&](int st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s.a[st][lr + 16 * i][kk] = va[i];
      s.b[st][lr + 16 * i][kk] = vb[i];
    }
  };
  fetch(0);
  stash(0);
  __syncthreads();
  int st = 0;
  for (int k0 = 0; k0 < dim; k0 += 16) {
    const bool more = k0 + 16 < dim;
    if (more) fetch(k0 + 16);                          // the next step's operands travel while this step multiplies
    f32x4 part[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) part[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 16; ks += 4) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = s.a[st][wm * 32 + i * 16 + (lane & 15)][ks + (lane >> 4)];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = s.b[st][wn * 32 + j * 16 + (lane & 15)][ks + (lane >> 4)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) part[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], part[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] += (double)part[i][j][r];
    if (more) stash(st ^ 1);
    __syncthreads();
    st ^= 1;
  }
  // the 16 threads of a row (they differ in the low four lane bits) add their column sums in a fixed butterfly
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
      sa[i] += __shfl_xor(sa[i], m, 64);
      sb[i] += __shfl_xor(sb[i], m, 64);
    }
    if (kk == 0) {
      s.na[lr + 16 * i] = sa[i];
      s.nb[lr + 16 * i] = sb[i];
    }
  }
  __syncthreads();
}

// the distance and the exponential in float64 (exp of the device library), rounded once to float32
__device__ inline float rbf_value(const TileLds& s, int arow, int brow, double dot, float gamma) {
  if (s.ra[arow] < 0 || s.rb[brow] < 0) return __builtin_nanf("");
  const double d2 = fmax(0.0, (s.na[arow] + s.nb[brow]) - 2.0 * dot);
  return (float)exp(-(double)gamma * d2);
}

__device__ inline int32_t bank_row(const int32_t* __restrict__ rows, int begin, int idx, int n, int n_rows) {
  if (idx >= n) return -1;
  const int32_t r = rows[(size_t)begin + idx];
  return (unsigned)r < (unsigned)n_rows ? r : -1;
}

__global__ __launch_bounds__(kTileThreads) void svc_kernel_kernel(const float* __restrict__ x, int n_rows, int dim, const int32_t* __restrict__ rows_a,
                                                                  const int32_t* __restrict__ off_a, int max_a, const int32_t* __restrict__ rows_b,
                                                                  const int32_t* __restrict__ off_b, int max_b, int tiles_a, int tiles_b,
                                                                  const float* __restrict__ centre, const float* __restrict__ inv,
                                                                  const float* __restrict__ gamma, const int32_t* __restrict__ info,
                                                                  float* __restrict__ out, size_t out_stride) {
  __shared__ TileLds s;
  const int per = tiles_a * tiles_b;
  const int p = blockIdx.x / per, rem = blockIdx.x % per;
  const int ta = rem / tiles_b, tb = rem % tiles_b;
  if (info && info[(size_t)p * 4] != 0) return;
  const int a0 = off_a[p], na = off_a[p + 1] - a0, b0 = off_b[p], nb = off_b[p + 1] - b0;
  if (na < 1 || nb < 1 || na > max_a || nb > max_b || (size_t)na * (size_t)nb > out_stride) return;
  if (ta * kTile >= na || tb * kTile >= nb) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < kTile)
    s.ra[tid] = bank_row(rows_a, a0, ta * kTile + tid, na, n_rows);
  else if (tid < 2 * kTile)
    s.rb[tid - kTile] = bank_row(rows_b, b0, tb * kTile + tid - kTile, nb, n_rows);
  double acc[2][2][4];
  rbf_tile(x, dim, centre + (size_t)p * dim, inv + (size_t)p * dim, s, acc);
  const float g = gamma[p];
  float* __restrict__ o = out + (size_t)p * out_stride;
  const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int arow = wm * 32 + i * 16 + 4 * (lane >> 4) + r, brow = wn * 32 + j * 16 + (lane & 15);
        const int ga = ta * kTile + arow, gb = tb * kTile + brow;
        if (ga < na && gb < nb) o[(size_t)ga * nb + gb] = rbf_value(s, arow, brow, acc[i][j][r], g);
      }
}

// ------------------------------------------------------------------------------------------------ prepare

// every thread gets the same sum: wave butterflies, then the wave sums in wave order; two barriers
__device__ inline double prep_block_sum(double v, double* s_red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kPrepThreads / 64; ++w) t += s_red[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(kPrepThreads) void svc_prepare_kernel(const float* __restrict__ x, int n_rows, int dim, const int32_t* __restrict__ rows,
                                                                   const int32_t* __restrict__ labels, const int32_t* __restrict__ offsets, int K,
                                                                   int max_rows, int standardize, double gamma_arg, float* __restrict__ centre,
                                                                   float* __restrict__ inv, float* __restrict__ gamma, int32_t* __restrict__ info,
                                                                   float* __restrict__ gap) {
  __shared__ int32_t s_rows[kMaxRows];
  __shared__ int s_cnt[kMaxK];
  __shared__ double s_red[kPrepThreads / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int begin = offsets[p];
  const int n = offsets[p + 1] - begin;
  int32_t* __restrict__ pinfo = info + (size_t)p * 4;
  if (n < 1 || n > max_rows || n > kMaxRows) {                        // nothing of the problem is touched
    if (tid < 4) pinfo[tid] = tid == 0 ? 2 : 0;
    return;
  }
  if (tid < kMaxK) s_cnt[tid] = 0;
  __syncthreads();
  int bad = 0;
  if (tid < n) {
    const int r = rows[(size_t)begin + tid], y = labels[(size_t)begin + tid];
    bad = (unsigned)r >= (unsigned)n_rows || (unsigned)y >= (unsigned)K;
    s_rows[tid] = r;
    if (!bad) atomicAdd(&s_cnt[y], 1);                                // (an integer count in LDS)
  }
  bad = __syncthreads_or(bad);
  int present = 0;
  for (int k = 0; k < K; ++k) present += s_cnt[k] > 0;
  if (bad || present < 2) {
    if (tid < 4) pinfo[tid] = tid == 0 ? 2 : 0;
    return;
  }
  // a thread per column, the rows added in list order in float64
  double cm = 0.0, term = 0.0, ssd = 0.0, inv_d = 1.0;
  if (tid < dim) {
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += (double)x[(size_t)s_rows[i] * dim + tid];
    const double mean = sum / (double)n;
    for (int i = 0; i < n; ++i) {
      const double d = (double)x[(size_t)s_rows[i] * dim + tid] - mean;
      ssd += d * d;
    }
    if (standardize) {
      const double sigma = sqrt(ssd / (double)n);
      inv_d = sigma == 0.0 ? 1.0 : 1.0 / sigma;
    }
    centre[(size_t)p * dim + tid] = (float)mean;
    inv[(size_t)p * dim + tid] = (float)inv_d;
    cm = standardize ? 0.0 : mean;                                    // the column's mean in the matrix the kernel sees
  }
  double g = gamma_arg;
  if (!(g > 0.0)) {
    // Var over all n * dim entries = [sum_j ssd_j / sigma_j^2 + n sum_j (mean_j - grand mean)^2] / (n dim)
    const double grand = prep_block_sum(cm, s_red) / (double)dim;
    if (tid < dim) term = ssd * inv_d * inv_d + (double)n * (cm - grand) * (cm - grand);
    const double var = prep_block_sum(term, s_red) / ((double)n * (double)dim);
    g = var > 0.0 ? 1.0 / ((double)dim * var) : 1.0;
  }
  if (tid == 0) {
    gamma[p] = (float)g;
    gap[p] = 0.0f;
    pinfo[0] = 0;
    pinfo[1] = present * (present - 1) / 2;
    pinfo[2] = 0;
    pinfo[3] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ fit (SMO)

constexpr size_t kFitLdsFixed = (size_t)kMaxRows * (8 + 8 + 4 + 4 + 4);                 // G, alpha, idx, idx of class j, diagonal
constexpr size_t kFitLdsBytes = kFitLdsFixed + (size_t)kCacheRows * kCacheRows * 4;
static_assert(kFitLdsBytes <= 160 * 1024 - 4096, "LDS");

struct FitArgs {
  const int32_t* labels;
  const int32_t* offsets;
  const double* C;
  const float* gram;
  size_t gram_stride;
  float* coef;
  float* rho;
  int32_t* info;
  float* gap;
  int K, max_rows, max_iter;
  double tol;
};

// pair q = (ci, cj) in the order (0,1), (0,2), ...
__device__ inline void pair_of(int q, int K, int& ci, int& cj) {
  int rest = q;
  ci = 0;
  for (int k = 0; k < kMaxK && rest >= K - 1 - ci; ++k) {
    rest -= K - 1 - ci;
    ++ci;
  }
  cj = ci + 1 + rest;
}

// the dynamic LDS of one pair's workgroup (kFitLdsFixed, then the cache)
struct PairLds {
  double* G;                            // the gradient
  double* alpha;
  int32_t* idx;                         // the pair's entries as positions in the problem's list: class i, then class j
  int32_t* idxJ;                        // class j's entries while list_pair appends them; smo_pair<true>'s held-out flags after that
  float* Kd;                            // the diagonal
  float* K;                             // [m, m] when m <= kCacheRows
};

__device__ inline PairLds pair_lds(char* raw) {
  PairLds lds;
  lds.G = reinterpret_cast<double*>(raw);
  lds.alpha = lds.G + kMaxRows;
  lds.idx = reinterpret_cast<int32_t*>(lds.alpha + kMaxRows);
  lds.idxJ = lds.idx + kMaxRows;
  lds.Kd = reinterpret_cast<float*>(lds.idxJ + kMaxRows);
  lds.K = lds.Kd + kMaxRows;
  return lds;
}

// lds.idx = the list positions of class ci's entries, then class cj's, each in list order; mi = class ci's count, -> the pair's.
// Two barriers, the second at the end.
__device__ inline int list_pair(const int32_t* __restrict__ lab, int n, int ci, int cj, const PairLds& lds, int& mi) {
  __shared__ int s_cnt[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (wave < 2) {                                                     // wave 0 lists class ci, wave 1 class cj
    const int cls = wave == 0 ? ci : cj;
    int32_t* dst = wave == 0 ? lds.idx : lds.idxJ;
    int cnt = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
      const int t = c0 + lane;
      const bool is = t < n && lab[t] == cls;
      const unsigned long long mask = __ballot(is);
      if (is) dst[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = t;
      cnt += __popcll(mask);
    }
    if (lane == 0) s_cnt[wave] = cnt;
  }
  __syncthreads();
  mi = s_cnt[0];
  const int mj = s_cnt[1];
  for (int t = tid; t < mj; t += kFitThreads) lds.idx[mi + t] = lds.idxJ[t];
  __syncthreads();
  return mi + mj;
}

struct PairFit {
  int it, cut;                          // iterations taken; 1 = stopped by max_iter
  double gap, rho;                      // the last m(a) - M(a); libsvm's rho
};

// libsvm's SMO on the m entries list_pair left in lds.idx (the first mi are the +1 class), on problem rows of the n x n matrix gram, and
// libsvm's rho: the one solver behind svc_fit_kernel (HELD = false) and svc_fit_cv_kernel (HELD = true).  With HELD the entries flagged
// in lds.idxJ get the box [0, 0], which the selection rules never pick, so nothing is compacted and the gradient kept for EVERY entry
// is a held-out entry's decision value: f(x_t) = y_t (G_t + 1) - rho; rho's rule skips them.  Without HELD no flag is read.
// each(t, t is of the +1 class, alpha_t) is called once per training entry, by thread t % kFitThreads, before rho's reduction (its
// stores travel meanwhile).  Every thread returns the same values.  Entry t's G and alpha are written by that thread alone: it may
// read them after the call without a barrier.
template <bool HELD, class Each>
__device__ inline PairFit smo_pair(const PairLds& lds, const float* __restrict__ gram, int n, int mi, int m, double C, double tol, int max_iter,
                                   Each each) {
  __shared__ double s_exv[kFitWaves], s_exm[kFitWaves], s_exo[kFitWaves], s_red[4][kFitWaves];
  __shared__ int s_exi[kFitWaves], s_exj[kFitWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* s_out = lds.idxJ;                                    // 1 = held out
  const bool cached = m <= kCacheRows;
  if (cached)
    for (int e = tid; e < m * m; e += kFitThreads) lds.K[e] = gram[(size_t)lds.idx[e / m] * n + lds.idx[e % m]];
  for (int t = tid; t < m; t += kFitThreads) {
    lds.Kd[t] = gram[(size_t)lds.idx[t] * n + lds.idx[t]];
    lds.G[t] = -1.0;
    lds.alpha[t] = 0.0;
  }
  __syncthreads();
  auto kval = [&](int r, int t) -> double { return (double)(cached ? lds.K[r * m + t] : gram[(size_t)lds.idx[r] * n + lds.idx[t]]); };
  const double inf = __builtin_inf();

  int it = 0, cut = 0;
  double gapv = 0.0;
  for (;; ++it) {
    // ---- i = argmax over I_up of -y G (the later index on ties), M = min over I_low ----
    double bv = -inf, mn = inf;
    int bi = -1;
    for (int t = tid; t < m; t += kFitThreads) {
      const bool pos = t < mi;
      const double Ct = (HELD && s_out[t]) ? 0.0 : C;
      const double al = lds.alpha[t], v = pos ? -lds.G[t] : lds.G[t];
      const bool up = pos ? al < Ct : al > 0.0, low = pos ? al > 0.0 : al < Ct;
      if (up && v >= bv) {
        bv = v;
        bi = t;
      }
      if (low) mn = fmin(mn, v);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const double ov = __shfl_xor(bv, s, 64);
      const int oi = __shfl_xor(bi, s, 64);
      if (ov > bv || (ov == bv && oi > bi)) {
        bv = ov;
        bi = oi;
      }
      mn = fmin(mn, __shfl_xor(mn, s, 64));
    }
    if (lane == 0) {
      s_exv[wave] = bv;
      s_exi[wave] = bi;
      s_exm[wave] = mn;
    }
    __syncthreads();
    bv = s_exv[0], bi = s_exi[0], mn = s_exm[0];
#pragma unroll
    for (int w = 1; w < kFitWaves; ++w) {
      if (s_exv[w] > bv || (s_exv[w] == bv && s_exi[w] > bi)) {
        bv = s_exv[w];
        bi = s_exi[w];
      }
      mn = fmin(mn, s_exm[w]);
    }
    const int i = bi;
    const double gmax = bv;
    gapv = gmax - mn;
    if (i < 0 || !(gapv >= tol)) break;                               // converged (or nothing can move)
    if (it >= max_iter) {
      cut = 1;
      break;
    }
    // ---- j = argmin over I_low with -y G < gmax of -(gmax + y G)^2 / (K_ii + K_tt - 2 K_it) ----
    const double kdi = (double)lds.Kd[i];
    double bo = inf;
    int bj = -1;
    for (int t = tid; t < m; t += kFitThreads) {
      const bool pos = t < mi;
      const double Ct = (HELD && s_out[t]) ? 0.0 : C;
      const double al = lds.alpha[t], v = pos ? -lds.G[t] : lds.G[t];
      const bool low = pos ? al > 0.0 : al < Ct;
      const double gd = gmax - v;
      if (low && gd > 0.0) {
        double quad = kdi + (double)lds.Kd[t] - 2.0 * kval(i, t);
        if (!(quad > 0.0)) quad = kTau;
        const double o = -(gd * gd) / quad;
        if (o <= bo) {
          bo = o;
          bj = t;
        }
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const double oo = __shfl_xor(bo, s, 64);
      const int oj = __shfl_xor(bj, s, 64);
      if (oo < bo || (oo == bo && oj > bj)) {
        bo = oo;
        bj = oj;
      }
    }
    if (lane == 0) {
      s_exo[wave] = bo;
      s_exj[wave] = bj;
    }
    __syncthreads();
    bo = s_exo[0], bj = s_exj[0];
#pragma unroll
    for (int w = 1; w < kFitWaves; ++w) {
      if (s_exo[w] < bo || (s_exo[w] == bo && s_exj[w] > bj)) {
        bo = s_exo[w];
        bj = s_exj[w];
      }
    }
    const int j = bj;
    if (j < 0) break;
    // ---- the two-variable step with libsvm's clipping; every thread computes it (i and j are never held out: their box is [0, C]) ----
    const double yi = i < mi ? 1.0 : -1.0, yj = j < mi ? 1.0 : -1.0;
    const double ai = lds.alpha[i], aj = lds.alpha[j], Gi = lds.G[i], Gj = lds.G[j];
    double quad = kdi + (double)lds.Kd[j] - 2.0 * kval(i, j);
    if (!(quad > 0.0)) quad = kTau;
    double ni, nj;
    if (yi != yj) {
      const double delta = (-Gi - Gj) / quad, diff = ai - aj;
      ni = ai + delta;
      nj = aj + delta;
      if (diff > 0.0) {
        if (nj < 0.0) {
          nj = 0.0;
          ni = diff;
        }
      } else if (ni < 0.0) {
        ni = 0.0;
        nj = -diff;
      }
      if (diff > 0.0) {
        if (ni > C) {
          ni = C;
          nj = C - diff;
        }
      } else if (nj > C) {
        nj = C;
        ni = C + diff;
      }
    } else {
      const double delta = (Gi - Gj) / quad, tot = ai + aj;
      ni = ai - delta;
      nj = aj + delta;
      if (tot > C) {
        if (ni > C) {
          ni = C;
          nj = tot - C;
        }
      } else if (nj < 0.0) {
        nj = 0.0;
        ni = tot;
      }
      if (tot > C) {
        if (nj > C) {
          nj = C;
          ni = tot - C;
        }
      } else if (ni < 0.0) {
        ni = 0.0;
        nj = tot;
      }
    }
    __syncthreads();                                                  // every thread has read alpha and G of i and j
    const double dai = ni - ai, daj = nj - aj;
    for (int t = tid; t < m; t += kFitThreads) {                      // (the held-out entries too: their G is what is asked for)
      const double yt = t < mi ? 1.0 : -1.0;
      lds.G[t] += yt * (yi * kval(i, t) * dai + yj * kval(j, t) * daj);
    }
    if (tid == (i & (kFitThreads - 1))) lds.alpha[i] = ni;            // (by the thread that owns the entry)
    if (tid == (j & (kFitThreads - 1))) lds.alpha[j] = nj;
  }

  // ---- rho by libsvm's rule over the training entries, each handed to the caller on the way ----
  double sum = 0.0, cnt = 0.0, ub = inf, lb = -inf;
  for (int t = tid; t < m; t += kFitThreads) {
    if (HELD && s_out[t]) continue;
    const bool pos = t < mi;
    const double al = lds.alpha[t], yG = pos ? lds.G[t] : -lds.G[t];
    const bool upper = al >= C, lower = al <= 0.0;
    if (!upper && !lower) {
      sum += yG;
      cnt += 1.0;
    } else if ((upper && !pos) || (lower && pos)) {
      ub = fmin(ub, yG);
    } else {
      lb = fmax(lb, yG);
    }
    each(t, pos, al);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    sum += __shfl_xor(sum, s, 64);
    cnt += __shfl_xor(cnt, s, 64);
    ub = fmin(ub, __shfl_xor(ub, s, 64));
    lb = fmax(lb, __shfl_xor(lb, s, 64));
  }
  if (lane == 0) {
    s_red[0][wave] = sum;
    s_red[1][wave] = cnt;
    s_red[2][wave] = ub;
    s_red[3][wave] = lb;
  }
  __syncthreads();
  sum = s_red[0][0], cnt = s_red[1][0], ub = s_red[2][0], lb = s_red[3][0];
  for (int w = 1; w < kFitWaves; ++w) {
    sum += s_red[0][w];
    cnt += s_red[1][w];
    ub = fmin(ub, s_red[2][w]);
    lb = fmax(lb, s_red[3][w]);
  }
  return {it, cut, gapv, cnt > 0.0 ? sum / cnt : (ub + lb) / 2.0};
}

__global__ __launch_bounds__(kFitThreads) void svc_fit_kernel(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char s_raw[];
  const PairLds lds = pair_lds(s_raw);
  const int K = a.K, npairs = K * (K - 1) / 2;
  const int p = blockIdx.x / npairs, q = blockIdx.x % npairs;
  const int tid = threadIdx.x;
  int32_t* __restrict__ pinfo = a.info + (size_t)p * 4;
  if (pinfo[0] != 0) return;                                          // refused by mkws_svc_prepare: nothing is written
  const int begin = a.offsets[p];
  const int n = a.offsets[p + 1] - begin;
  if (n < 1 || n > a.max_rows || n > kMaxRows) return;
  int ci, cj, mi;
  pair_of(q, K, ci, cj);
  const int m = list_pair(a.labels + begin, n, ci, cj, lds, mi);
  float* __restrict__ coef = a.coef + (size_t)begin * (K - 1);
  if (mi == 0 || mi == m) {                                           // a class without a row: zero coefficients, rho = 0
    for (int t = tid; t < m; t += kFitThreads) coef[(size_t)lds.idx[t] * (K - 1) + (mi ? cj - 1 : ci)] = 0.0f;
    if (tid == 0) a.rho[(size_t)p * npairs + q] = 0.0f;
    return;
  }
  const PairFit f = smo_pair<false>(lds, a.gram + (size_t)p * a.gram_stride, n, mi, m, a.C[p], a.tol, a.max_iter, [&](int t, bool pos, double al) {
    coef[(size_t)lds.idx[t] * (K - 1) + (pos ? cj - 1 : ci)] = (float)(pos ? al : -al);     // the coefficients in the row list's order
  });
  if (tid == 0) {
    a.rho[(size_t)p * npairs + q] = (float)f.rho;
    if (f.cut) atomicAdd(pinfo + 2, 1);                               // integer atomics: their order does not show
    atomicMax(pinfo + 3, f.it);
    atomicMax(reinterpret_cast<int*>(a.gap + p), __float_as_int(fmaxf((float)f.gap, 0.0f)));   // (non-negative floats order as their bits)
  }
}

// ------------------------------------------------------------------------------------------------ score

struct ScoreArgs {
  const float* x;
  const int32_t* train_rows;
  const int32_t* train_labels;
  const int32_t* train_offsets;
  const float* coef;
  const float* rho;
  const float* gamma;
  const float* centre;
  const float* inv;
  const int32_t* info;
  const int32_t* rows;
  const int32_t* truth;
  const int32_t* offsets;
  int32_t* pred;
  int32_t* correct;
  float* decision;
  int n_rows, dim, K, max_train, max_eval, tiles_e;
};

constexpr int kSlots = kMaxK * (kMaxK - 1);            // (class, other class) sums per evaluation row

__global__ __launch_bounds__(kTileThreads) void svc_score_kernel(ScoreArgs a) {
  __shared__ TileLds s;
  __shared__ float s_kt[kTile][kTile + 1];             // [training row][evaluation row] kernel values of the tile
  __shared__ float s_S[kTile][kSlots + 1];             // [evaluation row][class * (K - 1) + slot]
  __shared__ float s_coef[kTile][kMaxK - 1];
  __shared__ int32_t s_lab[kTile];
  __shared__ int s_present[kMaxK];
  const int K = a.K, npairs = K * (K - 1) / 2, dim = a.dim;
  const int p = blockIdx.x / a.tiles_e, te = blockIdx.x % a.tiles_e;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e0 = a.offsets[p], ne = a.offsets[p + 1] - e0;
  if (ne > a.max_eval || te * kTile >= ne) return;
  if (a.info && a.info[(size_t)p * 4] != 0) return;                   // a refused model: pred stays -1
  const int t0 = a.train_offsets[p], nt = a.train_offsets[p + 1] - t0;
  if (nt < 1 || nt > a.max_train || nt > kMaxRows) return;
  if (tid < kMaxK) s_present[tid] = 0;
  for (int e = tid; e < kTile * (kSlots + 1); e += kTileThreads) (&s_S[0][0])[e] = 0.0f;
  __syncthreads();
  for (int t = tid; t < nt; t += kTileThreads) {
    const int y = a.train_labels[(size_t)t0 + t];
    if ((unsigned)y < (unsigned)K) s_present[y] = 1;                  // (every writer writes the same value)
  }
  const float g = a.gamma[p];
  const int wm = wave >> 1, wn = wave & 1;
  const int ev = tid & 63, sl = tid >> 6;                             // the accumulation: evaluation row ev, slots sl and sl + 4
  for (int tt = 0; tt * kTile < nt; ++tt) {
    if (tid < kTile) {
      const int idx = tt * kTile + tid;
      s.ra[tid] = bank_row(a.train_rows, t0, idx, nt, a.n_rows);
      s_lab[tid] = idx < nt ? a.train_labels[(size_t)t0 + idx] : -1;
      for (int k = 0; k < kMaxK - 1; ++k) s_coef[tid][k] = (idx < nt && k < K - 1) ? a.coef[((size_t)t0 + idx) * (K - 1) + k] : 0.0f;
    } else if (tid < 2 * kTile) {
      s.rb[tid - kTile] = bank_row(a.rows, e0, te * kTile + tid - kTile, ne, a.n_rows);
    }
    double acc[2][2][4];
    rbf_tile(a.x, dim, a.centre + (size_t)p * dim, a.inv + (size_t)p * dim, s, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int arow = wm * 32 + i * 16 + 4 * (lane >> 4) + r, brow = wn * 32 + j * 16 + (lane & 15);
          s_kt[arow][brow] = (s.ra[arow] >= 0 && s.rb[brow] >= 0) ? rbf_value(s, arow, brow, acc[i][j][r], g) : 0.0f;
        }
    __syncthreads();
    const int rows_here = min(kTile, nt - tt * kTile);
    for (int t = 0; t < rows_here; ++t) {                              // the training rows in list order
      const int y = s_lab[t];
      if ((unsigned)y >= (unsigned)K) continue;
      const float kv = s_kt[t][ev];
      if (sl < K - 1) s_S[ev][y * (K - 1) + sl] = fmaf(s_coef[t][sl], kv, s_S[ev][y * (K - 1) + sl]);
      if (sl + 4 < K - 1) s_S[ev][y * (K - 1) + sl + 4] = fmaf(s_coef[t][sl + 4], kv, s_S[ev][y * (K - 1) + sl + 4]);
    }
    __syncthreads();                                                  // before the next tile overwrites the lists and s_kt
  }
  const int idx = te * kTile + tid;
  if (tid >= kTile || idx >= ne) return;
  if (bank_row(a.rows, e0, idx, ne, a.n_rows) < 0) return;            // a row outside the bank: pred stays -1, its decision values NaN
  int votes[kMaxK];
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) votes[k] = 0;
  int qd = 0;
#pragma unroll
  for (int i = 0; i < kMaxK; ++i)
#pragma unroll
    for (int j = i + 1; j < kMaxK; ++j) {
      if (j < K) {
        float f = 0.0f;
        if (s_present[i] && s_present[j]) {
          f = (s_S[tid][i * (K - 1) + (j - 1)] + s_S[tid][j * (K - 1) + i]) - a.rho[(size_t)p * npairs + qd];
          if (f > 0.0f)
            ++votes[i];
          else
            ++votes[j];
        }
        if (a.decision) a.decision[((size_t)e0 + idx) * npairs + qd] = f;
        ++qd;
      }
    }
  int best = -1, arg = -1;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k)
    if (k < K && s_present[k] && votes[k] > best) {                   // the lowest class on ties
      best = votes[k];
      arg = k;
    }
  a.pred[(size_t)e0 + idx] = arg;
  if (arg == a.truth[(size_t)e0 + idx]) atomicAdd(a.correct + p, 1);  // an integer count
}

// ------------------------------------------------------------------------------------------------ probability=True: cross-validated fit

struct FitCvArgs {
  const int32_t* labels;
  const int32_t* offsets;
  const int32_t* folds;
  const double* C;
  const float* gram;
  size_t gram_stride;
  const int32_t* info;
  float* cv_decision;
  int32_t* cv_info;
  int K, F, max_rows, max_iter;
  double tol;
};

// smo_pair<true> for one (problem, pair, fold): the pair's entries of that fold are held out, and nothing but their decision values
// is written.  The same LDS as the fit: the held-out flags take the list of class j's entries once that has been appended to class i's.
__global__ __launch_bounds__(kFitThreads) void svc_fit_cv_kernel(FitCvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char s_raw[];
  const PairLds lds = pair_lds(s_raw);
  __shared__ int s_act[3];

  const int K = a.K, F = a.F, npairs = K * (K - 1) / 2;
  const int p = blockIdx.x / (npairs * F), q = (blockIdx.x / F) % npairs, fold = blockIdx.x % F;
  const int tid = threadIdx.x, lane = tid & 63;
  int32_t* __restrict__ cinfo = a.cv_info + (size_t)p * 4;
  const bool first = q == 0 && fold == 0;
  const int begin = a.offsets[p];
  const int n = a.offsets[p + 1] - begin;
  if (a.info[(size_t)p * 4] != 0 || n < 1 || n > a.max_rows || n > kMaxRows) {      // refused by mkws_svc_prepare
    if (first && tid == 0) cinfo[0] = 2;
    return;
  }
  const int32_t* __restrict__ lab = a.labels + begin;
  const int32_t* __restrict__ fo = a.folds + begin;
  int bad = 0;
  for (int t = tid; t < n; t += kFitThreads) bad |= (unsigned)fo[t] >= (unsigned)F;
  if (__syncthreads_or(bad)) {                                        // every workgroup of the problem sees it: nothing else is written
    if (first && tid == 0) cinfo[0] = 2;
    return;
  }
  int ci, cj, mi;
  pair_of(q, K, ci, cj);
  if (tid < 3) s_act[tid] = 0;
  const int m = list_pair(lab, n, ci, cj, lds, mi), mj = m - mi;
  int32_t* s_out = lds.idxJ;                                          // 1 = held out
  {
    int ni = 0, nj = 0, no = 0;                                       // training entries of either class, held-out entries
    for (int t = tid; t < m; t += kFitThreads) {
      const int out = fo[lds.idx[t]] == fold;
      s_out[t] = out;
      no += out;
      if (!out) (t < mi ? ni : nj) += 1;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      ni += __shfl_xor(ni, s, 64);
      nj += __shfl_xor(nj, s, 64);
      no += __shfl_xor(no, s, 64);
    }
    if (lane == 0) {                                                  // (integer counts in LDS)
      atomicAdd(&s_act[0], ni);
      atomicAdd(&s_act[1], nj);
      atomicAdd(&s_act[2], no);
    }
  }
  __syncthreads();
  const int act_i = s_act[0], act_j = s_act[1];
  if (s_act[2] == 0) return;                                          // the fold holds no entry of the pair
  float* __restrict__ dec = a.cv_decision + (size_t)begin * (K - 1);
  auto slot = [&](int t) -> size_t { return (size_t)lds.idx[t] * (K - 1) + (t < mi ? cj - 1 : ci); };
  if (act_i == 0 || act_j == 0) {
    // a class absent from the problem: 0; libsvm's svm_binary_svc_probability otherwise: 0 without any training entry, +1 with class i's
    // alone, -1 with class j's alone
    const float v = (mi == 0 || mj == 0 || act_i == act_j) ? 0.0f : act_i ? 1.0f : -1.0f;
    for (int t = tid; t < m; t += kFitThreads)
      if (s_out[t]) dec[slot(t)] = v;
    return;
  }
  const PairFit f = smo_pair<true>(lds, a.gram + (size_t)p * a.gram_stride, n, mi, m, a.C[p], a.tol, a.max_iter, [](int, bool, double) {});
  for (int t = tid; t < m; t += kFitThreads)
    if (s_out[t]) dec[slot(t)] = (float)((t < mi ? lds.G[t] + 1.0 : -(lds.G[t] + 1.0)) - f.rho);
  if (tid == 0) {
    atomicAdd(cinfo + 1, 1);                                          // integer atomics: their order does not show
    if (f.cut) atomicAdd(cinfo + 2, 1);
    atomicMax(cinfo + 3, f.it);
  }
}

// ------------------------------------------------------------------------------------------------ probability=True: the sigmoids

struct PlattArgs {
  const int32_t* labels;
  const int32_t* offsets;
  const float* cv_decision;
  const int32_t* info;
  const int32_t* cv_info;
  double* probA;
  double* probB;
  int32_t* present;
  int K, max_rows;
  double eps;
};

struct PlattPoint {
  double f, g1, g2, h11, h21, h22;
};

// One wave per (problem, pair): Lin, Lin and Weng's Newton iteration on (A, B), float64 throughout.  The pair's entries are found by
// their labels on every pass over the problem's list (in list order; the values are a few KB and stay in cache), the six sums of a
// pass are per-lane partial sums added by one butterfly, so every lane holds the same bits and takes the same branches.
__global__ __launch_bounds__(64) void svc_platt_kernel(PlattArgs a) {
  const int K = a.K, npairs = K * (K - 1) / 2;
  const int p = blockIdx.x / npairs, q = blockIdx.x % npairs, lane = threadIdx.x;
  if (a.info && a.info[(size_t)p * 4] != 0) return;
  if (a.cv_info && a.cv_info[(size_t)p * 4] != 0) return;
  const int begin = a.offsets[p];
  const int n = a.offsets[p + 1] - begin;
  if (n < 1 || n > a.max_rows || n > kMaxRows) return;
  int ci, cj;
  pair_of(q, K, ci, cj);
  const int32_t* __restrict__ lab = a.labels + begin;
  const float* __restrict__ dec = a.cv_decision + (size_t)begin * (K - 1);
  int np_ = 0, nn_ = 0, mask = 0;
  for (int t = lane; t < n; t += 64) {
    const int y = lab[t];
    np_ += y == ci;
    nn_ += y == cj;
    if ((unsigned)y < (unsigned)K) mask |= 1 << y;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    np_ += __shfl_xor(np_, s, 64);
    nn_ += __shfl_xor(nn_, s, 64);
    mask |= __shfl_xor(mask, s, 64);
  }
  if (q == 0 && lane == 0 && a.present) a.present[p] = mask;
  double* __restrict__ outA = a.probA + (size_t)p * npairs + q;
  double* __restrict__ outB = a.probB + (size_t)p * npairs + q;
  if (np_ == 0 || nn_ == 0) {
    if (lane == 0) *outA = *outB = 0.0;
    return;
  }
  const double hi = ((double)np_ + 1.0) / ((double)np_ + 2.0), lo = 1.0 / ((double)nn_ + 2.0);
  auto pass = [&](double A, double B) -> PlattPoint {
    PlattPoint s = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = lane; t < n; t += 64) {
      const int y = lab[t];
      if (y != ci && y != cj) continue;
      const double d = (double)dec[(size_t)t * (K - 1) + (y == ci ? cj - 1 : ci)];
      const double tg = y == ci ? hi : lo;
      const double z = A * d + B, e = exp(-fabs(z));
      s.f += (z >= 0.0 ? tg : tg - 1.0) * z + log1p(e);
      const double pr = (z >= 0.0 ? e : 1.0) / (1.0 + e);              // 1 / (1 + exp(z))
      const double d1 = tg - pr, d2 = pr * (1.0 - pr);
      s.g1 += d * d1;
      s.g2 += d1;
      s.h11 += d * d * d2;
      s.h21 += d * d2;
      s.h22 += d2;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      s.f += __shfl_xor(s.f, m, 64);
      s.g1 += __shfl_xor(s.g1, m, 64);
      s.g2 += __shfl_xor(s.g2, m, 64);
      s.h11 += __shfl_xor(s.h11, m, 64);
      s.h21 += __shfl_xor(s.h21, m, 64);
      s.h22 += __shfl_xor(s.h22, m, 64);
    }
    return s;
  };
  double A = 0.0, B = log(((double)nn_ + 1.0) / ((double)np_ + 1.0));
  PlattPoint at = pass(A, B);
  for (int it = 0; it < 100; ++it) {
    const double gn = fmax(fabs(at.g1), fabs(at.g2));
    if (!(gn >= a.eps)) break;                                        // |g|_inf < eps (or NaN values: nothing to iterate on)
    const double h11 = at.h11 + 1e-12, h22 = at.h22 + 1e-12, h21 = at.h21;
    const double det = h11 * h22 - h21 * h21;
    const double dA = -(h22 * at.g1 - h21 * at.g2) / det, dB = -(-h21 * at.g1 + h11 * at.g2) / det;
    const double slope = at.g1 * dA + at.g2 * dB;
    double step = 1.0;
    bool moved = false;
    for (int hv = 0; hv <= 10; ++hv) {
      const PlattPoint to = pass(A + step * dA, B + step * dB);
      // at the rounding floor of f the sufficient-decrease test is noise: there a step that shrinks the gradient is taken
      if (to.f < at.f + 1e-4 * step * slope ||
          (fmax(fabs(to.g1), fabs(to.g2)) < gn && to.f <= at.f + 1e-9 * fmax(1.0, fabs(at.f)))) {
        A += step * dA;
        B += step * dB;
        at = to;
        moved = true;
        break;
      }
      step *= 0.5;
    }
    if (!moved) break;
  }
  if (lane == 0) {
    *outA = A;
    *outB = B;
  }
}

// ------------------------------------------------------------------------------------------------ probability=True: pairwise coupling

// the problem whose list holds entry e: the last p with offsets[p] <= e; -1 where e is outside every list
__device__ inline int problem_of(const int32_t* __restrict__ offsets, int P, int e) {
  if (P < 1 || e < offsets[0] || e >= offsets[P]) return -1;
  int lo = 0, hi = P;                                                 // offsets[lo] <= e < offsets[hi]
  for (int k = 0; k < 32 && hi - lo > 1; ++k) {
    const int mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= e)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

struct CoupleArgs {
  const float* decision;
  const int32_t* truth;
  const int32_t* offsets;
  const double* probA;
  const double* probB;
  const int32_t* present;
  float* probs;
  int32_t* pred;
  int32_t* correct;
  int P, total;
};

// A thread per entry.  Wu, Lin and Weng's method 2: p minimises p'Qp on the plane e'p = 1.  The minimiser is Q'^{-1} e scaled to sum
// 1 with Q' = Q + e e' (Q p = -b e and e'p = 1 give Q'p = (1 - b) e), and Q' is positive definite (a null vector of Q has entries of one
// sign), so the bordered KKT system of couple_host is solved here by a Cholesky factorisation without pivoting, every index a
// compile-time constant: the lower triangle lives in registers.  An absent class's row is that of the identity with a zero right side.
template <int K>
__global__ __launch_bounds__(256) void svc_couple_kernel(CoupleArgs a) {
  constexpr int npairs = K * (K - 1) / 2;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const int p = problem_of(a.offsets, a.P, e);
  if (p < 0) return;                                                  // pred -1, NaN probabilities (the call's presets)
  const int present = a.present[p];
  double L[K][K];                                                     // lower triangle of Q', then of its factor
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) L[i][j] = (i == j || (((present >> i) & 1) && ((present >> j) & 1))) ? 1.0 : 0.0;   // e e', or the identity
  bool nan = __popc(present & ((1 << K) - 1)) < 2;
  {
    int q = 0;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int j = i + 1; j < K; ++j, ++q) {
        const double f = (double)a.decision[(size_t)e * npairs + q];
        nan = nan || !(f == f);
        if (((present >> i) & 1) && ((present >> j) & 1)) {
          const double z = a.probA[(size_t)p * npairs + q] * f + a.probB[(size_t)p * npairs + q];
          nan = nan || !(z == z);
          const double ex = exp(-fabs(z));
          double r = (z >= 0.0 ? ex : 1.0) / (1.0 + ex);              // r_ij = 1 / (1 + exp(z))
          r = fmin(fmax(r, 1e-7), 1.0 - 1e-7);
          const double rji = 1.0 - r;
          L[i][i] += rji * rji;
          L[j][j] += r * r;
          L[j][i] -= r * rji;
        }
      }
  }
  if (nan) return;
  // Cholesky in place, then L y = e, L' x = y
#pragma unroll
  for (int j = 0; j < K; ++j) {
#pragma unroll
    for (int k = 0; k < j; ++k) L[j][j] -= L[j][k] * L[j][k];
    L[j][j] = sqrt(L[j][j]);
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
#pragma unroll
      for (int k = 0; k < j; ++k) L[i][j] -= L[i][k] * L[j][k];
      L[i][j] /= L[j][j];
    }
  }
  double x[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    x[i] = ((present >> i) & 1) ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < i; ++k) x[i] -= L[i][k] * x[k];
    x[i] /= L[i][i];
  }
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
#pragma unroll
    for (int k = i + 1; k < K; ++k) x[i] -= L[k][i] * x[k];
    x[i] /= L[i][i];
  }
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < K; ++i) sum += x[i];
  double best = -1.0;
  int arg = -1;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const float pr = ((present >> i) & 1) ? (float)(x[i] / sum) : 0.0f;
    a.probs[(size_t)e * K + i] = pr;
    if (((present >> i) & 1) && (double)pr > best) {                  // the first argmax of what is written
      best = (double)pr;
      arg = i;
    }
  }
  a.pred[e] = arg;
  if (arg >= 0 && arg == a.truth[e]) atomicAdd(a.correct + p, 1);      // an integer count
}

__global__ __launch_bounds__(256) void soft_vote_kernel(const float* __restrict__ pa, const float* __restrict__ pb, const int32_t* __restrict__ truth,
                                                        const int32_t* __restrict__ offsets, int P, int K, int total,
                                                        int32_t* __restrict__ pred, int32_t* __restrict__ correct, float* __restrict__ mean) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int p = problem_of(offsets, P, e);
  if (p < 0) return;
  float best = 0.0f;
  int arg = -1;
  bool nan = false;
  for (int k = 0; k < K; ++k) {
    const float u = pa[(size_t)e * K + k], v = pb[(size_t)e * K + k];
    nan = nan || !(u == u) || !(v == v);
    const float m = 0.5f * (u + v);
    if (mean) mean[(size_t)e * K + k] = m;
    if (arg < 0 || m > best) {                                        // the first argmax
      best = m;
      arg = k;
    }
  }
  if (nan) return;                                                    // pred stays -1
  pred[e] = arg;
  if (arg == truth[e]) atomicAdd(correct + p, 1);                     // an integer count
}

int check_shape(int n_rows, int dim, int n_problems) {
  if (n_rows < 0 || n_problems < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (dim < 1) return fail(MKWS_ERR_INVALID_ARG, "dim = %d: at least one column", dim);
  if (dim > kMaxDim) return fail(MKWS_ERR_UNSUPPORTED, "dim = %d: at most %d", dim, kMaxDim);
  return MKWS_OK;
}

int check_classes(int n_classes) {
  if (n_classes < 2) return fail(MKWS_ERR_INVALID_ARG, "n_classes = %d: at least two classes", n_classes);
  if (n_classes > kMaxK) return fail(MKWS_ERR_UNSUPPORTED, "%d classes: at most %d", n_classes, kMaxK);
  return MKWS_OK;
}

int check_rows(int max_rows, const char* what) {
  if (max_rows < 1) return fail(MKWS_ERR_INVALID_ARG, "%s = %d: at least one row", what, max_rows);
  if (max_rows > kMaxRows) return fail(MKWS_ERR_UNSUPPORTED, "%s = %d: at most %d", what, max_rows, kMaxRows);
  return MKWS_OK;
}

// what mkws_svc_fit and mkws_svc_fit_cv refuse alike
int check_fit(int n_problems, int n_classes, int max_rows, int max_iter, double tol, size_t gram_stride) {
  if (n_problems < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (int rc = check_classes(n_classes)) return rc;
  if (int rc = check_rows(max_rows, "max_rows")) return rc;
  if (max_iter < 1) return fail(MKWS_ERR_INVALID_ARG, "max_iter = %d: at least one iteration", max_iter);
  if (!(tol >= 0.0)) return fail(MKWS_ERR_INVALID_ARG, "tol is NaN or negative");
  if (n_problems > 0 && gram_stride < (size_t)max_rows * (size_t)max_rows)
    return fail(MKWS_ERR_INVALID_ARG, "gram_stride of %zu floats for problems of up to %d rows", gram_stride, max_rows);
  return MKWS_OK;
}

// the pair kernels ask for more than 64 KB of LDS: the limit is raised once per device, in the set the caller keeps for its kernel
int allow_fit_lds(const void* kernel, std::set<int>& done) {
  static std::mutex mu;
  int dev = 0;
  MKWS_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  if (!done.count(dev)) {
    MKWS_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitLdsBytes));
    done.insert(dev);
  }
  return MKWS_OK;
}

// a call whose problems all fit the LDS cache asks for no more than they need
size_t fit_lds_bytes(int max_rows) {
  const size_t side = max_rows < kCacheRows ? max_rows : kCacheRows;
  return kFitLdsFixed + side * side * 4;
}

}  // namespace

extern "C" size_t mkws_svc_work_bytes(int n_problems, int max_rows) {
  if (n_problems < 0 || max_rows < 0) return 0;
  return (size_t)n_problems * (size_t)max_rows * (size_t)max_rows * sizeof(float);
}

extern "C" int mkws_svc_prepare(const float* d_x, int n_rows, int dim, const int32_t* d_rows, const int32_t* d_labels, const int32_t* d_offsets,
                                int n_problems, int n_classes, int max_rows, int standardize, double gamma, float* d_centre, float* d_inv_scale,
                                float* d_gamma, int32_t* d_info, float* d_gap, void* stream) {
  if (int rc = check_shape(n_rows, dim, n_problems)) return rc;
  if (int rc = check_classes(n_classes)) return rc;
  if (int rc = check_rows(max_rows, "max_rows")) return rc;
  if (standardize != 0 && standardize != 1) return fail(MKWS_ERR_INVALID_ARG, "standardize = %d: 0 or 1", standardize);
  if (!std::isfinite(gamma)) return fail(MKWS_ERR_INVALID_ARG, "gamma is not finite");
  if (n_problems == 0) return MKWS_OK;
  if (!d_x || !d_rows || !d_labels || !d_offsets || !d_centre || !d_inv_scale || !d_gamma || !d_info || !d_gap)
    return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  hipLaunchKernelGGL(svc_prepare_kernel, dim3(n_problems), dim3(kPrepThreads), 0, static_cast<hipStream_t>(stream), d_x, n_rows, dim, d_rows, d_labels,
                     d_offsets, n_classes, max_rows, standardize, gamma, d_centre, d_inv_scale, d_gamma, d_info, d_gap);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

extern "C" int mkws_svc_kernel(const float* d_x, int n_rows, int dim, const int32_t* d_rows_a, const int32_t* d_offsets_a, int max_a,
                               const int32_t* d_rows_b, const int32_t* d_offsets_b, int max_b, int n_problems, const float* d_centre,
                               const float* d_inv_scale, const float* d_gamma, const int32_t* d_info, float* d_out, size_t out_stride, void* stream) {
  if (int rc = check_shape(n_rows, dim, n_problems)) return rc;
  if (max_a < 0 || max_b < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (n_problems == 0 || max_a == 0 || max_b == 0) return MKWS_OK;
  if (!d_x || !d_rows_a || !d_offsets_a || !d_rows_b || !d_offsets_b || !d_centre || !d_inv_scale || !d_gamma || !d_out)
    return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (out_stride < (size_t)max_a * (size_t)max_b)
    return fail(MKWS_ERR_INVALID_ARG, "out_stride of %zu floats for lists of up to %d and %d rows", out_stride, max_a, max_b);
  const long long tiles_a = (max_a + kTile - 1) / kTile, tiles_b = (max_b + kTile - 1) / kTile;
  const long long blocks = tiles_a * tiles_b * (long long)n_problems;
  if (blocks > 0x7fffffffLL) return fail(MKWS_ERR_UNSUPPORTED, "%lld tiles in one call", blocks);
  hipLaunchKernelGGL(svc_kernel_kernel, dim3((unsigned)blocks), dim3(kTileThreads), 0, static_cast<hipStream_t>(stream), d_x, n_rows, dim, d_rows_a,
                     d_offsets_a, max_a, d_rows_b, d_offsets_b, max_b, (int)tiles_a, (int)tiles_b, d_centre, d_inv_scale, d_gamma, d_info, d_out,
                     out_stride);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

extern "C" int mkws_svc_fit(const int32_t* d_labels, const int32_t* d_offsets, int n_problems, int n_classes, int max_rows, const double* d_C,
                            double tol, int max_iter, const float* d_gram, size_t gram_stride, float* d_coef, float* d_rho, int32_t* d_info,
                            float* d_gap, void* stream) {
  if (int rc = check_fit(n_problems, n_classes, max_rows, max_iter, tol, gram_stride)) return rc;
  if (n_problems == 0) return MKWS_OK;
  if (!d_labels || !d_offsets || !d_C || !d_gram || !d_coef || !d_rho || !d_info || !d_gap) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  const long long blocks = (long long)n_problems * (n_classes * (n_classes - 1) / 2);
  if (blocks > 0x7fffffffLL) return fail(MKWS_ERR_UNSUPPORTED, "%lld pairs in one call", blocks);
  static std::set<int> done;
  if (int rc = allow_fit_lds(reinterpret_cast<const void*>(svc_fit_kernel), done)) return rc;
  FitArgs a;
  a.labels = d_labels;
  a.offsets = d_offsets;
  a.C = d_C;
  a.gram = d_gram;
  a.gram_stride = gram_stride;
  a.coef = d_coef;
  a.rho = d_rho;
  a.info = d_info;
  a.gap = d_gap;
  a.K = n_classes;
  a.max_rows = max_rows;
  a.max_iter = max_iter;
  a.tol = tol;
  hipLaunchKernelGGL(svc_fit_kernel, dim3((unsigned)blocks), dim3(kFitThreads), fit_lds_bytes(max_rows), static_cast<hipStream_t>(stream), a);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

extern "C" int mkws_svc_score(const float* d_x, int n_rows, int dim, const int32_t* d_train_rows, const int32_t* d_train_labels,
                              const int32_t* d_train_offsets, int max_train, const float* d_coef, const float* d_rho, const float* d_gamma,
                              const float* d_centre, const float* d_inv_scale, const int32_t* d_info, int n_problems, int n_classes,
                              const int32_t* d_rows, const int32_t* d_true, const int32_t* d_offsets, int total, int max_eval, int32_t* d_pred,
                              int32_t* d_correct, float* d_decision, void* stream) {
  if (int rc = check_shape(n_rows, dim, n_problems)) return rc;
  if (int rc = check_classes(n_classes)) return rc;
  if (total < 0 || max_eval < 0 || max_train < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (max_train > kMaxRows) return fail(MKWS_ERR_UNSUPPORTED, "max_train = %d: at most %d", max_train, kMaxRows);
  if (!d_offsets || !d_train_offsets) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (n_problems > 0 && !d_correct) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (total > 0 && (!d_x || !d_rows || !d_true || !d_pred)) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_problems > 0) MKWS_HIP(hipMemsetAsync(d_correct, 0, (size_t)n_problems * sizeof(int32_t), s));
  if (total == 0) return MKWS_OK;
  // pred = -1 and NaN decision values (all bits set) wherever no workgroup writes: entries outside every list, rows outside the bank, refused models
  MKWS_HIP(hipMemsetAsync(d_pred, 0xff, (size_t)total * sizeof(int32_t), s));
  const int npairs = n_classes * (n_classes - 1) / 2;
  if (d_decision) MKWS_HIP(hipMemsetAsync(d_decision, 0xff, (size_t)total * npairs * sizeof(float), s));
  if (n_problems == 0 || max_eval == 0 || max_train == 0) return MKWS_OK;
  if (!d_train_rows || !d_train_labels || !d_coef || !d_rho || !d_gamma || !d_centre || !d_inv_scale) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  const long long tiles_e = (max_eval + kTile - 1) / kTile, blocks = tiles_e * (long long)n_problems;
  if (blocks > 0x7fffffffLL) return fail(MKWS_ERR_UNSUPPORTED, "%lld tiles in one call", blocks);
  ScoreArgs a;
  a.x = d_x;
  a.train_rows = d_train_rows;
  a.train_labels = d_train_labels;
  a.train_offsets = d_train_offsets;
  a.coef = d_coef;
  a.rho = d_rho;
  a.gamma = d_gamma;
  a.centre = d_centre;
  a.inv = d_inv_scale;
  a.info = d_info;
  a.rows = d_rows;
  a.truth = d_true;
  a.offsets = d_offsets;
  a.pred = d_pred;
  a.correct = d_correct;
  a.decision = d_decision;
  a.n_rows = n_rows;
  a.dim = dim;
  a.K = n_classes;
  a.max_train = max_train;
  a.max_eval = max_eval;
  a.tiles_e = (int)tiles_e;
  hipLaunchKernelGGL(svc_score_kernel, dim3((unsigned)blocks), dim3(kTileThreads), 0, s, a);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

// ------------------------------------------------------------------------------------------------ probability=True

extern "C" int mkws_svc_fit_cv(const int32_t* d_labels, const int32_t* d_offsets, const int32_t* d_folds, int n_folds, int n_problems,
                               int n_classes, int max_rows, const double* d_C, double tol, int max_iter, const float* d_gram,
                               size_t gram_stride, const int32_t* d_info, float* d_cv_decision, int32_t* d_cv_info, void* stream) {
  if (int rc = check_fit(n_problems, n_classes, max_rows, max_iter, tol, gram_stride)) return rc;
  if (n_folds < 2) return fail(MKWS_ERR_INVALID_ARG, "n_folds = %d: at least two folds", n_folds);
  if (n_folds > MKWS_SVC_MAX_FOLDS) return fail(MKWS_ERR_UNSUPPORTED, "n_folds = %d: at most %d", n_folds, MKWS_SVC_MAX_FOLDS);
  if (n_problems == 0) return MKWS_OK;
  if (!d_labels || !d_offsets || !d_folds || !d_C || !d_gram || !d_info || !d_cv_decision || !d_cv_info) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  const long long blocks = (long long)n_problems * (n_classes * (n_classes - 1) / 2) * n_folds;
  if (blocks > 0x7fffffffLL) return fail(MKWS_ERR_UNSUPPORTED, "%lld sub-fits in one call", blocks);
  static std::set<int> done;
  if (int rc = allow_fit_lds(reinterpret_cast<const void*>(svc_fit_cv_kernel), done)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MKWS_HIP(hipMemsetAsync(d_cv_info, 0, (size_t)n_problems * 4 * sizeof(int32_t), s));
  FitCvArgs a;
  a.labels = d_labels;
  a.offsets = d_offsets;
  a.folds = d_folds;
  a.C = d_C;
  a.gram = d_gram;
  a.gram_stride = gram_stride;
  a.info = d_info;
  a.cv_decision = d_cv_decision;
  a.cv_info = d_cv_info;
  a.K = n_classes;
  a.F = n_folds;
  a.max_rows = max_rows;
  a.max_iter = max_iter;
  a.tol = tol;
  hipLaunchKernelGGL(svc_fit_cv_kernel, dim3((unsigned)blocks), dim3(kFitThreads), fit_lds_bytes(max_rows), s, a);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

extern "C" int mkws_svc_platt(const int32_t* d_labels, const int32_t* d_offsets, int n_problems, int n_classes, int max_rows,
                              const float* d_cv_decision, const int32_t* d_info, const int32_t* d_cv_info, double eps, double* d_probA,
                              double* d_probB, int32_t* d_present, void* stream) {
  if (n_problems < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (int rc = check_classes(n_classes)) return rc;
  if (int rc = check_rows(max_rows, "max_rows")) return rc;
  if (!(eps >= 0.0)) return fail(MKWS_ERR_INVALID_ARG, "eps is NaN or negative");
  if (n_problems == 0) return MKWS_OK;
  if (!d_labels || !d_offsets || !d_cv_decision || !d_probA || !d_probB) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  const long long blocks = (long long)n_problems * (n_classes * (n_classes - 1) / 2);
  if (blocks > 0x7fffffffLL) return fail(MKWS_ERR_UNSUPPORTED, "%lld pairs in one call", blocks);
  PlattArgs a;
  a.labels = d_labels;
  a.offsets = d_offsets;
  a.cv_decision = d_cv_decision;
  a.info = d_info;
  a.cv_info = d_cv_info;
  a.probA = d_probA;
  a.probB = d_probB;
  a.present = d_present;
  a.K = n_classes;
  a.max_rows = max_rows;
  a.eps = eps;
  hipLaunchKernelGGL(svc_platt_kernel, dim3((unsigned)blocks), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

namespace {

// d_correct zeroed, d_pred = -1 and NaN probabilities (all bits set) wherever no thread writes
int preset_scores(int n_problems, int n_classes, int total, int32_t* d_pred, int32_t* d_correct, float* d_probs, hipStream_t s) {
  if (n_problems > 0) MKWS_HIP(hipMemsetAsync(d_correct, 0, (size_t)n_problems * sizeof(int32_t), s));
  if (total > 0) MKWS_HIP(hipMemsetAsync(d_pred, 0xff, (size_t)total * sizeof(int32_t), s));
  if (total > 0 && d_probs) MKWS_HIP(hipMemsetAsync(d_probs, 0xff, (size_t)total * n_classes * sizeof(float), s));
  return MKWS_OK;
}

}  // namespace

extern "C" int mkws_svc_couple(const float* d_decision, const int32_t* d_true, const int32_t* d_offsets, int n_problems, int n_classes,
                               int total, const double* d_probA, const double* d_probB, const int32_t* d_present, float* d_probs,
                               int32_t* d_pred, int32_t* d_correct, void* stream) {
  if (n_problems < 0 || total < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (int rc = check_classes(n_classes)) return rc;
  if (!d_offsets) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (n_problems > 0 && (!d_correct || !d_probA || !d_probB || !d_present)) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (total > 0 && (!d_decision || !d_true || !d_probs || !d_pred)) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = preset_scores(n_problems, n_classes, total, d_pred, d_correct, d_probs, s)) return rc;
  if (total == 0 || n_problems == 0) return MKWS_OK;
  CoupleArgs a;
  a.decision = d_decision;
  a.truth = d_true;
  a.offsets = d_offsets;
  a.probA = d_probA;
  a.probB = d_probB;
  a.present = d_present;
  a.probs = d_probs;
  a.pred = d_pred;
  a.correct = d_correct;
  a.P = n_problems;
  a.total = total;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  switch (n_classes) {
    case 2: hipLaunchKernelGGL(svc_couple_kernel<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(svc_couple_kernel<3>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(svc_couple_kernel<4>, grid, block, 0, s, a); break;
    case 5: hipLaunchKernelGGL(svc_couple_kernel<5>, grid, block, 0, s, a); break;
    case 6: hipLaunchKernelGGL(svc_couple_kernel<6>, grid, block, 0, s, a); break;
    case 7: hipLaunchKernelGGL(svc_couple_kernel<7>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(svc_couple_kernel<8>, grid, block, 0, s, a); break;
  }
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

extern "C" int mkws_soft_vote(const float* d_probs_a, const float* d_probs_b, const int32_t* d_true, const int32_t* d_offsets, int n_problems,
                              int n_classes, int total, int32_t* d_pred, int32_t* d_correct, float* d_mean, void* stream) {
  if (n_problems < 0 || total < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (int rc = check_classes(n_classes)) return rc;
  if (!d_offsets) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (n_problems > 0 && !d_correct) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (total > 0 && (!d_probs_a || !d_probs_b || !d_true || !d_pred)) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = preset_scores(n_problems, n_classes, total, d_pred, d_correct, d_mean, s)) return rc;
  if (total == 0 || n_problems == 0) return MKWS_OK;
  hipLaunchKernelGGL(soft_vote_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_probs_a, d_probs_b, d_true, d_offsets, n_problems,
                     n_classes, total, d_pred, d_correct, d_mean);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}
