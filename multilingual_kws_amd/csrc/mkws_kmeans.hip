// k-means of the MSWC outlier filter (mkws_kmeans_fit / mkws_kmeans_nearest, include/mkws.h): what
// sklearn.cluster.KMeans(n_clusters, random_state).fit does to the embeddings of one keyword's train clips -- mean-centring, greedy
// k-means++, Lloyd with both stopping rules, the final assignment -- for n_groups keywords in one launch, and the distance of every
// eval clip to the nearest centre of its keyword.  multilingual_kws_amd/kmeans.py (kmeans_host) is the specification.
//
// Fit: one workgroup of 16 waves per group.  The points stay in global memory / L2 and are re-read in every pass; the float64 centres,
// the column means, closest[], the labels and the counts live in LDS.  Distances: a wave per point, lanes across dim, a butterfly
// reduction in a fixed order.  Means: a thread per column summing the group's points in row order (coalesced, no atomics).  cumsum
// (closest) is formed sequentially in float64, as np.cumsum forms it.  Everything is float64 arithmetic on widened float32 inputs, there
// are no floating-point atomics and no workspace: two runs on the same input write the same bytes.  Every loop is bounded by max_iter,
// n_clusters, n_trials or the point count; no workgroup waits for another.
#include "mkws_common.h"

#include <cmath>
#include <cstdint>
#include <mutex>
#include <set>
#include <utility>

using mkws::fail;

namespace {

constexpr int kFitThreads = 1024;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kMaxPoints = MKWS_KMEANS_MAX_POINTS;
constexpr int kMaxClusters = MKWS_KMEANS_MAX_CLUSTERS;
constexpr int kMaxTrials = MKWS_KMEANS_MAX_TRIALS;
constexpr int kHeaderBytes = 1024;      // the small arrays in front of the dynamic LDS region (a multiple of 16)
constexpr int kLdsCap = 160 * 1024;
static_assert(kMaxPoints == kFitThreads, "a point per thread in the block sums");
static_assert(kMaxClusters == 16, "the distance loops are unrolled over 16 accumulators");

// centres [k * dim] + column means [dim] in float64, closest[] and a second per-point array in float64, the labels
size_t fit_lds_bytes(int dim, int k) {
  return kHeaderBytes + ((size_t)k + 1) * dim * sizeof(double) + 2 * (size_t)kMaxPoints * sizeof(double) + (size_t)kMaxPoints * sizeof(int);
}

struct FitArgs {
  const float* x;
  const int32_t* offsets;
  const double* draws;
  float* centers;
  double* centers64;
  int32_t* labels;
  int32_t* init;
  int32_t* info;
  int dim, k, trials, max_iter;
  double tol;
};

// every lane gets the same sum: a + b and b + a are the same bits
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// every thread gets the same sum (wave sums added in wave order); two barriers
__device__ inline double block_sum(double v, double* s_red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kFitWaves; ++w) t += s_red[w];
  __syncthreads();
  return t;
}

// |(xi - mean) - (xj - mean)|^2 of two rows, by one wave
__device__ inline double row_to_row(const float* __restrict__ xi, const float* __restrict__ xj, const double* s_mean, int dim, int lane) {
  double acc = 0.0;
  for (int col = lane; col < dim; col += 64) {
    const double m = s_mean[col];
    const double d = ((double)xi[col] - m) - ((double)xj[col] - m);
    acc += d * d;
  }
  return wave_sum(acc);
}

// first index of the smallest of |(xi - mean) - centre c|^2, c < k, by one wave
__device__ inline int nearest_centre(const float* __restrict__ xi, const double* s_mean, const double* s_c, int dim, int k, int lane) {
  double acc[kMaxClusters];
#pragma unroll
  for (int c = 0; c < kMaxClusters; ++c) acc[c] = 0.0;
  for (int col = lane; col < dim; col += 64) {
    const double v = (double)xi[col] - s_mean[col];
#pragma unroll
    for (int c = 0; c < kMaxClusters; ++c) {
      if (c < k) {
        const double d = v - s_c[(size_t)c * dim + col];
        acc[c] += d * d;
      }
    }
  }
  double best = 0.0;
  int arg = 0;
#pragma unroll
  for (int c = 0; c < kMaxClusters; ++c) {
    if (c < k) {
      const double s = wave_sum(acc[c]);
      if (c == 0 || s < best) {
        best = s;
        arg = c;
      }
    }
  }
  return arg;
}

__global__ __launch_bounds__(kFitThreads) void kmeans_fit_kernel(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char s_raw[];
  const int dim = a.dim, k = a.k, T = a.trials;
  // header: 16 wave sums, then counts [16], starts [17], candidates [kMaxTrials], the "a label changed" flag
  double* s_red = reinterpret_cast<double*>(s_raw);
  int* s_count = reinterpret_cast<int*>(s_raw + 128);
  int* s_start = s_count + kMaxClusters;
  int* s_cand = s_start + kMaxClusters + 1;
  int* s_changed = s_cand + kMaxTrials;
  static_assert(128 + (2 * kMaxClusters + 2 + kMaxTrials) * 4 <= kHeaderBytes, "header");
  double* s_c = reinterpret_cast<double*>(s_raw + kHeaderBytes);     // [k, dim] centres of the centred points
  double* s_mean = s_c + (size_t)k * dim;                            // [dim]
  double* s_closest = s_mean + dim;                                  // [kMaxPoints]
  double* s_tmp = s_closest + kMaxPoints;                            // [kMaxPoints] k-means++: min(closest, distance to a candidate)
  int* s_order = reinterpret_cast<int*>(s_tmp);                      //              Lloyd: the points sorted by label, row order kept
  int* s_label = reinterpret_cast<int*>(s_tmp + kMaxPoints);         // [kMaxPoints]

  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int begin = a.offsets[g];
  const int n = a.offsets[g + 1] - begin;
  int32_t* __restrict__ info = a.info + (size_t)g * 4;
  if (n < k || n > kMaxPoints) {                                     // (an n below 0 too: nothing of the group is touched)
    if (tid < 4) info[tid] = tid == 0 ? 2 : 0;
    return;
  }
  const float* __restrict__ x = a.x + (size_t)begin * dim;
  const double* __restrict__ draws = a.draws + (size_t)g * (1 + (size_t)(k - 1) * T);

  // column means (X.mean(0): the rows added in order) and tol_abs = mean over the columns of var(Xc) * tol
  double var_local = 0.0;
  for (int col = tid; col < dim; col += kFitThreads) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)x[(size_t)i * dim + col];
    const double m = s / (double)n;
    s_mean[col] = m;
    double s2 = 0.0;
    for (int i = 0; i < n; ++i) s2 += (double)x[(size_t)i * dim + col] - m;
    const double m2 = s2 / (double)n;
    double s3 = 0.0;
    for (int i = 0; i < n; ++i) {
      const double d = ((double)x[(size_t)i * dim + col] - m) - m2;
      s3 += d * d;
    }
    var_local += s3 / (double)n;
  }
  if (tid < n) s_label[tid] = -1;
  if (tid == 0) *s_changed = 0;
  const double tol_abs = block_sum(var_local, s_red) / (double)dim * a.tol;     // (its barriers publish s_mean)

  // ---- greedy k-means++ ----
  if (tid == 0) {                                                    // RandomState.choice(n, p = 1 / n): searchsorted(cdf / cdf[-1], u0, "right")
    const double p = 1.0 / (double)n, u0 = draws[0];
    double last = 0.0;
    for (int i = 0; i < n; ++i) last += p;
    double cs = 0.0;
    int idx = n - 1;
    bool found = false;
    for (int i = 0; i < n; ++i) {
      cs += p;
      if (!found && cs / last > u0) {
        idx = i;
        found = true;
      }
    }
    s_cand[0] = idx;
  }
  __syncthreads();
  int cand = s_cand[0];
  for (int col = tid; col < dim; col += kFitThreads) s_c[col] = (double)x[(size_t)cand * dim + col] - s_mean[col];
  if (a.init && tid == 0) a.init[(size_t)g * k] = cand;
  for (int i = wave; i < n; i += kFitWaves) {
    const double d = row_to_row(x + (size_t)i * dim, x + (size_t)cand * dim, s_mean, dim, lane);
    if (lane == 0) s_closest[i] = d;
  }
  __syncthreads();
  double pot = block_sum(tid < n ? s_closest[tid] : 0.0, s_red);
  for (int c = 1; c < k; ++c) {
    if (tid < T) {                                                   // searchsorted(cumsum(closest), U * pot), clipped to n - 1
      const double v = draws[1 + (size_t)(c - 1) * T + tid] * pot;
      double cs = 0.0;
      int idx = n - 1;
      bool found = false;
      for (int i = 0; i < n; ++i) {
        cs += s_closest[i];
        if (!found && cs >= v) {
          idx = i;
          found = true;
        }
      }
      s_cand[tid] = idx;
    }
    __syncthreads();
    double best_pot = 0.0;
    int best = 0;
    for (int t = 0; t < T; ++t) {                                    // the candidate's potential: sum of min(closest, distance to it)
      const float* __restrict__ xc = x + (size_t)s_cand[t] * dim;
      for (int i = wave; i < n; i += kFitWaves) {
        const double d = row_to_row(x + (size_t)i * dim, xc, s_mean, dim, lane);
        if (lane == 0) s_tmp[i] = fmin(s_closest[i], d);
      }
      __syncthreads();
      const double pt = block_sum(tid < n ? s_tmp[tid] : 0.0, s_red);
      if (t == 0 || pt < best_pot) {                                 // first argmin; the same value in every thread
        best_pot = pt;
        best = t;
      }
    }
    cand = s_cand[best];
    const float* __restrict__ xc = x + (size_t)cand * dim;
    for (int i = wave; i < n; i += kFitWaves) {                      // closest = that candidate's row (formed again: no room to keep n_trials rows)
      const double d = row_to_row(x + (size_t)i * dim, xc, s_mean, dim, lane);
      if (lane == 0) s_closest[i] = fmin(s_closest[i], d);
    }
    for (int col = tid; col < dim; col += kFitThreads) s_c[(size_t)c * dim + col] = (double)xc[col] - s_mean[col];
    if (a.init && tid == 0) a.init[(size_t)g * k + c] = cand;
    pot = best_pot;
    __syncthreads();                                                 // s_cand and s_closest are read before they are written again
  }
  __syncthreads();

  // ---- Lloyd ----
  int status = 0, n_iter = 0, reason = 2;
  for (int it = 0; it < a.max_iter; ++it) {
    for (int i = wave; i < n; i += kFitWaves) {
      const int arg = nearest_centre(x + (size_t)i * dim, s_mean, s_c, dim, k, lane);
      if (lane == 0) {
        if (s_label[i] != arg) *s_changed = 1;
        s_label[i] = arg;
      }
    }
    __syncthreads();
    const int changed = *s_changed;
    if (tid < k) {
      int cnt = 0;
      for (int i = 0; i < n; ++i) cnt += s_label[i] == tid;
      s_count[tid] = cnt;
    }
    __syncthreads();
    if (tid == 0) *s_changed = 0;                                    // every thread has read it; the next E-step is barriers away
    int smallest = n;
    for (int c = 0; c < k; ++c) smallest = min(smallest, s_count[c]);
    n_iter = it + 1;
    if (smallest == 0) {                                             // sklearn relocates a centre here: not restated, reported
      status = 1;
      break;
    }
    if (tid < k) {                                                   // the points of cluster tid, in row order
      int p = 0;
      for (int c = 0; c < tid; ++c) p += s_count[c];
      s_start[tid] = p;
      for (int i = 0; i < n; ++i)
        if (s_label[i] == tid) s_order[p++] = i;
    }
    if (tid == 0) s_start[k] = n;
    __syncthreads();
    double shift_local = 0.0;
    for (int col = tid; col < dim; col += kFitThreads) {
      const double m = s_mean[col];
      for (int c = 0; c < k; ++c) {
        const int j0 = s_start[c], j1 = j0 + s_count[c];
        double s = 0.0;
        for (int j = j0; j < j1; ++j) s += (double)x[(size_t)s_order[j] * dim + col] - m;
        const double nc = s / (double)s_count[c];
        const double d = nc - s_c[(size_t)c * dim + col];
        shift_local += d * d;
        s_c[(size_t)c * dim + col] = nc;
      }
    }
    const double shift = block_sum(shift_local, s_red);              // (its barriers publish the new centres)
    if (!changed) {
      reason = 0;
      break;
    }
    if (shift <= tol_abs) {
      reason = 1;
      break;
    }
  }
  if (status != 0) {
    if (tid < 4) info[tid] = tid == 0 ? status : tid == 1 ? n_iter : 0;
    return;
  }

  // ---- the final assignment and the outputs ----
  for (int i = wave; i < n; i += kFitWaves) {
    const int arg = nearest_centre(x + (size_t)i * dim, s_mean, s_c, dim, k, lane);
    if (lane == 0) s_label[i] = arg;
  }
  __syncthreads();
  if (tid < k) {
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += s_label[i] == tid;
    s_count[tid] = cnt;
  }
  __syncthreads();
  if (tid < n) a.labels[(size_t)begin + tid] = s_label[tid];
  const size_t kd = (size_t)k * dim;
  for (size_t e = tid; e < kd; e += kFitThreads) {
    const double v = s_c[e] + s_mean[e % dim];
    a.centers[(size_t)g * kd + e] = (float)v;
    if (a.centers64) a.centers64[(size_t)g * kd + e] = v;
  }
  if (tid == 0) {
    int smallest = n;
    for (int c = 0; c < k; ++c) smallest = min(smallest, s_count[c]);
    info[0] = 0;
    info[1] = n_iter;
    info[2] = reason;
    info[3] = smallest;
  }
}

constexpr int kNearThreads = 256;
constexpr int kNearRows = kNearThreads / 64;      // a wave per row

__global__ __launch_bounds__(kNearThreads) void kmeans_nearest_kernel(const float* __restrict__ x, int dim, int n_rows, const int32_t* __restrict__ group,
                                                                     const float* __restrict__ centers, int n_groups, int k,
                                                                     float* __restrict__ dist, int32_t* __restrict__ which, int32_t* invalid) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kNearRows + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int g = group[row];
  if ((unsigned)g >= (unsigned)n_groups) {                           // never dereferenced against a centre
    if (lane == 0) {
      dist[row] = __builtin_nanf("");
      which[row] = -1;
      atomicAdd(invalid, 1);                                         // an integer count
    }
    return;
  }
  const float* __restrict__ xr = x + (size_t)row * dim;
  const float* __restrict__ cg = centers + (size_t)g * k * dim;
  double acc[kMaxClusters];
#pragma unroll
  for (int c = 0; c < kMaxClusters; ++c) acc[c] = 0.0;
  for (int col = lane; col < dim; col += 64) {
    const double v = (double)xr[col];
#pragma unroll
    for (int c = 0; c < kMaxClusters; ++c) {
      if (c < k) {
        const double d = (double)cg[(size_t)c * dim + col] - v;
        acc[c] += d * d;
      }
    }
  }
  double best = 0.0;
  int arg = 0;
#pragma unroll
  for (int c = 0; c < kMaxClusters; ++c) {
    if (c < k) {
      const double s = sqrt(wave_sum(acc[c]));
      if (c == 0 || s < best) {
        best = s;
        arg = c;
      }
    }
  }
  if (lane == 0) {
    dist[row] = (float)best;
    which[row] = arg;
  }
}

// more than 64 KB of dynamic LDS: the limit is raised once per device
int raise_fit_lds() {
  static std::mutex mu;
  static std::set<int> done;
  int dev = 0;
  MKWS_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  if (done.count(dev)) return MKWS_OK;
  MKWS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_fit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap));
  done.insert(dev);
  return MKWS_OK;
}

}  // namespace

extern "C" int mkws_kmeans_fit(const float* d_x, int dim, const int32_t* d_offsets, int n_groups, int n_clusters, const double* d_draws,
                               int n_trials, int max_iter, double tol, float* d_centers, double* d_centers_f64, int32_t* d_labels,
                               int32_t* d_init, int32_t* d_info, void* stream) {
  if (n_groups < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (dim < 1) return fail(MKWS_ERR_INVALID_ARG, "dim = %d: at least one column", dim);
  if (n_clusters < 1) return fail(MKWS_ERR_INVALID_ARG, "n_clusters = %d: at least one cluster", n_clusters);
  if (n_trials < 1) return fail(MKWS_ERR_INVALID_ARG, "n_trials = %d: at least one trial", n_trials);
  if (max_iter < 1) return fail(MKWS_ERR_INVALID_ARG, "max_iter = %d: at least one iteration", max_iter);
  if (!(tol >= 0.0)) return fail(MKWS_ERR_INVALID_ARG, "tol is NaN or negative");
  if (n_groups == 0) return MKWS_OK;   // nothing to read or write: the buffers may be NULL
  if (!d_x || !d_offsets || !d_draws || !d_centers || !d_labels || !d_info) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (n_clusters > kMaxClusters) return fail(MKWS_ERR_UNSUPPORTED, "%d clusters: at most %d", n_clusters, kMaxClusters);
  if ((long long)n_clusters * dim > MKWS_KMEANS_MAX_CENTER_VALUES)
    return fail(MKWS_ERR_UNSUPPORTED, "n_clusters * dim = %lld: at most %d (the float64 centres live in LDS)", (long long)n_clusters * dim,
                MKWS_KMEANS_MAX_CENTER_VALUES);
  if (n_trials > kMaxTrials) return fail(MKWS_ERR_UNSUPPORTED, "%d trials: at most %d", n_trials, kMaxTrials);
  if (((long long)n_clusters + 1) * dim > MKWS_KMEANS_MAX_LDS_VALUES)
    return fail(MKWS_ERR_UNSUPPORTED, "(n_clusters + 1) * dim = %lld: at most %d (the centres and the column means live in LDS)",
                ((long long)n_clusters + 1) * dim, MKWS_KMEANS_MAX_LDS_VALUES);
  const size_t lds = fit_lds_bytes(dim, n_clusters);
  static_assert(kHeaderBytes + (size_t)MKWS_KMEANS_MAX_LDS_VALUES * 8 + 2 * (size_t)kMaxPoints * 8 + (size_t)kMaxPoints * 4 <= (size_t)kLdsCap, "LDS");
  if (int rc = raise_fit_lds()) return rc;
  FitArgs a;
  a.x = d_x;
  a.offsets = d_offsets;
  a.draws = d_draws;
  a.centers = d_centers;
  a.centers64 = d_centers_f64;
  a.labels = d_labels;
  a.init = d_init;
  a.info = d_info;
  a.dim = dim;
  a.k = n_clusters;
  a.trials = n_trials;
  a.max_iter = max_iter;
  a.tol = tol;
  hipLaunchKernelGGL(kmeans_fit_kernel, dim3(n_groups), dim3(kFitThreads), lds, static_cast<hipStream_t>(stream), a);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

extern "C" int mkws_kmeans_nearest(const float* d_x, int dim, int n_rows, const int32_t* d_group, const float* d_centers, int n_groups,
                                   int n_clusters, float* d_dist, int32_t* d_which, int32_t* d_invalid, void* stream) {
  if (n_rows < 0 || n_groups < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (dim < 1) return fail(MKWS_ERR_INVALID_ARG, "dim = %d: at least one column", dim);
  if (n_clusters < 1) return fail(MKWS_ERR_INVALID_ARG, "n_clusters = %d: at least one cluster", n_clusters);
  if (n_rows == 0) return MKWS_OK;     // nothing to read or write: the buffers may be NULL
  if (!d_x || !d_group || (!d_centers && n_groups > 0) || !d_dist || !d_which || !d_invalid) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  if (n_clusters > kMaxClusters) return fail(MKWS_ERR_UNSUPPORTED, "%d clusters: at most %d", n_clusters, kMaxClusters);
  hipStream_t s = static_cast<hipStream_t>(stream);
  MKWS_HIP(hipMemsetAsync(d_invalid, 0, sizeof(int32_t), s));
  const unsigned blocks = (unsigned)(((long long)n_rows + kNearRows - 1) / kNearRows);
  hipLaunchKernelGGL(kmeans_nearest_kernel, dim3(blocks), dim3(kNearThreads), 0, s, d_x, dim, n_rows, d_group, d_centers, n_groups, n_clusters,
                     d_dist, d_which, d_invalid);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}
