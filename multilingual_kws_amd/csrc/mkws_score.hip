// Point scores of classification evaluation (mkws_score_accumulate, include/mkws.h): for n_models classifiers over n_rows shared rows,
// the loss sum, the {rows, correct, ignored, invalid} counters, the confusion matrices and the per-group tallies that Keras'
// model.evaluate and tf.math.confusion_matrix report, accumulated into buffers the caller zeroed once.  multilingual_kws_amd/scoring.py
// (score_host) is the specification.
//
// Two row kernels, chosen by the class count alone, so that a row's loss is the same function of its bits in every batch:
//   classes <= kScoreSmallClasses (32): a workgroup stages its contiguous tile of 256 rows through LDS with coalesced loads (the row
//     stride in LDS is made odd, so the per-thread walks below hit distinct banks), then one thread takes one row.  The confusion matrix
//     is privatised in LDS (classes^2 <= 1024 cells of 32 bits: a workgroup adds at most 256) and only its non-zero cells are flushed.
//   classes  > 32: one wave per row, lanes striding over the classes (coalesced), eight rows per wave; the (value, index) and first-NaN
//     reductions and the sum of exponentials cross the lanes in a fixed xor butterfly; confusion cells go straight to 64-bit atomics in
//     global memory.
// In both, the four counters and (up to kScoreLdsGroups groups) the group tallies are privatised in LDS and flushed once per workgroup.
// Every integer output is a sum of ones: exact, the same on every run and however the rows were cut into calls.
// Row losses are float64 and go to the workspace (0 for a row that is not tallied); a second kernel, one workgroup per model, adds a
// model's rows in an order that depends on n_rows alone (thread t takes rows t, t + 256, ...; then a halving tree over the 256 partial
// sums) and adds the result to d_loss.  No floating-point atomics anywhere: two runs write the same bits.
#include "mkws_common.h"

#include <climits>
#include <cmath>
#include <cstdint>

using mkws::fail;

namespace {

constexpr int kScoreThreads = 256;
constexpr int kScoreSmallClasses = 32;     // at most this many classes: the LDS-staged kernel with the privatised matrix
constexpr int kScoreSmallTile = 256;       // rows of a workgroup there (one per thread)
constexpr int kScoreLargeTile = 32;        // rows of a workgroup of the wave-per-row kernel (4 waves x 8 rows)
constexpr int kScoreLdsGroups = 256;       // at most this many groups: their tallies are privatised in LDS
constexpr int kScoreMaxClasses = MKWS_SCORE_MAX_CLASSES;

typedef unsigned long long u64;

struct ScoreArgs {
  const float* scores;
  const int32_t* labels;
  const int32_t* groups;
  double* work;
  double* loss;
  u64* tally;
  u64* confusion;
  u64* group_tally;
  double* row_loss;
  int32_t* pred;
  int n_models, n_rows, classes, mode, labels_per_model, n_groups, tiles;
};

// Keras' backend clips the probability to [epsilon, 1 - epsilon] in float32 (epsilon = float32 1e-7, 1 - epsilon rounded to float32 =
// 1 - 2^-23) and takes the log; here the log is taken in double of the clipped float32 value.  A NaN probability stays a NaN.
__device__ inline double prob_loss(float p) {
  if (p != p) return (double)NAN;
  const float lo = 1e-7f, hi = 1.0f - 1e-7f;
  const float q = p < lo ? lo : (p > hi ? hi : p);
  return -log((double)q);
}

// 0 = tallied, 1 = ignored (label -1), 2 = invalid (any other label outside [0, classes), or a group outside [0, n_groups))
__device__ inline int row_kind(const ScoreArgs& a, int y, int g) {
  if (y == -1) return 1;
  if ((unsigned)y >= (unsigned)a.classes) return 2;
  if (a.groups && (unsigned)g >= (unsigned)a.n_groups) return 2;
  return 0;
}

// what the lane that owns a row does once the row's prediction and loss are known
__device__ inline void store_row(const ScoreArgs& a, int m, int r, int kind, int y, int g, int pred, double loss, int* s_group,
                                 bool lds_groups) {
  const size_t at = (size_t)m * a.n_rows + r;
  a.work[at] = kind == 0 ? loss : 0.0;
  if (a.row_loss) a.row_loss[at] = kind == 0 ? loss : (double)NAN;
  if (a.pred) a.pred[at] = pred;
  if (kind == 0 && a.groups && a.group_tally) {
    if (lds_groups) {
      atomicAdd(&s_group[2 * g], 1);
      if (pred == y) atomicAdd(&s_group[2 * g + 1], 1);
    } else {
      u64* cell = a.group_tally + ((size_t)m * a.n_groups + g) * 2;
      atomicAdd(cell, (u64)1);
      if (pred == y) atomicAdd(cell + 1, (u64)1);
    }
  }
}

// the four counters of a workgroup: one LDS add per wave and counter, then one global add per non-zero counter
__device__ inline void count_rows(int* s_tally, bool has_row, int kind, bool correct) {
  const int lane = threadIdx.x & 63;
  const bool flags[4] = {has_row && kind == 0, has_row && kind == 0 && correct, has_row && kind == 1, has_row && kind == 2};
  for (int k = 0; k < 4; ++k) {
    const int n = __popcll(__ballot(flags[k]));
    if (lane == 0 && n) atomicAdd(&s_tally[k], n);
  }
}

__device__ inline void flush_counts(const ScoreArgs& a, int m, const int* s_tally, const int* s_group, bool lds_groups) {
  const int tid = threadIdx.x;
  if (tid < 4 && s_tally[tid]) atomicAdd(a.tally + (size_t)m * 4 + tid, (u64)s_tally[tid]);
  if (lds_groups)
    for (int j = tid; j < 2 * a.n_groups; j += kScoreThreads)
      if (s_group[j]) atomicAdd(a.group_tally + (size_t)m * a.n_groups * 2 + j, (u64)s_group[j]);
}

__global__ __launch_bounds__(kScoreThreads) void score_small_kernel(ScoreArgs a) {
  extern __shared__ int s_dyn[];
  __shared__ int s_tally[4];
  const int C = a.classes;
  const int S = C | 1;                                               // odd row stride: thread t's walk over its row stays in its own banks
  float* s_tile = reinterpret_cast<float*>(s_dyn);                   // [kScoreSmallTile, S]
  int* s_conf = s_dyn + kScoreSmallTile * S;                         // [C, C] when the matrix is wanted
  const bool lds_groups = a.groups && a.group_tally && a.n_groups <= kScoreLdsGroups;
  int* s_group = s_conf + (a.confusion ? C * C : 0);                 // [n_groups, 2] when privatised
  const int tid = threadIdx.x;
  const int m = blockIdx.x / a.tiles;
  const int r0 = (blockIdx.x - m * a.tiles) * kScoreSmallTile;
  const int rows = min(kScoreSmallTile, a.n_rows - r0);

  if (tid < 4) s_tally[tid] = 0;
  if (a.confusion)
    for (int j = tid; j < C * C; j += kScoreThreads) s_conf[j] = 0;
  if (lds_groups)
    for (int j = tid; j < 2 * a.n_groups; j += kScoreThreads) s_group[j] = 0;
  // the tile is rows * C contiguous floats: consecutive threads read consecutive floats; (row, column) advance without a division
  {
    const float* __restrict__ src = a.scores + ((size_t)m * a.n_rows + r0) * C;
    const int total = rows * C, dr = kScoreThreads / C, dc = kScoreThreads - dr * C;
    int r = tid / C, c = tid - r * C;
    for (int i = tid; i < total; i += kScoreThreads) {
      s_tile[r * S + c] = src[i];
      r += dr;
      c += dc;
      if (c >= C) {
        c -= C;
        ++r;
      }
    }
  }
  __syncthreads();

  const bool has_row = tid < rows;
  int kind = 0, y = 0, pred = 0;
  if (has_row) {
    const int r = r0 + tid;
    const float* z = s_tile + tid * S;
    // np.argmax: the first index of the maximum; the first NaN wins over everything
    float best = z[0];
    bool nan_seen = best != best;
    for (int c = 1; c < C; ++c) {
      const float v = z[c];
      if (!nan_seen && (v != v || v > best)) {
        best = v;
        pred = c;
        nan_seen = v != v;
      }
    }
    y = a.labels[a.labels_per_model ? (size_t)m * a.n_rows + r : (size_t)r];
    const int g = a.groups ? a.groups[r] : 0;
    kind = row_kind(a, y, g);
    double loss = 0.0;
    if (kind == 0) {
      if (a.mode == 0) {
        loss = prob_loss(z[y]);
      } else if (nan_seen) {
        loss = (double)NAN;
      } else {
        double sum = 0.0;                                            // in index order
        for (int c = 0; c < C; ++c) sum += exp((double)z[c] - (double)best);
        loss = (log(sum) + (double)best) - (double)z[y];
      }
      if (a.confusion) atomicAdd(&s_conf[y * C + pred], 1);
    }
    store_row(a, m, r, kind, y, g, pred, loss, s_group, lds_groups);
  }
  count_rows(s_tally, has_row, kind, pred == y);
  __syncthreads();
  flush_counts(a, m, s_tally, s_group, lds_groups);
  if (a.confusion) {
    u64* __restrict__ out = a.confusion + (size_t)m * C * C;
    for (int j = tid; j < C * C; j += kScoreThreads)
      if (s_conf[j]) atomicAdd(out + j, (u64)s_conf[j]);
  }
}

__global__ __launch_bounds__(kScoreThreads) void score_large_kernel(ScoreArgs a) {
  extern __shared__ int s_dyn[];
  __shared__ int s_tally[4];
  const int C = a.classes;
  const bool lds_groups = a.groups && a.group_tally && a.n_groups <= kScoreLdsGroups;
  int* s_group = s_dyn;                                              // [n_groups, 2] when privatised
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = blockIdx.x / a.tiles;
  const int r0 = (blockIdx.x - m * a.tiles) * kScoreLargeTile;
  const int rows = min(kScoreLargeTile, a.n_rows - r0);

  if (tid < 4) s_tally[tid] = 0;
  if (lds_groups)
    for (int j = tid; j < 2 * a.n_groups; j += kScoreThreads) s_group[j] = 0;
  __syncthreads();

  for (int i = wave; i < rows; i += kScoreThreads / 64) {            // the wave's rows; every value below is uniform across its lanes
    const int r = r0 + i;
    const float* __restrict__ z = a.scores + ((size_t)m * a.n_rows + r) * C;
    // per lane: the first index of its maximum over the non-NaN values it reads, and the first index at which it read a NaN
    float best = -INFINITY;
    int arg = INT_MAX, first_nan = INT_MAX;
    for (int c = lane; c < C; c += 64) {
      const float v = z[c];
      if (v != v) {
        first_nan = min(first_nan, c);
      } else if (v > best || arg == INT_MAX) {
        best = v;
        arg = c;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {                         // xor butterfly: the larger value, among equals the smaller index
      const float ov = __shfl_xor(best, off);
      const int oa = __shfl_xor(arg, off);
      const int on = __shfl_xor(first_nan, off);
      if (oa != INT_MAX && (arg == INT_MAX || ov > best || (ov == best && oa < arg))) {   // INT_MAX: that lane read no number
        best = ov;
        arg = oa;
      }
      first_nan = min(first_nan, on);
    }
    const bool nan_seen = first_nan != INT_MAX;
    const int pred = nan_seen ? first_nan : arg;
    const int y = a.labels[a.labels_per_model ? (size_t)m * a.n_rows + r : (size_t)r];
    const int g = a.groups ? a.groups[r] : 0;
    const int kind = row_kind(a, y, g);
    double loss = 0.0;
    if (kind == 0) {
      if (a.mode == 0) {
        loss = prob_loss(z[y]);
      } else if (nan_seen) {
        loss = (double)NAN;
      } else {
        double sum = 0.0;                                            // the lane's classes in index order, then the butterfly
        for (int c = lane; c < C; c += 64) sum += exp((double)z[c] - (double)best);
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        loss = (log(sum) + (double)best) - (double)z[y];
      }
    }
    if (lane == 0) {
      if (kind == 0 && a.confusion) atomicAdd(a.confusion + ((size_t)m * C + y) * C + pred, (u64)1);
      store_row(a, m, r, kind, y, g, pred, loss, s_group, lds_groups);
      const int which[3] = {0, 2, 3};
      atomicAdd(&s_tally[which[kind]], 1);
      if (kind == 0 && pred == y) atomicAdd(&s_tally[1], 1);
    }
  }
  __syncthreads();
  flush_counts(a, m, s_tally, s_group, lds_groups);
}

// d_loss[m] += the model's row losses, in an order fixed by n_rows
__global__ __launch_bounds__(kScoreThreads) void score_sum_kernel(const double* __restrict__ work, double* __restrict__ loss, int n_rows) {
  __shared__ double s_part[kScoreThreads];
  const int tid = threadIdx.x;
  const double* __restrict__ w = work + (size_t)blockIdx.x * n_rows;
  double acc = 0.0;
  for (int r = tid; r < n_rows; r += kScoreThreads) acc += w[r];
  s_part[tid] = acc;
  __syncthreads();
  for (int off = kScoreThreads / 2; off > 0; off >>= 1) {
    if (tid < off) s_part[tid] += s_part[tid + off];
    __syncthreads();
  }
  if (tid == 0) loss[blockIdx.x] += s_part[0];
}

}  // namespace

extern "C" size_t mkws_score_work_bytes(int n_models, int n_rows) {
  if (n_models <= 0 || n_rows <= 0) return 0;
  return (size_t)n_models * (size_t)n_rows * sizeof(double);
}

extern "C" int mkws_score_accumulate(const float* d_scores, int n_models, int n_rows, int classes, int mode, const int32_t* d_labels,
                                     int labels_per_model, const int32_t* d_groups, int n_groups, double* d_loss, int64_t* d_tally,
                                     int64_t* d_confusion, int64_t* d_group_tally, double* d_row_loss, int32_t* d_pred, void* d_work,
                                     void* stream) {
  if (n_models < 0 || n_rows < 0) return fail(MKWS_ERR_INVALID_ARG, "negative size");
  if (classes < 2) return fail(MKWS_ERR_INVALID_ARG, "classes = %d: at least two classes", classes);
  if (mode != 0 && mode != 1) return fail(MKWS_ERR_INVALID_ARG, "mode %d: 0 (probabilities) or 1 (logits)", mode);
  if (labels_per_model != 0 && labels_per_model != 1) return fail(MKWS_ERR_INVALID_ARG, "labels_per_model %d: 0 (shared) or 1", labels_per_model);
  if (n_groups < 0) return fail(MKWS_ERR_INVALID_ARG, "n_groups = %d", n_groups);
  if (d_groups && n_groups == 0) return fail(MKWS_ERR_INVALID_ARG, "d_groups given with n_groups = 0");
  if (classes > kScoreMaxClasses) return fail(MKWS_ERR_UNSUPPORTED, "%d classes: at most %d", classes, kScoreMaxClasses);
  if (n_models == 0 || n_rows == 0) return MKWS_OK;   // nothing to read, nothing touched: the buffers may be NULL
  if (!d_scores || !d_labels || !d_loss || !d_tally || !d_work) return fail(MKWS_ERR_INVALID_ARG, "NULL buffer");
  const bool small = classes <= kScoreSmallClasses;
  const int tile = small ? kScoreSmallTile : kScoreLargeTile;
  const int tiles = (n_rows + tile - 1) / tile;
  if ((long long)tiles * n_models > INT_MAX) return fail(MKWS_ERR_UNSUPPORTED, "%d models x %d rows: a grid beyond one launch", n_models, n_rows);
  ScoreArgs a;
  a.scores = d_scores;
  a.labels = d_labels;
  a.groups = d_groups;
  a.work = static_cast<double*>(d_work);
  a.loss = d_loss;
  a.tally = reinterpret_cast<u64*>(d_tally);
  a.confusion = reinterpret_cast<u64*>(d_confusion);
  a.group_tally = d_groups ? reinterpret_cast<u64*>(d_group_tally) : nullptr;
  a.row_loss = d_row_loss;
  a.pred = d_pred;
  a.n_models = n_models;
  a.n_rows = n_rows;
  a.classes = classes;
  a.mode = mode;
  a.labels_per_model = labels_per_model;
  a.n_groups = n_groups;
  a.tiles = tiles;
  const size_t lds_groups = (a.group_tally && n_groups <= kScoreLdsGroups) ? (size_t)n_groups * 2 * sizeof(int) : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (small) {
    const size_t lds = (size_t)kScoreSmallTile * (classes | 1) * sizeof(float) + (d_confusion ? (size_t)classes * classes * sizeof(int) : 0) + lds_groups;
    hipLaunchKernelGGL(score_small_kernel, dim3(tiles * n_models), dim3(kScoreThreads), lds, s, a);
  } else {
    hipLaunchKernelGGL(score_large_kernel, dim3(tiles * n_models), dim3(kScoreThreads), lds_groups, s, a);
  }
  MKWS_HIP(hipGetLastError());
  hipLaunchKernelGGL(score_sum_kernel, dim3(n_models), dim3(kScoreThreads), 0, s, static_cast<const double*>(d_work), d_loss, n_rows);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}
