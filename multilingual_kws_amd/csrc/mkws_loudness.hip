// Level normalisation (include/mkws.h, "Loudness and true peak"): the BS.1770 integrated loudness, the 4x oversampled true peak, the sample
// peak and the mean square of every row, and the linear gain that brings a row to its target.
//
// The K-weighting cascade is a linear map on a state of four doubles, s' = A s + B x.  A row is cut into chunks of C samples (C divides
// the hop, so that a chunk never straddles two hops) and a workgroup of 256 lanes owns a TILE of 256 consecutive chunks, lane t chunk t.
//   zero    every lane runs its chunk from the zero state: g_c.  A Kogge-Stone scan with the constant matrices A^C, A^2C .. A^128C gives
//           the tile's end state from zero, G.
//   tiles   one wave per row walks the row's tiles: S_{t+1} = A^256C S_t + G_t, the state every tile really starts from.
//   run     the same scan with S_t fed into chunk 0 gives every chunk its true start state; the lane filters its chunk again and writes
//           the chunk's energy.  The same launch takes the oversampled maximum, the sample peak and the sum of squares of its tile.
//   hops    one lane per (row, hop): chunk energies -> hop sums, in chunk order.
//   finish  one workgroup per row: hop sums -> block means, the two gates, the loudness, the gain, the statistics.
// Every sum and maximum across lanes is a tree of fixed shape; there are no atomics.  The samples of a tile are staged once in LDS as
// float32 (coalesced) with one word of padding after every 32, so that lanes reading at a stride of C words fall on different banks.
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "mkws_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxChunk = 32;                    // C = the largest divisor of the hop that is at most this
constexpr int kScan = 8;                         // log2(kThreads): A^C .. A^128C; entry kScan of the table is A^256C
constexpr int kApplyPerLane = 4;
constexpr size_t kMaxLdsBytes = 64 * 1024;       // dynamic LDS a launch may ask for without an attribute
constexpr double kShelfF0 = 1681.974450955533, kShelfG = 3.999843853973347, kShelfQ = 0.7071752369554196;
constexpr double kHighF0 = 38.13547087602444, kHighQ = 0.5003270373238773;

struct Geometry {
  int64_t hop, block, C, tile, cph;              // cph = chunks per hop
  int zc, T;
};

// c[0..4] = shelf b0 b1 b2 a1 a2, c[5..9] = high-pass b0 b1 b2 a1 a2
void design(int rate, double* c) {
  const double pi = 3.14159265358979323846;
  double K = std::tan(pi * kShelfF0 / (double)rate), Vh = std::pow(10.0, kShelfG / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
  double a0 = 1.0 + K / kShelfQ + K * K;
  c[0] = (Vh + Vb * K / kShelfQ + K * K) / a0;
  c[1] = 2.0 * (K * K - Vh) / a0;
  c[2] = (Vh - Vb * K / kShelfQ + K * K) / a0;
  c[3] = 2.0 * (K * K - 1.0) / a0;
  c[4] = (1.0 - K / kShelfQ + K * K) / a0;
  K = std::tan(pi * kHighF0 / (double)rate);
  a0 = 1.0 + K / kHighQ + K * K;
  c[5] = 1.0;
  c[6] = -2.0;
  c[7] = 1.0;
  c[8] = 2.0 * (K * K - 1.0) / a0;
  c[9] = (1.0 - K / kHighQ + K * K) / a0;
}

int check_cfg(const mkws_loudness_cfg* cfg, Geometry* g) {
  if (!cfg) return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness: NULL cfg");
  if (cfg->rate < 1) return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness: rate = %d (at least 1)", cfg->rate);
  if (cfg->mode != MKWS_LOUDNESS_MODE_LOUDNESS && cfg->mode != MKWS_LOUDNESS_MODE_PEAK)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness: mode = %d (0 = loudness, 1 = peak)", cfg->mode);
  if (!std::isfinite(cfg->target_lufs) || !std::isfinite(cfg->true_peak_db) || !std::isfinite(cfg->headroom_db))
    return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness: target_lufs = %g, true_peak_db = %g, headroom_db = %g (all finite)", cfg->target_lufs,
                      cfg->true_peak_db, cfg->headroom_db);
  if (cfg->zero_crossings < 1) return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness: zero_crossings = %d (at least 1)", cfg->zero_crossings);
  if (cfg->zero_crossings > MKWS_LOUDNESS_MAX_ZERO_CROSSINGS)
    return mkws::fail(MKWS_ERR_UNSUPPORTED, "loudness: zero_crossings = %d (at most %d: one tile and its margins are staged in LDS)", cfg->zero_crossings,
                      MKWS_LOUDNESS_MAX_ZERO_CROSSINGS);
  if (!(cfg->rolloff > 0.0f && cfg->rolloff <= 1.0f)) return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness: rolloff = %g outside (0, 1]", (double)cfg->rolloff);
  if (!(cfg->kaiser_beta >= 0.0f) || !std::isfinite(cfg->kaiser_beta))
    return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness: kaiser_beta = %g (finite, not negative)", (double)cfg->kaiser_beta);
  if (cfg->rate % 10 != 0) return mkws::fail(MKWS_ERR_UNSUPPORTED, "loudness: rate = %d Hz is not a multiple of 10 (the hop is rate / 10 samples)", cfg->rate);
  if ((double)cfg->rate <= 2.0 * kShelfF0)
    return mkws::fail(MKWS_ERR_UNSUPPORTED, "loudness: rate = %d Hz puts the K-weighting shelf (%.0f Hz) at or above Nyquist", cfg->rate, kShelfF0);
  g->hop = cfg->rate / 10;
  g->block = 4 * g->hop;
  g->C = 1;
  for (int64_t d = kMaxChunk; d >= 1; --d)
    if (g->hop % d == 0) {
      g->C = d;
      break;
    }
  g->tile = g->C * kThreads;
  g->cph = g->hop / g->C;
  g->zc = cfg->zero_crossings;
  g->T = 2 * cfg->zero_crossings + 1;
  return MKWS_OK;
}

__host__ __device__ __forceinline__ int phys(int u) { return u + (u >> 5); }

size_t lds_bytes_of(const Geometry& g) { return 4 * kThreads * sizeof(double) + (size_t)(phys((int)g.tile + 2 * g.zc) + 1) * sizeof(float); }

// one sample through the cascade (each biquad in the transposed direct form II, as scipy.signal.lfilter runs it)
__host__ __device__ __forceinline__ double kstep(const double* __restrict__ c, double s[4], double x) {
  double y1 = c[0] * x + s[0];
  s[0] = c[1] * x - c[3] * y1 + s[1];
  s[1] = c[2] * x - c[4] * y1;
  double y2 = c[5] * y1 + s[2];
  s[2] = c[6] * y1 - c[8] * y2 + s[3];
  s[3] = c[7] * y1 - c[9] * y2;
  return y2;
}

void matmul4(const double* a, const double* b, double* o) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double v = 0.0;
      for (int k = 0; k < 4; ++k) v += a[r * 4 + k] * b[k * 4 + c];
      o[r * 4 + c] = v;
    }
}

}  // namespace

struct mkws_loudness {
  mkws_loudness_cfg cfg;
  Geometry g;
  int max_rows;
  int64_t max_samples, max_tiles, max_hops;
  size_t lds;
  char* d_mem;              // everything below, one allocation
  double* d_cst;            // [10] coefficients, then [kScan + 1][16] powers of A^C, row-major
  double* d_tab;            // [T, 4] true-peak taps: the float32 tab[j * 4 + p] of mkws_resample_host_taps(L = 4, M = 1), widened
  double* ws_g;             // [rows, tiles, 4, 256] every chunk's end state from zero
  double* ws_G;             // [rows, tiles, 4] every tile's end state from zero
  double* ws_S;             // [rows, tiles, 4] every tile's start state
  double* ws_e;             // [rows, tiles * 256] chunk energies
  double* ws_hop;           // [rows, hops] hop energies
  double* ws_tile;          // [rows, tiles, 3] true peak, sample peak, sum of squares
};

namespace {

template <bool I16>
__device__ __forceinline__ float load_sample(const void* p, int64_t i) {
  if (I16) return (float)((const int16_t*)p)[i] / 32768.0f;
  return ((const float*)p)[i];
}

template <bool I16>
__device__ __forceinline__ const void* row_of(const void* in, int64_t b, int64_t stride) {
  return I16 ? (const void*)((const int16_t*)in + b * stride) : (const void*)((const float*)in + b * stride);
}

__device__ __forceinline__ int64_t row_len(const int64_t* __restrict__ lengths, int64_t b, int64_t n) {
  int64_t len = lengths ? lengths[b] : n;
  return len < 0 ? 0 : (len > n ? n : len);
}

// xs[phys(u)] = x[first + u] for u < count, zero outside [0, len): nothing beyond the row's own length is read
template <bool I16>
__device__ __forceinline__ void stage(float* xs, const void* row, int64_t first, int count, int64_t len) {
  for (int u = threadIdx.x; u < count; u += kThreads) {
    int64_t gi = first + u;
    xs[phys(u)] = (gi >= 0 && gi < len) ? load_sample<I16>(row, gi) : 0.0f;
  }
}

__device__ __forceinline__ void matvec_add(const double* __restrict__ m, const double u[4], double v[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] += (m[r * 4 + 0] * u[0] + m[r * 4 + 1] * u[1]) + (m[r * 4 + 2] * u[2] + m[r * 4 + 3] * u[3]);
}

// v_k <- sum_{i <= k} (A^C)^(k - i) v_i over the 256 lanes; sb: [4][256] doubles; mp: the table of powers.  Fixed shape, fixed order.
__device__ __forceinline__ void tile_scan(double* sb, const double* __restrict__ mp, double v[4]) {
  const int t = threadIdx.x;
  for (int d = 0; d < kScan; ++d) {
#pragma unroll
    for (int c = 0; c < 4; ++c) sb[c * kThreads + t] = v[c];
    __syncthreads();
    const int off = 1 << d;
    if (t >= off) {
      double u[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) u[c] = sb[c * kThreads + t - off];
      matvec_add(mp + d * 16, u, v);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ double wg_sum(double* sb, double v) {
  const int t = threadIdx.x;
  sb[t] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) sb[t] = sb[t] + sb[t + s];
    __syncthreads();
  }
  double r = sb[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ double wg_max(double* sb, double v) {
  const int t = threadIdx.x;
  sb[t] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) sb[t] = fmax(sb[t], sb[t + s]);
    __syncthreads();
  }
  double r = sb[0];
  __syncthreads();
  return r;
}

struct Call {
  const void* in;
  const int64_t* lengths;
  int64_t n, in_stride;
  uint32_t tiles;
  int C, zc, T;
};

template <bool I16>
__global__ __launch_bounds__(kThreads) void loud_zero_kernel(Call a, const double* __restrict__ cst, double* __restrict__ ws_g,
                                                             double* __restrict__ ws_G) {
  extern __shared__ double lds_d[];
  double* sb = lds_d;
  float* xs = (float*)(lds_d + 4 * kThreads);
  const uint32_t b = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int t = threadIdx.x;
  const int64_t len = row_len(a.lengths, b, a.n), t0 = (int64_t)tile * a.C * kThreads;
  if (t0 >= len) return;
  stage<I16>(xs, row_of<I16>(a.in, b, a.in_stride), t0, a.C * kThreads, len);
  __syncthreads();
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const int u0 = t * a.C;
  for (int k = 0; k < a.C; ++k) (void)kstep(cst, s, (double)xs[phys(u0 + k)]);
  const size_t at = (size_t)b * a.tiles + tile;
#pragma unroll
  for (int c = 0; c < 4; ++c) ws_g[(at * 4 + c) * kThreads + t] = s[c];
  tile_scan(sb, cst + 10, s);
  if (t == kThreads - 1) {
#pragma unroll
    for (int c = 0; c < 4; ++c) ws_G[at * 4 + c] = s[c];
  }
}

// One wave per row: the start state of every tile that holds samples.  The lanes load 64 tiles' end states at once; every lane then walks
// them in order (the state of tile k read from lane k), all 64 computing the same state, and lane k keeps the one tile k starts from.
__global__ __launch_bounds__(64) void loud_tiles_kernel(int64_t n, const int64_t* __restrict__ lengths, uint32_t tiles, int64_t tile_samples,
                                                        const double* __restrict__ cst, const double* __restrict__ ws_G,
                                                        double* __restrict__ ws_S) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t len = row_len(lengths, b, n);
  const int64_t used = (len + tile_samples - 1) / tile_samples;        // <= tiles
  const double* m = cst + 10 + kScan * 16;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t base = 0; base < used; base += 64) {
    const int64_t t = base + lane;
    const size_t at = ((size_t)b * tiles + (size_t)(t < used ? t : base)) * 4;
    double g[4], mine[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; ++c) g[c] = ws_G[at + c];
    const int cnt = (int)(used - base < 64 ? used - base : 64);          // the same for every lane
    for (int k = 0; k < cnt; ++k) {
      double v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (lane == k) mine[c] = s[c];
        v[c] = __shfl(g[c], k);
      }
      matvec_add(m, s, v);
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] = v[c];
    }
    if (t < used) {
#pragma unroll
      for (int c = 0; c < 4; ++c) ws_S[at + c] = mine[c];
    }
  }
}

// one lane per (row, hop): the hop's energy from its chunks, in chunk order
__global__ __launch_bounds__(kThreads) void loud_hops_kernel(int64_t total, int64_t hops_n, int64_t n, const int64_t* __restrict__ lengths, int64_t hop,
                                                            int64_t cph, uint32_t tiles, int64_t hop_cap, const double* __restrict__ ws_e,
                                                            double* __restrict__ ws_hop) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / hops_n, h = i % hops_n;
  if (h >= row_len(lengths, b, n) / hop) return;
  const double* e = ws_e + (size_t)b * tiles * kThreads + h * cph;
  double v = 0.0;
  for (int64_t k = 0; k < cph; ++k) v += e[k];
  ws_hop[(size_t)b * hop_cap + h] = v;
}

template <bool I16>
__global__ __launch_bounds__(kThreads) void loud_run_kernel(Call a, const double* __restrict__ cst, const double* __restrict__ tab,
                                                            const double* __restrict__ ws_g, const double* __restrict__ ws_S,
                                                            double* __restrict__ ws_e, double* __restrict__ ws_tile) {
  extern __shared__ double lds_d[];
  double* sb = lds_d;
  float* xs = (float*)(lds_d + 4 * kThreads);
  const uint32_t b = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int t = threadIdx.x;
  const int tile_samples = a.C * kThreads;
  const int64_t len = row_len(a.lengths, b, a.n), t0 = (int64_t)tile * tile_samples;
  if (t0 >= len) return;
  stage<I16>(xs, row_of<I16>(a.in, b, a.in_stride), t0 - a.zc, tile_samples + 2 * a.zc, len);
  const size_t at = (size_t)b * a.tiles + tile;
  // every chunk's true start state: the scan of the zero-start end states with the tile's start state fed into chunk 0
  double S[4], v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    S[c] = ws_S[at * 4 + c];
    v[c] = ws_g[(at * 4 + c) * kThreads + t];
  }
  if (t == 0) matvec_add(cst + 10, S, v);
  tile_scan(sb, cst + 10, v);                      // (its first barrier also covers the staging)
#pragma unroll
  for (int c = 0; c < 4; ++c) sb[c * kThreads + t] = v[c];
  __syncthreads();
  double s[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) s[c] = t == 0 ? S[c] : sb[c * kThreads + t - 1];
  __syncthreads();
  const int64_t left = len - t0;                    // samples of the row in this tile and beyond: >= 1
  const int valid = (int)(left < tile_samples ? left : tile_samples);
  {
    const int u0 = t * a.C;
    int mine = valid - u0;
    mine = mine < 0 ? 0 : (mine > a.C ? a.C : mine);
    double e = 0.0;
    for (int k = 0; k < mine; ++k) {
      double y = kstep(cst, s, (double)xs[phys(a.zc + u0 + k)]);
      e += y * y;
    }
    ws_e[at * kThreads + t] = e;
  }
  // the unweighted row: 4x oversampled maximum (float32 taps and samples; every product is exact in float64 and the sums are float64, j
  // ascending, so that the gain of a peak-limited row carries no float32 rounding of its true peak), sample peak, squares
  double tp = 0.0;
  float sp = 0.0f;
  double sq = 0.0;
  for (int r = 0; r < a.C; r += 2) {
    const int w0 = t + r * kThreads, w1 = r + 1 < a.C ? w0 + kThreads : w0;
    double acc0[4] = {0.0, 0.0, 0.0, 0.0}, acc1[4] = {0.0, 0.0, 0.0, 0.0};
    const int base0 = w0 + 2 * a.zc, base1 = w1 + 2 * a.zc;
    for (int j = 0; j < a.T; ++j) {
      const double4 h = *(const double4*)(tab + 4 * j);
      const double x0 = (double)xs[phys(base0 - j)], x1 = (double)xs[phys(base1 - j)];
      acc0[0] += h.x * x0;
      acc0[1] += h.y * x0;
      acc0[2] += h.z * x0;
      acc0[3] += h.w * x0;
      acc1[0] += h.x * x1;
      acc1[1] += h.y * x1;
      acc1[2] += h.z * x1;
      acc1[3] += h.w * x1;
    }
    if (w0 < valid) {
      const float x = xs[phys(a.zc + w0)];
      tp = fmax(tp, fmax(fmax(fabs(acc0[0]), fabs(acc0[1])), fmax(fabs(acc0[2]), fabs(acc0[3]))));
      sp = fmaxf(sp, fabsf(x));
      sq += (double)x * (double)x;
    }
    if (w1 != w0 && w1 < valid) {
      const float x = xs[phys(a.zc + w1)];
      tp = fmax(tp, fmax(fmax(fabs(acc1[0]), fabs(acc1[1])), fmax(fabs(acc1[2]), fabs(acc1[3]))));
      sp = fmaxf(sp, fabsf(x));
      sq += (double)x * (double)x;
    }
  }
  const double tpm = wg_max(sb, tp), spm = wg_max(sb, (double)sp), sqs = wg_sum(sb, sq);
  if (t == 0) {
    ws_tile[at * 3 + 0] = tpm;
    ws_tile[at * 3 + 1] = spm;
    ws_tile[at * 3 + 2] = sqs;
  }
}

struct Finish {
  const int64_t* lengths;
  int64_t n, hop, cph, tile_samples, hop_cap;
  uint32_t tiles;
  int mode;
  double target, tp_limit, headroom;
};

__global__ __launch_bounds__(kThreads) void loud_finish_kernel(Finish f, const double* __restrict__ ws_hop,
                                                               const double* __restrict__ ws_tile, double* __restrict__ stats,
                                                               int32_t* __restrict__ counts, float* __restrict__ gain) {
  __shared__ double sb[kThreads];
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t len = row_len(f.lengths, b, f.n);
  const int64_t hops = len / f.hop, used = (len + f.tile_samples - 1) / f.tile_samples;
  const int64_t nb = hops >= 4 ? hops - 3 : 0;
  const double* hs = ws_hop + (size_t)b * f.hop_cap;
  const double inv_block = 1.0 / (double)(4 * f.hop);
  double sa = 0.0, ca = 0.0;
  for (int64_t j = t; j < nb; j += kThreads) {
    const double z = (((hs[j] + hs[j + 1]) + hs[j + 2]) + hs[j + 3]) * inv_block;
    if (-0.691 + 10.0 * log10(z) > -70.0) {
      sa += z;
      ca += 1.0;
    }
  }
  sa = wg_sum(sb, sa);
  ca = wg_sum(sb, ca);
  double L = -INFINITY, cr = 0.0;
  if (ca > 0.0) {
    const double rel = -0.691 + 10.0 * log10(sa / ca) - 10.0;
    double sr = 0.0;
    for (int64_t j = t; j < nb; j += kThreads) {
      const double z = (((hs[j] + hs[j + 1]) + hs[j + 2]) + hs[j + 3]) * inv_block;
      const double l = -0.691 + 10.0 * log10(z);
      if (l > -70.0 && l > rel) {
        sr += z;
        cr += 1.0;
      }
    }
    sr = wg_sum(sb, sr);
    cr = wg_sum(sb, cr);
    if (cr > 0.0) L = -0.691 + 10.0 * log10(sr / cr);
  }
  const double* tl = ws_tile + (size_t)b * f.tiles * 3;
  double tp = 0.0, sp = 0.0, sq = 0.0;
  for (int64_t i = t; i < used; i += kThreads) {
    tp = fmax(tp, tl[i * 3 + 0]);
    sp = fmax(sp, tl[i * 3 + 1]);
    sq += tl[i * 3 + 2];
  }
  tp = wg_max(sb, tp);
  sp = wg_max(sb, sp);
  sq = wg_sum(sb, sq);
  if (t != 0) return;
  int flags = 0;
  float g = 1.0f;
  if (f.mode == MKWS_LOUDNESS_MODE_PEAK) {
    if (sp > 0.0)
      g = (float)(pow(10.0, -f.headroom / 20.0) / sp);
    else
      flags |= MKWS_LOUDNESS_FLAG_UNMEASURED;
  } else if (L == -INFINITY) {
    flags |= MKWS_LOUDNESS_FLAG_UNMEASURED;
  } else {
    double g_db = f.target - L;
    const double tp_db = 20.0 * log10(tp);
    if (tp_db + g_db > f.tp_limit) {
      g_db = f.tp_limit - tp_db;
      flags |= MKWS_LOUDNESS_FLAG_PEAK_LIMITED;
    }
    g = (float)pow(10.0, g_db / 20.0);
  }
  stats[(size_t)b * 4 + 0] = L;
  stats[(size_t)b * 4 + 1] = tp;
  stats[(size_t)b * 4 + 2] = sp;
  stats[(size_t)b * 4 + 3] = len > 0 ? sq / (double)len : 0.0;
  counts[(size_t)b * 4 + 0] = (int32_t)nb;
  counts[(size_t)b * 4 + 1] = (int32_t)ca;
  counts[(size_t)b * 4 + 2] = (int32_t)cr;
  counts[(size_t)b * 4 + 3] = flags;
  gain[b] = g;
}

template <bool I16>
__global__ __launch_bounds__(kThreads) void loud_apply_kernel(const void* __restrict__ in, int64_t n, int64_t in_stride,
                                                              const int64_t* __restrict__ lengths, const float* __restrict__ gain,
                                                              float* __restrict__ out, int64_t out_stride, uint32_t tiles) {
  const uint32_t b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int64_t len = row_len(lengths, b, n);
  const void* row = row_of<I16>(in, b, in_stride);
  float* orow = out + (int64_t)b * out_stride;
  const float g = gain[b];
#pragma unroll
  for (int i = 0; i < kApplyPerLane; ++i) {
    const int64_t k = ((int64_t)tile * kApplyPerLane + i) * kThreads + threadIdx.x;
    if (k < n) orow[k] = k < len ? __fmul_rn(load_sample<I16>(row, k), g) : 0.0f;
  }
}

int check_call(const char* who, const mkws_loudness* h, const void* d_in, int B, int64_t n, int64_t in_stride) {
  if (!h) return mkws::fail(MKWS_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (B < 0 || n < 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "%s: B = %d, n = %lld", who, B, (long long)n);
  if (B > h->max_rows || n > h->max_samples)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "%s: %d rows of %lld samples, the handle was created for %d rows of %lld", who, B, (long long)n,
                      h->max_rows, (long long)h->max_samples);
  if (B > 0 && n > 0 && !d_in) return mkws::fail(MKWS_ERR_INVALID_ARG, "%s: NULL buffer", who);
  if (B > 1 && in_stride < n) return mkws::fail(MKWS_ERR_INVALID_ARG, "%s: a row stride of %lld shorter than the rows (%lld)", who, (long long)in_stride, (long long)n);
  return MKWS_OK;
}

}  // namespace

extern "C" {

void mkws_loudness_default_cfg(mkws_loudness_cfg* cfg, int rate) {
  if (!cfg) return;
  cfg->rate = rate;
  cfg->mode = MKWS_LOUDNESS_MODE_LOUDNESS;
  cfg->target_lufs = -16.0;
  cfg->true_peak_db = -1.5;
  cfg->headroom_db = 0.1;
  cfg->zero_crossings = 32;
  cfg->kaiser_beta = 9.0f;
  cfg->rolloff = 0.95f;
}

int mkws_loudness_coeffs(const mkws_loudness_cfg* cfg, double out[10]) {
  if (!out) return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness_coeffs: NULL out");
  Geometry g;
  int rc = check_cfg(cfg, &g);
  if (rc != MKWS_OK) return rc;
  design(cfg->rate, out);
  return MKWS_OK;
}

int mkws_loudness_geometry(const mkws_loudness_cfg* cfg, int32_t out[4]) {
  if (!out) return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness_geometry: NULL out");
  Geometry g;
  int rc = check_cfg(cfg, &g);
  if (rc != MKWS_OK) return rc;
  out[0] = (int32_t)g.hop;
  out[1] = (int32_t)g.block;
  out[2] = (int32_t)g.C;
  out[3] = (int32_t)g.tile;
  return MKWS_OK;
}

int mkws_loudness_create(const mkws_loudness_cfg* cfg, int max_rows, int64_t max_samples, mkws_loudness** out) {
  if (!out) return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness_create: NULL out");
  *out = nullptr;
  Geometry g;
  int rc = check_cfg(cfg, &g);
  if (rc != MKWS_OK) return rc;
  if (max_rows < 1 || max_samples < 1)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness_create: max_rows = %d, max_samples = %lld (at least 1 each)", max_rows, (long long)max_samples);
  if (lds_bytes_of(g) > kMaxLdsBytes)
    return mkws::fail(MKWS_ERR_UNSUPPORTED, "loudness: zero_crossings = %d: one tile and its margins do not fit the LDS", g.zc);
  // sizes in doubles per row; refuse on the factors first, so that nothing below can overflow
  const int64_t kMaxSamples = (int64_t)1 << 40;
  int64_t tiles = max_samples <= kMaxSamples ? (max_samples + g.tile - 1) / g.tile : 0, hops = max_samples <= kMaxSamples ? max_samples / g.hop + 1 : 0;
  int64_t per_row = tiles * (4 * kThreads + 4 + 4 + kThreads + 3) + hops;
  size_t fixed = (10 + (kScan + 1) * 16) * sizeof(double) + (size_t)g.T * 4 * sizeof(double) + 64;
  if (tiles == 0 || tiles * (int64_t)max_rows > 0x7fffffffLL || per_row > MKWS_LOUDNESS_MAX_WORKSPACE_BYTES / 8 / max_rows)
    return mkws::fail(MKWS_ERR_UNSUPPORTED, "loudness_create: the workspace for %d rows of %lld samples exceeds %lld bytes", max_rows,
                      (long long)max_samples, (long long)MKWS_LOUDNESS_MAX_WORKSPACE_BYTES);
  rc = mkws::require_device();
  if (rc != MKWS_OK) return rc;
  std::vector<double> cst(10 + (kScan + 1) * 16);
  design(cfg->rate, cst.data());
  double* mp = cst.data() + 10;
  for (int col = 0; col < 4; ++col) {                 // column col of A^C: C silent samples from the unit state
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[col] = 1.0;
    for (int64_t k = 0; k < g.C; ++k) (void)kstep(cst.data(), s, 0.0);
    for (int r = 0; r < 4; ++r) mp[r * 4 + col] = s[r];
  }
  for (int d = 1; d <= kScan; ++d) matmul4(mp + (d - 1) * 16, mp + (d - 1) * 16, mp + d * 16);
  std::vector<float> tab((size_t)g.T * 4);
  mkws_resample_cfg rcfg = {1, 4, cfg->zero_crossings, cfg->kaiser_beta, cfg->rolloff};
  if (mkws_resample_host_taps(&rcfg, tab.data(), tab.size()) != g.T * 4) return mkws::fail(MKWS_ERR_UNSUPPORTED, "loudness_create: the true-peak table");
  std::vector<double> tabd(tab.begin(), tab.end());
  mkws_loudness* h = new (std::nothrow) mkws_loudness();
  if (!h) return mkws::fail(MKWS_ERR_ALLOC, "loudness_create: out of host memory");
  h->cfg = *cfg;
  h->g = g;
  h->max_rows = max_rows;
  h->max_samples = max_samples;
  h->max_tiles = tiles;
  h->max_hops = hops;
  h->lds = lds_bytes_of(g);
  h->d_mem = nullptr;
  size_t bytes = fixed + (size_t)per_row * (size_t)max_rows * sizeof(double);
  if (hipMalloc((void**)&h->d_mem, bytes) != hipSuccess) {
    (void)hipGetLastError();
    delete h;
    return mkws::fail(MKWS_ERR_ALLOC, "loudness_create: hipMalloc of %zu bytes failed", bytes);
  }
  const size_t R = (size_t)max_rows, Tn = (size_t)tiles;
  double* p = (double*)h->d_mem;
  h->d_cst = p;
  p += cst.size();
  h->ws_g = p;
  p += R * Tn * 4 * kThreads;
  h->ws_G = p;
  p += R * Tn * 4;
  h->ws_S = p;
  p += R * Tn * 4;
  h->ws_e = p;
  p += R * Tn * kThreads;
  h->ws_hop = p;
  p += R * (size_t)hops;
  h->ws_tile = p;
  p += R * Tn * 3;
  h->d_tab = (double*)(((uintptr_t)p + 31) & ~(uintptr_t)31);
  if (hipMemcpy(h->d_cst, cst.data(), cst.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->d_tab, tabd.data(), tabd.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(h->d_mem);
    delete h;
    return mkws::fail(MKWS_ERR_HIP, "loudness_create: upload of the tables failed");
  }
  *out = h;
  return MKWS_OK;
}

void mkws_loudness_destroy(mkws_loudness* h) {
  if (!h) return;
  if (h->d_mem) (void)hipFree(h->d_mem);
  delete h;
}

int mkws_loudness_measure(mkws_loudness* h, const void* d_in, int in_i16, int B, int64_t n, int64_t in_stride, const int64_t* d_lengths,
                          double* d_stats, int32_t* d_counts, float* d_gain, void* stream) {
  int rc = check_call("loudness_measure", h, d_in, B, n, in_stride);
  if (rc != MKWS_OK) return rc;
  if (B == 0) return MKWS_OK;
  if (!d_stats || !d_counts || !d_gain) return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness_measure: NULL output");
  const Geometry& g = h->g;
  hipStream_t st = (hipStream_t)stream;
  const int64_t tiles = (n + g.tile - 1) / g.tile;                      // <= max_tiles, and tiles * B fits a launch (create)
  if (tiles > 0) {
    Call a = {d_in, d_lengths, n, in_stride, (uint32_t)tiles, (int)g.C, g.zc, g.T};
    dim3 grid((uint32_t)(tiles * B)), block(kThreads);
    if (in_i16)
      hipLaunchKernelGGL((loud_zero_kernel<true>), grid, block, h->lds, st, a, h->d_cst, h->ws_g, h->ws_G);
    else
      hipLaunchKernelGGL((loud_zero_kernel<false>), grid, block, h->lds, st, a, h->d_cst, h->ws_g, h->ws_G);
    MKWS_HIP(hipGetLastError());
    hipLaunchKernelGGL(loud_tiles_kernel, dim3((uint32_t)B), dim3(64), 0, st, n, d_lengths, (uint32_t)tiles, g.tile, h->d_cst, h->ws_G,
                       h->ws_S);
    MKWS_HIP(hipGetLastError());
    if (in_i16)
      hipLaunchKernelGGL((loud_run_kernel<true>), grid, block, h->lds, st, a, h->d_cst, h->d_tab, h->ws_g, h->ws_S, h->ws_e, h->ws_tile);
    else
      hipLaunchKernelGGL((loud_run_kernel<false>), grid, block, h->lds, st, a, h->d_cst, h->d_tab, h->ws_g, h->ws_S, h->ws_e, h->ws_tile);
    MKWS_HIP(hipGetLastError());
  }
  Finish f = {d_lengths, n, g.hop, g.cph, g.tile, h->max_hops, (uint32_t)tiles, h->cfg.mode, h->cfg.target_lufs, h->cfg.true_peak_db, h->cfg.headroom_db};
  const int64_t hops_n = n / g.hop, total = hops_n * B;                 // hops_n <= max_hops, total / 256 fits a launch (create)
  if (total > 0) {
    hipLaunchKernelGGL(loud_hops_kernel, dim3((uint32_t)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, total, hops_n, n, d_lengths, g.hop,
                       g.cph, (uint32_t)tiles, h->max_hops, h->ws_e, h->ws_hop);
    MKWS_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(loud_finish_kernel, dim3((uint32_t)B), dim3(kThreads), 0, st, f, h->ws_hop, h->ws_tile, d_stats, d_counts, d_gain);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

int mkws_loudness_apply(mkws_loudness* h, const void* d_in, int in_i16, int B, int64_t n, int64_t in_stride, const int64_t* d_lengths,
                        const float* d_gain, float* d_out, int64_t out_stride, void* stream) {
  int rc = check_call("loudness_apply", h, d_in, B, n, in_stride);
  if (rc != MKWS_OK) return rc;
  if (B == 0 || n == 0) return MKWS_OK;
  if (!d_gain || !d_out) return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness_apply: NULL buffer");
  if (B > 1 && out_stride < n) return mkws::fail(MKWS_ERR_INVALID_ARG, "loudness_apply: an output stride of %lld shorter than the rows (%lld)", (long long)out_stride, (long long)n);
  const int64_t per = (int64_t)kThreads * kApplyPerLane, tiles = (n + per - 1) / per;
  if (tiles * B > 0x7fffffffLL) return mkws::fail(MKWS_ERR_UNSUPPORTED, "loudness_apply: %lld tiles x %d rows exceed one launch", (long long)tiles, B);
  dim3 grid((uint32_t)(tiles * B)), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (in_i16)
    hipLaunchKernelGGL((loud_apply_kernel<true>), grid, block, 0, st, d_in, n, in_stride, d_lengths, d_gain, d_out, out_stride, (uint32_t)tiles);
  else
    hipLaunchKernelGGL((loud_apply_kernel<false>), grid, block, 0, st, d_in, n, in_stride, d_lengths, d_gain, d_out, out_stride, (uint32_t)tiles);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

}  // extern "C"
