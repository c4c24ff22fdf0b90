// Sample-rate conversion in front of the frontend (include/mkws.h, "Sample-rate conversion"): the filter design on the host in double,
// a stateless batch kernel and a live kernel whose per-stream state lives in a device block of the caller's.
//
// Both kernels share one tile routine.  A workgroup of 256 lanes produces kTile = 1024 consecutive outputs, lane t the outputs
// t, t + 256, t + 512, t + 768 of the tile: four independent add chains per lane (the summation order is fixed and unfused, so a single
// chain would wait for every add), and neighbouring lanes store neighbouring outputs.  The input span [q_first - T + 1, q_last] of the
// tile is staged in LDS once (zero-filled outside the row; the live kernel reads below the push from the state's history); neighbouring
// lanes read it at a stride of M / L samples.  The device table is arranged by phase ORDER, not by phase: entry r of a tap row holds
// phase (r * M) mod L, so that output n reads entry (n + const) mod L and neighbouring lanes read neighbouring floats of the row; with
// L == 1 the tap is the same for every lane and the load is uniform.
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "mkws_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 4;
constexpr int kTile = kThreads * kPerLane;
constexpr size_t kMaxLdsBytes = 64 * 1024;       // dynamic LDS a launch may ask for without an attribute

struct Geometry {
  int64_t L, M, T, half;
};

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

int geometry_of(const mkws_resample_cfg* cfg, Geometry* g) {
  if (!cfg) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample: NULL cfg");
  if (cfg->rate_in < 1 || cfg->rate_out < 1) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample: rates %d -> %d (at least 1)", cfg->rate_in, cfg->rate_out);
  if (cfg->zero_crossings < 1) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample: zero_crossings = %d (at least 1)", cfg->zero_crossings);
  if (!(cfg->rolloff > 0.0f && cfg->rolloff <= 1.0f)) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample: rolloff = %g outside (0, 1]", (double)cfg->rolloff);
  if (!(cfg->kaiser_beta >= 0.0f) || !std::isfinite(cfg->kaiser_beta))
    return mkws::fail(MKWS_ERR_INVALID_ARG, "resample: kaiser_beta = %g (finite, not negative)", (double)cfg->kaiser_beta);
  int64_t d = gcd64(cfg->rate_in, cfg->rate_out);
  g->L = cfg->rate_out / d;
  g->M = cfg->rate_in / d;
  int64_t big = g->L > g->M ? g->L : g->M;
  // T * L >= 2 * zero_crossings * big + 1: refuse on the factors first, so that nothing below can overflow
  bool fits = big <= MKWS_RESAMPLE_MAX_TABLE_FLOATS && cfg->zero_crossings <= MKWS_RESAMPLE_MAX_TABLE_FLOATS;
  g->half = fits ? (int64_t)cfg->zero_crossings * big : 0;
  g->T = (2 * g->half + 1 + g->L - 1) / g->L;
  if (!fits || g->T * g->L > MKWS_RESAMPLE_MAX_TABLE_FLOATS)
    return mkws::fail(MKWS_ERR_UNSUPPORTED, "resample: %d -> %d Hz needs a table of %lld floats (limit %d)", cfg->rate_in, cfg->rate_out,
                      fits ? (long long)(g->T * g->L) : -1LL, MKWS_RESAMPLE_MAX_TABLE_FLOATS);
  return MKWS_OK;
}

// I0 by its power series: every term is positive, so the sum is good to a few ulp for any beta a window uses.
double bessel_i0(double x) {
  double q = 0.25 * x * x, term = 1.0, sum = 1.0;
  for (int k = 1; k < 1000; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-20 * sum) break;
  }
  return sum;
}

// tab[j * L + p] = (float) h[p + j * L]
void build_taps(const mkws_resample_cfg* cfg, const Geometry& g, float* tab) {
  const double pi = 3.14159265358979323846;
  int64_t big = g.L > g.M ? g.L : g.M;
  double fc = (double)cfg->rolloff / (double)big, beta = (double)cfg->kaiser_beta, i0b = bessel_i0(beta);
  for (int64_t k = 0; k < g.T * g.L; ++k) {
    if (k > 2 * g.half) {
      tab[k] = 0.0f;
      continue;
    }
    double i = (double)(k - g.half), x = pi * fc * i;
    double sinc = (k == g.half) ? 1.0 : std::sin(x) / x;
    double r = i / (double)g.half, a = 1.0 - r * r;
    double win = bessel_i0(beta * std::sqrt(a > 0.0 ? a : 0.0)) / i0b;
    tab[k] = (float)((double)g.L * fc * sinc * win);
  }
}

int64_t span_max_of(const Geometry& g) { return ((g.L - 1) + (int64_t)(kTile - 1) * g.M) / g.L + g.T; }

}  // namespace

struct mkws_resample {
  mkws_resample_cfg cfg;
  Geometry g;
  int64_t roff_centred;     // (half * M^-1) mod L: the phase-order index of output 0 of the centred form (the causal form's is 0)
  int64_t span_max;         // floats of LDS one tile's input span can need
  float* d_tab;             // [T, L] by phase order
};

namespace {

template <bool I16>
__device__ __forceinline__ float load_sample(const void* p, int64_t i) {
  if (I16) return (float)((const int16_t*)p)[i] / 32768.0f;
  return ((const float*)p)[i];
}

// The kPerLane outputs of this lane from the staged span: lds[i] = x[q0 - (T - 1) + i], q0 = m0 div L, p0 = m0 mod L for the tile's first
// output, r0 its phase-order index.  Every index stays inside the span, also for outputs past the end of the row (they are not stored).
template <bool L1>
__device__ __forceinline__ void tile_outputs(const float* __restrict__ tab, const float* lds, uint32_t L, uint32_t M, int T, uint32_t p0,
                                             uint32_t r0, float acc[kPerLane]) {
  uint32_t at[kPerLane], r[kPerLane];
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) {
    uint32_t dn = threadIdx.x + i * kThreads;
    at[i] = (L1 ? p0 + dn * M : (p0 + dn * M) / L) + (uint32_t)(T - 1);
    r[i] = L1 ? 0u : (r0 + dn) % L;
    acc[i] = 0.0f;
  }
  const float* row = tab;
  for (int j = 0; j < T; ++j, row += L) {
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(row[r[i]], lds[at[i] - j]));
  }
}

template <bool L1, bool I16>
__global__ __launch_bounds__(kThreads) void resample_batch_kernel(const float* __restrict__ tab, uint32_t L, uint32_t M, int T, int64_t off,
                                                                  uint32_t roff, const void* __restrict__ in, int64_t n_in, int64_t in_stride,
                                                                  float* __restrict__ out, int64_t n_out, int64_t out_stride, uint32_t tiles) {
  extern __shared__ float lds[];
  const uint32_t b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int64_t n0 = (int64_t)tile * kTile, m0 = n0 * (int64_t)M + off;
  const int64_t q0 = m0 / (int64_t)L;
  const uint32_t p0 = (uint32_t)(m0 % (int64_t)L), r0 = (uint32_t)((n0 + roff) % (int64_t)L);
  const void* row = I16 ? (const void*)((const int16_t*)in + (int64_t)b * in_stride) : (const void*)((const float*)in + (int64_t)b * in_stride);
  const int64_t lo = q0 - (T - 1);
  const int span = (int)((p0 + (uint32_t)(kTile - 1) * M) / L) + T;
  for (int i = threadIdx.x; i < span; i += kThreads) {
    int64_t gidx = lo + i;
    lds[i] = (gidx >= 0 && gidx < n_in) ? load_sample<I16>(row, gidx) : 0.0f;
  }
  __syncthreads();
  float acc[kPerLane];
  tile_outputs<L1>(tab, lds, L, M, T, p0, r0, acc);
  float* orow = out + (int64_t)b * out_stride;
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) {
    int64_t n = n0 + threadIdx.x + i * kThreads;
    if (n < n_out) orow[n] = acc[i];
  }
}

// One workgroup per stream: it stages the new history in LDS first, reads the old history while it produces the push's outputs, and
// writes the new history behind a barrier -- nothing else touches this stream's block.
template <bool L1, bool I16>
__global__ __launch_bounds__(kThreads) void resample_live_kernel(const float* __restrict__ tab, uint32_t L, uint32_t M, int T, char* states,
                                                                 size_t state_stride, const int32_t* __restrict__ active, const void* in,
                                                                 int in_samples, float* out, int out_samples, int span_max) {
  extern __shared__ float lds[];
  const int s = blockIdx.x;
  if (active && active[s] == 0) return;
  char* st = states + (size_t)s * state_stride;
  float* hist = (float*)(st + 8);
  const void* row = I16 ? (const void*)((const int16_t*)in + (int64_t)s * in_samples) : (const void*)((const float*)in + (int64_t)s * in_samples);
  const int H = T - 1;
  float* fresh = lds + span_max;
  for (int k = threadIdx.x; k < H; k += kThreads) {
    int gidx = in_samples - H + k;
    fresh[k] = gidx < 0 ? hist[gidx + H] : load_sample<I16>(row, gidx);
  }
  float* orow = out + (int64_t)s * out_samples;
  for (int n0 = 0; n0 < out_samples; n0 += kTile) {
    const int64_t m0 = (int64_t)n0 * (int64_t)M;
    const int64_t q0 = m0 / (int64_t)L;
    const uint32_t p0 = (uint32_t)(m0 % (int64_t)L), r0 = (uint32_t)(n0 % (int64_t)L);
    const int64_t lo = q0 - H;                                  // >= -H: the history reaches exactly that far back
    const int span = (int)((p0 + (uint32_t)(kTile - 1) * M) / L) + T;
    __syncthreads();                                            // the previous tile has been read
    for (int i = threadIdx.x; i < span; i += kThreads) {
      int64_t gidx = lo + i;
      lds[i] = gidx < 0 ? hist[gidx + H] : (gidx < in_samples ? load_sample<I16>(row, gidx) : 0.0f);
    }
    __syncthreads();
    float acc[kPerLane];
    tile_outputs<L1>(tab, lds, L, M, T, p0, r0, acc);
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
      int n = n0 + (int)threadIdx.x + i * kThreads;
      if (n < out_samples) orow[n] = acc[i];
    }
  }
  __syncthreads();                                              // every read of the old history is done
  for (int k = threadIdx.x; k < H; k += kThreads) hist[k] = fresh[k];
  if (threadIdx.x == 0) *(int64_t*)st += in_samples;
}

}  // namespace

extern "C" {

void mkws_resample_default_cfg(mkws_resample_cfg* cfg, int rate_in, int rate_out) {
  if (!cfg) return;
  cfg->rate_in = rate_in;
  cfg->rate_out = rate_out;
  cfg->zero_crossings = 32;
  cfg->kaiser_beta = 9.0f;
  cfg->rolloff = 0.95f;
}

int mkws_resample_geometry(const mkws_resample_cfg* cfg, int32_t out[4]) {
  if (!out) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_geometry: NULL out");
  Geometry g;
  int rc = geometry_of(cfg, &g);
  if (rc != MKWS_OK) return rc;
  out[0] = (int32_t)g.L;
  out[1] = (int32_t)g.M;
  out[2] = (int32_t)g.T;
  out[3] = (int32_t)g.half;
  return MKWS_OK;
}

int mkws_resample_host_taps(const mkws_resample_cfg* cfg, float* dst, size_t cap_floats) {
  Geometry g;
  int rc = geometry_of(cfg, &g);
  if (rc != MKWS_OK) return rc;
  if (dst && cap_floats >= (size_t)(g.T * g.L)) build_taps(cfg, g, dst);
  return (int)(g.T * g.L);
}

int64_t mkws_resample_out_samples(const mkws_resample_cfg* cfg, int64_t n_in) {
  Geometry g;
  int rc = geometry_of(cfg, &g);
  if (rc != MKWS_OK) return rc;
  if (n_in < 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_out_samples: n_in = %lld", (long long)n_in);
  if (n_in > INT64_MAX / g.L - 1) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_out_samples: n_in = %lld overflows", (long long)n_in);
  return (n_in * g.L + g.M - 1) / g.M;
}

int mkws_resample_create(const mkws_resample_cfg* cfg, mkws_resample** out) {
  if (!out) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_create: NULL out");
  *out = nullptr;
  Geometry g;
  int rc = geometry_of(cfg, &g);
  if (rc != MKWS_OK) return rc;
  int64_t span_max = span_max_of(g);
  if ((size_t)(span_max + g.T - 1) * sizeof(float) > kMaxLdsBytes)
    return mkws::fail(MKWS_ERR_UNSUPPORTED, "resample: %d -> %d Hz: the input span of one tile (%lld samples) does not fit the LDS", cfg->rate_in,
                      cfg->rate_out, (long long)span_max);
  rc = mkws::require_device();
  if (rc != MKWS_OK) return rc;
  std::vector<float> tab((size_t)(g.T * g.L)), dev(tab.size());
  build_taps(cfg, g, tab.data());
  int64_t minv = 0;                                   // M^-1 mod L (L == 1: 0)
  for (int64_t r = 0; r < g.L; ++r)
    if ((r * g.M) % g.L == 1 % g.L) {
      minv = r;
      break;
    }
  for (int64_t j = 0; j < g.T; ++j)
    for (int64_t r = 0; r < g.L; ++r) dev[(size_t)(j * g.L + r)] = tab[(size_t)(j * g.L + (r * g.M) % g.L)];
  mkws_resample* rs = new (std::nothrow) mkws_resample();
  if (!rs) return mkws::fail(MKWS_ERR_ALLOC, "resample_create: out of host memory");
  rs->cfg = *cfg;
  rs->g = g;
  rs->roff_centred = ((g.half % g.L) * minv) % g.L;
  rs->span_max = span_max;
  rs->d_tab = nullptr;
  if (hipMalloc((void**)&rs->d_tab, dev.size() * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    delete rs;
    return mkws::fail(MKWS_ERR_ALLOC, "resample_create: hipMalloc of %zu bytes failed", dev.size() * sizeof(float));
  }
  if (hipMemcpy(rs->d_tab, dev.data(), dev.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(rs->d_tab);
    delete rs;
    return mkws::fail(MKWS_ERR_HIP, "resample_create: upload of the table failed");
  }
  *out = rs;
  return MKWS_OK;
}

void mkws_resample_destroy(mkws_resample* rs) {
  if (!rs) return;
  if (rs->d_tab) (void)hipFree(rs->d_tab);
  delete rs;
}

int mkws_resample_forward(mkws_resample* rs, const void* d_in, int in_i16, int B, int64_t n_in, int64_t in_stride, int centred, float* d_out,
                          int64_t out_stride, void* stream) {
  if (!rs) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_forward: NULL handle");
  if (B < 0 || n_in < 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_forward: B = %d, n_in = %lld", B, (long long)n_in);
  if (B == 0 || n_in == 0) return MKWS_OK;
  if (!d_in || !d_out) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_forward: NULL buffer");
  const Geometry& g = rs->g;
  if (n_in > INT64_MAX / (g.L + g.M) / 2) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_forward: n_in = %lld overflows", (long long)n_in);
  int64_t n_out = (n_in * g.L + g.M - 1) / g.M;
  if (in_stride < n_in || out_stride < n_out)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_forward: strides %lld / %lld shorter than the rows %lld / %lld", (long long)in_stride,
                      (long long)out_stride, (long long)n_in, (long long)n_out);
  int64_t tiles = (n_out + kTile - 1) / kTile;
  if (tiles * B > 0x7fffffffLL) return mkws::fail(MKWS_ERR_UNSUPPORTED, "resample_forward: %lld tiles x %d rows exceed one launch", (long long)tiles, B);
  int64_t off = centred ? g.half : 0;
  uint32_t roff = centred ? (uint32_t)rs->roff_centred : 0u;
  dim3 grid((uint32_t)(tiles * B)), block(kThreads);
  size_t lds = (size_t)rs->span_max * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
#define MKWS_RS_BATCH(L1, I16)                                                                                                              \
  hipLaunchKernelGGL((resample_batch_kernel<L1, I16>), grid, block, lds, st, rs->d_tab, (uint32_t)g.L, (uint32_t)g.M, (int)g.T, off, roff, \
                     d_in, n_in, in_stride, d_out, n_out, out_stride, (uint32_t)tiles)
  if (g.L == 1) {
    if (in_i16) MKWS_RS_BATCH(true, true); else MKWS_RS_BATCH(true, false);
  } else {
    if (in_i16) MKWS_RS_BATCH(false, true); else MKWS_RS_BATCH(false, false);
  }
#undef MKWS_RS_BATCH
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

int mkws_resample_live_in_samples(const mkws_resample* rs, int out_samples) {
  if (!rs) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_live_in_samples: NULL handle");
  if (out_samples < 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_live_in_samples: out_samples = %d", out_samples);
  int64_t m = (int64_t)out_samples * rs->g.M;
  if (m % rs->g.L != 0)
    return mkws::fail(MKWS_ERR_UNSUPPORTED, "resample: a push of %d output samples is %lld/%lld input samples at %d -> %d Hz, not a whole number",
                      out_samples, (long long)m, (long long)rs->g.L, rs->cfg.rate_in, rs->cfg.rate_out);
  if (m / rs->g.L > 0x7fffffffLL) return mkws::fail(MKWS_ERR_UNSUPPORTED, "resample: a push of %lld input samples", (long long)(m / rs->g.L));
  return (int)(m / rs->g.L);
}

size_t mkws_resample_live_state_bytes(const mkws_resample* rs) {
  if (!rs) return 0;
  return (8 + 4 * (size_t)(rs->g.T - 1) + 7) / 8 * 8;
}

int mkws_resample_live_push_many(mkws_resample* rs, void* d_states, size_t state_stride_bytes, int n_streams, const int32_t* d_active,
                                 const void* d_in, int in_i16, int out_samples, float* d_out, void* stream) {
  if (!rs) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_live_push_many: NULL handle");
  if (n_streams < 0 || out_samples < 0)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_live_push_many: n_streams = %d, out_samples = %d", n_streams, out_samples);
  int in_samples = mkws_resample_live_in_samples(rs, out_samples);
  if (in_samples < 0) return in_samples;
  if (state_stride_bytes % 8 != 0 || state_stride_bytes < mkws_resample_live_state_bytes(rs))
    return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_live_push_many: a state stride of %zu bytes (a multiple of 8, at least %zu)", state_stride_bytes,
                      mkws_resample_live_state_bytes(rs));
  if (n_streams == 0 || out_samples == 0) return MKWS_OK;
  if (!d_states || !d_in || !d_out) return mkws::fail(MKWS_ERR_INVALID_ARG, "resample_live_push_many: NULL buffer");
  const Geometry& g = rs->g;
  dim3 grid((uint32_t)n_streams), block(kThreads);
  size_t lds = (size_t)(rs->span_max + g.T - 1) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
#define MKWS_RS_LIVE(L1, I16)                                                                                                                  \
  hipLaunchKernelGGL((resample_live_kernel<L1, I16>), grid, block, lds, st, rs->d_tab, (uint32_t)g.L, (uint32_t)g.M, (int)g.T, (char*)d_states, \
                     state_stride_bytes, d_active, d_in, in_samples, d_out, out_samples, (int)rs->span_max)
  if (g.L == 1) {
    if (in_i16) MKWS_RS_LIVE(true, true); else MKWS_RS_LIVE(true, false);
  } else {
    if (in_i16) MKWS_RS_LIVE(false, true); else MKWS_RS_LIVE(false, false);
  }
#undef MKWS_RS_LIVE
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

}  // extern "C"
