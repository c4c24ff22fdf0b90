// wav2vec 2.0 encoder, inference (mkws_w2v2_* of include/mkws.h).
//
// Activations are channels-last.  A clip's rows in the feature encoder are padded to Tp_i = 2^(6-i) * P rows (P the smallest count that
// holds every layer: 16000 samples -> 3200, 1600, ..., 50), so that row b * Tp_i + t of layer i starts at row s_i * (b * Tp_i + t) of
// layer i - 1: the stride-s, kernel-k convolution of the WHOLE batch is one GEMM with lda = s * C_in and K = k * C_in over overlapping
// row views (the fp32 MFMA GEMM of mkws_op_gemm).  Rows t >= T_i of a clip are computed from whatever lies there and never read as valid rows.
// From the projection on the rows are compact ([B * T, .]).  Every sum that crosses threads is taken in a fixed order (strided partial
// sums, then an LDS tree or wave shuffles; the GroupNorm statistics cross workgroups through per-chunk partial sums folded in chunk
// order): no atomics, the same call twice gives the same bits.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "mkws_common.h"

using mkws::fail;

namespace {

constexpr int kThreads = 256;
constexpr int kConvLayers = 7;
constexpr int kKernel[kConvLayers] = {10, 3, 3, 3, 3, 2, 2};
constexpr int kStride[kConvLayers] = {5, 2, 2, 2, 2, 2, 2};
constexpr int kConv0Chunk = 64;       // positions of layer 0 per workgroup = one chunk of the GroupNorm statistics
constexpr int kPosTile = 32;          // frames of the positional convolution per workgroup
constexpr int kPosPer = 8;            // consecutive frames per thread
constexpr int kGridCap = 8192;        // workgroups of an elementwise launch; larger tensors are walked by grid-stride loops
constexpr size_t kPartFloats = (size_t)1 << 26;   // the slice buffer of the split GEMMs never holds more
constexpr int kMaxSlices = 16;
constexpr size_t kLdsDefault = 64 * 1024, kLdsMax = 160 * 1024;
constexpr double kProcessorEps = 1e-7, kGroupNormEps = 1e-5;

__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// ---- stage 0: per-clip normalisation.  One workgroup per clip; two passes in float64 (mean, then squared deviations), each a strided
// partial sum per thread folded by an LDS tree.  normalize == 0 copies.
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kThreads) void w2v2_norm_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int normalize) {
  __shared__ double red[kThreads];
  const float* xb = x + (size_t)blockIdx.x * n;
  float* yb = y + (size_t)blockIdx.x * n;
  if (!normalize) {
    for (int i = threadIdx.x; i < n; i += kThreads) yb[i] = xb[i];
    return;
  }
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) s += (double)xb[i];
  const double mean = block_sum(s, red) / (double)n;
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) { const double d = (double)xb[i] - mean; q += d * d; }
  const double rstd = 1.0 / sqrt(block_sum(q, red) / (double)n + kProcessorEps);
  for (int i = threadIdx.x; i < n; i += kThreads) yb[i] = (float)(((double)xb[i] - mean) * rstd);
}

// ---- layer 0: C_in = 1, kernel 10, stride 5.  A workgroup takes 64 positions of one clip (325 samples in LDS) and all channels; a thread
// owns a channel (its ten taps in registers), stores the raw outputs (coalesced over channels) and leaves the chunk's float64 sum and
// sum of squares per channel.
__global__ __launch_bounds__(kThreads) void w2v2_conv0_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ out,
                                                              double* __restrict__ part, int n, int T0, int Tp0, int C0, int chunks) {
  __shared__ float xs[kConv0Chunk * 5 + 5];
  const int b = blockIdx.y, chunk = blockIdx.x, t0 = chunk * kConv0Chunk;
  const int nt = min(kConv0Chunk, T0 - t0);
  const int ns = nt * 5 + 5;                                          // <= n - 5 * t0: the last position reads samples 5 t .. 5 t + 9 <= n - 1
  const float* xb = x + (size_t)b * n + (size_t)t0 * 5;
  for (int i = threadIdx.x; i < ns; i += kThreads) xs[i] = xb[i];
  __syncthreads();
  for (int c = threadIdx.x; c < C0; c += kThreads) {
    float wk[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) wk[j] = w[j * C0 + c];
    double s = 0.0, q = 0.0;
    float* o = out + ((size_t)b * Tp0 + t0) * C0 + c;
    for (int t = 0; t < nt; ++t) {
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < 10; ++j) acc = fmaf(wk[j], xs[t * 5 + j], acc);
      o[(size_t)t * C0] = acc;
      s += (double)acc;
      q += (double)acc * (double)acc;
    }
    double* p = part + (((size_t)b * chunks + chunk) * C0 + c) * 2;
    p[0] = s;
    p[1] = q;
  }
}

// chunk sums folded in chunk order -> (mean, 1 / sqrt(var + eps)) per (clip, channel)
__global__ __launch_bounds__(kThreads) void w2v2_gn_stats_kernel(const double* __restrict__ part, float* __restrict__ stats, int B, int C0, int chunks, int T0) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= B * C0) return;
  const int b = i / C0, c = i % C0;
  double s = 0.0, q = 0.0;
  for (int k = 0; k < chunks; ++k) {
    const double* p = part + (((size_t)b * chunks + k) * C0 + c) * 2;
    s += p[0];
    q += p[1];
  }
  const double mean = s / (double)T0;
  double var = q / (double)T0 - mean * mean;
  if (var < 0.0) var = 0.0;
  stats[2 * (size_t)i] = (float)mean;
  stats[2 * (size_t)i + 1] = (float)(1.0 / sqrt(var + kGroupNormEps));
}

__global__ __launch_bounds__(kThreads) void w2v2_gn_gelu_kernel(float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, int B, int T0, int Tp0, int C0) {
  const size_t total = (size_t)B * T0 * C0;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const int c = (int)(i % C0);
    const size_t r = i / C0;
    const int b = (int)(r / T0), t = (int)(r % T0);
    float* p = x + ((size_t)b * Tp0 + t) * C0 + c;
    const float mean = stats[2 * ((size_t)b * C0 + c)], rstd = stats[2 * ((size_t)b * C0 + c) + 1];
    *p = gelu((*p - mean) * rstd * gamma[c] + beta[c]);
  }
}

// ---- x <- act(x + bias) over a contiguous [M, N]; bias may be NULL; act 0 none, 1 GELU
__global__ __launch_bounds__(kThreads) void w2v2_bias_act_kernel(float* __restrict__ x, const float* __restrict__ bias, size_t total, int N, int act) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    float v = x[i];
    if (bias) v += bias[i % N];
    x[i] = act ? gelu(v) : v;
  }
}

// ---- dst [B, T, C] compact <- src rows b * P + t
__global__ __launch_bounds__(kThreads) void w2v2_copy_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int T, int P, int C) {
  const size_t total = (size_t)B * T * C;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const int c = (int)(i % C);
    const size_t r = i / C;
    dst[i] = src[((r / T) * P + (r % T)) * C + c];
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- out[r] = LayerNorm(x[src(r)] + bias + res[r]) * gamma + beta; one wave per row, two-pass statistics.  src(r) = (r / T) * P + r % T
// reads the padded rows of the feature encoder (T = P = M: compact).  bias and res may be NULL.  out must not alias x or res.
__global__ __launch_bounds__(kThreads) void w2v2_ln_kernel(const float* __restrict__ x, const float* __restrict__ bias, const float* __restrict__ res,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out, int M,
                                                           int N, float eps, int T, int P) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (r >= M) return;                                                  // (whole waves leave together: the shuffles below stay full)
  const float* xr = x + ((size_t)(r / T) * P + (r % T)) * N;
  const float* rr = res ? res + (size_t)r * N : nullptr;
  auto at = [&](int c) { float v = xr[c]; if (bias) v += bias[c]; if (rr) v += rr[c]; return v; };
  float s = 0.0f;
  for (int c = lane; c < N; c += 64) s += at(c);
  const float mean = wave_sum(s) / (float)N;
  float q = 0.0f;
  for (int c = lane; c < N; c += 64) { const float d = at(c) - mean; q += d * d; }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)N + eps);
  float* o = out + (size_t)r * N;
  for (int c = lane; c < N; c += 64) o[c] = (at(c) - mean) * rstd * gamma[c] + beta[c];
}

// ---- positional convolution: out[b,t,co] = h[b,t,co] + GELU(bias[co] + sum_{j,ci} w[g][j][ci][co'] * hpad[b, t + j, g * cg + ci]), hpad = h with
// K / 2 zero rows in front (and as many behind as the K taps reach).  A workgroup: 32 frames of one group of one clip, the 32 + K - 1 input
// rows of the group in LDS; a thread owns an output channel and eight consecutive frames and walks the taps with a sliding window of
// eight inputs in registers, so that every weight it loads and every input it reads from LDS serves eight sums.
__global__ __launch_bounds__(kThreads) void w2v2_pos_conv_kernel(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ bias,
                                                                 float* __restrict__ out, int T, int H, int K, int cg) {
  extern __shared__ __attribute__((aligned(16))) float pos_lds[];
  const int t0 = blockIdx.x * kPosTile, g = blockIdx.y, b = blockIdx.z;
  const int rows = kPosTile + K - 1, pad = K / 2;
  for (int i = threadIdx.x; i < rows * cg; i += kThreads) {
    const int p = i / cg, ci = i % cg, t = t0 + p - pad;
    pos_lds[i] = (t >= 0 && t < T) ? h[((size_t)b * T + t) * H + g * cg + ci] : 0.0f;
  }
  __syncthreads();
  const float* wg = w + (size_t)g * K * cg * cg;
  for (int item = threadIdx.x; item < cg * (kPosTile / kPosPer); item += kThreads) {
    const int col = item % cg, tq = (item / cg) * kPosPer;
    float acc[kPosPer];
#pragma unroll
    for (int i = 0; i < kPosPer; ++i) acc[i] = 0.0f;
    for (int ci = 0; ci < cg; ++ci) {
      const float* xc = pos_lds + tq * cg + ci;                        // input row tq + r of channel ci at xc[r * cg], r < kPosPer + K - 1
      const float* wc = wg + (size_t)ci * cg + col;                    // tap j at wc[j * cg * cg]
      float win[kPosPer];
#pragma unroll
      for (int i = 1; i < kPosPer; ++i) win[i] = xc[(i - 1) * cg];
#pragma unroll 8
      for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int i = 0; i + 1 < kPosPer; ++i) win[i] = win[i + 1];
        win[kPosPer - 1] = xc[(j + kPosPer - 1) * cg];
        const float wv = wc[(size_t)j * cg * cg];
#pragma unroll
        for (int i = 0; i < kPosPer; ++i) acc[i] = fmaf(wv, win[i], acc[i]);
      }
    }
    const int co = g * cg + col;
#pragma unroll
    for (int i = 0; i < kPosPer; ++i) {
      const int t = t0 + tq + i;
      if (t < T) {
        const size_t at = ((size_t)b * T + t) * H + co;
        out[at] = h[at] + gelu(acc[i] + bias[co]);
      }
    }
  }
}

// ---- attention of one (clip, head): K and V of the head (bias added) stay in LDS; a wave takes a query row at a time: scores over all T
// keys (a lane per key), softmax through wave shuffles, then the product with V (a lane per output channel).  The [T, T] scores never
// leave the chip.  K rows are padded to an odd stride, so that the lanes of a score step hit distinct banks.
__global__ __launch_bounds__(kThreads) void w2v2_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ bqkv, float* __restrict__ out, int T, int H,
                                                             int d, float scale) {
  extern __shared__ __attribute__((aligned(16))) float att_lds[];
  const int head = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dk = d | 1;
  float* Ks = att_lds;
  float* Vs = Ks + (size_t)T * dk;
  float* qs = Vs + (size_t)T * d + wave * d;
  float* ps = Vs + (size_t)T * d + (kThreads / 64) * d + wave * T;
  const float* base = qkv + (size_t)b * T * 3 * H + head * d;
  for (int i = tid; i < T * d; i += kThreads) {
    const int j = i / d, c = i % d;
    Ks[j * dk + c] = base[(size_t)j * 3 * H + H + c] + bqkv[H + head * d + c];
    Vs[j * d + c] = base[(size_t)j * 3 * H + 2 * H + c] + bqkv[2 * H + head * d + c];
  }
  __syncthreads();
  for (int i0 = 0; i0 < T; i0 += kThreads / 64) {
    const int i = i0 + wave;
    const bool live = i < T;
    if (live)
      for (int c = lane; c < d; c += 64) qs[c] = (base[(size_t)i * 3 * H + c] + bqkv[head * d + c]) * scale;
    __syncthreads();
    float m = -INFINITY;
    if (live)
      for (int j = lane; j < T; j += 64) {
        float s = 0.0f;
        for (int c = 0; c < d; ++c) s = fmaf(qs[c], Ks[j * dk + c], s);
        ps[j] = s;
        m = fmaxf(m, s);
      }
    m = wave_max(m);
    float sum = 0.0f;
    if (live)
      for (int j = lane; j < T; j += 64) {
        const float e = expf(ps[j] - m);
        ps[j] = e;
        sum += e;
      }
    sum = wave_sum(sum);
    if (live)
      for (int j = lane; j < T; j += 64) ps[j] = ps[j] / sum;
    __syncthreads();
    if (live)
      for (int c = lane; c < d; c += 64) {
        float o = 0.0f;
        for (int j = 0; j < T; ++j) o = fmaf(ps[j], Vs[j * d + c], o);
        out[((size_t)b * T + i) * H + head * d + c] = o;
      }
    __syncthreads();
  }
}

// ---- out[b, c] = max_t h[b, t, c]
__global__ __launch_bounds__(kThreads) void w2v2_max_kernel(const float* __restrict__ h, float* __restrict__ out, int B, int T, int H) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= B * H) return;
  const int b = i / H, c = i % H;
  const float* p = h + (size_t)b * T * H + c;
  float m = p[0];
  for (int t = 1; t < T; ++t) m = fmaxf(m, p[(size_t)t * H]);
  out[i] = m;
}

// ------------------------------------------------------------------------------------------------ host side
struct Tensor {
  std::string name;
  std::vector<int> shape;
  size_t offset, count;
};

int check_cfg(const mkws_w2v2_cfg* c) {
  if (!c) return fail(MKWS_ERR_INVALID_ARG, "w2v2: cfg is NULL");
  for (int i = 0; i < kConvLayers; ++i) {
    if (c->conv_kernel[i] != kKernel[i] || c->conv_stride[i] != kStride[i])
      return fail(MKWS_ERR_UNSUPPORTED, "w2v2: conv layer %d has kernel %d stride %d; the build implements kernels (10,3,3,3,3,2,2), strides (5,2,2,2,2,2,2)", i,
                  c->conv_kernel[i], c->conv_stride[i]);
    if (c->conv_dim[i] < 1 || c->conv_dim[i] > 4096) return fail(MKWS_ERR_INVALID_ARG, "w2v2: conv_dim[%d] = %d outside [1, 4096]", i, c->conv_dim[i]);
  }
  if (c->group_norm != 1) return fail(MKWS_ERR_UNSUPPORTED, "w2v2: feat_extract_norm must be \"group\"");
  if (c->conv_bias != 0) return fail(MKWS_ERR_UNSUPPORTED, "w2v2: conv_bias = True is not implemented");
  if (c->stable_layer_norm != 0) return fail(MKWS_ERR_UNSUPPORTED, "w2v2: do_stable_layer_norm = True is not implemented");
  if (c->exact_gelu != 1) return fail(MKWS_ERR_UNSUPPORTED, "w2v2: only the exact GELU is implemented (hidden_act and feat_extract_activation \"gelu\")");
  if (c->hidden_size < 1 || c->hidden_size > 8192) return fail(MKWS_ERR_INVALID_ARG, "w2v2: hidden_size %d outside [1, 8192]", c->hidden_size);
  if (c->num_hidden_layers < 0 || c->num_hidden_layers > 256) return fail(MKWS_ERR_INVALID_ARG, "w2v2: num_hidden_layers %d outside [0, 256]", c->num_hidden_layers);
  if (c->num_attention_heads < 1 || c->hidden_size % c->num_attention_heads)
    return fail(MKWS_ERR_INVALID_ARG, "w2v2: num_attention_heads %d does not divide hidden_size %d", c->num_attention_heads, c->hidden_size);
  if (c->intermediate_size < 1 || c->intermediate_size > 65536) return fail(MKWS_ERR_INVALID_ARG, "w2v2: intermediate_size %d outside [1, 65536]", c->intermediate_size);
  if (c->num_conv_pos_embeddings < 1 || c->num_conv_pos_embeddings > 1024)
    return fail(MKWS_ERR_INVALID_ARG, "w2v2: num_conv_pos_embeddings %d outside [1, 1024]", c->num_conv_pos_embeddings);
  if (c->num_conv_pos_embedding_groups < 1 || c->hidden_size % c->num_conv_pos_embedding_groups)
    return fail(MKWS_ERR_INVALID_ARG, "w2v2: num_conv_pos_embedding_groups %d does not divide hidden_size %d", c->num_conv_pos_embedding_groups, c->hidden_size);
  if (!(c->layer_norm_eps > 0.0f) || !std::isfinite(c->layer_norm_eps)) return fail(MKWS_ERR_INVALID_ARG, "w2v2: layer_norm_eps must be positive and finite");
  const size_t pos_lds = (size_t)(kPosTile + c->num_conv_pos_embeddings - 1) * (c->hidden_size / c->num_conv_pos_embedding_groups) * sizeof(float);
  if (pos_lds > kLdsDefault) return fail(MKWS_ERR_UNSUPPORTED, "w2v2: the positional convolution needs %zu bytes of LDS per workgroup, above %zu", pos_lds, kLdsDefault);
  return MKWS_OK;
}

std::vector<Tensor> enumerate_tensors(const mkws_w2v2_cfg& c) {
  std::vector<Tensor> v;
  size_t at = 0;
  auto add = [&](const std::string& name, std::vector<int> shape) {
    size_t n = 1;
    for (int d : shape) n *= (size_t)d;
    v.push_back({name, shape, at, n});
    at += n;
  };
  const int H = c.hidden_size, I = c.intermediate_size;
  for (int i = 0; i < kConvLayers; ++i) {
    const std::string p = "feature_extractor.conv_layers." + std::to_string(i);
    add(p + ".conv.weight", {c.conv_dim[i], i ? c.conv_dim[i - 1] : 1, kKernel[i]});
    if (i == 0) {
      add(p + ".layer_norm.weight", {c.conv_dim[0]});
      add(p + ".layer_norm.bias", {c.conv_dim[0]});
    }
  }
  add("feature_projection.layer_norm.weight", {c.conv_dim[6]});
  add("feature_projection.layer_norm.bias", {c.conv_dim[6]});
  add("feature_projection.projection.weight", {H, c.conv_dim[6]});
  add("feature_projection.projection.bias", {H});
  add("encoder.pos_conv_embed.conv.bias", {H});
  add("encoder.pos_conv_embed.conv.parametrizations.weight.original0", {1, 1, c.num_conv_pos_embeddings});
  add("encoder.pos_conv_embed.conv.parametrizations.weight.original1", {H, H / c.num_conv_pos_embedding_groups, c.num_conv_pos_embeddings});
  add("encoder.layer_norm.weight", {H});
  add("encoder.layer_norm.bias", {H});
  for (int l = 0; l < c.num_hidden_layers; ++l) {
    const std::string p = "encoder.layers." + std::to_string(l);
    for (const char* proj : {"k_proj", "v_proj", "q_proj", "out_proj"}) {
      add(p + ".attention." + proj + ".weight", {H, H});
      add(p + ".attention." + proj + ".bias", {H});
    }
    add(p + ".layer_norm.weight", {H});
    add(p + ".layer_norm.bias", {H});
    add(p + ".feed_forward.intermediate_dense.weight", {I, H});
    add(p + ".feed_forward.intermediate_dense.bias", {I});
    add(p + ".feed_forward.output_dense.weight", {H, I});
    add(p + ".feed_forward.output_dense.bias", {H});
    add(p + ".final_layer_norm.weight", {H});
    add(p + ".final_layer_norm.bias", {H});
  }
  return v;
}

// frames per layer and the row padding for clips of n samples; false below 400 samples
struct Geometry {
  int T[kConvLayers], Tp[kConvLayers], P;
};
bool geometry(int n, Geometry* g) {
  int t = n;
  for (int i = 0; i < kConvLayers; ++i) {
    if (t < kKernel[i]) return false;
    t = (t - kKernel[i]) / kStride[i] + 1;
    g->T[i] = t;
  }
  int P = g->T[6];
  for (int i = 0; i < 6; ++i) {
    const int f = 1 << (6 - i), need = (g->T[i] + f - 1) / f;
    if (need > P) P = need;
  }
  g->P = P;
  for (int i = 0; i < kConvLayers; ++i) g->Tp[i] = P << (6 - i);
  return true;
}

struct LayerW {
  float *wqkv, *bqkv, *wo, *bo, *ln1g, *ln1b, *w1, *b1, *w2, *b2, *ln2g, *ln2b;
};

}  // namespace

struct mkws_w2v2 {
  mkws_w2v2_cfg cfg;
  int max_batch = 0, max_samples = 0, device = 0;
  size_t attn_lds = 0;
  float* d_w = nullptr;             // the re-laid-out weights
  float* d_work = nullptr;          // all workspace
  // views into d_w
  float *conv0_w, *gn_g, *gn_b, *conv_w[kConvLayers], *fp_lng, *fp_lnb, *fp_w, *fp_b, *pos_w, *pos_b, *enc_lng, *enc_lnb;
  std::vector<LayerW> layers;
  // views into d_work
  float *xn, *bufA, *bufB, *part, *gn_stats, *feat, *hA, *hB, *tmp, *qkv, *att, *ffn;
  double* gn_part;
};

namespace {

// Slices of a GEMM's reduction -- a function of the shapes only.  Enough of them to give a small output about one workgroup per CU
// (slices of at least 32 columns), and no slice longer than 512 columns: the MFMA sums a slice as one k-ordered chain of roundings, whose
// error grows with its length, and the fold adds the slice sums in slice order.  Never more than the slice buffer holds, never an empty slice.
int gemm_slices(int M, int N, int K) {
  const long tiles = (long)((M + 63) / 64) * ((N + 63) / 64);
  long fill = (256 + tiles - 1) / tiles;
  if (fill > K / 32) fill = K / 32;
  const long chain = (K + 511) / 512;
  long s = fill > chain ? fill : chain;
  if (s > kMaxSlices) s = kMaxSlices;
  const size_t fit = kPartFloats / ((size_t)M * N);
  if ((size_t)s > fit) s = (long)fit;
  auto per = [&](long n) { return ((K + n - 1) / n + 15) / 16 * 16; };
  while (s > 1 && (s - 1) * per(s) >= K) --s;
  return s < 1 ? 1 : (int)s;
}

size_t attn_lds_bytes(int T, int d) { return ((size_t)T * (d | 1) + (size_t)T * d + (size_t)(kThreads / 64) * (d + T)) * sizeof(float); }

int grid_for(size_t total) {
  const size_t g = (total + kThreads - 1) / kThreads;
  return (int)(g < (size_t)kGridCap ? (g ? g : 1) : (size_t)kGridCap);
}

// the chain up to `stage` (-1: all of it); see mkws_w2v2_tap for the stages
int run(mkws_w2v2* m, const float* d_audio, int B, int n, int normalize, int stage, float* d_tap, float* d_hidden, float* d_embed, void* stream) {
  if (!m) return fail(MKWS_ERR_INVALID_ARG, "w2v2 handle is NULL");
  if (B < 0 || B > m->max_batch) return fail(MKWS_ERR_INVALID_ARG, "w2v2: batch %d outside [0, max_batch=%d]", B, m->max_batch);
  Geometry g;
  if (n > m->max_samples || !geometry(n, &g)) return fail(MKWS_ERR_INVALID_ARG, "w2v2: %d samples outside [400, max_samples=%d]", n, m->max_samples);
  if (B == 0) return MKWS_OK;
  if (!d_audio) return fail(MKWS_ERR_INVALID_ARG, "w2v2: d_audio is NULL");
  const mkws_w2v2_cfg& c = m->cfg;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int H = c.hidden_size, I = c.intermediate_size, T = g.T[6], M = B * T;
  auto copy_out = [&](const float* src, float* dst, int rows, int padded, int C) {
    hipLaunchKernelGGL(w2v2_copy_rows_kernel, dim3(grid_for((size_t)B * rows * C)), dim3(kThreads), 0, s, src, dst, B, rows, padded, C);
  };
  auto bias_act = [&](float* x, const float* bias, size_t rows, int N, int act) {
    hipLaunchKernelGGL(w2v2_bias_act_kernel, dim3(grid_for(rows * N)), dim3(kThreads), 0, s, x, bias, rows * (size_t)N, N, act);
  };
  auto layer_norm = [&](const float* x, const float* bias, const float* res, const float* gamma, const float* beta, float* out, int N, int Tsrc, int Psrc) {
    hipLaunchKernelGGL(w2v2_ln_kernel, dim3((M + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads), 0, s, x, bias, res, gamma, beta, out, M, N, c.layer_norm_eps,
                       Tsrc, Psrc);
  };
  auto gemm = [&](const float* A, const float* W, float* C, int rows, int N, int K, int lda) {
    return mkws::gemm_split(A, W, C, rows, N, K, lda, N, N, gemm_slices(rows, N, K), m->part, s);
  };
  auto done = [&]() { MKWS_HIP(hipGetLastError()); return (int)MKWS_OK; };

  hipLaunchKernelGGL(w2v2_norm_kernel, dim3(B), dim3(kThreads), 0, s, d_audio, m->xn, n, normalize ? 1 : 0);
  if (stage == 0) { copy_out(m->xn, d_tap, n, n, 1); return done(); }

  // layer 0 and its GroupNorm
  const int C0 = c.conv_dim[0], chunks = (g.T[0] + kConv0Chunk - 1) / kConv0Chunk;
  hipLaunchKernelGGL(w2v2_conv0_kernel, dim3(chunks, B), dim3(kThreads), 0, s, m->xn, m->conv0_w, m->bufA, m->gn_part, n, g.T[0], g.Tp[0], C0, chunks);
  hipLaunchKernelGGL(w2v2_gn_stats_kernel, dim3((B * C0 + kThreads - 1) / kThreads), dim3(kThreads), 0, s, m->gn_part, m->gn_stats, B, C0, chunks, g.T[0]);
  hipLaunchKernelGGL(w2v2_gn_gelu_kernel, dim3(grid_for((size_t)B * g.T[0] * C0)), dim3(kThreads), 0, s, m->bufA, m->gn_stats, m->gn_g, m->gn_b, B, g.T[0], g.Tp[0], C0);
  float *cur = m->bufA, *nxt = m->bufB;
  if (stage == 1) { copy_out(cur, d_tap, g.T[0], g.Tp[0], C0); return done(); }

  // layers 1..6: one GEMM each over the overlapping row views, rows up to the last clip's last valid one
  for (int i = 1; i < kConvLayers; ++i) {
    const int Cin = c.conv_dim[i - 1], Cout = c.conv_dim[i], rows = (B - 1) * g.Tp[i] + g.T[i];
    if (int rc = gemm(cur, m->conv_w[i], nxt, rows, Cout, kKernel[i] * Cin, kStride[i] * Cin)) return rc;
    bias_act(nxt, nullptr, (size_t)rows, Cout, 1);
    float* t = cur; cur = nxt; nxt = t;
    if (stage == i + 1) { copy_out(cur, d_tap, g.T[i], g.Tp[i], Cout); return done(); }
  }

  // projection
  const int C6 = c.conv_dim[6];
  layer_norm(cur, nullptr, nullptr, m->fp_lng, m->fp_lnb, m->feat, C6, T, g.Tp[6]);
  if (int rc = gemm(m->feat, m->fp_w, m->hB, M, H, C6, C6)) return rc;
  bias_act(m->hB, m->fp_b, (size_t)M, H, 0);
  if (stage == 8) { copy_out(m->hB, d_tap, T, T, H); return done(); }

  // positional convolution, residual, LayerNorm
  const int K = c.num_conv_pos_embeddings, G = c.num_conv_pos_embedding_groups, cg = H / G;
  hipLaunchKernelGGL(w2v2_pos_conv_kernel, dim3((T + kPosTile - 1) / kPosTile, G, B), dim3(kThreads), (size_t)(kPosTile + K - 1) * cg * sizeof(float), s, m->hB, m->pos_w,
                     m->pos_b, m->tmp, T, H, K, cg);
  layer_norm(m->tmp, nullptr, nullptr, m->enc_lng, m->enc_lnb, m->hA, H, M, M);
  if (stage == 9) { copy_out(m->hA, d_tap, T, T, H); return done(); }

  const int heads = c.num_attention_heads, d = H / heads;
  const float scale = 1.0f / sqrtf((float)d);
  for (int l = 0; l < c.num_hidden_layers; ++l) {
    const LayerW& w = m->layers[l];
    if (int rc = gemm(m->hA, w.wqkv, m->qkv, M, 3 * H, H, H)) return rc;
    hipLaunchKernelGGL(w2v2_attn_kernel, dim3(heads, B), dim3(kThreads), attn_lds_bytes(T, d), s, m->qkv, w.bqkv, m->att, T, H, d, scale);
    if (int rc = gemm(m->att, w.wo, m->tmp, M, H, H, H)) return rc;
    layer_norm(m->tmp, w.bo, m->hA, w.ln1g, w.ln1b, m->hB, H, M, M);
    if (int rc = gemm(m->hB, w.w1, m->ffn, M, I, H, H)) return rc;
    bias_act(m->ffn, w.b1, (size_t)M, I, 1);
    if (int rc = gemm(m->ffn, w.w2, m->tmp, M, H, I, I)) return rc;
    layer_norm(m->tmp, w.b2, m->hB, w.ln2g, w.ln2b, m->hA, H, M, M);
    if (stage == 10 + l) { copy_out(m->hA, d_tap, T, T, H); return done(); }
  }
  if (stage >= 0) return fail(MKWS_ERR_INVALID_ARG, "w2v2: stage %d outside [0, %d]", stage, 9 + c.num_hidden_layers);
  if (d_hidden) copy_out(m->hA, d_hidden, T, T, H);
  if (d_embed) hipLaunchKernelGGL(w2v2_max_kernel, dim3((B * H + kThreads - 1) / kThreads), dim3(kThreads), 0, s, m->hA, d_embed, B, T, H);
  return done();
}

}  // namespace

extern "C" {

void mkws_w2v2_default_cfg(mkws_w2v2_cfg* c) {
  if (!c) return;
  for (int i = 0; i < kConvLayers; ++i) { c->conv_dim[i] = 512; c->conv_kernel[i] = kKernel[i]; c->conv_stride[i] = kStride[i]; }
  c->hidden_size = 768; c->num_hidden_layers = 12; c->num_attention_heads = 12; c->intermediate_size = 3072;
  c->num_conv_pos_embeddings = 128; c->num_conv_pos_embedding_groups = 16;
  c->layer_norm_eps = 1e-5f;
  c->group_norm = 1; c->conv_bias = 0; c->stable_layer_norm = 0; c->exact_gelu = 1;
}

size_t mkws_w2v2_param_count(const mkws_w2v2_cfg* c) {
  if (check_cfg(c) != MKWS_OK) return 0;
  const auto v = enumerate_tensors(*c);
  return v.back().offset + v.back().count;
}

int mkws_w2v2_weight_manifest(const mkws_w2v2_cfg* c, char* dst, size_t cap) {
  if (int rc = check_cfg(c)) return rc;
  const auto v = enumerate_tensors(*c);
  std::string s = "{\"tensors\": [";
  for (size_t i = 0; i < v.size(); ++i) {
    if (i) s += ", ";
    s += "{\"name\": \"" + v[i].name + "\", \"shape\": [";
    for (size_t d = 0; d < v[i].shape.size(); ++d) { if (d) s += ", "; s += std::to_string(v[i].shape[d]); }
    s += "], \"offset\": " + std::to_string(v[i].offset) + ", \"count\": " + std::to_string(v[i].count) + "}";
  }
  s += "]}";
  if (dst && cap > 0) {
    const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
    memcpy(dst, s.data(), n);
    dst[n] = 0;
  }
  return (int)s.size();
}

int mkws_w2v2_num_frames(const mkws_w2v2_cfg* c, int n_samples) {
  if (check_cfg(c) != MKWS_OK) return 0;
  Geometry g;
  return geometry(n_samples, &g) ? g.T[6] : 0;
}

int mkws_w2v2_create(const mkws_w2v2_cfg* c, const float* h, size_t n_floats, int max_batch, int max_samples, mkws_w2v2** out) {
  if (!out) return fail(MKWS_ERR_INVALID_ARG, "w2v2: out is NULL");
  *out = nullptr;
  if (int rc = check_cfg(c)) return rc;
  if (!h) return fail(MKWS_ERR_INVALID_ARG, "w2v2: params is NULL");
  const auto tensors = enumerate_tensors(*c);
  const size_t want = tensors.back().offset + tensors.back().count;
  if (n_floats != want) return fail(MKWS_ERR_BAD_WEIGHTS, "w2v2: parameter blob has %zu floats, this configuration needs %zu", n_floats, want);
  for (size_t i = 0; i < n_floats; ++i)
    if (!std::isfinite(h[i])) return fail(MKWS_ERR_BAD_WEIGHTS, "w2v2: parameter blob has a non-finite value at %zu", i);
  const int H = c->hidden_size, I = c->intermediate_size, K = c->num_conv_pos_embeddings, G = c->num_conv_pos_embedding_groups, cg = H / G, L = c->num_hidden_layers;
  size_t ti = 0;
  auto next = [&]() { return h + tensors[ti++].offset; };

  // the device blob: every tensor starts on a 256-byte boundary
  std::vector<float> f;
  auto place = [&](size_t count) { const size_t at = (f.size() + 63) / 64 * 64; f.resize(at + count, 0.0f); return at; };
  struct { size_t conv0_w, gn_g, gn_b, conv_w[kConvLayers], fp_lng, fp_lnb, fp_w, fp_b, pos_w, pos_b, enc_lng, enc_lnb; } o;
  auto put = [&](const float* src, size_t count) { const size_t at = place(count); memcpy(&f[at], src, count * sizeof(float)); return at; };
  // w [out][in] -> [in][ld] at column col0
  auto put_t = [&](size_t at, const float* src, int rows_out, int cols_in, int ld, int col0) {
    for (int r = 0; r < rows_out; ++r)
      for (int k = 0; k < cols_in; ++k) f[at + (size_t)k * ld + col0 + r] = src[(size_t)r * cols_in + k];
  };
  for (int i = 0; i < kConvLayers; ++i) {
    const float* w = next();
    const int Cout = c->conv_dim[i], Cin = i ? c->conv_dim[i - 1] : 1, k = kKernel[i];
    const size_t at = place((size_t)k * Cin * Cout);
    for (int co = 0; co < Cout; ++co)
      for (int ci = 0; ci < Cin; ++ci)
        for (int j = 0; j < k; ++j) f[at + ((size_t)j * Cin + ci) * Cout + co] = w[((size_t)co * Cin + ci) * k + j];
    if (i == 0) { o.conv0_w = at; o.gn_g = put(next(), Cout); o.gn_b = put(next(), Cout); }
    o.conv_w[i] = at;
  }
  const int C6 = c->conv_dim[6];
  o.fp_lng = put(next(), C6);
  o.fp_lnb = put(next(), C6);
  o.fp_w = place((size_t)C6 * H);
  put_t(o.fp_w, next(), H, C6, H, 0);
  o.fp_b = put(next(), H);
  o.pos_b = put(next(), H);
  {
    const float* gk = next();
    const float* v = next();
    o.pos_w = place((size_t)G * K * cg * cg);
    for (int j = 0; j < K; ++j) {
      double ss = 0.0;
      for (size_t r = 0; r < (size_t)H * cg; ++r) ss += (double)v[r * K + j] * (double)v[r * K + j];
      if (!(ss > 0.0)) return fail(MKWS_ERR_BAD_WEIGHTS, "w2v2: the weight-normalised positional kernel has ||v|| = 0 at kernel position %d", j);
      const double sc = (double)gk[j] / std::sqrt(ss);
      for (int co = 0; co < H; ++co)
        for (int ci = 0; ci < cg; ++ci)
          f[o.pos_w + (((size_t)(co / cg) * K + j) * cg + ci) * cg + co % cg] = (float)((double)v[((size_t)co * cg + ci) * K + j] * sc);
    }
  }
  o.enc_lng = put(next(), H);
  o.enc_lnb = put(next(), H);
  struct LayerO { size_t wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b; };
  std::vector<LayerO> lo((size_t)L);
  for (int l = 0; l < L; ++l) {
    LayerO& q = lo[l];
    q.wqkv = place((size_t)H * 3 * H);
    q.bqkv = place((size_t)3 * H);
    const int col[3] = {H, 2 * H, 0};                                   // the state dict's order is k, v, q; the device's columns are q | k | v
    for (int p = 0; p < 3; ++p) {
      put_t(q.wqkv, next(), H, H, 3 * H, col[p]);
      memcpy(&f[q.bqkv + col[p]], next(), (size_t)H * sizeof(float));
    }
    q.wo = place((size_t)H * H);
    put_t(q.wo, next(), H, H, H, 0);
    q.bo = put(next(), H);
    q.ln1g = put(next(), H);
    q.ln1b = put(next(), H);
    q.w1 = place((size_t)H * I);
    put_t(q.w1, next(), I, H, I, 0);
    q.b1 = put(next(), I);
    q.w2 = place((size_t)I * H);
    put_t(q.w2, next(), H, I, H, 0);
    q.b2 = put(next(), H);
    q.ln2g = put(next(), H);
    q.ln2b = put(next(), H);
  }

  if (max_batch < 1) return fail(MKWS_ERR_INVALID_ARG, "w2v2: max_batch must be positive");
  Geometry g;
  if (!geometry(max_samples, &g)) return fail(MKWS_ERR_INVALID_ARG, "w2v2: max_samples %d is shorter than one frame (400 samples)", max_samples);
  const int T = g.T[6], d = H / c->num_attention_heads;
  const size_t attn_lds = attn_lds_bytes(T, d);
  if (attn_lds > kLdsMax)
    return fail(MKWS_ERR_UNSUPPORTED, "w2v2: attention over %d frames of head_dim %d needs %zu bytes of LDS, above %zu", T, d, attn_lds, kLdsMax);
  // workspace, in floats; every view starts on a 256-byte boundary
  size_t conv_buf = 0;
  for (int i = 0; i < kConvLayers; ++i) { const size_t v = (size_t)max_batch * g.Tp[i] * c->conv_dim[i]; if (v > conv_buf) conv_buf = v; }
  const size_t limit = (size_t)1 << 30, rows = (size_t)max_batch * T;
  int widest = 3 * H > I ? 3 * H : I;
  if (conv_buf >= limit || (size_t)max_batch * max_samples >= limit || rows * widest >= limit)
    return fail(MKWS_ERR_UNSUPPORTED, "w2v2: max_batch %d x max_samples %d is beyond what one handle addresses (2^30 values per activation)", max_batch, max_samples);
  const int chunks = (g.T[0] + kConv0Chunk - 1) / kConv0Chunk;
  size_t work = 0;
  auto carve = [&](size_t count) { const size_t at = work; work += (count + 63) / 64 * 64; return at; };
  const size_t w_xn = carve((size_t)max_batch * max_samples), w_a = carve(conv_buf), w_b = carve(conv_buf),
               w_part = carve((size_t)max_batch * chunks * c->conv_dim[0] * 2 * 2 /* doubles */), w_stats = carve((size_t)max_batch * c->conv_dim[0] * 2),
               w_feat = carve(rows * C6), w_hA = carve(rows * H), w_hB = carve(rows * H), w_tmp = carve(rows * H), w_qkv = carve(rows * 3 * H),
               w_att = carve(rows * H), w_ffn = carve(rows * I),
               w_slices = carve(std::min(kPartFloats, (size_t)kMaxSlices * std::max(conv_buf, rows * widest)));

  int rc = mkws::require_device();
  if (rc != MKWS_OK) return rc;
  mkws_w2v2* m = new (std::nothrow) mkws_w2v2();
  if (!m) return fail(MKWS_ERR_ALLOC, "out of host memory");
  m->cfg = *c;
  m->max_batch = max_batch;
  m->max_samples = max_samples;
  m->attn_lds = attn_lds;
  if (hipGetDevice(&m->device) != hipSuccess) { delete m; return fail(MKWS_ERR_HIP, "hipGetDevice failed"); }
  if (attn_lds > kLdsDefault &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(w2v2_attn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_lds) != hipSuccess) {
    delete m;
    return fail(MKWS_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed", attn_lds);
  }
  if (hipMalloc(reinterpret_cast<void**>(&m->d_w), f.size() * sizeof(float)) != hipSuccess) { delete m; return fail(MKWS_ERR_ALLOC, "hipMalloc(%zu) for weights failed", f.size() * sizeof(float)); }
  if (hipMalloc(reinterpret_cast<void**>(&m->d_work), work * sizeof(float)) != hipSuccess) { mkws_w2v2_destroy(m); return fail(MKWS_ERR_ALLOC, "hipMalloc(%zu) for workspace failed", work * sizeof(float)); }
  if (hipMemcpy(m->d_w, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || hipMemset(m->d_work, 0, work * sizeof(float)) != hipSuccess) {
    mkws_w2v2_destroy(m);
    return fail(MKWS_ERR_HIP, "w2v2: weight upload failed");
  }
  float* w = m->d_w;
  m->conv0_w = w + o.conv0_w; m->gn_g = w + o.gn_g; m->gn_b = w + o.gn_b;
  for (int i = 0; i < kConvLayers; ++i) m->conv_w[i] = w + o.conv_w[i];
  m->fp_lng = w + o.fp_lng; m->fp_lnb = w + o.fp_lnb; m->fp_w = w + o.fp_w; m->fp_b = w + o.fp_b;
  m->pos_w = w + o.pos_w; m->pos_b = w + o.pos_b; m->enc_lng = w + o.enc_lng; m->enc_lnb = w + o.enc_lnb;
  for (const LayerO& q : lo)
    m->layers.push_back({w + q.wqkv, w + q.bqkv, w + q.wo, w + q.bo, w + q.ln1g, w + q.ln1b, w + q.w1, w + q.b1, w + q.w2, w + q.b2, w + q.ln2g, w + q.ln2b});
  float* k = m->d_work;
  m->xn = k + w_xn; m->bufA = k + w_a; m->bufB = k + w_b; m->gn_part = reinterpret_cast<double*>(k + w_part); m->gn_stats = k + w_stats;
  m->feat = k + w_feat; m->hA = k + w_hA; m->hB = k + w_hB; m->tmp = k + w_tmp; m->qkv = k + w_qkv; m->att = k + w_att; m->ffn = k + w_ffn; m->part = k + w_slices;
  *out = m;
  return MKWS_OK;
}

void mkws_w2v2_destroy(mkws_w2v2* m) {
  if (!m) return;
  if (m->d_w) (void)hipFree(m->d_w);
  if (m->d_work) (void)hipFree(m->d_work);
  delete m;
}

int mkws_w2v2_forward(mkws_w2v2* m, const float* d_audio, int B, int n, int normalize, float* d_hidden, float* d_embed, void* stream) {
  if (B > 0 && !d_hidden && !d_embed) return fail(MKWS_ERR_INVALID_ARG, "w2v2: d_hidden and d_embed are both NULL");
  return run(m, d_audio, B, n, normalize, -1, nullptr, d_hidden, d_embed, stream);
}

int mkws_w2v2_tap(mkws_w2v2* m, const float* d_audio, int B, int n, int normalize, int stage, float* d_out, void* stream) {
  if (!m) return fail(MKWS_ERR_INVALID_ARG, "w2v2 handle is NULL");
  if (stage < 0 || stage > 9 + m->cfg.num_hidden_layers) return fail(MKWS_ERR_INVALID_ARG, "w2v2: stage %d outside [0, %d]", stage, 9 + m->cfg.num_hidden_layers);
  if (B > 0 && !d_out) return fail(MKWS_ERR_INVALID_ARG, "w2v2: d_out is NULL");
  return run(m, d_audio, B, n, normalize, stage, d_out, nullptr, nullptr, stream);
}

}  // extern "C"
