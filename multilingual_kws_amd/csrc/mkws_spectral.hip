// The mfcc and average feature modes on gfx950 (mkws_spectral_*, include/mkws.h): the reference's non-micro pipeline,
// tf_v1_speechcommands/input_data_fix_bg.py:444-475 -- audio_spectrogram(magnitude_squared=True), then mfcc or an average pool.
//
// One workgroup per clip, one wave per frame at a time (mkws_frontend.hip's shape).  A frame of NFFT real samples is an M = NFFT / 2
// point complex FFT of even/odd packed samples plus the split post-pass.  The FFT is decimation in time, in place in wave-private LDS:
// the load stores pair j at its bit-reversed place, then two radix-2 stages are done per pass in registers (one lone radix-2 pass
// first when log2 M is odd).  Twiddles, window, mel weights and the DCT come from the host tables (mkws_spectral_tables.cpp), staged
// into LDS once per workgroup.  Everything after the FFT is a per-lane sum in a fixed ascending order: lane = channel for the
// filterbank, lane = coefficient for the DCT, lane = output for the average pool.  No atomics, no cross-frame state, so a frame's
// result depends on its samples alone: not on the clip, the batch, the alignment of its row or the launch that computes it (the
// streaming form relies on exactly that).
#include "mkws_common.h"
#include "mkws_spectral_tables.h"

#include <new>
#include <vector>

namespace mkws {

constexpr int kSpWaves = 4;            // waves per workgroup
constexpr int kSpStreamFrames = 16;    // frames per workgroup of the streaming form's frame launch

struct SpectralParams {
  const float* window;      // [NFFT]  the window, zero padded to the FFT size
  const float2* tw;         // [M / 2] exp(-2 pi i j / M)
  const float2* stw;        // [M + 1] exp(-2 pi i k / NFFT)
  const float* melw;        // [bins]
  const int* band;          // [bins]
  const int* chan_lo;       // [64]
  const int* chan_hi;       // [64]
  const float* dct_t;       // [channels][width]: the DCT matrix transposed, so that lane = coefficient reads consecutive words
  int window_size, stride, bins, width, channels, mode, avg_w;
};

__host__ __device__ constexpr size_t sp_al16(size_t x) { return (x + 15) & ~size_t(15); }

// LDS carve, the same arithmetic on both sides.  Every offset is a multiple of 16 bytes.
struct SpectralCarve {
  size_t o_tw, o_stw, o_win, o_melw, o_band, o_dct, o_wave, wave_bytes, total;
};
__host__ __device__ inline SpectralCarve sp_carve(int nfft, int bins, int channels, int width, bool mfcc) {
  const size_t M = nfft / 2;
  SpectralCarve c;
  c.o_tw = 0;
  c.o_stw = c.o_tw + sp_al16((M / 2) * 8);
  c.o_win = c.o_stw + sp_al16((M + 1) * 8);
  c.o_melw = c.o_win + sp_al16((size_t)nfft * 4);
  c.o_band = c.o_melw + (mfcc ? sp_al16((size_t)bins * 4) : 0);
  c.o_dct = c.o_band + (mfcc ? sp_al16((size_t)bins * 4) : 0);
  c.o_wave = c.o_dct + (mfcc ? sp_al16((size_t)channels * width * 4) : 0);
  c.wave_bytes = M * 8 + sp_al16((M + 1) * 4) + 64 * 4;      // z | magnitude or power | log mel
  c.total = c.o_wave + kSpWaves * c.wave_bytes;
  return c;
}

__device__ __forceinline__ void sp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float2 sp_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ float2 sp_cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 sp_csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

template <typename T> struct SpLoad;
template <> struct SpLoad<float> {
  static __device__ __forceinline__ float one(const float* p) { return *p; }
  // (the vector path and the scalar path move the same bits: the arithmetic starts after the load)
  static __device__ __forceinline__ void pair(const float* p, bool aligned, float& a, float& b) {
    if (aligned) { const float2 v = *reinterpret_cast<const float2*>(p); a = v.x; b = v.y; }
    else { a = p[0]; b = p[1]; }
  }
};
template <> struct SpLoad<int16_t> {
  static __device__ __forceinline__ float cvt(int v) { return (float)v * (1.0f / 32768.0f); }      // exact
  static __device__ __forceinline__ float one(const int16_t* p) { return cvt(*p); }
  static __device__ __forceinline__ void pair(const int16_t* p, bool aligned, float& a, float& b) {
    if (aligned) { const uint32_t v = *reinterpret_cast<const uint32_t*>(p); a = cvt((int)(int16_t)(v & 0xFFFFu)); b = cvt(((int)v) >> 16); }
    else { a = cvt(p[0]); b = cvt(p[1]); }
  }
};

// This lane's sample pairs of one frame: pair j = lane + 64 q holds samples 2j and 2j + 1; what lies past the window is zero (and is not read).
template <typename T, int NFFT>
__device__ __forceinline__ void sp_load_frame(const T* frame, int window_size, int lane, float (&xa)[NFFT / 128], float (&xb)[NFFT / 128]) {
  const bool aligned = (reinterpret_cast<uintptr_t>(frame) % (2 * sizeof(T))) == 0;
#pragma unroll
  for (int q = 0; q < NFFT / 128; ++q) {
    const int n0 = 2 * (lane + 64 * q);
    float a = 0.0f, b = 0.0f;
    if (n0 + 1 < window_size) SpLoad<T>::pair(frame + n0, aligned, a, b);
    else if (n0 < window_size) a = SpLoad<T>::one(frame + n0);
    xa[q] = a; xb[q] = b;
  }
}

// frames [f0, f1) of the row `audio` -> rows out_row0 + f of the outputs
template <typename T, int NFFT>
__device__ __forceinline__ void sp_body(const SpectralParams& p, const T* __restrict__ audio, int f0, int f1, size_t out_row0, float* __restrict__ feat,
                                        float* __restrict__ power, float* __restrict__ mel) {
  constexpr int M = NFFT / 2;
  constexpr int LOG2M = (M == 128) ? 7 : (M == 256) ? 8 : 9;
  constexpr int NP = NFFT / 128;                     // pairs per lane
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const bool mfcc = p.mode == MKWS_SPECTRAL_MFCC;
  const SpectralCarve cv = sp_carve(NFFT, p.bins, p.channels, p.width, mfcc);
  float2* s_tw = reinterpret_cast<float2*>(smem + cv.o_tw);
  float2* s_stw = reinterpret_cast<float2*>(smem + cv.o_stw);
  float* s_win = reinterpret_cast<float*>(smem + cv.o_win);
  float* s_melw = reinterpret_cast<float*>(smem + cv.o_melw);
  int* s_band = reinterpret_cast<int*>(smem + cv.o_band);
  float* s_dct = reinterpret_cast<float*>(smem + cv.o_dct);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = p.channels, W = p.width, bins = p.bins;

  for (int i = tid; i < M / 2; i += kSpWaves * 64) s_tw[i] = p.tw[i];
  for (int i = tid; i <= M; i += kSpWaves * 64) s_stw[i] = p.stw[i];
  for (int i = tid; i < NFFT; i += kSpWaves * 64) s_win[i] = p.window[i];
  int c_lo = 0, c_hi = 0;
  if (mfcc) {
    for (int i = tid; i < bins; i += kSpWaves * 64) { s_melw[i] = p.melw[i]; s_band[i] = p.band[i]; }
    for (int i = tid; i < C * W; i += kSpWaves * 64) s_dct[i] = p.dct_t[i];
    c_lo = p.chan_lo[lane]; c_hi = p.chan_hi[lane];
  }
  __syncthreads();

  unsigned char* wbase = smem + cv.o_wave + (size_t)wave * cv.wave_bytes;
  float2* z = reinterpret_cast<float2*>(wbase);
  float* s_pw = reinterpret_cast<float*>(wbase + (size_t)M * 8);
  float* s_lg = reinterpret_cast<float*>(wbase + (size_t)M * 8 + sp_al16((size_t)(M + 1) * 4));

  float xa[NP], xb[NP];
  int f = f0 + wave;
  if (f < f1) sp_load_frame<T, NFFT>(audio + (size_t)f * p.stride, p.window_size, lane, xa, xb);
  for (; f < f1; f += kSpWaves) {
    // window, pack, bit-reversed store
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int j = lane + 64 * q;
      const float2 w = reinterpret_cast<const float2*>(s_win)[j];
      z[__brev((unsigned)j) >> (32 - LOG2M)] = make_float2(xa[q] * w.x, xb[q] * w.y);
    }
    const int fn = f + kSpWaves;
    if (fn < f1) sp_load_frame<T, NFFT>(audio + (size_t)fn * p.stride, p.window_size, lane, xa, xb);      // in flight under the FFT
    sp_wave_sync();
    int s = 1;
    if (LOG2M & 1) {
#pragma unroll
      for (int q = 0; q < (M / 2 + 63) / 64; ++q) {
        const int i = lane + 64 * q;
        if (i < M / 2) {
          const float2 u = z[2 * i], t = z[2 * i + 1];
          z[2 * i] = sp_cadd(u, t);
          z[2 * i + 1] = sp_csub(u, t);
        }
      }
      sp_wave_sync();
      s = 2;
    }
#pragma unroll
    for (; s < M; s *= 4) {
#pragma unroll
      for (int q = 0; q < (M / 4 + 63) / 64; ++q) {
        const int q4 = lane + 64 * q;
        if (q4 < M / 4) {
          const int k = q4 & (s - 1);
          const int i0 = (q4 - k) * 4 + k;
          const float2 wA = s_tw[k * (M / (2 * s))];
          const float2 wB0 = s_tw[k * (M / (4 * s))];
          const float2 wB1 = s_tw[(k + s) * (M / (4 * s))];
          const float2 a0 = z[i0], a1 = sp_cmul(z[i0 + s], wA), a2 = z[i0 + 2 * s], a3 = sp_cmul(z[i0 + 3 * s], wA);
          const float2 b0 = sp_cadd(a0, a1), b1 = sp_csub(a0, a1);
          const float2 b2 = sp_cmul(sp_cadd(a2, a3), wB0), b3 = sp_cmul(sp_csub(a2, a3), wB1);
          z[i0] = sp_cadd(b0, b2);
          z[i0 + s] = sp_cadd(b1, b3);
          z[i0 + 2 * s] = sp_csub(b0, b2);
          z[i0 + 3 * s] = sp_csub(b1, b3);
        }
      }
      sp_wave_sync();
    }
    // split post-pass: X[k] = (Z[k] + conj Z[M-k]) / 2 - i W^k (Z[k] - conj Z[M-k]) / 2, k <= M
    const size_t row = out_row0 + (size_t)f;
#pragma unroll
    for (int q = 0; q < (M + 1 + 63) / 64; ++q) {
      const int k = lane + 64 * q;
      if (k <= M) {
        const float2 zk = z[k & (M - 1)], zm = z[(M - k) & (M - 1)], w = s_stw[k];
        const float ex = 0.5f * (zk.x + zm.x), ey = 0.5f * (zk.y - zm.y);
        const float dx = zk.x - zm.x, dy = zk.y + zm.y;
        const float re = ex + 0.5f * (w.x * dy + w.y * dx);
        const float im = ey - 0.5f * (w.x * dx - w.y * dy);
        const float pw = re * re + im * im;
        if (power) power[row * bins + k] = pw;
        s_pw[k] = mfcc ? sqrtf(pw) : pw;
      }
    }
    sp_wave_sync();
    if (mfcc) {
      if (lane < C) {
        float acc = 0.0f;
        for (int i = c_lo; i < c_hi; ++i) {
          const float w = s_melw[i];
          acc += s_pw[i] * ((s_band[i] == lane) ? w : (1.0f - w));
        }
        if (mel) mel[row * C + lane] = acc;
        s_lg[lane] = logf(fmaxf(acc, 1e-12f));
      }
      sp_wave_sync();
      if (lane < W) {
        float acc = 0.0f;
        for (int j = 0; j < C; ++j) acc += s_dct[j * W + lane] * s_lg[j];
        feat[row * W + lane] = acc;
      }
    } else {
      for (int o = lane; o < W; o += 64) {
        const int lo = o * p.avg_w, hi = min(lo + p.avg_w, bins);
        float acc = 0.0f;
        for (int i = lo; i < hi; ++i) acc += s_pw[i];
        feat[row * W + o] = acc / (float)(hi - lo);
      }
    }
    // (the next frame's first LDS writes go to z, which nobody reads after the post-pass's barrier; s_pw and s_lg are rewritten only
    //  after further barriers)
  }
}

// grid (B, chunks): workgroup (b, y) computes frames [y * frames_per_block, ...) of clip b
template <typename T, int NFFT>
__global__ __launch_bounds__(kSpWaves * 64) void spectral_kernel(SpectralParams p, const T* __restrict__ audio, int n_samples, int num_frames, int frames_per_block,
                                                                 float* __restrict__ feat, float* __restrict__ power, float* __restrict__ mel) {
  const size_t clip = blockIdx.x;
  const int f0 = blockIdx.y * frames_per_block;
  const int f1 = min(num_frames, f0 + frames_per_block);
  sp_body<T, NFFT>(p, audio + clip * (size_t)n_samples, f0, f1, clip * (size_t)num_frames, feat, power, mel);
}

// the streaming form's second launch: d_feat[w][f][k] = frames[w * hop_frames + f][k]
__global__ __launch_bounds__(256) void spectral_windows_kernel(const float* __restrict__ frames, int hop_frames, int frames_per_window, int width, size_t total,
                                                               float* __restrict__ feat) {
  const size_t per_window = (size_t)frames_per_window * width;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t w = i / per_window, r = i - w * per_window;
    feat[i] = frames[w * (size_t)hop_frames * width + r];
  }
}

}  // namespace mkws

// ================================================================================================
using namespace mkws;

struct mkws_spectral {
  mkws_spectral_cfg cfg;
  SpectralTables tab;
  SpectralParams prm;
  void* d_blob = nullptr;
  float* d_frames = nullptr;     // [max_frames, width]: the streaming form's frames
  int max_samples = 0, max_frames = 0;
  size_t lds = 0;
};

extern "C" {

void mkws_spectral_default_cfg(mkws_spectral_cfg* c) {
  if (!c) return;
  c->sample_rate = 16000; c->window_size_samples = 480; c->window_stride_samples = 320; c->mode = MKWS_SPECTRAL_MFCC;
  c->num_features = 40; c->filterbank_channels = 40; c->lower_frequency_limit = 20.0f; c->upper_frequency_limit = 4000.0f;
  c->average_window_width = 1;
}

int mkws_spectral_geometry(const mkws_spectral_cfg* cfg, int* fft_size, int* bins, int* width) {
  if (!cfg) return fail(MKWS_ERR_INVALID_ARG, "cfg is NULL");
  return check_spectral_cfg(*cfg, fft_size, bins, width);
}

int mkws_spectral_num_frames(const mkws_spectral_cfg* cfg, int n_samples) {
  if (!cfg) return fail(MKWS_ERR_INVALID_ARG, "cfg is NULL");
  if (cfg->window_size_samples < 1) return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: window_size_samples %d must be positive", cfg->window_size_samples);
  if (cfg->window_stride_samples < 1) return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: window_stride_samples %d must be positive", cfg->window_stride_samples);
  if (n_samples < cfg->window_size_samples) return 0;
  return 1 + (n_samples - cfg->window_size_samples) / cfg->window_stride_samples;
}

int mkws_spectral_host_table(const mkws_spectral_cfg* cfg, int which, void* dst, size_t cap) {
  if (!cfg) return fail(MKWS_ERR_INVALID_ARG, "cfg is NULL");
  SpectralTables t;
  const int rc = build_spectral_tables(*cfg, &t);
  if (rc != MKWS_OK) return rc;
  const int32_t scalars[8] = {t.window, t.stride, t.fft_size, t.bins, t.width, t.channels, t.start_index, t.end_index};
  const void* src = nullptr;
  size_t n = 0;
  if ((which == MKWS_ST_MEL_WEIGHTS || which == MKWS_ST_BAND_MAPPER || which == MKWS_ST_DCT) && cfg->mode != MKWS_SPECTRAL_MFCC)
    return fail(MKWS_ERR_INVALID_ARG, "table %d exists in mfcc mode only (mode is %d)", which, cfg->mode);
  switch (which) {
    case MKWS_ST_WINDOW: src = t.window_coef.data(); n = t.window_coef.size() * 4; break;
    case MKWS_ST_MEL_WEIGHTS: src = t.mel_weights.data(); n = t.mel_weights.size() * 4; break;
    case MKWS_ST_BAND_MAPPER: src = t.band_mapper.data(); n = t.band_mapper.size() * 4; break;
    case MKWS_ST_DCT: src = t.dct.data(); n = t.dct.size() * 4; break;
    case MKWS_ST_SCALARS: src = scalars; n = sizeof(scalars); break;
    default: return fail(MKWS_ERR_INVALID_ARG, "unknown table id %d", which);
  }
  if (dst && cap > 0) memcpy(dst, src, n < cap ? n : cap);
  return (int)n;
}

int mkws_spectral_create(const mkws_spectral_cfg* cfg, int max_samples, mkws_spectral** out) {
  if (!cfg || !out) return fail(MKWS_ERR_INVALID_ARG, "cfg/out is NULL");
  *out = nullptr;
  if (max_samples <= 0) return fail(MKWS_ERR_INVALID_ARG, "max_samples must be positive");
  mkws_spectral* h = new (std::nothrow) mkws_spectral();
  if (!h) return fail(MKWS_ERR_ALLOC, "out of host memory");
  h->cfg = *cfg;
  int rc = build_spectral_tables(*cfg, &h->tab);
  if (rc == MKWS_OK) rc = require_device();
  if (rc != MKWS_OK) { delete h; return rc; }
  const SpectralTables& t = h->tab;
  const bool mfcc = cfg->mode == MKWS_SPECTRAL_MFCC;
  const int N = t.fft_size, M = N / 2, C = t.channels, W = t.width, bins = t.bins;
  h->lds = sp_carve(N, bins, C, W, mfcc).total;
  if (h->lds > 64 * 1024) { delete h; return fail(MKWS_ERR_UNSUPPORTED, "spectral tables need %zu B of LDS", h->lds); }
  // one device blob
  const size_t o_win = 0, o_tw = sp_al16(o_win + (size_t)N * 4), o_stw = sp_al16(o_tw + (size_t)(M / 2) * 8), o_melw = sp_al16(o_stw + (size_t)(M + 1) * 8),
               o_band = sp_al16(o_melw + (size_t)bins * 4), o_lo = sp_al16(o_band + (size_t)bins * 4), o_hi = sp_al16(o_lo + 64 * 4),
               o_dct = sp_al16(o_hi + 64 * 4), total = sp_al16(o_dct + (size_t)C * W * 4 + 16);
  std::vector<unsigned char> b(total, 0);
  memcpy(b.data() + o_win, t.window_coef.data(), t.window_coef.size() * 4);
  memcpy(b.data() + o_tw, t.twiddles.data(), t.twiddles.size() * 4);
  memcpy(b.data() + o_stw, t.split_twiddles.data(), t.split_twiddles.size() * 4);
  if (mfcc) {
    memcpy(b.data() + o_melw, t.mel_weights.data(), (size_t)bins * 4);
    memcpy(b.data() + o_band, t.band_mapper.data(), (size_t)bins * 4);
    memcpy(b.data() + o_lo, t.chan_lo.data(), (size_t)C * 4);
    memcpy(b.data() + o_hi, t.chan_hi.data(), (size_t)C * 4);
    float* dt = reinterpret_cast<float*>(b.data() + o_dct);
    for (int k = 0; k < W; ++k)
      for (int j = 0; j < C; ++j) dt[(size_t)j * W + k] = t.dct[(size_t)k * C + j];
  }
  h->max_samples = max_samples;
  h->max_frames = mkws_spectral_num_frames(cfg, max_samples);
  const size_t ws = (size_t)(h->max_frames > 0 ? h->max_frames : 1) * W * 4;
  if (hipMalloc(&h->d_blob, total) != hipSuccess) { delete h; return fail(MKWS_ERR_ALLOC, "hipMalloc(%zu) failed", total); }
  if (hipMalloc(reinterpret_cast<void**>(&h->d_frames), ws) != hipSuccess) {
    (void)hipFree(h->d_blob); delete h; return fail(MKWS_ERR_ALLOC, "hipMalloc(%zu) failed", ws);
  }
  if (hipMemcpy(h->d_blob, b.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(h->d_blob); (void)hipFree(h->d_frames); delete h; return fail(MKWS_ERR_HIP, "table upload failed");
  }
  unsigned char* d = static_cast<unsigned char*>(h->d_blob);
  SpectralParams& p = h->prm;
  p.window = reinterpret_cast<const float*>(d + o_win);
  p.tw = reinterpret_cast<const float2*>(d + o_tw);
  p.stw = reinterpret_cast<const float2*>(d + o_stw);
  p.melw = reinterpret_cast<const float*>(d + o_melw);
  p.band = reinterpret_cast<const int*>(d + o_band);
  p.chan_lo = reinterpret_cast<const int*>(d + o_lo);
  p.chan_hi = reinterpret_cast<const int*>(d + o_hi);
  p.dct_t = reinterpret_cast<const float*>(d + o_dct);
  p.window_size = t.window; p.stride = t.stride; p.bins = bins; p.width = W; p.channels = C; p.mode = cfg->mode;
  p.avg_w = mfcc ? 1 : cfg->average_window_width;
  *out = h;
  return MKWS_OK;
}

void mkws_spectral_destroy(mkws_spectral* h) {
  if (!h) return;
  if (h->d_blob) (void)hipFree(h->d_blob);
  if (h->d_frames) (void)hipFree(h->d_frames);
  delete h;
}

}  // extern "C"

namespace {

template <typename T>
int spectral_launch(const mkws_spectral* h, const T* d_audio, int B, int n_samples, int frames, int frames_per_block, float* d_feat, float* d_power,
                    float* d_mel, hipStream_t s) {
  const dim3 grid(B, (frames + frames_per_block - 1) / frames_per_block), block(kSpWaves * 64);
  switch (h->tab.fft_size) {
    case 256: hipLaunchKernelGGL((spectral_kernel<T, 256>), grid, block, h->lds, s, h->prm, d_audio, n_samples, frames, frames_per_block, d_feat, d_power, d_mel); break;
    case 512: hipLaunchKernelGGL((spectral_kernel<T, 512>), grid, block, h->lds, s, h->prm, d_audio, n_samples, frames, frames_per_block, d_feat, d_power, d_mel); break;
    default: hipLaunchKernelGGL((spectral_kernel<T, 1024>), grid, block, h->lds, s, h->prm, d_audio, n_samples, frames, frames_per_block, d_feat, d_power, d_mel); break;
  }
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

template <typename T>
int spectral_forward_impl(mkws_spectral* h, const T* d_audio, int B, int n_samples, float* d_feat, float* d_power, float* d_mel, void* stream) {
  if (!h) return fail(MKWS_ERR_INVALID_ARG, "spectral handle is NULL");
  if (B < 0 || n_samples < 0) return fail(MKWS_ERR_INVALID_ARG, "negative batch or sample count");
  if (n_samples > h->max_samples) return fail(MKWS_ERR_INVALID_ARG, "n_samples %d exceeds max_samples %d given at create", n_samples, h->max_samples);
  if (d_mel && h->cfg.mode != MKWS_SPECTRAL_MFCC) return fail(MKWS_ERR_INVALID_ARG, "d_mel: the average mode has no filterbank to tap");
  const int frames = mkws_spectral_num_frames(&h->cfg, n_samples);
  if (B == 0 || frames == 0) return MKWS_OK;
  if (!d_audio || !d_feat) return fail(MKWS_ERR_INVALID_ARG, "d_audio / d_feat is NULL");
  return spectral_launch<T>(h, d_audio, B, n_samples, frames, frames, d_feat, d_power, d_mel, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

int mkws_spectral_forward_f32(mkws_spectral* h, const float* d_audio, int B, int n_samples, float* d_feat, float* d_power, float* d_mel, void* stream) {
  return spectral_forward_impl<float>(h, d_audio, B, n_samples, d_feat, d_power, d_mel, stream);
}

int mkws_spectral_forward_i16(mkws_spectral* h, const int16_t* d_audio, int B, int n_samples, float* d_feat, float* d_power, float* d_mel, void* stream) {
  return spectral_forward_impl<int16_t>(h, d_audio, B, n_samples, d_feat, d_power, d_mel, stream);
}

int mkws_spectral_stream_f32(mkws_spectral* h, const float* d_audio, int n_samples, int window_samples, int hop_samples, float* d_feat, int max_windows,
                             void* stream) {
  if (!h) return fail(MKWS_ERR_INVALID_ARG, "spectral handle is NULL");
  if (n_samples < 0 || window_samples <= 0 || hop_samples <= 0) return fail(MKWS_ERR_INVALID_ARG, "n_samples / window_samples / hop_samples: bad sample counts");
  if (n_samples > h->max_samples) return fail(MKWS_ERR_INVALID_ARG, "n_samples %d exceeds max_samples %d given at create", n_samples, h->max_samples);
  const int stride = h->prm.stride;
  if (hop_samples % stride != 0)
    return fail(MKWS_ERR_UNSUPPORTED, "hop_samples %d is not a multiple of the %d-sample frame stride (frame sharing needs that)", hop_samples, stride);
  const int fpw = mkws_spectral_num_frames(&h->cfg, window_samples);
  if (n_samples < window_samples) return 0;
  const int num_windows = 1 + (n_samples - window_samples) / hop_samples;
  if (num_windows > max_windows) return fail(MKWS_ERR_INVALID_ARG, "%d windows exceed max_windows %d", num_windows, max_windows);
  if (fpw <= 0) return num_windows;
  if (!d_audio || !d_feat) return fail(MKWS_ERR_INVALID_ARG, "d_audio / d_feat is NULL");
  const int hop_frames = hop_samples / stride;
  const long long total_frames = (long long)(num_windows - 1) * hop_frames + fpw;     // all of them lie inside n_samples <= max_samples
  if (total_frames > h->max_frames) return fail(MKWS_ERR_INVALID_ARG, "%lld frames exceed the %d of max_samples", total_frames, h->max_frames);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = spectral_launch<float>(h, d_audio, 1, n_samples, (int)total_frames, kSpStreamFrames, h->d_frames, nullptr, nullptr, s);
  if (rc != MKWS_OK) return rc;
  const size_t total = (size_t)num_windows * fpw * h->prm.width;
  size_t grid = (total + 255) / 256;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(spectral_windows_kernel, dim3((unsigned)grid), dim3(256), 0, s, h->d_frames, hop_frames, fpw, h->prm.width, total, d_feat);
  MKWS_HIP(hipGetLastError());
  return num_windows;
}

}  // extern "C"
