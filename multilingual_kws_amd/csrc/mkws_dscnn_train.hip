// DS-CNN baseline, training operators (include/mkws.h "DS-CNN baseline, training").
//
// What the training step of the DS-CNN needs beyond the operators of mkws_train.hip:
//   stem        the 10x4 stride-2 SAME convolution in training form: raw output for the BatchNorm operator, and its weight gradient.
//               Both on v_mfma_f32_16x16x4_f32 with the patches gathered on the fly from the spectrograms (which stay in L2: 7.8 KB a clip).
//   dropout     counter-based: the keep decision of element i is a hash of (seed, *d_step, site, i), so nothing is stored, the backward
//               pass regenerates the mask, and a captured step draws fresh masks on every replay (the step counter lives on the device).
//   pool        Dropout + the mean over rows 0..23, and its backward.
// Conventions as in mkws_train.hip: device float32, NHWC viewed as [M, C], asynchronous on the given stream, no allocation, no
// synchronisation, cross-workgroup sums two-level and in index order through the bound context's scratch arena.
#include <cstdint>

#include "mkws_common.h"

using mkws::fail;

#define MKWS_REQ(cond, ...) do { if (!(cond)) return fail(MKWS_ERR_INVALID_ARG, __VA_ARGS__); } while (0)

namespace {

constexpr int kInH = 49, kInW = 40, kSpec = kInH * kInW;
constexpr int kH = 25, kW = 20, kC = 64, kPix = kH * kW;
constexpr int kPoolRows = 24, kPoolPix = kPoolRows * kW;     // int(49 / 2): row 24 is computed and not pooled
constexpr int kKH = 10, kKW = 4, kTaps = kKH * kKW;
constexpr int kPadTop = 4, kPadLeft = 1;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- dropout mask ------------------------------------------------------------------------------------------------------------------
// splitmix64 as multilingual_kws_amd/synth.py has it; dscnn_trainer.dropout_mask_host is the host twin of mask_base / mask_keep.
__device__ __host__ inline uint64_t splitmix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __host__ inline uint64_t mask_base(uint64_t seed, uint64_t step, uint64_t site) {
  return splitmix64(splitmix64(splitmix64(seed) + step) + site);
}
// element i is kept when the top 24 bits of its hash reach `thresh` = floor(rate * 2^24)
__device__ inline bool mask_keep(uint64_t base, uint64_t i, uint32_t thresh) {
  return (uint32_t)(splitmix64(base + (i + 1) * 0x9E3779B97F4A7C15ull) >> 40) >= thresh;
}

__global__ __launch_bounds__(256) void dropout_kernel(const float* X, float* out /* may be X */, size_t n, uint64_t seed, const int* __restrict__ d_step,
                                                      uint64_t site, uint32_t thresh, float scale, int vec) {
  const uint64_t base = mask_base(seed, (uint64_t)(uint32_t)*d_step, site);
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  if (vec) {                                                   // both pointers 16-byte aligned: four elements a thread, then the tail
    const size_t n4 = n >> 2;
    for (size_t q = tid; q < n4; q += stride) {
      const f32x4 x = reinterpret_cast<const f32x4*>(X)[q];
      f32x4 y;
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = mask_keep(base, 4 * q + r, thresh) ? x[r] * scale : 0.0f;
      reinterpret_cast<f32x4*>(out)[q] = y;
    }
    const size_t i = 4 * n4 + tid;
    if (i < n) out[i] = mask_keep(base, i, thresh) ? X[i] * scale : 0.0f;
  } else {
    for (size_t i = tid; i < n; i += stride) out[i] = mask_keep(base, i, thresh) ? X[i] * scale : 0.0f;
  }
}

// ---- pool --------------------------------------------------------------------------------------------------------------------------
// pooled[b][c] = scale / 480 * sum over the kept cells of rows 0..23.  One workgroup per clip, lane = channel, the four waves take the cells
// q = wave, wave + 4, ...; float64 sums (480 terms; the inference kernel does the same), the four partial sums folded in wave order.
__global__ __launch_bounds__(256) void pool_fwd_kernel(const float* __restrict__ A, float* __restrict__ pooled, uint64_t seed, const int* __restrict__ d_step,
                                                       uint64_t site, uint32_t thresh, float scale) {
  __shared__ double s_part[4][kC];
  const uint64_t base = mask_base(seed, (uint64_t)(uint32_t)*d_step, site);
  const int b = blockIdx.x, c = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t clip0 = (size_t)b * (kPix * kC);
  double sum = 0.0;
#pragma unroll 4
  for (int q = wave; q < kPoolPix; q += 4) {
    const size_t i = clip0 + (size_t)q * kC + c;
    const float v = A[i];
    sum += mask_keep(base, i, thresh) ? (double)v : 0.0;
  }
  s_part[wave][c] = sum;
  __syncthreads();
  if (wave == 0) {
    const double t = ((s_part[0][c] + s_part[1][c]) + s_part[2][c]) + s_part[3][c];
    pooled[(size_t)b * kC + c] = (float)(t * (double)scale / (double)kPoolPix);
  }
}

// dA[b][q][c] = kept ? dpooled[b][c] * gscale : 0 for q < 480 (gscale = scale / 480), exact zeros in row 24.  Four channels a thread.
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ dpooled, float* __restrict__ dA, size_t n4, uint64_t seed,
                                                       const int* __restrict__ d_step, uint64_t site, uint32_t thresh, float gscale) {
  const uint64_t base = mask_base(seed, (uint64_t)(uint32_t)*d_step, site);
  for (size_t q4 = (size_t)blockIdx.x * 256 + threadIdx.x; q4 < n4; q4 += (size_t)gridDim.x * 256) {
    const size_t pix = q4 >> 4;                                // 16 quads per pixel
    const int c4 = (int)(q4 & 15);
    const size_t b = pix / kPix;
    const int q = (int)(pix - b * kPix);
    f32x4 y = {0.0f, 0.0f, 0.0f, 0.0f};
    if (q < kPoolPix) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(dpooled + b * kC + 4 * c4);
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = mask_keep(base, 4 * q4 + r, thresh) ? g[r] * gscale : 0.0f;
    }
    reinterpret_cast<f32x4*>(dA)[q4] = y;
  }
}

// ---- stem ----------------------------------------------------------------------------------------------------------------------------
// patch element (pixel p of the [B*500] rows, tap k = 4 ky + kx) = spec[b][2 oy + ky - 4][2 ox + kx - 1], zero outside the 49 x 40
__device__ __forceinline__ float patch_at(const float* __restrict__ spec, int p, int npix, int ky, int kx) {
  const int pc = p < npix ? p : npix - 1;
  const int b = pc / kPix, r = pc - b * kPix, oy = r / kW, ox = r - oy * kW;
  const int iy = 2 * oy + ky - kPadTop, ix = 2 * ox + kx - kPadLeft;
  const bool ok = p < npix && ky < kKH && iy >= 0 && iy < kInH && ix >= 0 && ix < kInW;
  const float v = spec[(size_t)b * kSpec + (ok ? iy * kInW + ix : 0)];          // read from a valid address either way, so that the loads issue together
  return ok ? v : 0.0f;
}

// Z [B*500, 64] = patches [B*500, 40] . W [40, 64].  A wave owns tiles of 16 pixels x 64 channels: one k-step of the MFMA is one kernel row
// (the four lane groups are the four kernel columns), the four accumulators are the four 16-channel slabs; the wave keeps W in 40 registers.
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ spec, const float* __restrict__ W, float* __restrict__ Z, int npix, int tiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i16 = lane & 15;
  float bw[kKH][4];
#pragma unroll
  for (int ky = 0; ky < kKH; ++ky)
#pragma unroll
    for (int n = 0; n < 4; ++n) bw[ky][n] = W[(ky * kKW + g) * kC + 16 * n + i16];
#pragma unroll 1
  for (int t = blockIdx.x * 4 + wave; t < tiles; t += gridDim.x * 4) {
    float a[kKH];
#pragma unroll
    for (int ky = 0; ky < kKH; ++ky) a[ky] = patch_at(spec, 16 * t + i16, npix, ky, g);
    f32x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ky = 0; ky < kKH; ++ky)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ky], bw[ky][n], acc[n], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = 16 * t + 4 * g + r;                        // result row 4 g + r, column i16
      if (p < npix) {
#pragma unroll
        for (int n = 0; n < 4; ++n) Z[(size_t)p * kC + 16 * n + i16] = acc[n][r];
      }
    }
  }
}

// dW [40, 64] = patches^T . dZ, summed over the pixels.  The MFMA's rows are the taps (three tiles of 16: taps 40..47 are zero padding), its
// columns the channels, and one k-step sums four pixels (one per lane group).  A wave walks `wave_px` pixels (a multiple of four) in order, the
// four waves of a workgroup are folded in wave order through LDS, and the workgroup leaves its [40, 64] in part[blockIdx.x]: every sum has a
// fixed order.
__global__ __launch_bounds__(256) void stem_bwd_weight_kernel(const float* __restrict__ spec, const float* __restrict__ dZ, float* __restrict__ part, int npix,
                                                              int wave_px) {
  __shared__ float s_w[3][kTaps * kC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i16 = lane & 15;
  const int p0 = (blockIdx.x * 4 + wave) * wave_px;
  f32x4 acc[3][4];
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
  for (int s = 0; s < wave_px; s += 4) {
    const int p = p0 + s + g;                                  // this lane group's pixel of the k-step
    float a[3], bz[4];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const int k = 16 * m + i16;
      a[m] = patch_at(spec, p, npix, k >> 2, k & 3);           // (k >= 40: ky >= 10, zero)
    }
    const bool ok = p < npix;
    const float* row = dZ + (size_t)(ok ? p : 0) * kC + i16;
#pragma unroll
    for (int n = 0; n < 4; ++n) { const float v = row[16 * n]; bz[n] = ok ? v : 0.0f; }
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], bz[n], acc[m][n], 0, 0, 0);
  }
  // result row (tap) 16 m + 4 g + r, column (channel) 16 n + i16
  if (wave > 0) {
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * m + 4 * g + r;
        if (k < kTaps) {
#pragma unroll
          for (int n = 0; n < 4; ++n) s_w[wave - 1][k * kC + 16 * n + i16] = acc[m][n][r];
        }
      }
  }
  __syncthreads();
  if (wave == 0) {
    float* mine = part + (size_t)blockIdx.x * (kTaps * kC);
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * m + 4 * g + r;
        if (k < kTaps) {
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            const int i = k * kC + 16 * n + i16;
            mine[i] = ((acc[m][n][r] + s_w[0][i]) + s_w[1][i]) + s_w[2][i];
          }
        }
      }
  }
}

// second stage: dW[i] = sum over the workgroups' partials in index order
__global__ __launch_bounds__(256) void stem_fold_kernel(const float* __restrict__ part, int chunks, float* __restrict__ dW) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= kTaps * kC) return;
  float v = part[i];
#pragma unroll 8
  for (int z = 1; z < chunks; ++z) v += part[(size_t)z * (kTaps * kC) + i];      // (unrolled: eight loads in flight, the adds stay in index order)
  dW[i] = v;
}

inline int grid_for(size_t work_items) {
  const size_t cap = (size_t)mkws::train_grid_cap();
  const size_t g = (work_items + 255) / 256;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

inline bool rate_ok(float rate) { return rate >= 0.0f && rate < 1.0f; }
inline uint32_t rate_thresh(float rate) { return (uint32_t)(rate * 16777216.0f); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int dropout_launch(const float* X, float* out, int64_t n, float rate, uint64_t seed, const int* d_step, int site, void* stream) {
  MKWS_REQ(X && out && d_step && n > 0 && site >= 0 && rate_ok(rate), "dropout: bad arguments (rate in [0, 1), site >= 0, n > 0)");
  const int vec = aligned16(X) && aligned16(out);
  hipLaunchKernelGGL(dropout_kernel, dim3(grid_for(vec ? ((size_t)n + 3) / 4 : (size_t)n)), dim3(256), 0, static_cast<hipStream_t>(stream), X, out, (size_t)n, seed, d_step,
                     (uint64_t)site, rate_thresh(rate), 1.0f / (1.0f - rate), vec);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

}  // namespace

extern "C" {

int mkws_op_dscnn_stem_fwd(const float* d_spec, const float* d_W, float* d_Z, int B, void* stream) {
  MKWS_REQ(d_spec && d_W && d_Z && B > 0 && B <= (1 << 20), "dscnn_stem_fwd: bad arguments");
  const int npix = B * kPix, tiles = (npix + 15) / 16;
  int grid = (tiles + 3) / 4;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(stem_fwd_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), d_spec, d_W, d_Z, npix, tiles);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

int mkws_op_dscnn_stem_bwd_weight(const float* d_spec, const float* d_dZ, float* d_dW, int B, void* stream) {
  MKWS_REQ(d_spec && d_dZ && d_dW && B > 0 && B <= (1 << 20), "dscnn_stem_bwd_weight: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int npix = B * kPix;
  int target = (npix + 63) / 64;                               // 16 pixels a wave at the least, 256 workgroups at the most
  if (target > 256) target = 256;
  const int wave_px = ((npix + 4 * target - 1) / (4 * target) + 3) & ~3;
  const int grid = (npix + 4 * wave_px - 1) / (4 * wave_px);
  float* part = mkws::train_scratch_at((size_t)grid * (kTaps * kC), s);
  MKWS_REQ(part, "dscnn_stem_bwd_weight: needs %zu floats of scratch (mkws_train_ctx_create / mkws_op_set_scratch)", (size_t)grid * (kTaps * kC));
  hipLaunchKernelGGL(stem_bwd_weight_kernel, dim3(grid), dim3(256), 0, s, d_spec, d_dZ, part, npix, wave_px);
  hipLaunchKernelGGL(stem_fold_kernel, dim3((kTaps * kC + 255) / 256), dim3(256), 0, s, part, grid, d_dW);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

int mkws_op_dropout_fwd(const float* d_X, float* d_out, int64_t n, float rate, uint64_t seed, const int* d_step, int site, void* stream) {
  return dropout_launch(d_X, d_out, n, rate, seed, d_step, site, stream);
}

int mkws_op_dropout_bwd(const float* d_dOut, float* d_dX, int64_t n, float rate, uint64_t seed, const int* d_step, int site, void* stream) {
  return dropout_launch(d_dOut, d_dX, n, rate, seed, d_step, site, stream);
}

int mkws_op_dscnn_pool_fwd(const float* d_A, int B, float rate, uint64_t seed, const int* d_step, int site, float* d_pooled, void* stream) {
  MKWS_REQ(d_A && d_pooled && d_step && B > 0 && B <= (1 << 20) && site >= 0 && rate_ok(rate), "dscnn_pool_fwd: bad arguments (rate in [0, 1), site >= 0)");
  hipLaunchKernelGGL(pool_fwd_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), d_A, d_pooled, seed, d_step, (uint64_t)site, rate_thresh(rate),
                     1.0f / (1.0f - rate));
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

int mkws_op_dscnn_pool_bwd(const float* d_dpooled, int B, float rate, uint64_t seed, const int* d_step, int site, float* d_dA, void* stream) {
  MKWS_REQ(d_dpooled && d_dA && d_step && B > 0 && B <= (1 << 20) && site >= 0 && rate_ok(rate), "dscnn_pool_bwd: bad arguments (rate in [0, 1), site >= 0)");
  MKWS_REQ(aligned16(d_dpooled) && aligned16(d_dA), "dscnn_pool_bwd: d_dpooled and d_dA must be 16-byte aligned");
  const size_t n4 = (size_t)B * kPix * (kC / 4);
  hipLaunchKernelGGL(pool_bwd_kernel, dim3(grid_for(n4)), dim3(256), 0, static_cast<hipStream_t>(stream), d_dpooled, d_dA, n4, seed, d_step, (uint64_t)site,
                     rate_thresh(rate), (1.0f / (1.0f - rate)) / (float)kPoolPix);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

}  // extern "C"
