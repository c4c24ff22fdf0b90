// mkws_embed.hip -- EfficientNet-B0 (49x40x1) + GAP + Dense 2048/2048/1024 forward on gfx950, fp32.
//
// Replaces `embedding.predict(x)` of the Keras model defined at
// multilingual_kws/train_multilingual_embedding.py:58-83 (cut at "dense_2" by
// multilingual_kws/embedding/transfer_learning.py:36-43).  Layer table: SURVEY.md Appendix B.
//
// Layout: activations NHWC fp32, viewed as row-major [M = B*H*W, C].  Every contraction with K >= 16 runs on the exact-fp32
// MFMA (v_mfma_f32_16x16x4_f32) TRANSPOSED: packed weights are the "A" operand, activation rows the "B" operand, so a lane ends
// up with 4 consecutive output channels of one row (float4 stores).  The reduction index is permuted (lane group g of chunk j
// owns k = 16j+4g..+3) and the weights are pre-packed on the host in exactly that order: operands go memory -> registers as
// float4 without an LDS transpose.  Kernels (DESIGN.md section 4 has the measured numbers):
//   stem_block1a_kernel          stem conv + whole block 1a, a workgroup walks clips
//   mbconv_front_kernel          expand (MFMA) + BN + swish -> LDS -> depthwise + BN + swish, SE sums
//   mbconv_back_kernel           SE FCs + gated projection + BN (+ residual) behind the front kernel
//   mbconv_mid_kernel            whole block, big images (2a .. 4a), depthwise output resident in LDS
//   mbconv_block_kernel          whole block, 4x3 / 2x2 images (4b .. 7a), 4, 2 or 1 clips per workgroup
//   mbconv_chain_kernel          consecutive 4x3-image blocks in one launch, activations in LDS
//   mbconv_pair_kernel           whole block, stride-1 2x2 images (6b .. 7a): two workgroups of one XCD share the clips, split the channels
//   mbconv_pair_chain_kernel     consecutive paired blocks in one launch, optionally + top conv + global average pool
//   mbconv_cluster_kernel        whole block, 4x3 / 2x2 images: up to 14 workgroups share one 16-row tile and split the channels
//   mbconv_cluster_chain_kernel  every cluster block of a one-clip forward in one launch
//   pw_gemm_kernel               top conv (+ pool), dense layers, every 1x1 conv of the unfused path (+ splitk_reduce_kernel when K is split)
//   gemv_kernel                  the same layers at up to 4 rows (one clip)
//   stem_kernel, dw_kernel, se_reduce / se_expand_kernel, mean_hw_kernel: the unfused path (parity taps, A/B options)
// Which of them a forward pass launches is decided per block by route_block() from the handle's options, and those default by handle
// size at create.  With the defaults, no tap, and the pair probe passed (pair_layout_ok), per block group:
//   1a            every handle: inside stem_block1a_kernel                                                              1 launch
//   2a .. 4a      one clip: front + back per block (10); larger: mid for 2b, 3a, 4a, front + back for 2a, 3b             10 / 7
//   4b .. 6a      one clip: ONE cluster chain launch for 4b .. 7a; up to kClusterMaxBatch (32) clips: a cluster
//                 launch per block (6); larger: ONE chain launch                                                          1 / 6 / 1
//   6b .. 7a, top one clip: in the cluster chain above, top conv + pool on gemv (1); up to 32: a cluster launch per block
//                 + pw_gemm with the pool (5); larger: ONE pair chain launch that ends in the top conv + pool             1 / 5 / 1
//   dense x 3     up to 4 clips: gemv (3); larger: pw_gemm, + a split-K fold for every layer pick_tile() splits           3 .. 6
// Launches per forward: one clip 16; 2 .. 4 clips 22; 5 .. 32 clips 25; 33 .. 256 clips 14 at 256 (dense_2 splits K); larger 13 at 1024.
// Handles of 129 .. 256 clips differ from larger ones in workgroup shape only: one clip per workgroup of 4a's mid kernel and of the chain.
// Without the probe the pair / cluster kernels fall to mbconv_block_kernel.  tests/golden/embed_launch_sequences.json records the sequences.
// Streaming loops address their operands as buffer descriptor + per-lane 32-bit offset + SGPR chunk offset (WBuf): VALU and MFMA
// work serialize on a SIMD of this part, so the MFMA loops contain no VALU instructions.
#include "mkws_common.h"
#include "mkws_embed_arch.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

// fp32 multiply-adds of the convolution / epilogue code may fuse (v_pk_fma_f32): one rounding instead of two,
// like the MFMA accumulation itself; the build's default (-ffp-contract=off) stays in force for the other files.
#pragma clang fp contract(fast)
#include "mkws_embed_dev.h"

namespace mkws {

// value the optimizer cannot see through (stops loop-invariant hoisting of cheap index arithmetic into spilled registers)
__device__ __forceinline__ int opaque_(int v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case ACT_SWISH: return swishf_(v);
    case ACT_RELU: return v > 0.0f ? v : 0.0f;
    case ACT_SELU: return 1.0507009873554805f * (v > 0.0f ? v : 1.6732632423543772f * expm1f(v));
    case ACT_SIGMOID: return sigmoidf_(v);
    default: return v;
  }
}
__device__ __forceinline__ f32x4 apply_act4(f32x4 v, int act) {
  if (act == ACT_SWISH) return swish4_(v);
  if (act == ACT_SIGMOID) return sigmoid4_(v);
  v.x = apply_act(v.x, act); v.y = apply_act(v.y, act); v.z = apply_act(v.z, act); v.w = apply_act(v.w, act);
  return v;
}

// ------------------------------------------------------------------------------------------------
#ifdef MKWS_FRONT_TIMING
// timing build: every workgroup of the early-block kernels leaves (start, end, CU id) so that the host can rebuild the per-CU
// timeline: how many workgroups were resident at a time and how long a CU's slots sat empty between workgroups.
__device__ unsigned long long* g_wgtrace = nullptr;
__device__ int g_ablate = 0;            // MKWS_ABLATE bit mask: phases a kernel SKIPS (wrong results, honest timing of what is left)
#define MKWS_ABLATE(bit) (g_ablate & (bit))
__device__ __forceinline__ void wg_trace_begin() {
  if (threadIdx.x == 0 && g_wgtrace) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    unsigned long long* p = g_wgtrace + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
    p[0] = wall_clock64();
    p[2] = ((unsigned long long)(xcc & 15) << 8) | ((hw >> 8) & 0xff);
  }
}
__device__ __forceinline__ void wg_trace_end() {
  __syncthreads();
  if (threadIdx.x == 0 && g_wgtrace) g_wgtrace[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + 1] = wall_clock64();
}
// per-phase shader-clock sums of a persistent workgroup (thread 0): MKWS_PH_DECL; MKWS_PH(k) after phase k; MKWS_PH_STORE at the end
#define MKWS_PH_DECL long long ph_acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}; long long ph_t_ = clock64()
#define MKWS_PH(k) do { const long long n_ = clock64(); ph_acc_[k] += n_ - ph_t_; ph_t_ = n_; } while (0)
#define MKWS_PH_STORE() do { if (threadIdx.x == 0 && g_wgtrace) { unsigned long long* p_ = g_wgtrace + 3 * 131072 + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8; \
    for (int k_ = 0; k_ < 8; ++k_) p_[k_] = (unsigned long long)ph_acc_[k_]; } } while (0)
#define MKWS_WG_BEGIN() wg_trace_begin()
#define MKWS_WG_END() wg_trace_end()
// mbconv_mid_kernel: thread 0 adds the wall-clock time since its last stamp to slot k of an LDS table that it copies out at the end
// (timing_report_mid prints the means).  Slots: 0 start, 1 prologue, 2 + 4 * chunk + {0 P1 tasks of wave 0 done, 1 P1 constants stored +
// barrier passed, 2 P2 items done, 3 P2 constants stored + barrier passed}, 26.. SE tail per barrier, 32 projection: wait for the
// weight ring, 33 projection MFMA loop + epilogue of wave 0, 34 last wave done, 35 end.
constexpr int kMidStamps = 40, kMidStampSE = 26, kMidStampProj = 32;
constexpr int kMidStampFloats = 2 * kMidStamps + 2;     // the table follows the kernel's LDS carve
#define MID_STAMP(k) do { if (threadIdx.x == 0) { const unsigned long long t_ = wall_clock64(); s_stamp[k] += t_ - t_mark; t_mark = t_; } } while (0)
#else
#define MID_STAMP(k)
constexpr int kMidStampFloats = 0;
#define MKWS_WG_BEGIN()
#define MKWS_WG_END()
#define MKWS_ABLATE(bit) false
#define MKWS_PH_DECL
#define MKWS_PH(k)
#define MKWS_PH_STORE()
#endif

// stem: spec [B,49,40] -> [B,25,20,32]; ZeroPadding2D(((1,1),(0,1))) + Conv2D(32,3,s2,valid) + BN + swish
// 8 threads per output pixel, each 4 output channels (float4 store, fully coalesced).
__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ spec, const float* __restrict__ w /*[9][32]*/,
                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                   float norm_mean, float norm_std, float* __restrict__ out, int B) {
  constexpr int H = kInH, W = kInW, Ho = 25, Wo = 20;
  const int q = threadIdx.x & 7;
  f32x4 wk[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wk[t] = *reinterpret_cast<const f32x4*>(w + t * 32 + q * 4);
  const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + q * 4);
  const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + q * 4);
  const long total = (long)B * Ho * Wo;
  for (long pix = (long)blockIdx.x * 32 + (threadIdx.x >> 3); pix < total; pix += (long)gridDim.x * 32) {
    const int b = (int)(pix / (Ho * Wo));
    const int r = (int)(pix % (Ho * Wo));
    const int oh = r / Wo, ow = r % Wo;
    const float* img = spec + (size_t)b * H * W;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int ih = oh * 2 - 1 + i;          // pad top 1
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int iw = ow * 2 + j;            // pad left 0
        float v = 0.0f;
        if (ih >= 0 && ih < H && iw < W) v = __fdiv_rn(img[ih * W + iw] * (1.0f / 255.0f) - norm_mean, norm_std);
        acc += wk[i * 3 + j] * v;
      }
    }
    f32x4 y = acc * sc + sh;
    y = swish4_(y);
    *reinterpret_cast<f32x4*>(out + pix * 32 + q * 4) = y;
  }
}

// ------------------------------------------------------------------------------------------------
// Stem + the whole of block 1a (no expand conv: depthwise 3x3 -> SE -> gated 32->16 projection) for one clip
// per workgroup.  Spectrogram [49,40] in, block-1a output [25,20,16] out; the 64 KB stem output and the 64 KB
// depthwise output stay in LDS, so the network's two largest activations never reach HBM.
//   1. input tile (+Rescaling/Normalization) -> LDS;  2. stem 3x3 s2 conv + BN + swish -> s_E (zero halo)
//   3. depthwise 3x3 + BN + swish -> s_D [500][36], channel sums by shuffles
//   4. SE: r = swish(mean.Wr + br) (8 units), gate = sigmoid(r.We + be)                    (VALU, tiny)
//   5. projection on the fp32 MFMA: weights (A operand, 2 K chunks) in registers, (D * gate) rows from LDS
__global__ __launch_bounds__(512) void stem_block1a_kernel(const float* __restrict__ spec, const float* __restrict__ w /*[9][32]*/,
                                                           const float* __restrict__ scale, const float* __restrict__ shift, float norm_mean,
                                                           float norm_std, const float* __restrict__ Wd /*[9][32]*/, const float* __restrict__ scD,
                                                           const float* __restrict__ shD, const float* __restrict__ Wr /*[32][se]*/,
                                                           const float* __restrict__ br, const float* __restrict__ We /*[se][32]*/,
                                                           const float* __restrict__ be, int se, const float* __restrict__ WpP,
                                                           const float* __restrict__ scP, const float* __restrict__ shP, float* __restrict__ Y, int B) {
  constexpr int H = kInH, W = kInW, Ho = 25, Wo = 20, C = 32, CO = 16, NTHR = 512;
  MKWS_WG_BEGIN();
  constexpr int TH = H + 2, TW = W + 1;                 // input tile with halo: rows -1..49, cols 0..40
  constexpr int EH = Ho + 2, EW = Wo + 2;               // stem-output tile with a 1-pixel zero halo
  constexpr int LDD = C + 4;                            // depthwise-output row stride (conflict-free MFMA operand reads)
  constexpr int NIN = (TH * TW + NTHR - 1) / NTHR;      // input-tile elements per thread
  constexpr int NRT = (Ho * Wo + 15) / 16, RTW = NRT / (NTHR / 64);      // projection row tiles, per wave
  static_assert(RTW * (NTHR / 64) == NRT, "every wave owns the same number of projection row tiles");
  extern __shared__ __attribute__((aligned(16))) float s_sb[];
  float* s_in = s_sb;                                   // [TH][TW]
  float* s_E = s_in + ((TH * TW + 3) & ~3);             // [EH][EW][C]
  float* s_D = s_E + EH * EW * C;                       // [Ho*Wo][LDD]
  f32x4* s_red = reinterpret_cast<f32x4*>(s_D + Ho * Wo * LDD);   // [8 waves][8 quads]
  float* s_gate = reinterpret_cast<float*>(s_red + 64);  // [32]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform by construction: keeps wave-dependent offsets / branches on the scalar unit
  // The workgroup is PERSISTENT: it walks clips blockIdx.x, + gridDim.x, ... (one workgroup per CU fits: 157 KB of LDS), so the
  // constants below are fetched once per CU instead of once per clip, and the NEXT clip's spectrogram is requested (into registers)
  // while this clip computes: the ~2 us a lone workgroup waited for its input at the top of every clip are gone.
  int ioff[NIN];                                        // this thread's input-tile elements: image offset, -1 = zero halo, -2 = none
#pragma unroll
  for (int k = 0; k < NIN; ++k) {
    const int i = tid + k * NTHR;
    const int r = i / TW - 1, cc = i % TW;
    ioff[k] = (i < TH * TW) ? ((r >= 0 && r < H && cc < W) ? r * W + cc : -1) : -2;
  }
  float pre[NIN];
  auto request = [&](size_t clip) {
    const float* img = spec + clip * H * W;
#pragma unroll
    for (int k = 0; k < NIN; ++k) pre[k] = (ioff[k] >= 0) ? img[ioff[k]] : 0.0f;
  };
  if (blockIdx.x < (unsigned)B) request(blockIdx.x);
  for (int i = tid; i < EH * EW * C / 4; i += NTHR) {    // zero the halo once (the interior is overwritten by every clip)
    const int pix = i / (C / 4);
    const int r = pix / EW, cc = pix % EW;
    if (r == 0 || r == EH - 1 || cc == 0 || cc == EW - 1) reinterpret_cast<f32x4*>(s_E)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const int q = tid & 7;                                 // channel quad of this thread
  const int g = lane >> 4, c = lane & 15;
  // SE constants of wave 0.  Reduce: lane = (channel group cg = lane >> 3 of 4 channels, unit n = lane & 7);  expand: lane = channel.
  const int se_n = lane & 7, se_cg = lane >> 3, ch = lane & 31;
  float wr4[4] = {0.f, 0.f, 0.f, 0.f}, we8[8], br_n = 0.0f, be_c = 0.0f;
#pragma unroll
  for (int n = 0; n < 8; ++n) we8[n] = 0.0f;
  if (wave == 0) {
    if (se_n < se) {
#pragma unroll
      for (int i = 0; i < 4; ++i) wr4[i] = Wr[(4 * se_cg + i) * se + se_n];
      br_n = br[se_n];
    }
#pragma unroll
    for (int n = 0; n < 8; ++n)
      if (n < se) we8[n] = We[n * C + ch];
    be_c = be[ch];
  }
  f32x4 wp[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) wp[j] = *reinterpret_cast<const f32x4*>(WpP + ((size_t)j * 4 + g) * 64 + c * 4);
  const f32x4 scp = *reinterpret_cast<const f32x4*>(scP + 4 * g), shp = *reinterpret_cast<const f32x4*>(shP + 4 * g);
  f32x4 wk[9], wkd[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) { wk[t] = *reinterpret_cast<const f32x4*>(w + t * C + q * 4); wkd[t] = *reinterpret_cast<const f32x4*>(Wd + t * C + q * 4); }
  const f32x4 sc_s = *reinterpret_cast<const f32x4*>(scale + q * 4), sh_s = *reinterpret_cast<const f32x4*>(shift + q * 4);
  const f32x4 sc_d = *reinterpret_cast<const f32x4*>(scD + q * 4), sh_d = *reinterpret_cast<const f32x4*>(shD + q * 4);
  // input tile of a clip: Rescaling(1/255) + Normalization on the way from the prefetch registers into LDS
  auto stage = [&]() {
#pragma unroll
    for (int k = 0; k < NIN; ++k)
      if (ioff[k] != -2) s_in[tid + k * NTHR] = (ioff[k] >= 0) ? __fdiv_rn(pre[k] * (1.0f / 255.0f) - norm_mean, norm_std) : 0.0f;
  };
  MKWS_PH_DECL;
  if (blockIdx.x < (unsigned)B) {
    stage();
    if (blockIdx.x + gridDim.x < (unsigned)B) request((size_t)blockIdx.x + gridDim.x);
  }
  __syncthreads();
  MKWS_PH(0);

  for (size_t b = blockIdx.x; b < (size_t)B; b += gridDim.x) {
    // 1. stem conv (s_in holds this clip; the clip after it is on its way into the prefetch registers)
    {
      const f32x4 sc = sc_s, sh = sh_s;
      for (int pix = tid >> 3; pix < Ho * Wo; pix += NTHR / 8) {
        const int oh = pix / Wo, ow = pix % Wo;
        const float* in0 = s_in + (2 * oh) * TW + 2 * ow;   // tile row 2*oh == image row 2*oh - 1
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) acc += wk[i * 3 + j] * in0[i * TW + j];
        f32x4 y = acc * sc + sh;
        y = swish4_(y);
        *reinterpret_cast<f32x4*>(s_E + ((size_t)(oh + 1) * EW + (ow + 1)) * C + q * 4) = y;
      }
    }
    __syncthreads();
    MKWS_PH(1);
    // 2. depthwise conv in row strips: an item = SEG adjacent outputs of one row and one channel quad reads its 3 x (SEG + 2)
    //    inputs once (4.5 LDS reads per output instead of 9: the phase was LDS-bound)
    f32x4 ssum = {0.f, 0.f, 0.f, 0.f};
    {
      constexpr int SEG = 4, NSG = Wo / SEG;
      static_assert(NSG * SEG == Wo && NTHR % 8 == 0, "strips tile the output row; an item's channel quad is the thread's");
      const f32x4 sc = sc_d, sh = sh_d;
      for (int item = tid; item < Ho * NSG * 8; item += NTHR) {
        const int sp = item >> 3;
        const int oh = sp / NSG, ow0 = (sp - oh * NSG) * SEG;
        const float* e0 = s_E + ((size_t)oh * EW + ow0) * C + q * 4;     // top-left tap (halo offset cancels the -1)
        f32x4 acc[SEG];
#pragma unroll
        for (int o = 0; o < SEG; ++o) acc[o] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          f32x4 v[SEG + 2];
#pragma unroll
          for (int ci = 0; ci < SEG + 2; ++ci) v[ci] = *reinterpret_cast<const f32x4*>(e0 + ((size_t)i * EW + ci) * C);
#pragma unroll
          for (int o = 0; o < SEG; ++o)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[o] += v[o + j] * wkd[i * 3 + j];
        }
#pragma unroll
        for (int o = 0; o < SEG; ++o) {
          f32x4 y = acc[o] * sc + sh;
          y = swish4_(y);
          *reinterpret_cast<f32x4*>(s_D + (size_t)(oh * Wo + ow0 + o) * LDD + q * 4) = y;
          ssum += y;
        }
      }
    }
    // the next clip's input tile goes to LDS now (s_in was last read by the stem conv above, one barrier ago) and the clip after
    // that is requested: by the time anybody waits for these loads again, a whole clip of work has passed
    if (b + gridDim.x < (size_t)B) {
      stage();
      if (b + 2 * (size_t)gridDim.x < (size_t)B) request(b + 2 * (size_t)gridDim.x);
    }
    // channel sums: lanes of a wave that share the quad fold by shuffles, the 8 wave partials in fixed order
#pragma unroll
    for (int m = 8; m < 64; m <<= 1) {
      ssum.x += __shfl_xor(ssum.x, m); ssum.y += __shfl_xor(ssum.y, m);
      ssum.z += __shfl_xor(ssum.z, m); ssum.w += __shfl_xor(ssum.w, m);
    }
    if (lane < 8) s_red[wave * 8 + lane] = ssum;
    __syncthreads();
    MKWS_PH(2);
    // 3. SE on ONE wave without further barriers; meanwhile every wave requests its projection operands
    if (wave == 0) {
      f32x4 m4 = s_red[se_cg];
#pragma unroll
      for (int k = 1; k < NTHR / 64; ++k) m4 += s_red[k * 8 + se_cg];
      m4 = m4 * (1.0f / (Ho * Wo));
      float pr = ((m4.x * wr4[0] + m4.y * wr4[1]) + m4.z * wr4[2]) + m4.w * wr4[3];
#pragma unroll
      for (int m = 8; m < 64; m <<= 1) pr += __shfl_xor(pr, m);          // over the 8 channel groups: every lane of a unit ends with the same sum
      const float rn = (se_n < se) ? swishf_(pr + br_n) : 0.0f;
      float v = be_c;
#pragma unroll
      for (int n = 0; n < 8; ++n) v += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rn), n)) * we8[n];      // units in fixed order
      if (lane < C) s_gate[ch] = sigmoidf_(v);
    }
    constexpr int NWV = NTHR / 64;
    f32x4 x[RTW][2];
#pragma unroll
    for (int i = 0; i < RTW; ++i) {
      const int row = (wave + i * NWV) * 16 + c;
      const int rr = row < Ho * Wo ? row : Ho * Wo - 1;
#pragma unroll
      for (int j = 0; j < 2; ++j) x[i][j] = *reinterpret_cast<const f32x4*>(s_D + (size_t)rr * LDD + 16 * j + 4 * g);
    }
    __syncthreads();
    MKWS_PH(3);
    // 4. projection: Y[500, 16] = BN(D[500, 32] . (gate * Wp)[32, 16]): the gate scales the K rows of the weight fragments (8 multiplies
    //    per lane instead of 8 per row tile); a wave's row tiles and K chunks are independent accumulation chains
    {
      f32x4 wpg[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) wpg[j] = wp[j] * *reinterpret_cast<const f32x4*>(s_gate + 16 * j + 4 * g);
      float* yout = Y + b * Ho * Wo * CO;
      f32x4 acc[RTW][2];
#pragma unroll
      for (int i = 0; i < RTW; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int i = 0; i < RTW; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wpg[j][s4], x[i][j][s4], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < RTW; ++i) {
        const int row = (wave + i * NWV) * 16 + c;
        if (row < Ho * Wo) *reinterpret_cast<f32x4*>(yout + (size_t)row * CO + 4 * g) = (acc[i][0] + acc[i][1]) * scp + shp;
      }
    }
    MKWS_PH(4);
    // (no barrier here: every LDS write of the next clip sits behind one of its own barriers, and s_in was refilled two barriers ago)
  }
  MKWS_PH_STORE();
  MKWS_WG_END();
}

// ------------------------------------------------------------------------------------------------
// 1x1 conv / dense GEMM.  Y[m, n] = act((sum_k X[m,k] * gate[m/HW, k] * W[k,n]) * scale[n] + shift[n]) + R[m,n]
// Packed weights (chunk-major): Wp[((j*NTtot + nt)*4 + g)*64 + c*4 + s] = W[16j + 4g + s][16nt + c], zero
// padded -- the NT tiles a wave needs for one K chunk are contiguous, consecutive n-blocks read consecutive
// KBs (no power-of-two strides that would alias onto one L2 channel).
// Block = 4 waves; wave w owns MT row tiles (16 rows each) starting at blockIdx.x*64*MT + 16*MT*w and NT
// n-tiles starting at blockIdx.y*NT.  (MT, NT) is picked per layer so that small-M layers still put several
// waves on every SIMD (launch_gemm).
struct GemmArgs {
  const float* X; int ldx;
  const float* Wp; const float* scale; const float* shift;
  const float* gate; int HW;          // gate [B, K] (K = ldg), rows of one clip = HW
  const float* R; int ldr;
  float* Y; int ldy;
  int M, K, N, KC, NTtot, act;
  int pool4;       // 1: global average pool fused into the epilogue: the 4 rows of a clip (2x2 image) are averaged, Y is [M/4, N]
  int splitk;      // > 1: blockIdx.z owns a slice of the K chunks and writes raw sums to part[z][M][ldp]
  float* part; int ldp;
  const int* poison;   // optional device word: nonzero = an earlier kernel of this forward failed (mbconv_pair_kernel's exchange): store NaN
#ifdef MKWS_FRONT_TIMING
  unsigned long long* dbg_clk;   // timing build: [workgroup][2] = shader-clock cycles, 100 MHz ticks of wave 0
#endif
};

template <int MT, int NT, bool GATE>
__global__ __launch_bounds__(256) void pw_gemm_kernel(GemmArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  // XCD-aware tile order.  Workgroups are dealt round-robin over the 8 XCDs in linear-id order (x fastest), so with the plain
  // (x = row block, y = tile group) grid XCD k would own row blocks k, k+8, ... for EVERY tile group and each of the 8 L2s
  // would pull the whole weight matrix (dense_1: 125 MB fetched for 34 MB of operands).  Instead XCD k owns one rectangle
  // of the 2 x 4 split of the (row block, tile group) plane: half of X and a quarter of W per L2.
  int bx = blockIdx.x, by = blockIdx.y;
#ifndef MKWS_GEMM_PLAIN_ORDER                      // dev aid: -DMKWS_GEMM_PLAIN_ORDER builds the A/B library without the remap
  if ((gridDim.x & 1) == 0 && (gridDim.y & 3) == 0) {
    const int lin = blockIdx.x + gridDim.x * blockIdx.y, xcd = lin & 7, idx = lin >> 3;
    const int rx = gridDim.x >> 1, ry = gridDim.y >> 2;
    bx = (xcd & 1) * rx + idx % rx;
    by = (xcd >> 1) * ry + idx / rx;
  }
#endif
  const int m0 = bx * (64 * MT) + wave * (16 * MT);
  const int nt0 = by * NT;
  if (m0 >= a.M) return;
#ifdef MKWS_FRONT_TIMING
  const unsigned long long dbg_c0 = clock64(), dbg_w0 = wall_clock64();
#endif

  // Operand pointers are CLAMPED instead of predicated (rows past M re-read row M-1, tiles past NTtot
  // re-read the last tile; their results are never stored), so the K loop has no per-load branches.
  // Only the K tail (K % 16 == 8: lane groups 2,3 of the last chunk) needs a zero, done by a select.
  // Addressing: buffer descriptors of the three operands (uniform), a 32-bit byte offset per lane, and the K-chunk offset in an
  // SGPR (buffer_load_dwordx4 v, voffset, rsrc, soffset offen): the steady state issues NO VALU instruction per load.  With
  // per-lane 64-bit pointers every load cost a v_lshl_add_u64 / v_mad_u64_u32, and VALU work takes MFMA issue time
  // (tools/microbench/mfma_valu_overlap.hip).
  const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.X), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.Wp), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rG = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(GATE ? a.gate : a.X), 0, 0x7fffffff, 0x00020000);
  unsigned xoff[MT], goff[MT];
  bool rowok[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + mt * 16 + c;
    rowok[mt] = m < a.M;
    const int mm = rowok[mt] ? m : (a.M - 1);
    xoff[mt] = (unsigned)(((size_t)mm * a.ldx + 4 * g) * sizeof(float));
    goff[mt] = GATE ? (unsigned)(((size_t)(mm / a.HW) * a.K + 4 * g) * sizeof(float)) : 0u;
  }
  const unsigned woff = (unsigned)((g * 64 + c * 4) * sizeof(float));
  unsigned wtile[NT];                              // uniform: byte offset of this block's n-tiles inside a K chunk
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int t = (nt0 + nt < a.NTtot) ? nt0 + nt : a.NTtot - 1;
    wtile[nt] = (unsigned)t * 1024u;
  }
  const unsigned wchunk = (unsigned)a.NTtot * 1024u;   // bytes per K chunk of the packed weights
  // K range of this block (split-K over blockIdx.z)
  int jbeg = 0, jend = a.KC;
  if (a.splitk > 1) {
    const int per = (a.KC + a.splitk - 1) / a.splitk;
    jbeg = blockIdx.z * per;
    jend = (jbeg + per < a.KC) ? jbeg + per : a.KC;
  }
  // K tail (K % 16 == 8, only the unfused expand convs with Cin = 24 / 40): the last chunk's lane groups
  // 2,3 have no X columns.  It is peeled off the pipelined loop so the steady state stays branch-free.
  const bool ktail = (a.K & 15) != 0;          // uniform
  const int jpipe_end = (ktail && jend == a.KC) ? jend - 1 : jend;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // D-deep register ring over the K chunks.  Shape matters for hipcc's s_waitcnt placement: with
  // conditional reloads inside the loop it falls back to vmcnt(0) at the loop head (measured: the ring
  // degenerated to depth 1).  So: unconditional prologue, a steady-state loop in which every slot does
  // exactly "MFMAs, then reload" (the compiler then emits counted vmcnt(N) and D-1 chunks stay in flight),
  // and a drain.
  constexpr int D = (MT * NT >= 10) ? 3 : 4;   // deeper rings measured slower (6: +2 %, 8: +3 % on the dense layers, profiles/r02_notes.md)
  constexpr int XW = GATE ? 2 * MT : MT;        // the SE gate rides the ring as raw fragments next to X: multiplying it in at
  f32x4 xq[D][XW], wq[D][NT];                   // load time would touch the fresh registers and force an immediate wait
  auto load = [&](int j, f32x4 (&xv)[XW], f32x4 (&wv)[NT]) {
    const unsigned kx = 64u * (unsigned)j;         // 16 floats of K per chunk
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      xv[mt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rX, xoff[mt], kx, 0));
      if (GATE) xv[MT + mt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rG, goff[mt], kx, 0));
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wv[nt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rW, woff, wtile[nt] + wchunk * (unsigned)j, 0));
  };
  auto compute = [&](const f32x4 (&xv)[XW], const f32x4 (&wv)[NT]) {
    f32x4 x[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) x[mt] = GATE ? xv[mt] * xv[MT + (GATE ? mt : 0)] : xv[mt];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[nt][s], x[mt][s], acc[mt][nt], 0, 0, 0);
  };
  const int n = jpipe_end - jbeg;
  if (n >= D) {
#pragma unroll
    for (int d = 0; d < D; ++d) load(jbeg + d, xq[d], wq[d]);
    int j = jbeg;
    for (; j + 2 * D <= jpipe_end; j += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        compute(xq[d], wq[d]);
        load(j + D + d, xq[d], wq[d]);
        // without this hipcc sinks all D reloads to the end of the loop body: every iteration then starts by
        // waiting a full memory latency for slot 0 (the ring keeps nothing in flight across iterations)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // here D <= jpipe_end - j < 2D: one more group with partial reloads, then the drain
#pragma unroll
    for (int d = 0; d < D; ++d) {
      compute(xq[d], wq[d]);
      if (j + D + d < jpipe_end) load(j + D + d, xq[d], wq[d]);
      __builtin_amdgcn_sched_barrier(0);
    }
    j += D;
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (j + d < jpipe_end) compute(xq[d], wq[d]);
  } else {
    for (int j = jbeg; j < jpipe_end; ++j) {
      load(j, xq[0], wq[0]);
      compute(xq[0], wq[0]);
    }
  }
  if (jpipe_end != jend) {        // peeled K-tail chunk
    load(jend - 1, xq[0], wq[0]);
    if (g >= 2) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xq[0][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    compute(xq[0], wq[0]);
  }
  if (a.splitk > 1) {     // raw partial sums; epilogue happens in splitk_reduce_kernel
    float* P = a.part + (size_t)blockIdx.z * a.M * a.ldp;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = (nt0 + nt) * 16 + 4 * g;
      if (n >= a.N) continue;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        if (rowok[mt]) *reinterpret_cast<f32x4*>(P + (size_t)(m0 + mt * 16 + c) * a.ldp + n) = acc[mt][nt];
    }
    return;
  }
#ifdef MKWS_FRONT_TIMING
  if (a.dbg_clk && threadIdx.x == 0) { a.dbg_clk[2 * (blockIdx.x + gridDim.x * blockIdx.y)] = clock64() - dbg_c0; a.dbg_clk[2 * (blockIdx.x + gridDim.x * blockIdx.y) + 1] = wall_clock64() - dbg_w0; }
#endif
  // epilogue: lane (g, c) holds rows m = m0 + mt*16 + c, channels n = 16*(nt0+nt) + 4g .. +3
  const bool poisoned = a.poison != nullptr && *a.poison != 0;       // uniform (scalar load)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = (nt0 + nt) * 16 + 4 * g;
    if (n >= a.N) continue;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scale + n);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(a.shift + n);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      if (!rowok[mt]) continue;
      const size_t m = (size_t)(m0 + mt * 16 + c);
      f32x4 y = acc[mt][nt] * sc + sh;
      if (a.act != ACT_NONE) {
        y = apply_act4(y, a.act);
      }
      if (a.R) y += *reinterpret_cast<const f32x4*>(a.R + m * a.ldr + n);
      if (poisoned) y = (f32x4){__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
      if (a.pool4) {
        // rows 4i..4i+3 of the tile sit in lanes c = 4i..4i+3 of the same lane group: two xor-shuffles fold them
        // (M is a multiple of 4, so a clip's rows are valid together; shuffles run on all lanes of the wave)
        y.x += __shfl_xor(y.x, 1); y.y += __shfl_xor(y.y, 1); y.z += __shfl_xor(y.z, 1); y.w += __shfl_xor(y.w, 1);
        y.x += __shfl_xor(y.x, 2); y.y += __shfl_xor(y.y, 2); y.z += __shfl_xor(y.z, 2); y.w += __shfl_xor(y.w, 2);
        if ((c & 3) == 0) *reinterpret_cast<f32x4*>(a.Y + (m >> 2) * a.ldy + n) = y * 0.25f;
      } else {
        *reinterpret_cast<f32x4*>(a.Y + m * a.ldy + n) = y;
      }
    }
  }
}

// split-K epilogue: Y = act(sum_z part[z] * scale + shift) + R, one float4 per thread
// ------------------------------------------------------------------------------------------------
// Matrix-vector form of the dense tail for live-serving handles (at most 4 rows: dense / dense_1 / dense_2 of a one-clip handle, and its top
// conv over the clip's 2x2 pixels with the average pool).  With one row the MFMA tile is 1/16 full and the work is the weight stream:
// pw_gemm_kernel + its split-K fold took 4 x 5.7 + 3 x 4.5 us of a 354 us window (profiles/r06_latency_stats.txt).  Here ONE workgroup of 16
// waves owns one 16-column tile and splits K sixteen ways: every wave requests ALL its weight fragments (at most NJ, 1 KB each, the packed
// layout the GEMMs read) and row fragments before the first multiply -- one memory round trip per layer -- and the sixteen partial columns
// meet in LDS, folded in (wave, lane group) order by the lanes that own the outputs: no second launch, fixed order.
// Epilogue as pw_gemm_kernel / splitk_reduce_kernel: acc * scale + shift, activation, (pool: ((r0 + r1) + (r2 + r3)) * 0.25), poison.
template <int ROWS, int NJ>
__global__ __launch_bounds__(1024) void gemv_kernel(GemmArgs a) {
  __shared__ float s_part[16][ROWS][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int t = blockIdx.x;
  const float* wl = a.Wp + ((size_t)t * 64 + lane) * 4;          // + j * NTtot * 256
  f32x4 w[NJ], x[ROWS][NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    const int j = wave + 16 * i, jc = j < a.KC ? j : a.KC - 1;    // past the end: a harmless reload, masked below
    w[i] = *reinterpret_cast<const f32x4*>(wl + (size_t)jc * a.NTtot * 256);
    const int k = (16 * jc + 4 * g < a.K - 4) ? 16 * jc + 4 * g : a.K - 4;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) x[r][i] = *reinterpret_cast<const f32x4*>(a.X + (size_t)(r < a.M ? r : 0) * a.ldx + k);
  }
  float acc[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) acc[r] = 0.0f;
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    const bool live = wave + 16 * i < a.KC && 16 * (wave + 16 * i) + 4 * g < a.K;      // (rows of W past K are zero in the packed layout; the row fragment was clamped)
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) acc[r] += live ? w[i][s4] * x[r][i][s4] : 0.0f;
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) s_part[wave][r][lane] = acc[r];
  __syncthreads();
  if (threadIdx.x < 16) {
    const int n = 16 * t + c;
    if (n < a.N) {
      const float sc = a.scale[n], sh = a.shift[n];
      const bool poisoned = a.poison != nullptr && *a.poison != 0;
      float y[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        float v = 0.0f;
#pragma unroll
        for (int wv = 0; wv < 16; ++wv)
#pragma unroll
          for (int gg = 0; gg < 4; ++gg) v += s_part[wv][r][16 * gg + c];
        y[r] = apply_act(v * sc + sh, a.act);
        if (poisoned) y[r] = __builtin_nanf("");
      }
      if (a.pool4) {
        if (ROWS == 4) a.Y[n] = ((y[0] + y[ROWS > 1 ? 1 : 0]) + (y[ROWS > 2 ? 2 : 0] + y[ROWS > 3 ? 3 : 0])) * 0.25f;
      } else {
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
          if (r < a.M) a.Y[(size_t)r * a.ldy + n] = y[r];
      }
    }
  }
}

__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int splitk, int M, int N, int ldp,
                                                            const float* __restrict__ scale, const float* __restrict__ shift, int act,
                                                            const float* __restrict__ R, int ldr, float* __restrict__ Y, int ldy,
                                                            const int* __restrict__ poison) {
  const int nq = N / 4;
  const bool poisoned = poison != nullptr && *poison != 0;
  const long total = (long)M * nq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / nq;
    const int n = (int)(i % nq) * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(part + (size_t)m * ldp + n);
    for (int z = 1; z < splitk; ++z) v += *reinterpret_cast<const f32x4*>(part + ((size_t)z * M + m) * ldp + n);
    f32x4 y = v * *reinterpret_cast<const f32x4*>(scale + n) + *reinterpret_cast<const f32x4*>(shift + n);
    if (act != ACT_NONE) y = apply_act4(y, act);
    if (R) y += *reinterpret_cast<const f32x4*>(R + (size_t)m * ldr + n);
    if (poisoned) y = (f32x4){__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
    *reinterpret_cast<f32x4*>(Y + (size_t)m * ldy + n) = y;
  }
}

// ------------------------------------------------------------------------------------------------
// depthwise conv: X [B,H,W,C] -> Y [B,Ho,Wo,C], + BN + swish, and per-(b,c) sums of Y for SE squeeze.
// block = one clip x CQB channel quads; thread = (pixel lane tp, quad tq), tq fastest (coalesced).
template <int KS, int S>
__global__ __launch_bounds__(256) void dw_kernel(const float* __restrict__ X, const float* __restrict__ Wd /*[KS*KS][C]*/,
                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                 float* __restrict__ Y, float* __restrict__ sums /*[B,C]*/,
                                                 int H, int W, int C, int Ho, int Wo, int pt, int pl, int CQB, int P) {
  __shared__ f32x4 s_red[256];
  const int b = blockIdx.x;
  const int tq = threadIdx.x % CQB, tp = threadIdx.x / CQB;
  const int cq = blockIdx.y * CQB + tq;
  const bool active = tp < P && cq * 4 < C;
  f32x4 ssum = {0.f, 0.f, 0.f, 0.f};
  if (active) {
    const int c0 = cq * 4;
    f32x4 wk[KS * KS];
#pragma unroll
    for (int t = 0; t < KS * KS; ++t) wk[t] = *reinterpret_cast<const f32x4*>(Wd + (size_t)t * C + c0);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c0);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + c0);
    const float* xin = X + (size_t)b * H * W * C + c0;
    float* yout = Y + (size_t)b * Ho * Wo * C + c0;
    int oh = tp / Wo, ow = tp % Wo;
    const int dh = P / Wo, dwo = P % Wo;
    for (int p = tp; p < Ho * Wo; p += P) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < KS; ++i) {
        const int ih = oh * S - pt + i;
        if (ih < 0 || ih >= H) continue;
#pragma unroll
        for (int j = 0; j < KS; ++j) {
          const int iw = ow * S - pl + j;
          if (iw < 0 || iw >= W) continue;
          acc += *reinterpret_cast<const f32x4*>(xin + ((size_t)ih * W + iw) * C) * wk[i * KS + j];
        }
      }
      f32x4 y = acc * sc + sh;
      y = swish4_(y);
      *reinterpret_cast<f32x4*>(yout + (size_t)p * C) = y;
      ssum += y;
      oh += dh; ow += dwo;
      if (ow >= Wo) { ow -= Wo; ++oh; }
    }
  }
  s_red[threadIdx.x] = ssum;
  __syncthreads();
  if (tp == 0 && cq * 4 < C && threadIdx.x < CQB) {
    f32x4 t = s_red[tq];
    for (int k = 1; k < P; ++k) t += s_red[k * CQB + tq];
    *reinterpret_cast<f32x4*>(sums + (size_t)b * C + cq * 4) = t;
  }
}

// ------------------------------------------------------------------------------------------------
// Fused MBConv front half: 1x1 expand conv (+BN+swish) -> LDS -> depthwise kxk (+BN+swish) -> Y, + SE sums.
// The expanded activation (6x the block input, the largest tensor of every block) never leaves the CU.
//   block = G consecutive clips x CC expanded channels.
//   phase 1: E[G*H*W, CC] = swish(BN(X[G*H*W, Cin] . We[:, chunk])) on the fp32 MFMA (same transposed
//            operand scheme and packed weights as pw_gemm_kernel), written to LDS as float4 rows.
//   phase 2: depthwise from LDS.  PIXEL_LANES (big images): thread = (pixel lane, channel quad), one clip at
//            a time, SE sums reduced through LDS;  otherwise (tiny images): thread = (clip, channel quad)
//            walks all output pixels itself and owns its SE sums.
struct FrontArgs {
  const float* X; int Cin;
  const float* WpE; const float* scE; const float* shE; int KC; int NTtotE;
  const float* Wd; const float* scD; const float* shD;
  float* Y; float* sums;
  int B, H, W, Ho, Wo, pt, pl, Cexp, G;
  int ncb;                         // big-image mode: channel blocks a workgroup walks (grid.y = blocks / ncb)
#ifdef MKWS_FRONT_TIMING
  unsigned long long* dbg_t;
#endif
};

// Row-strip depthwise item of the big-image blocks (front kernel phase 2, whole-block kernel P2): SEG adjacent outputs of one output row
// for one channel pair / quad (VT), from E in LDS ([pixel][LDE]) and the taps in LDS ([KS*KS][CC]).  A strip reads each of its
// KS x NC inputs once.  Where a read lands is decided once, not per read:
//   columns  the image size is a template constant, so column ci of the strip is inside the image for every row segment, for none, or
//            (first / last column of a two-segment row only) for some.  The first kind is read at one base register + an immediate
//            offset, the second at the zero row, and only the third takes a select;
//   rows     a tap row outside the image is skipped as a whole (one EXEC predicate around its reads and multiply-adds; it used to add
//            0 * w to every sum, which changes no value), and a tap row that is inside for every output row takes no test at all.
// The multiply-adds run in the order (tap row, output, tap column), as they always did.  ROW_UNROLL: tap rows per loop trip (KS: unrolled).
template <int KS, int S, int HT, int WT, int SEG>
struct StripGeom {
  static constexpr int HoT = (S == 1) ? HT : (HT + 1) / 2, WoT = (S == 1) ? WT : (WT + 1) / 2;
  static constexpr int PT = (S == 1) ? KS / 2 : KS / 2 - (1 - HT % 2), PLF = (S == 1) ? KS / 2 : KS / 2 - (1 - WT % 2);
  static constexpr int NSEG = WoT / SEG;
  static constexpr int NC = (SEG - 1) * S + KS;
  static_assert(NSEG * SEG == WoT, "segments tile the output row");
  __host__ __device__ static constexpr int col_class(int ci) {      // segments whose column ci is inside the image: 1 = all, 0 = none, 2 = some
    int in = 0;
    for (int sg = 0; sg < NSEG; ++sg) in += ((unsigned)(sg * SEG * S - PLF + ci) < (unsigned)WT) ? 1 : 0;
    return in == NSEG ? 1 : (in == 0 ? 0 : 2);
  }
  __host__ __device__ static constexpr bool row_always(int i) {     // tap row i is inside the image for every output row
    return i - PT >= 0 && (HoT - 1) * S - PT + i < HT;
  }
};

template <typename VT, int KS, int S, int HT, int WT, int SEG, int LDE, int CC, int ROW_UNROLL>
__device__ __forceinline__ void dw_strip_(const float* p,         // E at the strip's first input (ih0, iw0), outside the image for a border item (never read there), at the item's channels
                                          const float* zcol,      // the zero row, at the item's channels
                                          const float* wd,        // the taps, at the item's channels
                                          int ih0, int iw0, VT (&acc)[SEG]) {
  using SG = StripGeom<KS, S, HT, WT, SEG>;
  constexpr int NC = SG::NC;
  auto load = [&](int i, VT (&v)[NC]) {
#pragma unroll
    for (int ci = 0; ci < NC; ++ci) {
      const int cls = SG::col_class(ci);
      const float* q = p + (i * WT + ci) * LDE;
      if (cls == 0) q = zcol;
      else if (cls == 2) q = ((unsigned)(iw0 + ci) < (unsigned)WT) ? q : zcol;
      v[ci] = *reinterpret_cast<const VT*>(q);
    }
  };
  auto mac = [&](int i, const VT (&v)[NC]) {
    VT w[KS];
#pragma unroll
    for (int jx = 0; jx < KS; ++jx) w[jx] = *reinterpret_cast<const VT*>(wd + (i * KS + jx) * CC);
#pragma unroll
    for (int o = 0; o < SEG; ++o)
#pragma unroll
      for (int jx = 0; jx < KS; ++jx) acc[o] += v[o * S + jx] * w[jx];
  };
  if constexpr (ROW_UNROLL == KS) {
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      if (SG::row_always(i) || (unsigned)(ih0 + i) < (unsigned)HT) {
        VT v[NC];
        load(i, v);
        mac(i, v);
      }
    }
  } else {
#pragma unroll ROW_UNROLL
    for (int i = 0; i < KS; ++i) {
      if ((unsigned)(ih0 + i) < (unsigned)HT) {
        VT v[NC];
        load(i, v);
        mac(i, v);
      }
    }
  }
}

// The form every strip had before dw_strip_: all tap rows run, and every read chooses between its input row and the zero row (index
// zrow of E).  Kept for the instantiation that measured no faster with dw_strip_ (block 4a, profiles/strip_addressing.txt).
template <typename VT, int KS, int S, int HT, int WT, int SEG, int LDE, int CC, int ROW_UNROLL>
__device__ __forceinline__ void dw_strip_per_read_(const float* E0,    // E at the item's channels
                                                   int row0,           // the item's clip: its first row of E
                                                   int zrow, const float* wd, int ih0, int iw0, VT (&acc)[SEG]) {
  constexpr int NC = (SEG - 1) * S + KS;
  int coff[NC];
#pragma unroll
  for (int ci = 0; ci < NC; ++ci) coff[ci] = ((unsigned)(iw0 + ci) < (unsigned)WT) ? iw0 + ci : -1;
#pragma unroll ROW_UNROLL
  for (int i = 0; i < KS; ++i) {
    const int ih = ih0 + i;
    const bool rok = (unsigned)ih < (unsigned)HT;
    const int rbase = row0 + ih * WT;
    VT v[NC], w[KS];
#pragma unroll
    for (int ci = 0; ci < NC; ++ci) {
      const int row = (rok && coff[ci] >= 0) ? rbase + coff[ci] : zrow;
      v[ci] = *reinterpret_cast<const VT*>(E0 + (size_t)row * LDE);
    }
#pragma unroll
    for (int jx = 0; jx < KS; ++jx) w[jx] = *reinterpret_cast<const VT*>(wd + (i * KS + jx) * CC);
#pragma unroll
    for (int o = 0; o < SEG; ++o)
#pragma unroll
      for (int jx = 0; jx < KS; ++jx) acc[o] += v[o * S + jx] * w[jx];
  }
}

// Template: KS/S depthwise kernel & stride; CC channels per block; KCT > 0: big-image mode with exactly KCT
// K chunks (weights in registers); KCT == 0: tiny-image mode with compile-time image size HT x WT.
template <int KS, int S, int CC, int KCT, int HT, int WT>
__global__ __launch_bounds__(KCT > 0 ? 256 : 512) void mbconv_front_kernel(FrontArgs a) {
  constexpr bool PIXEL_LANES = KCT > 0;
  constexpr int NTHREADS = PIXEL_LANES ? 256 : 512;
  extern __shared__ __attribute__((aligned(16))) float s_front[];
  constexpr int LDE = CC + 4;
  constexpr int NT = CC / 16;
  constexpr int Q = CC / 4;
  const int HW = a.H * a.W;
  float* s_E = s_front;                        // [G*HW][LDE]
  f32x4* s_red = reinterpret_cast<f32x4*>(s_front + ((size_t)a.G * HW + 1) * LDE);   // [256], after the zero row
  float* s_sumc = reinterpret_cast<float*>(s_red + 256);                              // [G][CC] channel sums (SE squeeze)
  float* s_wd = s_sumc + (size_t)a.G * CC;                                           // [KS*KS][CC] depthwise taps (big-image mode)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform by construction: keeps wave-dependent offsets / branches on the scalar unit
  const int g = lane >> 4, c = lane & 15;
  const int b0 = blockIdx.x * a.G;
  const int gvalid = (a.B - b0 < a.G) ? (a.B - b0) : a.G;
  const int rows = gvalid * HW;
  MKWS_WG_BEGIN();
  if (tid < LDE / 4) *reinterpret_cast<f32x4*>(s_front + (size_t)a.G * HW * LDE + 4 * tid) = (f32x4){0.f, 0.f, 0.f, 0.f};
#ifdef MKWS_FRONT_TIMING
  unsigned long long* dbgp = a.dbg_t + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4;
  if (tid == 0) dbgp[0] = wall_clock64();
#endif
  // Channel blocks this workgroup walks one after the other (a.ncb; 1 = one block per blockIdx.y, the shape until round 5).  Block 2a's three
  // 32-channel blocks used to be three workgroups per clip, each pulling the clip's 32 KB input from HBM (94 MB fetched per launch for 33 MB
  // of input, profiles/pmc_traffic.json); walked by ONE workgroup the second and third pass find it in L2.
  const int ncb = PIXEL_LANES ? a.ncb : 1;
  for (int cb = 0; cb < ncb; ++cb) {
    const int ch0 = (blockIdx.y * ncb + cb) * CC;   // first expanded channel of this pass
    // nt_valid: n-tiles of this block that exist (the last chunk of a layer may be partial)
    const int nt_valid = ((a.Cexp - ch0) / 16 < NT) ? (a.Cexp - ch0) / 16 : NT;
    // depthwise BN constants of this thread's channel quad (item % Q == tid % Q for every item of the thread):
    // requested now, used after the barrier
    f32x4 scd_pre = {0.f, 0.f, 0.f, 0.f}, shd_pre = {0.f, 0.f, 0.f, 0.f};
    if constexpr (PIXEL_LANES) {
      const int tq0 = tid % Q;
      const int cq0 = (tq0 < nt_valid * 4) ? ch0 + 4 * tq0 : ch0;
      scd_pre = *reinterpret_cast<const f32x4*>(a.scD + cq0);
      shd_pre = *reinterpret_cast<const f32x4*>(a.shD + cq0);
    }
    if constexpr (PIXEL_LANES) {                 // depthwise taps of this channel chunk -> LDS (consumed after phase 1)
      for (int i = tid; i < KS * KS * Q; i += NTHREADS) {
        const int t = i / Q, q4 = (i - t * Q) * 4;
        const int cq = (q4 < nt_valid * 16) ? ch0 + q4 : ch0;
        *reinterpret_cast<f32x4*>(s_wd + t * CC + q4) = *reinterpret_cast<const f32x4*>(a.Wd + (size_t)t * a.Cexp + cq);
      }
    }
    // ---- phase 1: expand into LDS ----
    // Operand fragments go global -> registers through the vector L1 (64 B/clk/CU), which is what bounds
    // small MFMA tiles; so weights are fetched as rarely as possible:
    //   PIXEL_LANES (few K chunks, many row tiles): all weight fragments of the block live in registers;
    //   tiny images (many K chunks, CC = 128): each weight fragment feeds MT = 2 row tiles.
    {
      const float* Xb = a.X + (size_t)b0 * HW * a.Cin;
      const float* wbase = a.WpE + ((size_t)(ch0 / 16) * 4 + g) * 64 + c * 4;     // + (j*NTtotE + nt)*256
      const size_t wchunk = (size_t)a.NTtotE * 256;
      const int ntiles = (rows + 15) / 16;
      if constexpr (PIXEL_LANES) {
        // All loads of the tile loop are unconditional (clamped row / k offsets; padded k positions meet zero
        // weights), the BN constants sit in registers, and the X ring is prologue / steady state / tail, so
        // hipcc emits counted vmcnt waits instead of draining the ring at every tile.
        constexpr int MAXKC = KCT;             // exact K chunk count of the layer (Cin = 16, 24, 40 -> 1, 2, 3)
        f32x4 wreg[MAXKC][NT], scr[NT], shr[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int ntc = nt < nt_valid ? nt : nt_valid - 1;
          scr[nt] = *reinterpret_cast<const f32x4*>(a.scE + ch0 + ntc * 16 + 4 * g);
          shr[nt] = *reinterpret_cast<const f32x4*>(a.shE + ch0 + ntc * 16 + 4 * g);
#pragma unroll
          for (int j = 0; j < MAXKC; ++j) wreg[j][nt] = *reinterpret_cast<const f32x4*>(wbase + (size_t)j * wchunk + ntc * 256);
        }
        int koff[MAXKC];
#pragma unroll
        for (int j = 0; j < MAXKC; ++j) koff[j] = (16 * j + 4 * g < a.Cin - 4) ? 16 * j + 4 * g : a.Cin - 4;
        constexpr int NW = NTHREADS / 64;
        const int nmy = (ntiles - wave + NW - 1) / NW;          // row tiles of this wave: wave, wave + NW, ...
        constexpr int D = 4;
        f32x4 xq[D][MAXKC];
        auto loadx = [&](int i, f32x4 (&xv)[MAXKC]) {
          int row = (wave + NW * i) * 16 + c;
          row = row < rows ? row : rows - 1;
          const float* xp = Xb + (size_t)row * a.Cin;
#pragma unroll
          for (int j = 0; j < MAXKC; ++j) xv[j] = *reinterpret_cast<const f32x4*>(xp + koff[j]);
        };
        auto tile = [&](int i, const f32x4 (&xv)[MAXKC]) {
          f32x4 acc[NT];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < MAXKC; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
              for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[j][nt][s], xv[j][s], acc[nt], 0, 0, 0);
          const int row = (wave + NW * i) * 16 + c;
          if (row < rows) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              if (nt < nt_valid) {
                f32x4 y = acc[nt] * scr[nt] + shr[nt];
                y = swish4_(y);
                *reinterpret_cast<f32x4*>(s_E + (size_t)row * LDE + nt * 16 + 4 * g) = y;
              }
            }
          }
        };
#pragma unroll
        for (int d = 0; d < D; ++d) loadx(d, xq[d]);
        int i = 0;
        for (; i + D <= nmy; i += D) {
#pragma unroll
          for (int d = 0; d < D; ++d) {
            tile(i + d, xq[d]);
            loadx(i + d + D, xq[d]);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
#pragma unroll
        for (int d = 0; d < D; ++d)
          if (i + d < nmy) tile(i + d, xq[d]);
      } else {
        // 8 waves = 4 row-pair lanes x 2 column halves: wave tile = 2 row tiles x NT/2 column tiles, so one
        // K chunk costs 2 X + NT/2 weight fragments for 2*(NT/2)*4 MFMAs.  Same load discipline as above.
        constexpr int NTW = (NT >= 2) ? NT / 2 : 1;
        const int nhalf = wave >> 2, plane = wave & 3;
        const int npairs = (ntiles + 1) / 2;
        f32x4 scr[NTW], shr[NTW];
        const float* wpq[NTW];
#pragma unroll
        for (int q = 0; q < NTW; ++q) {
          const int nt = nhalf * NTW + q;
          const int ntc = nt < nt_valid ? nt : nt_valid - 1;
          scr[q] = *reinterpret_cast<const f32x4*>(a.scE + ch0 + ntc * 16 + 4 * g);
          shr[q] = *reinterpret_cast<const f32x4*>(a.shE + ch0 + ntc * 16 + 4 * g);
          wpq[q] = wbase + (size_t)ntc * 256;
        }
        for (int pr = plane; pr < npairs; pr += 4) {
          const int row0 = pr * 32 + c, row1 = row0 + 16;
          const float* xp0 = Xb + (size_t)(row0 < rows ? row0 : rows - 1) * a.Cin;
          const float* xp1 = Xb + (size_t)(row1 < rows ? row1 : rows - 1) * a.Cin;
          f32x4 acc0[NTW], acc1[NTW];
#pragma unroll
          for (int q = 0; q < NTW; ++q) { acc0[q] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc1[q] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
          constexpr int D = 3;
          f32x4 x0[D], x1[D], wq[D][NTW];
          auto load = [&](int j, f32x4& v0, f32x4& v1, f32x4 (&wv)[NTW]) {
            j = j < a.KC ? j : a.KC - 1;                      // past the end: harmless reload, never consumed
            const int ko = (16 * j + 4 * g < a.Cin - 4) ? 16 * j + 4 * g : a.Cin - 4;
            v0 = *reinterpret_cast<const f32x4*>(xp0 + ko);
            v1 = *reinterpret_cast<const f32x4*>(xp1 + ko);
#pragma unroll
            for (int q = 0; q < NTW; ++q) wv[q] = *reinterpret_cast<const f32x4*>(wpq[q] + (size_t)j * wchunk);
          };
          auto compute = [&](const f32x4& v0, const f32x4& v1, const f32x4 (&wv)[NTW]) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
              for (int q = 0; q < NTW; ++q) {
                acc0[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[q][s], v0[s], acc0[q], 0, 0, 0);
                acc1[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[q][s], v1[s], acc1[q], 0, 0, 0);
              }
          };
#pragma unroll
          for (int d = 0; d < D; ++d) load(d, x0[d], x1[d], wq[d]);
          int j = 0;
          for (; j + D <= a.KC; j += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
              compute(x0[d], x1[d], wq[d]);
              load(j + d + D, x0[d], x1[d], wq[d]);
              __builtin_amdgcn_sched_barrier(0);     // keep the reload right behind its slot's MFMAs
            }
          }
#pragma unroll
          for (int d = 0; d < D; ++d)
            if (j + d < a.KC) compute(x0[d], x1[d], wq[d]);
#pragma unroll
          for (int q = 0; q < NTW; ++q) {
            const int nt = nhalf * NTW + q;
            if (nt < nt_valid) {
              if (row0 < rows) {
                f32x4 y = acc0[q] * scr[q] + shr[q];
                y = swish4_(y);
                *reinterpret_cast<f32x4*>(s_E + (size_t)row0 * LDE + nt * 16 + 4 * g) = y;
              }
              if (row1 < rows) {
                f32x4 y = acc1[q] * scr[q] + shr[q];
                y = swish4_(y);
                *reinterpret_cast<f32x4*>(s_E + (size_t)row1 * LDE + nt * 16 + 4 * g) = y;
              }
            }
          }
        }
      }
    }
#ifdef MKWS_FRONT_TIMING
    if (tid == 0) dbgp[1] = wall_clock64();
#endif
    __syncthreads();
#ifdef MKWS_FRONT_TIMING
    if (tid == 0) dbgp[2] = wall_clock64();
#endif
    // ---- phase 2: depthwise from LDS ----
    if constexpr (PIXEL_LANES) {
      // Row strips: item = (clip, output row, column segment, channel quad) computes SEG adjacent outputs of one
      // row (dw_strip_: each of its KS x ((SEG-1)*S + KS) inputs is read once instead of KS*KS times per output,
      // at an immediate offset from one base register), and the taps come from LDS.
      constexpr int HoT = (S == 1) ? HT : (HT + 1) / 2, WoT = (S == 1) ? WT : (WT + 1) / 2;
      constexpr int SEG = (WoT % 5 == 0) ? 5 : WoT;
      constexpr int NSEG = WoT / SEG;
      const int zrow = a.G * HW;
      const int nitems = gvalid * HoT * NSEG * Q;
      for (int item = tid; item < nitems; item += NTHREADS) {
        const int tq = item % Q;
        int r = item / Q;
        const int sg = r % NSEG; r /= NSEG;
        const int oh = r % HoT, gi = r / HoT;
        f32x4 ssum = {0.f, 0.f, 0.f, 0.f};
        if (tq < nt_valid * 4) {
          const int cq = ch0 + 4 * tq;
          f32x4 acc[SEG];
#pragma unroll
          for (int o = 0; o < SEG; ++o) acc[o] = (f32x4){0.f, 0.f, 0.f, 0.f};
          using SG = StripGeom<KS, S, HT, WT, SEG>;
          const int ih0 = oh * S - SG::PT, iw0 = sg * SEG * S - SG::PLF;
          dw_strip_<f32x4, KS, S, HT, WT, SEG, LDE, CC, KS>(s_E + (gi * HW + ih0 * WT + iw0) * LDE + 4 * tq, s_E + zrow * LDE + 4 * tq, s_wd + 4 * tq, ih0, iw0, acc);
          const f32x4 sc = scd_pre, sh = shd_pre;
          float* yout = a.Y + ((size_t)(b0 + gi) * (HoT * WoT) + oh * WoT + sg * SEG) * a.Cexp + cq;
#pragma unroll
          for (int o = 0; o < SEG; ++o) {
            f32x4 y = acc[o] * sc + sh;
            y = swish4_(y);
            *reinterpret_cast<f32x4*>(yout + (size_t)o * a.Cexp) = y;
            ssum += y;
          }
        }
        s_red[item] = ssum;
      }
      __syncthreads();
      // channel sums per clip: the strips' partial sums are added in fixed (row, segment) order
      if (tid < gvalid * Q) {
        const int gi = tid / Q, tq = tid - gi * Q;
        if (tq < nt_valid * 4) {
          f32x4 t = {0.f, 0.f, 0.f, 0.f};
          for (int k = 0; k < HoT * NSEG; ++k) t += s_red[(gi * HoT * NSEG + k) * Q + tq];
          *reinterpret_cast<f32x4*>(a.sums + (size_t)(b0 + gi) * a.Cexp + ch0 + 4 * tq) = t;
          *reinterpret_cast<f32x4*>(s_sumc + (size_t)gi * CC + 4 * tq) = t;
        }
      }
    } else {
      // image size is a template constant here: the tap loops unroll completely and taps that fall outside
      // the 4x3 / 2x2 image disappear at compile time (most of a 5x5 kernel does)
      constexpr int HoT = (S == 1) ? HT : (HT == 4 ? 2 : 1), WoT = (S == 1) ? WT : (WT == 3 ? 2 : 1);
      // Keras padding as constants: "same" for stride 1, correct_pad for stride 2
      constexpr int PT = (S == 1) ? KS / 2 : KS / 2 - (1 - HT % 2), PLF = (S == 1) ? KS / 2 : KS / 2 - (1 - WT % 2);
      for (int task = tid; task < gvalid * Q; task += NTHREADS) {
        const int tq = task % Q, gi = task / Q;
        if (tq >= nt_valid * 4) continue;
        const int cq = ch0 + 4 * tq;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scD + cq);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(a.shD + cq);
        const float* E = s_E + (size_t)gi * (HT * WT) * LDE + 4 * tq;
        const float* wd = a.Wd + cq;
        float* yout = a.Y + (size_t)(b0 + gi) * (HoT * WoT) * a.Cexp + cq;
        f32x4 ein[HT * WT];
#pragma unroll
        for (int pix = 0; pix < HT * WT; ++pix) ein[pix] = *reinterpret_cast<const f32x4*>(E + (size_t)pix * LDE);
        f32x4 ssum = {0.f, 0.f, 0.f, 0.f};
        f32x4 acc[HoT * WoT];
#pragma unroll
        for (int o = 0; o < HoT * WoT; ++o) acc[o] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < KS; ++i) {
#pragma unroll
          for (int jx = 0; jx < KS; ++jx) {
            // is this tap used by any output pixel?
            bool used = false;
#pragma unroll
            for (int oh = 0; oh < HoT; ++oh)
#pragma unroll
              for (int ow = 0; ow < WoT; ++ow) {
                const int ih = oh * S - PT + i, iw = ow * S - PLF + jx;
                used |= (ih >= 0 && ih < HT && iw >= 0 && iw < WT);
              }
            if (!used) continue;
            const f32x4 wv = *reinterpret_cast<const f32x4*>(wd + (size_t)(i * KS + jx) * a.Cexp);
#pragma unroll
            for (int oh = 0; oh < HoT; ++oh)
#pragma unroll
              for (int ow = 0; ow < WoT; ++ow) {
                const int ih = oh * S - PT + i, iw = ow * S - PLF + jx;
                if (ih >= 0 && ih < HT && iw >= 0 && iw < WT) acc[oh * WoT + ow] += ein[ih * WT + iw] * wv;
              }
          }
        }
#pragma unroll
        for (int o = 0; o < HoT * WoT; ++o) {
          f32x4 y = acc[o] * sc + sh;
          y = swish4_(y);
          *reinterpret_cast<f32x4*>(yout + (size_t)o * a.Cexp) = y;
          ssum += y;
        }
        *reinterpret_cast<f32x4*>(a.sums + (size_t)(b0 + gi) * a.Cexp + cq) = ssum;
        *reinterpret_cast<f32x4*>(s_sumc + (size_t)gi * CC + 4 * tq) = ssum;
      }
    }
    if (cb + 1 < ncb) __syncthreads();             // the next pass overwrites s_E / s_wd / s_red
  }
#ifdef MKWS_FRONT_TIMING
  __syncthreads();
  if (tid == 0) dbgp[3] = wall_clock64();
#endif
  MKWS_WG_END();
}

// Where a weight stream comes from.  The stream helpers below only call ld(idx) (idx = float index of the fragment: tile and
// chunk offsets) through wload(), so a kernel chooses the addressing:
//   const float*  a per-lane pointer; hipcc addresses every load with a 64-bit VALU add (v_lshl_add_u64)
//   WBuf  a UNIFORM base as a buffer descriptor + a 32-bit per-lane byte offset; the fragment offset rides in an SGPR
//         (buffer_load_dwordx4 v, voffset, rsrc, soffset offen): NO VALU instruction per load.  That matters because VALU and MFMA
//         work of a SIMD serialize (tools/microbench/mfma_valu_overlap.hip).  idx must be wave-uniform: kernels that use WBuf take
//         their wave index through readfirstlane.
__device__ __forceinline__ f32x4 wload(const float* p, size_t idx) { return *reinterpret_cast<const f32x4*>(p + idx); }
__device__ __forceinline__ f32x4 wload(const WBuf& b, size_t idx) { return b.ld(idx); }

// acc[q][m] += sum_j W(j, tile0 + tstride*q) . xfrag(j, m) for j in [0, KC): weight fragments via a
// DEPTH-deep register ring (prologue / branch-free steady state / drain, so hipcc emits counted vmcnt
// waits); every weight fragment feeds MT activation tiles.
template <int NTWR, int DEPTH, typename WP>
__device__ __forceinline__ void stream_mfma_prefetch(f32x4 (&wq)[DEPTH][NTWR], WP wlane, size_t chunk_stride, int tile0,
                                                     int tstride, int ntiles, int KC) {
  if (KC >= DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
      for (int q = 0; q < NTWR; ++q) {
        int t = tile0 + tstride * q;
        if (t >= ntiles) t = ntiles - 1;
        wq[d][q] = wload(wlane, (size_t)t * 256 + (size_t)d * chunk_stride);
      }
  }
}

// PRE: the first DEPTH chunks were already requested by stream_mfma_prefetch (issued a phase earlier, so
// their latency hides behind other work); wq is the caller's ring (NTWR >= NTW columns).
// Activation fragments come from LDS in two steps so that they can be software-pipelined: xload(j, m) issues the
// ds_reads of chunk j (called one chunk ahead), xmake(raw) turns them into the MFMA operand at use.
template <int NTW, int DEPTH, int MT, bool PRE, int NTWR, typename WP, typename XL, typename XM>
__device__ __forceinline__ void stream_mfma(f32x4 (&acc)[NTW][MT], f32x4 (&wq)[DEPTH][NTWR], WP wlane, size_t chunk_stride,
                                            int tile0, int tstride, int ntiles, int KC, XL xload, XM xmake) {
  size_t wt[NTW];
#pragma unroll
  for (int q = 0; q < NTW; ++q) {
    int t = tile0 + tstride * q;
    if (t >= ntiles) t = ntiles - 1;             // clamped: result unused
    wt[q] = (size_t)t * 256;
  }
  auto load = [&](int j, f32x4 (&wv)[NTWR]) {
#pragma unroll
    for (int q = 0; q < NTW; ++q) wv[q] = wload(wlane, wt[q] + (size_t)j * chunk_stride);
  };
  // fragment buffers alternate with the ring slot (distinct registers, so the next chunk's ds_reads really
  // issue before this chunk's MFMAs instead of waiting for their operands to die)
  constexpr int XB = (DEPTH % 2 == 0) ? 2 : DEPTH;
  decltype(xload(0, 0)) xr[XB][MT];
  if (KC > 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m) xr[0][m] = xload(0, m);
  }
  // a wave with a single accumulator (one tile, one row tile) would issue 4 dependent MFMAs per chunk (40-cycle dependent
  // latency vs 32-cycle issue): its odd k-steps go to a second accumulator, folded in once at the end
  constexpr bool SPLIT = (NTW * MT == 1);
  f32x4 acc_odd = {0.f, 0.f, 0.f, 0.f};
  auto compute = [&](int d, int j, const f32x4 (&wv)[NTWR]) {
    const int nj = (j + 1 < KC) ? j + 1 : j;
#pragma unroll
    for (int m = 0; m < MT; ++m) xr[((d + 1) % DEPTH) % XB][m] = xload(nj, m);
    __builtin_amdgcn_sched_barrier(0);           // the next chunk's ds_reads go out BEFORE this chunk's MFMAs, not after them
    f32x4 x[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) x[m] = xmake(xr[d % XB][m]);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int q = 0; q < NTW; ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          if (SPLIT && (s & 1)) acc_odd = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[q][s], x[m][s], acc_odd, 0, 0, 0);
          else acc[q][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[q][s], x[m][s], acc[q][m], 0, 0, 0);
        }
  };
  if (KC >= DEPTH) {
    if (!PRE) {
#pragma unroll
      for (int d = 0; d < DEPTH; ++d) load(d, wq[d]);
    }
    int j = 0;
    for (; j + 2 * DEPTH <= KC; j += DEPTH) {
#pragma unroll
      for (int d = 0; d < DEPTH; ++d) {
        compute(d, j + d, wq[d]);
        load(j + DEPTH + d, wq[d]);
        __builtin_amdgcn_sched_barrier(0);     // keep each reload behind its slot's MFMAs (hipcc otherwise sinks them all to the loop end)
      }
    }
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      compute(d, j + d, wq[d]);
      if (j + DEPTH + d < KC) load(j + DEPTH + d, wq[d]);
      __builtin_amdgcn_sched_barrier(0);
    }
    j += DEPTH;
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (j + d < KC) compute(d, j + d, wq[d]);
  } else {
    // short stream (KC < DEPTH): chunk j uses ring slot j, so the fragment buffers still alternate; all requests first (one latency)
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (d < KC) load(d, wq[d]);
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (d < KC) compute(d, d, wq[d]);
  }
  if (SPLIT) acc[0][0] += acc_odd;
}

// Sum of v over the 64 lanes of a wave (all active), the same bits in every lane and one fixed tree: within each row of 16 lanes by DPP
// (lane pairs, quads, halves, the row), then the four row sums as (r0 + r1) + (r2 + r3).  No LDS round trip.
__device__ __forceinline__ float wave_sum64_(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));   // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));   // row_mirror
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}

// ------------------------------------------------------------------------------------------------
// Whole-MBConv kernel for big-image blocks (used for 3a and 4a): expand -> depthwise -> squeeze-excite -> gated
// projection (+ residual) in ONE launch, G clips per workgroup, two workgroups per CU.  Only the block input and
// the block output touch HBM: the 6x-expanded tensor lives in LDS one CC-channel chunk at a time, the depthwise
// output of ALL channels stays in LDS, the SE FCs run inside the workgroup and the projection reads its gated
// operand rows straight from LDS.
//   once       block input -> LDS as MFMA B-operand fragments (zero padded rows / k)
//   per chunk  P1: E[G*HW, CC] = swish(BN(X . We[:, chunk])): wave tasks = (row tile, n-tile); both operands are
//                  lane-linear ds_read_b128 fragments
//              P2: depthwise (one output pixel x channel quad per item, out-of-image taps read a zero row) + BN +
//                  swish -> D[:, chunk]
//              Constants are staged global -> registers -> LDS one phase ahead ("load early, write late"): P1
//              requests the depthwise taps / BN constants that P2 of the same chunk needs and stores them just
//              before the barrier; P2 does the same for the expand weights / BN constants of the next chunk.
//              Two barriers per chunk.
//   SE         three barriers.  Channel means: a strip item of P2 leaves the sum of its SEG outputs in a slot, and a thread per
//              (clip, channel) adds the slots of its channel in ascending order during the next chunk's P1 (quad-item
//              instantiations: fixed-order two-step column sums of D after the loop);  r = swish(mean . Wr + br): a wave per
//              unit, lanes stride the channels, one fixed DPP / readlane tree;  gate = sigmoid(r . We + be), thread per channel
//   project    wave = (n-tile, row-tile lane): the K fragments of its n-tile stream through a register ring
//              (requested before the SE phase), each feeding the wave's row tiles; gated D rows are the MFMA B
//              operands, read from LDS; BN, residual
// Every reduction has a fixed order and nothing depends on the batch size: results are bit-identical across batches.
// Measured (profiles/r02_notes.md): wins for 3a (50 vs 68 us) and 4a (33 vs 49 us); for 2a / 2b / 3b the per-clip
// serialisation of MFMA and VALU phases (their depthwise outputs leave room for one or two clips per CU only) ties
// the three-kernel path, which therefore stays in place for those blocks.
template <int KS, int S, int KCT, int HT, int WT, int CEXP, int CC, int G, int SEG>
struct MidGeom {
  static constexpr int HW = HT * WT;
  static constexpr int HoT = (S == 1) ? HT : (HT + 1) / 2, WoT = (S == 1) ? WT : (WT + 1) / 2;
  static constexpr int HoWo = HoT * WoT;
  static constexpr int PT = (S == 1) ? KS / 2 : KS / 2 - (1 - HT % 2), PLF = (S == 1) ? KS / 2 : KS / 2 - (1 - WT % 2);
  static constexpr int NSEG = WoT / SEG;
  static constexpr int NC = (SEG - 1) * S + KS;
  static constexpr int Q = CC / 4, NTC = CC / 16, LDE = CC + 4, LDD = CEXP + 4;
  static constexpr int NCH = CEXP / CC;
  static constexpr int KC = CEXP / 16;
  static constexpr int MTI = (G * HW + 15) / 16, MTO = (G * HoWo + 15) / 16;
  // constants staged per chunk, in float4 units: [expand weight fragments | scE | shE] for P1, [taps | scD | shD] for P2
  static constexpr int NW4 = KCT * NTC * 64, NS1 = NW4 + 2 * Q, NS2 = KS * KS * Q + 2 * Q;
  // LDS carve (floats)
  static constexpr int oX = 0;                                   // [KCT][MTI][256]; after the chunk loop: SE partials
  static constexpr int oS1 = oX + KCT * MTI * 256;               // P1 constants of the current chunk
  static constexpr int oS2 = oS1 + NS1 * 4;                      // P2 constants of the current chunk
  static constexpr int oE = oS2 + NS2 * 4;                       // [G*HW + 1 zero row][LDE]   (oS1 .. oD: column-sum partials after the chunk loop)
  static constexpr int oD = oE + (G * HW + 1) * LDE;             // [G*HoWo][LDD]
  static constexpr int oMean = oD + G * HoWo * LDD;
  static constexpr int oGate = oMean + G * CEXP;
  static constexpr int oR = oGate + G * CEXP;
  // strip items (SEG > 1) leave the sum of their SEG outputs here, one slot per (clip, output row, row segment) and channel of the chunk
  static constexpr bool SQ = SEG > 1;
  static constexpr int NSLOT = HoT * NSEG;
  static constexpr int oSq = oR + G * 16;                        // [G][NSLOT][CC]
  static constexpr int lds_floats = oSq + (SQ ? G * NSLOT * CC : 0);
  static_assert(NSEG * SEG == WoT, "segments tile the output row");
  static_assert(CEXP % CC == 0 && CC % 16 == 0, "chunks are whole MFMA tiles");
};

template <int KS, int S, int KCT, int HT, int WT, int CEXP, int CC, int NTP, int G, int SEG, int NTHR, int WPE, bool PAIR = false>
__global__ __launch_bounds__(NTHR, WPE) void mbconv_mid_kernel(MidArgs a) {
  using GM = MidGeom<KS, S, KCT, HT, WT, CEXP, CC, G, SEG>;
  constexpr int HW = GM::HW, HoT = GM::HoT, WoT = GM::WoT, HoWo = GM::HoWo;
  constexpr int NSEG = GM::NSEG, Q = GM::Q, NTC = GM::NTC, LDE = GM::LDE, LDD = GM::LDD, NCH = GM::NCH, KC = GM::KC;
  constexpr int MTI = GM::MTI, MTO = GM::MTO, NW4 = GM::NW4, NS1 = GM::NS1, NS2 = GM::NS2;
  constexpr int NW = NTHR / 64;
  constexpr int SE_MAX = 10;                                     // SE units of blocks 2a..4a: 4, 6, 6, 10, 10
  constexpr int TAP_ROW_UNROLL = (KS == 5) ? 1 : KS;             // 5x5: one tap row at a time (two measured no faster: profiles/strip_addressing.txt)
  // Block 4a (3x3 stride 2 on 7x5) measured no faster with the per-row form of dw_strip_ (profiles/strip_addressing.txt): its strips
  // keep the per-read form and their decode inside the chunk loop.
  constexpr bool STRIP_PER_READ = PAIR && KS == 3 && S == 2 && HT == 7 && WT == 5;
  constexpr int UPW = (SE_MAX + NW - 1) / NW;                    // SE reduce FC: units per wave (wave w owns units w, w + NW, ..)
  constexpr int CPL = (CEXP + 63) / 64;                          // ... and channels per lane (lane l takes channels l, l + 64, ..)
  constexpr bool SQ = GM::SQ;                                    // channel sums come from the depthwise phase's strip items
  constexpr int NSLOT = GM::NSLOT;
  constexpr int CQ = CEXP / 4;                                   // channel quads of D
  constexpr int RS = NTHR / (G * CQ);                            // row slices of the column-sum pass
  constexpr int R1 = (NS1 + NTHR - 1) / NTHR, R2 = (NS2 + NTHR - 1) / NTHR;
  static_assert(NTHR % 64 == 0 && NTHR >= CEXP && NTHR >= 16 * G && RS >= 1, "thread roles");
  static_assert(G * RS * CEXP <= GM::oD - GM::oS1, "aliased scratch fits");
  static_assert(SQ == PAIR && NTHR >= G * CC, "strip items are channel-pair items; a thread per (clip, channel of the chunk) folds their sums");
  extern __shared__ __attribute__((aligned(16))) float s_mid[];
  MKWS_WG_BEGIN();
  float* s_X = s_mid + GM::oX;
  float* s_W = s_mid + GM::oS1;                                  // [KCT][NTC][256] expand weight fragments
  float* s_scE = s_W + NW4 * 4;                                  // [CC], then shE [CC]
  float* s_wd = s_mid + GM::oS2;                                 // [KS*KS][CC] depthwise taps
  float* s_scD = s_wd + KS * KS * CC;                            // [CC], then shD [CC]
  float* s_E = s_mid + GM::oE;
  f32x4* s_csum = reinterpret_cast<f32x4*>(s_W);                 // [G][RS][CQ] column-sum partials (staged constants and E are dead by then)
  float* s_D = s_mid + GM::oD;
  float* s_mean = s_mid + GM::oMean;                             // [G][CEXP]
  float* s_gate = s_mid + GM::oGate;                             // [G][CEXP]
  float* s_r = s_mid + GM::oR;                                   // [G][16]
  float* s_sq = s_mid + GM::oSq;                                 // [G][NSLOT][CC] strip sums of the chunk whose depthwise phase ran last
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform by construction: keeps wave-dependent offsets / branches on the scalar unit
  const int g = lane >> 4, c = lane & 15;
  const int b0 = blockIdx.x * G;
  const int gvalid = (a.B - b0 < G) ? (a.B - b0) : G;
  const int rows = gvalid * HW, rows_out = gvalid * HoWo;
  const size_t row0_in = (size_t)b0 * HW, row0_out = (size_t)b0 * HoWo;
#ifdef MKWS_FRONT_TIMING
  unsigned long long* s_stamp = reinterpret_cast<unsigned long long*>(s_mid + ((GM::lds_floats + 1) & ~1));
  unsigned long long t_mark = 0;
  if (tid == 0) {
    for (int k = 0; k < kMidStamps; ++k) s_stamp[k] = 0;
    t_mark = wall_clock64(); s_stamp[0] = t_mark;
  }
#endif
  // staged constants: element e (float4) of a phase's list comes from base + chunk * stride
  auto src1 = [&](int e, int chn) -> const float* {
    if (e < NW4) {
      const int l = e & 63, jn = e >> 6, j = jn / NTC, ntl = jn - j * NTC;
      return a.WpE + (((size_t)j * a.NTtotE + chn * NTC + ntl) * 64 + l) * 4;
    }
    const int q = e - NW4;
    return (q < Q ? a.scE + 4 * q : a.shE + 4 * (q - Q)) + chn * CC;
  };
  auto src2 = [&](int e, int chn) -> const float* {
    if (e < KS * KS * Q) {
      const int t = e / Q, q = e - t * Q;
      return a.Wd + (size_t)t * CEXP + chn * CC + 4 * q;
    }
    const int q = e - KS * KS * Q;
    return (q < Q ? a.scD + 4 * q : a.shD + 4 * (q - Q)) + chn * CC;
  };
  f32x4 st1[R1], st2[R2];
  auto load1 = [&](int chn) {
#pragma unroll
    for (int k = 0; k < R1; ++k) { const int e = tid + k * NTHR; st1[k] = *reinterpret_cast<const f32x4*>(src1(e < NS1 ? e : NS1 - 1, chn)); }
  };
  auto store1 = [&]() {
#pragma unroll
    for (int k = 0; k < R1; ++k) { const int e = tid + k * NTHR; if (e < NS1) *reinterpret_cast<f32x4*>(s_W + 4 * e) = st1[k]; }
  };
  auto load2 = [&](int chn) {
#pragma unroll
    for (int k = 0; k < R2; ++k) { const int e = tid + k * NTHR; st2[k] = *reinterpret_cast<const f32x4*>(src2(e < NS2 ? e : NS2 - 1, chn)); }
  };
  auto store2 = [&]() {
#pragma unroll
    for (int k = 0; k < R2; ++k) { const int e = tid + k * NTHR; if (e < NS2) *reinterpret_cast<f32x4*>(s_wd + 4 * e) = st2[k]; }
  };
  // ---- prologue: P1 constants of chunk 0, the block input as B fragments, the zero row ----
  load1(0);
  for (int jm = wave; jm < KCT * MTI; jm += NW) {
    const int j = jm / MTI, m = jm - j * MTI;
    const int r = m * 16 + c;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < rows && 16 * j + 4 * g < a.Cin) v = *reinterpret_cast<const f32x4*>(a.X + (row0_in + r) * a.Cin + 16 * j + 4 * g);
    *reinterpret_cast<f32x4*>(s_X + ((size_t)jm * 64 + lane) * 4) = v;
  }
  if (tid < LDE / 4) *reinterpret_cast<f32x4*>(s_E + (size_t)G * HW * LDE + 4 * tid) = (f32x4){0.f, 0.f, 0.f, 0.f};
  store1();
  __syncthreads();
  MID_STAMP(1);

  // The SE weights of this thread's role are requested HERE, a whole chunk loop ahead of their use (round 4: requested at the top of the SE
  // phase, two barriers in front of the reduce FC, their L2 round trip was part of every clip's 3 us of SE; the kernel holds 80-92 of the
  // 128 registers a wave may use, the ~16 these occupy during the loop are free).
  float wr_pre[UPW][CPL], we_pre[SE_MAX], br_pre[UPW], be_pre = 0.0f;
  auto request_se = [&]() {
#pragma unroll
    for (int u = 0; u < UPW; ++u) {
      const int n = wave + NW * u;
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const int ch = lane + 64 * i;
        wr_pre[u][i] = (ch < CEXP && n < a.se) ? a.Wr[(size_t)ch * a.se + n] : 0.0f;
      }
      br_pre[u] = (n < a.se) ? a.br[n] : 0.0f;
    }
#pragma unroll
    for (int n2 = 0; n2 < SE_MAX; ++n2) we_pre[n2] = (tid < CEXP && n2 < a.se) ? a.We[(size_t)n2 * CEXP + tid] : 0.0f;
    be_pre = (tid < CEXP) ? a.be[tid] : 0.0f;
  };
  // SE squeeze, strip instantiations: the last G * CC threads (waves with the fewest P1 tasks) add the NSLOT strip sums of their
  // (clip, channel) in ascending slot order, whatever gvalid is, while the other waves already expand the next chunk
  auto fold_sq = [&](int chn) {
    const int f = tid - (NTHR - G * CC);
    if (f >= 0) {
      const int gi = f / CC, cc = f - gi * CC;
      float t = s_sq[(size_t)gi * NSLOT * CC + cc];
#pragma unroll
      for (int sl = 1; sl < NSLOT; ++sl) t += s_sq[((size_t)gi * NSLOT + sl) * CC + cc];
      s_mean[gi * CEXP + chn * CC + cc] = t * (1.0f / (float)HoWo);
    }
  };
  if (!MKWS_ABLATE(16)) request_se();                            // (timing build, MKWS_ABLATE=16: the round-3 position, for the A/B)
  // P2's strip items: (clip, output row, row segment, channel pair / quad).  Where every thread gets at most one item (ONE_ITEM: all
  // instantiations so far) it is decoded here, once, and not once per chunk.
  using VT = std::conditional_t<PAIR, f32x2, f32x4>;
  constexpr int VW = PAIR ? 2 : 4;                               // channels of an item
  constexpr int QI = CC / VW;                                    // items across the chunk's channels
  constexpr int ITEMS_PER_CLIP = HoT * NSEG * QI;
  constexpr bool ONE_ITEM = G * ITEMS_PER_CLIP <= NTHR;
  using SG = StripGeom<KS, S, HT, WT, SEG>;
  struct StripItem { int tc, ih0, iw0, row0, poff, doff, sqoff; };   // row0: the clip's first row of E; poff / doff / sqoff: float offsets into s_E (first input) / s_D (chunk 0) / s_sq
  auto strip_item = [&](int item) {
    StripItem it;
    int r = item / QI;
    it.tc = item - r * QI;
    const int sg = r % NSEG; r /= NSEG;
    const int oh = r % HoT, gi = r / HoT;
    it.ih0 = oh * S - SG::PT;
    it.iw0 = sg * SEG * S - SG::PLF;
    it.row0 = gi * HW;
    it.poff = (it.row0 + it.ih0 * WT + it.iw0) * LDE + VW * it.tc;
    it.doff = (gi * HoWo + oh * WoT + sg * SEG) * LDD + VW * it.tc;
    it.sqoff = ((gi * HoT + oh) * NSEG + sg) * CC + VW * it.tc;
    return it;
  };
  const StripItem it0 = strip_item(tid);

  for (int chn = 0; chn < NCH; ++chn) {
    const int ch0 = chn * CC;
    // ---- P1: expand this chunk into LDS ----
    load2(chn);
    if constexpr (SQ) {
      if (chn > 0) fold_sq(chn - 1);
    }
    {
      const int ntasks = MKWS_ABLATE(1) ? 0 : ((rows + 15) / 16) * NTC;
      for (int t = wave; t < ntasks; t += NW) {
        const int rt = t / NTC, ntl = t - rt * NTC;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KCT; ++j) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(s_W + ((size_t)(j * NTC + ntl) * 64 + lane) * 4);
          const f32x4 x = *reinterpret_cast<const f32x4*>(s_X + ((size_t)(j * MTI + rt) * 64 + lane) * 4);
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s4], x[s4], acc, 0, 0, 0);
        }
        const int row = rt * 16 + c;
        if (row < rows) {
          f32x4 y = acc * *reinterpret_cast<const f32x4*>(s_scE + ntl * 16 + 4 * g) + *reinterpret_cast<const f32x4*>(s_scE + CC + ntl * 16 + 4 * g);
          y = swish4_(y);
          *reinterpret_cast<f32x4*>(s_E + (size_t)row * LDE + ntl * 16 + 4 * g) = y;
        }
      }
    }
    MID_STAMP(2 + 4 * chn);
    store2();
    __syncthreads();
    MID_STAMP(3 + 4 * chn);
    // ---- P2: depthwise from LDS -> D[:, chunk] ----
    if (chn + 1 < NCH) load1(chn + 1);
    {
      // Row strips (dw_strip_) of channel PAIRS (2b, 3a, 4a) or quads (2a, 3b).  With one output pixel x channel quad per item the
      // phase was LDS-bound: 25 input + 25 tap ds_read_b128 per output of a 5x5 kernel, 336 KB per chunk of block 3a = 2 600 LDS cycles,
      // twice that with the CU's second workgroup in the same phase (measured 2.5 us per chunk).  A strip reads each input of its rows
      // once and each tap once per strip (90 reads for 5 outputs), and pairs instead of quads keep three waves busy instead of one and
      // a half.
      const int nitems = MKWS_ABLATE(2) ? 0 : gvalid * ITEMS_PER_CLIP;
      for (int item = tid; item < nitems; item += NTHR) {
        const StripItem it = (ONE_ITEM && !STRIP_PER_READ) ? it0 : strip_item(item);
        VT acc[SEG];
#pragma unroll
        for (int o = 0; o < SEG; ++o) acc[o] = VT(0.f);
        if constexpr (STRIP_PER_READ) dw_strip_per_read_<VT, KS, S, HT, WT, SEG, LDE, CC, TAP_ROW_UNROLL>(s_E + VW * it.tc, it.row0, G * HW, s_wd + VW * it.tc, it.ih0, it.iw0, acc);
        else dw_strip_<VT, KS, S, HT, WT, SEG, LDE, CC, TAP_ROW_UNROLL>(s_E + it.poff, s_E + G * HW * LDE + VW * it.tc, s_wd + VW * it.tc, it.ih0, it.iw0, acc);
        const VT scd = *reinterpret_cast<const VT*>(s_scD + VW * it.tc), shd = *reinterpret_cast<const VT*>(s_scD + CC + VW * it.tc);
        float* dout = s_D + it.doff + ch0;
        VT ysum = VT(0.f);
#pragma unroll
        for (int o = 0; o < SEG; ++o) {
          VT y = acc[o] * scd + shd;
          y = swishv_(y);
          *reinterpret_cast<VT*>(dout + (size_t)o * LDD) = y;
          if constexpr (PAIR) ysum += y;
        }
        if constexpr (PAIR) *reinterpret_cast<VT*>(s_sq + it.sqoff) = ysum;
      }
    }
    MID_STAMP(4 + 4 * chn);
    if (chn + 1 < NCH) store1();
    __syncthreads();
    MID_STAMP(5 + 4 * chn);
  }
  // The first fragments of the projection weight stream of this wave's n-tile are requested here (L2 hits: every workgroup uses the
  // same ones); the SE weights of this thread's role were requested in front of the chunk loop.
  if (MKWS_ABLATE(16)) request_se();
  constexpr int NWP = NW / NTP;                                  // row-tile lanes per n-tile (waves beyond NWP*NTP idle in the projection)
  constexpr int MTW = (MTO + NWP - 1) / NWP;                     // row tiles per wave
  // Depth of the projection weight ring.  Every wave requests its ring at once and the CU's vector-memory path takes 16 cycles per
  // buffer_load_dwordx4: eight deep, the 16 waves of 2b queued 128 KB = 2048 cycles (1 us, all of it in front of the next barrier:
  // profiles/mid_phases.txt).  Four fragments are 1000 cycles of a SIMD's MFMA time ahead, more than an L2 round trip.
  constexpr int PD = 4;
  const int ntp = wave % NTP, rlp = wave / NTP;
  const WBuf p_w(a.WpP, (unsigned)(g * 64 + c * 4));
  f32x4 wqp[PD][1];
  if (rlp < NWP) stream_mfma_prefetch<1, PD>(wqp, p_w, (size_t)NTP * 256, ntp, 1, NTP, KC);
  if (a.dbg_dw) {
    for (int i = tid; i < rows_out * CQ; i += NTHR) {
      const int r = i / CQ, q4 = (i - r * CQ) * 4;
      *reinterpret_cast<f32x4*>(a.dbg_dw + (row0_out + r) * CEXP + q4) = *reinterpret_cast<const f32x4*>(s_D + (size_t)r * LDD + q4);
    }
  }
  if (!MKWS_ABLATE(4)) {
  if constexpr (SQ) {
    // ---- SE squeeze: the strip sums of the last chunk (those of the earlier chunks were folded during the following P1) ----
    fold_sq(NCH - 1);
  } else {
    // ---- SE squeeze: column sums of D in two fixed-order steps (row slices, then slices) ----
    if (tid < G * RS * CQ) {
      const int q = tid % CQ, rs = (tid / CQ) % RS, gi = tid / (CQ * RS);
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      for (int r = rs; r < HoWo; r += RS) t += *reinterpret_cast<const f32x4*>(s_D + (size_t)(gi * HoWo + r) * LDD + 4 * q);
      s_csum[tid] = t;
    }
    __syncthreads();
    MID_STAMP(kMidStampSE + 0);
    if (tid < G * CQ) {
      const int q = tid % CQ, gi = tid / CQ;
      f32x4 t = s_csum[(size_t)gi * RS * CQ + q];
#pragma unroll 4
      for (int rs = 1; rs < RS; ++rs) t += s_csum[((size_t)gi * RS + rs) * CQ + q];
      *reinterpret_cast<f32x4*>(s_mean + (size_t)gi * CEXP + 4 * q) = t * (1.0f / (float)HoWo);
    }
  }
  __syncthreads();
  MID_STAMP(kMidStampSE + 1);
  // ---- SE reduce: wave w owns units w, w + NW, ..; a lane multiplies its CPL channels in ascending order, the 64 lane sums meet in the
  // fixed tree of wave_sum64_ (every clip of the workgroup the same way: nothing depends on gvalid) and lane 0 finishes the unit ----
  if (tid < 16 * G && (tid & 15) >= a.se) s_r[tid] = 0.0f;
#pragma unroll
  for (int u = 0; u < UPW; ++u) {
    if (wave + NW * u < a.se) {
      float v[G];
#pragma unroll
      for (int gi = 0; gi < G; ++gi) {
        v[gi] = 0.0f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
          const int ch = lane + 64 * i;
          v[gi] += s_mean[gi * CEXP + (ch < CEXP ? ch : 0)] * wr_pre[u][i];
        }
      }
#pragma unroll
      for (int gi = 0; gi < G; ++gi) v[gi] = wave_sum64_(v[gi]);
      if (lane == 0) {
#pragma unroll
        for (int gi = 0; gi < G; ++gi) s_r[gi * 16 + wave + NW * u] = swishf_(v[gi] + br_pre[u]);
      }
    }
  }
  __syncthreads();
  MID_STAMP(kMidStampSE + 3);
  if (tid < CEXP) {
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      float v = be_pre;
#pragma unroll
      for (int n2 = 0; n2 < SE_MAX; ++n2) v += s_r[gi * 16 + n2] * we_pre[n2];
      const float gt = sigmoidf_(v);
      s_gate[gi * CEXP + tid] = gt;
      if (a.dbg_gate && gi < gvalid) a.dbg_gate[(size_t)(b0 + gi) * CEXP + tid] = gt;
    }
  }
  __syncthreads();
  }
  MID_STAMP(kMidStampSE + 4);
#ifdef MKWS_FRONT_TIMING
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // the projection's weight ring, requested in front of the SE tail, has arrived
  MID_STAMP(kMidStampProj + 0);
#endif
  // ---- gated projection (+ BN, residual): every weight fragment of the stream feeds this wave's MTW row tiles ----
  if (rlp < NWP && !MKWS_ABLATE(8)) {
    // Row-tile lanes past MTO - NWP * (MTW - 1) own one row tile fewer: they run the MTW - 1 instantiation instead of multiplying a
    // padding tile (3a: lane 1 used to stream a whole extra tile = 25 % of the projection's MFMA time on the busiest SIMDs).
    constexpr int MT_LO = MTO / NWP;
    const int my_tiles = (MTO - rlp + NWP - 1) / NWP;
    auto run = [&](auto mt_tag) {
      constexpr int MT = decltype(mt_tag)::value;
      const float* erow[MT];
      const float* grow[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        int r = (rlp + NWP * m) * 16 + c;
        if (r >= G * HoWo) r = G * HoWo - 1;                     // padding rows of the last tile: any finite row, never stored
        erow[m] = s_D + (size_t)r * LDD + 4 * g;
        grow[m] = s_gate + (size_t)(r / HoWo) * CEXP + 4 * g;
      }
      struct EG { f32x4 e, g; };
      auto xload = [&](int j, int m) { return EG{*reinterpret_cast<const f32x4*>(erow[m] + 16 * j), *reinterpret_cast<const f32x4*>(grow[m] + 16 * j)}; };
      auto xmake = [](const EG& v) { return v.e * v.g; };
      f32x4 acc[1][MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[0][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      stream_mfma<1, PD, MT, true>(acc, wqp, p_w, (size_t)NTP * 256, ntp, 1, NTP, KC, xload, xmake);
      const int n = ntp * 16 + 4 * g;
      if (n < a.Cout) {
        const f32x4 scp = *reinterpret_cast<const f32x4*>(a.scP + n), shp = *reinterpret_cast<const f32x4*>(a.shP + n);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int r = (rlp + NWP * m) * 16 + c;
          if (r < rows_out) {
            f32x4 y = acc[0][m] * scp + shp;
            if (a.residual) y += *reinterpret_cast<const f32x4*>(a.X + (row0_in + r) * a.Cin + n);
            *reinterpret_cast<f32x4*>(a.Y + (row0_out + r) * a.Cout + n) = y;
          }
        }
      }
    };
    if constexpr (MT_LO >= 1 && MT_LO < MTW) {
      if (my_tiles >= MTW) run(std::integral_constant<int, MTW>{});
      else run(std::integral_constant<int, MT_LO>{});
    } else {
      run(std::integral_constant<int, MTW>{});
    }
  }
#ifdef MKWS_FRONT_TIMING
  MID_STAMP(kMidStampProj + 1);
  __syncthreads();
  MID_STAMP(kMidStampProj + 2);
  if (tid == 0 && a.dbg_t) {
    s_stamp[kMidStampProj + 3] = t_mark;
    unsigned long long* dbgp = a.dbg_t + (size_t)blockIdx.x * kMidStamps;
    for (int k = 0; k < kMidStamps; ++k) dbgp[k] = s_stamp[k];
  }
#endif
  MKWS_WG_END();
}

// ------------------------------------------------------------------------------------------------
// Back half of a big-image MBConv block (2a, 2b, 3b, after mbconv_front_kernel): squeeze-excite + gated projection
// (+ BN, residual) in ONE launch, one clip per workgroup, 2-4 workgroups per CU.  The clip's depthwise output
// (34-75 KB) is read from HBM exactly once into LDS; the channel means are fixed-order column sums of that tile, the SE
// FCs run in the workgroup (weights requested at kernel start, consumed after the staging), and the projection reads its
// gated operand rows from LDS while its weight fragments stream through a register ring that was requested at kernel
// start.  Replaces se_reduce_kernel + se_expand_kernel + the gated pw_gemm_kernel (three launches, a [B, C] gate round
// trip and a second pass over D per N split).
struct BackArgs {
  const float* D; const float* X; int Cin;
  const float* Wr; const float* br; const float* We; const float* be; int se;
  const float* WpP; const float* scP; const float* shP;
  float* Y; int Cout; int residual;
  float* dbg_gate;
  int B;
};

template <int HOWO, int CEXP, int NTP, int RS, int NTHR, int WPE>
__global__ __launch_bounds__(NTHR, WPE) void mbconv_back_kernel(BackArgs a) {
  constexpr int LDD = CEXP + 4, CQ = CEXP / 4, KC = CEXP / 16, MTO = (HOWO + 15) / 16, NW = NTHR / 64;
  constexpr int SE_MAX = 10;                                     // SE units of blocks 2a..4a: 4, 6, 6, 10, 10
  constexpr int NSL = NTHR / 16, CPS = (CEXP + NSL - 1) / NSL;
  constexpr int NLD = (HOWO * CQ + NTHR - 1) / NTHR;             // float4 per thread of the clip's D tile
  constexpr int NWP = NW / NTP, MTW = (MTO + NWP - 1) / NWP;
  constexpr int PD = (KC >= 8) ? 8 : 4;
  static_assert(RS * CQ <= NTHR && NTHR >= CEXP && NWP >= 1, "thread roles");
  extern __shared__ __attribute__((aligned(16))) float s_bk[];
  MKWS_WG_BEGIN();
  float* s_D = s_bk;                                             // [HOWO][LDD]
  float* s_mean = s_D + HOWO * LDD;                              // [CEXP]
  float* s_gate = s_mean + CEXP;                                 // [CEXP]
  float* s_r = s_gate + CEXP;                                    // [16]
  float* s_scr = s_r + 16;                                       // [max(RS*CEXP, NTHR)]: column-sum partials, then SE partials
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform by construction: keeps wave-dependent offsets / branches on the scalar unit
  const int g = lane >> 4, c = lane & 15;
  const size_t b = blockIdx.x;
  const float* Dc = a.D + b * HOWO * CEXP;
  // everything this workgroup will need from global memory is requested up front: the D tile, the SE weights of this
  // thread's role and the head of the projection weight stream of this wave's n-tile
  f32x4 dreg[NLD];
#pragma unroll
  for (int k = 0; k < NLD; ++k) {
    const int e = tid + k * NTHR;
    dreg[k] = *reinterpret_cast<const f32x4*>(Dc + 4 * (size_t)(e < HOWO * CQ ? e : HOWO * CQ - 1));
  }
  float wr_pre[CPS], we_pre[SE_MAX];
  {
    const int n = tid & 15, sl = tid >> 4;
#pragma unroll
    for (int i = 0; i < CPS; ++i) {
      const int ch = sl * CPS + i;
      wr_pre[i] = (ch < CEXP && n < a.se) ? a.Wr[(size_t)ch * a.se + n] : 0.0f;
    }
#pragma unroll
    for (int n2 = 0; n2 < SE_MAX; ++n2) we_pre[n2] = (tid < CEXP && n2 < a.se) ? a.We[(size_t)n2 * CEXP + tid] : 0.0f;
  }
  const float br_pre = (tid < 16 && tid < a.se) ? a.br[tid] : 0.0f;
  const float be_pre = (tid < CEXP) ? a.be[tid] : 0.0f;
  const int ntp = wave % NTP, rlp = wave / NTP;
  const WBuf p_w(a.WpP, (unsigned)(g * 64 + c * 4));
  f32x4 wqp[PD][1];
  if (rlp < NWP) stream_mfma_prefetch<1, PD>(wqp, p_w, (size_t)NTP * 256, ntp, 1, NTP, KC);
#pragma unroll
  for (int k = 0; k < NLD; ++k) {
    const int e = tid + k * NTHR;
    if (e < HOWO * CQ) { const int r = e / CQ, q = e - r * CQ; *reinterpret_cast<f32x4*>(s_D + (size_t)r * LDD + 4 * q) = dreg[k]; }
  }
  __syncthreads();
  // ---- SE squeeze: column sums of D in two fixed-order steps (row slices, then slices) ----
  f32x4* s_csum = reinterpret_cast<f32x4*>(s_scr);
  if (tid < RS * CQ) {
    const int q = tid % CQ, rs = tid / CQ;
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    for (int r = rs; r < HOWO; r += RS) t += *reinterpret_cast<const f32x4*>(s_D + (size_t)r * LDD + 4 * q);
    s_csum[tid] = t;
  }
  __syncthreads();
  if (tid < CQ) {
    f32x4 t = s_csum[tid];
#pragma unroll
    for (int rs = 1; rs < RS; ++rs) t += s_csum[rs * CQ + tid];
    *reinterpret_cast<f32x4*>(s_mean + 4 * tid) = t * (1.0f / (float)HOWO);
  }
  __syncthreads();
  // ---- SE reduce (thread = (unit, channel slice), slices folded in fixed order), expand, gate ----
  {
    const int n = tid & 15, sl = tid >> 4;
    float v = 0.0f;
#pragma unroll
    for (int i = 0; i < CPS; ++i) {
      const int ch = sl * CPS + i;
      v += s_mean[ch < CEXP ? ch : 0] * wr_pre[i];
    }
    s_scr[sl * 16 + n] = v;
  }
  __syncthreads();
  if (tid < 16) {
    float v = 0.0f;
#pragma unroll 8
    for (int sl = 0; sl < NSL; ++sl) v += s_scr[sl * 16 + tid];
    s_r[tid] = (tid < a.se) ? swishf_(v + br_pre) : 0.0f;
  }
  __syncthreads();
  if (tid < CEXP) {
    float v = be_pre;
#pragma unroll
    for (int n2 = 0; n2 < SE_MAX; ++n2) v += s_r[n2] * we_pre[n2];
    const float gt = sigmoidf_(v);
    s_gate[tid] = gt;
    if (a.dbg_gate) a.dbg_gate[b * CEXP + tid] = gt;
  }
  __syncthreads();
  // ---- gated projection (+ BN, residual) ----
  if (rlp < NWP) {
    // row-tile lanes that own one row tile fewer run the MTW - 1 instantiation instead of multiplying a padding tile (2a / 2b: three of
    // the four lanes, a third of their MFMAs; 3b: lane 1, half of them)
    constexpr int MT_LO = MTO / NWP;
    const int my_tiles = (MTO - rlp + NWP - 1) / NWP;
    auto run = [&](auto mt_tag) {
      constexpr int MT = decltype(mt_tag)::value;
      const float* erow[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        int r = (rlp + NWP * m) * 16 + c;
        if (r >= HOWO) r = HOWO - 1;                               // padding rows of the last tile: any finite row, never stored
        erow[m] = s_D + (size_t)r * LDD + 4 * g;
      }
      const float* grow = s_gate + 4 * g;
      struct EG { f32x4 e, g; };
      auto xload = [&](int j, int m) { return EG{*reinterpret_cast<const f32x4*>(erow[m] + 16 * j), *reinterpret_cast<const f32x4*>(grow + 16 * j)}; };
      auto xmake = [](const EG& v) { return v.e * v.g; };
      f32x4 acc[1][MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[0][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      stream_mfma<1, PD, MT, true>(acc, wqp, p_w, (size_t)NTP * 256, ntp, 1, NTP, KC, xload, xmake);
      const int n = ntp * 16 + 4 * g;
      if (n < a.Cout) {
        const f32x4 scp = *reinterpret_cast<const f32x4*>(a.scP + n), shp = *reinterpret_cast<const f32x4*>(a.shP + n);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int r = (rlp + NWP * m) * 16 + c;
          if (r < HOWO) {
            f32x4 y = acc[0][m] * scp + shp;
            if (a.residual) y += *reinterpret_cast<const f32x4*>(a.X + (b * HOWO + r) * a.Cin + n);
            *reinterpret_cast<f32x4*>(a.Y + (b * HOWO + r) * a.Cout + n) = y;
          }
        }
      }
    };
    if constexpr (MT_LO >= 1 && MT_LO < MTW) {
      if (my_tiles >= MTW) run(std::integral_constant<int, MTW>{});
      else run(std::integral_constant<int, MT_LO>{});
    } else {
      run(std::integral_constant<int, MTW>{});
    }
  }
  MKWS_WG_END();
}

// ------------------------------------------------------------------------------------------------
// Whole-MBConv kernel for the tiny-image blocks (4x3 and 2x2 inputs: blocks 4b..7a).
// One workgroup owns one 16-row MFMA tile of activations (4 clips of 2x2, or 1 clip of 4x3) and carries it
// through expand -> depthwise -> SE -> gated project entirely in LDS; every weight of the block streams
// through the workgroup exactly once as MFMA A-operand fragments, the activations are the B operand read
// from LDS.  Nothing but the block input and output touches HBM, and there is one launch per block.
//   phase A  E[16, Cexp]   = swish(BN(X[16, Cin] . We))                     (waves split the Cexp/16 tiles)
//   phase B  E <- swish(BN(depthwise(E))) in place, S[clip, Cexp] = sum over pixels   (thread = clip x quad)
//   phase C  r = swish(S/HW . Wr + br);  gate = sigmoid(r . We2 + be)       (K split over waves / tiles over waves)
//   phase D  Y[16, Cout]   = BN((E * gate) . Wp) (+ X)                      (waves split the Cout/16 tiles)
struct BlockArgs {
  const float* X; int Cin;
  const float* WpE; const float* scE; const float* shE; int KCe; int NTe;
  const float* Wd; const float* scD; const float* shD;
  const float* WrP; const float* br; int NTR;
  const float* We2P; const float* be;
  const float* WpP; const float* scP; const float* shP; int NTp;
  float* Y; int Cout; int residual;
  float* dbg_dw; float* dbg_gate;
  int B, Cexp, se;
  // squeeze-excite on the 4x4x1 matrix instruction (4x3-image blocks, see Se4 below): null / 0 = the 16x16x4 streams above
  const float* WrQ; const float* We2Q; int seT0, seNQ;
#ifdef MKWS_FRONT_TIMING
  unsigned long long* dbg_t;
#endif
};

// ------------------------------------------------------------------------------------------------
// Squeeze-excite FCs of a 4x3-image workgroup on v_mfma_f32_4x4x1_16b_f32 (round 6).
// A workgroup holds G <= 4 clips, so both FCs are [4 x K] . [K x N] products.  On the 16x16x4 instruction the clips were 4 of 16 columns
// (and a 20 / 28-unit reduce FC 2 of 3 streamed tiles): 72 + 48 MFMAs per wave and block at 1 / 6 and 1 / 4 of their work useful -- 2 us of
// matrix issue per SIMD in C1 alone, which nothing overlaps (an fp32 MFMA blocks its SIMD's vector issue: tools/microbench/issue_costs.hip).
// The 4x4x1 form is 16 independent 4x4 outer products per instruction (lane l = 4 blk + r: A = a(i = r, blk), B = b(j = r, blk),
// D VGPR v = d(i = v, j = r, blk); checked by tools/microbench/mfma_4x4.hip, 5.1 ns per instruction) with j = the clip:
//   C1 (reduce)  i = 4 SE units, blocks = 8 unit groups x 2 channel halves: one instruction = 2 channels x 32 units x 4 clips.  Wave w owns channels
//                [w cpw, (w + 1) cpw), cpw = Cexp / 8; its lanes 32..63 (half 1) take the LAST T0 = 4 ceil(cpw / 8) of them, lanes 0..31 the first
//                cpw - T0 (their last T0 - (cpw - T0) instructions multiply zero weights against the other half's means).  A comes from WrQ
//                [wave][T0 / 4][lane][4] (the lane's weights of four consecutive instructions in one dwordx4), B from the means in LDS
//                (a float4 = four consecutive channels of clip l & 3).  32 / 44 instructions per wave for Cexp = 480 / 672 (was 72 x 14 ns).
//                Halves are added through ds_bpermute (half 0 + half 1), waves through LDS in wave order: a fixed order.
//   C2 (expand)  i = 4 channels, blocks = 16 channel quads: one instruction = 64 channels x 4 clips x 1 unit, A from We2Q
//                [group of 64 channels][ceil(se / 4)][lane][4], B = r[clip][unit] from LDS.  The lane that ends up with the gate of channels
//                4 blk .. + 3 of clip j multiplies the clip's HoWo depthwise rows by it on the spot: the gate never goes to LDS and the
//                separate gate pass (a phase and a barrier of 1.9-2.6 us per block) is gone.
// Both kernels that run these blocks (mbconv_block_kernel, mbconv_chain_kernel's chain_block) call the same functions: bit-identical.
constexpr int kSe4MaxTQ = 11, kSe4MaxNQ = 7, kSe4MaxGroups = 2;
__device__ __forceinline__ f32x4 mfma4x4_(const f32x4& a, const f32x4& b, f32x4 acc) {
#pragma unroll
  for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a[e], b[e], acc, 0, 0, 0);
  return acc;
}
// requests wave `wave`'s reduce weights.  The packing is padded with zero weights to kSe4MaxTQ dwordx4 per lane whatever T0 is, and the
// loops below run that fixed count (straight-line code: a bound taken from the block table made every step its own basic block with its
// own s_waitcnt); the padding steps multiply zero weights against the slice's last four means (address clamped: finite).
__device__ __forceinline__ void se4_request_c1(f32x4 (&wq)[kSe4MaxTQ], const float* WrQ, int wave, int lane) {
  const WBuf w(WrQ + (size_t)wave * kSe4MaxTQ * 256, (unsigned)lane * 4u);
#pragma unroll
  for (int q = 0; q < kSe4MaxTQ; ++q) wq[q] = w.ld((size_t)q * 256);
}
// partial r[clip][unit] of this wave's channels -> s_P[wave][G][32]
template <int G, int NWAVES>
__device__ __forceinline__ void se4_c1(const f32x4 (&wq)[kSe4MaxTQ], int T0, int Cexp, const float* s_S, float* s_P, int wave, int lane) {
  const int TQ = T0 >> 2, cpw = Cexp / NWAVES;
  const int j = lane & 3, ug = (lane >> 2) & 7, kh = lane >> 5;
  const float* mrow = s_S + (size_t)(j < G ? j : G - 1) * Cexp + wave * cpw + (kh ? cpw - T0 : 0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < kSe4MaxTQ; ++q) acc = mfma4x4_(wq[q], *reinterpret_cast<const f32x4*>(mrow + 4 * (q < TQ ? q : TQ - 1)), acc);
  // the other half's partial, component by component through named scalars: hipcc (ROCm 7.2) folds the loop form
  // `other[r] = bit_cast<float>(ds_bpermute(idx, bit_cast<int>(acc[r])))` into ONE ds_bpermute of acc[0] that feeds all four components
  // (units 4 ug + 1..3 wrong, unit 4 ug right: tools/microbench/se4_unit.hip found it)
  const int px = (lane ^ 32) << 2;
  const float a0 = acc.x, a1 = acc.y, a2 = acc.z, a3 = acc.w;
  f32x4 other;
  other.x = __int_as_float(__builtin_amdgcn_ds_bpermute(px, __float_as_int(a0)));
  other.y = __int_as_float(__builtin_amdgcn_ds_bpermute(px, __float_as_int(a1)));
  other.z = __int_as_float(__builtin_amdgcn_ds_bpermute(px, __float_as_int(a2)));
  other.w = __int_as_float(__builtin_amdgcn_ds_bpermute(px, __float_as_int(a3)));
  if (lane < 32 && j < G) *reinterpret_cast<f32x4*>(s_P + ((size_t)(wave * G + j) * 32 + 4 * ug)) = acc + other;
}
// r[clip][unit] = swish(sum over waves + br) -> s_R[clip][LDR]; thread = (clip, unit); br_pre = this thread's bias (0 past se)
template <int G, int NWAVES, int LDR>
__device__ __forceinline__ void se4_fold(const float* s_P, float* s_R, int se, float br_pre, int tid) {
  if (tid < 32 * G) {
    const int clip = tid >> 5, n = tid & 31;
    float v = 0.0f;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) v += s_P[(size_t)(w * G + clip) * 32 + n];
    s_R[clip * LDR + n] = (n < se) ? swishf_(v + br_pre) : 0.0f;
  }
}
// requests the expand weights of this wave's channel groups (wave, wave + NWAVES); kSe4MaxNQ dwordx4 per lane and group, zero padded like the reduce weights
template <int NWAVES>
__device__ __forceinline__ void se4_request_c2(f32x4 (&wq)[kSe4MaxGroups][kSe4MaxNQ], const float* We2Q, int Cexp, int wave, int lane) {
  const int NG = (Cexp + 63) >> 6;
#pragma unroll
  for (int k = 0; k < kSe4MaxGroups; ++k) {
    const int gq = wave + k * NWAVES;
    const WBuf w(We2Q + (size_t)(gq < NG ? gq : NG - 1) * kSe4MaxNQ * 256, (unsigned)lane * 4u);
#pragma unroll
    for (int q = 0; q < kSe4MaxNQ; ++q) wq[k][q] = w.ld((size_t)q * 256);
  }
}
// gate = sigmoid(r . We2 + be) for this wave's channel groups, applied to the clips' depthwise rows in place (rows clip * HW + o, o < HoWo)
template <int G, int HW, int HoWo, int NWAVES, int LDR>
__device__ __forceinline__ void se4_c2_gate(const f32x4 (&wq)[kSe4MaxGroups][kSe4MaxNQ], int Cexp, const float* s_R, const float* s_be, float* s_E,
                                            int wave, int lane, float* dbg_gate_clip0, int gvalid) {
  const int NG = (Cexp + 63) >> 6, LDE = Cexp + 4;
  const int j = lane & 3;
  f32x4 rb[kSe4MaxNQ];
#pragma unroll
  for (int q = 0; q < kSe4MaxNQ; ++q) rb[q] = *reinterpret_cast<const f32x4*>(s_R + (j < G ? j : 0) * LDR + 4 * q);      // (units < 28: written by the fold)
#pragma unroll
  for (int k = 0; k < kSe4MaxGroups; ++k) {
    const int gq = wave + k * NWAVES;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < kSe4MaxNQ; ++q) acc = mfma4x4_(wq[k][q], rb[q], acc);
    const int ch = 64 * gq + 4 * (lane >> 2);
    if (gq < NG && j < G && ch < Cexp) {
      const f32x4 y = sigmoid4_(acc + *reinterpret_cast<const f32x4*>(s_be + ch));
      float* e0 = s_E + (size_t)(j * HW) * LDE + ch;
#pragma unroll
      for (int o = 0; o < HoWo; ++o) *reinterpret_cast<f32x4*>(e0 + (size_t)o * LDE) = *reinterpret_cast<const f32x4*>(e0 + (size_t)o * LDE) * y;
      if (dbg_gate_clip0 && j < gvalid) *reinterpret_cast<f32x4*>(dbg_gate_clip0 + (size_t)j * Cexp + ch) = y;
    }
  }
}

// Flattened variant of stream_mfma for MANY short accumulation runs (phase A, SE expand): run r = tiles
// [tile_of(r), +NTW), each KC chunks long.  The weight ring keeps DEPTH chunks in flight ACROSS runs, so a
// run's first loads are already issued while the previous run computes (no per-run latency bubble).  The
// epilogue must not issue global loads (they would drain the in-order vmcnt ring): constants come from LDS.
template <int NTW, int DEPTH, typename WP, typename TOF>
__device__ __forceinline__ void stream_mfma_runs_prefetch(f32x4 (&wq)[DEPTH][NTW], WP wlane, size_t chunk_stride, int ntiles,
                                                          int nruns, int KC, TOF tile_of) {
  const int T = nruns * KC;                              // a stream shorter than the ring is requested whole (stream_mfma_runs<PRE> then only computes)
  int lr = 0, lj = 0;
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    if (d < T) {
      const int t0 = tile_of(lr);
#pragma unroll
      for (int q = 0; q < NTW; ++q) {
        int t = t0 + q;
        if (t >= ntiles) t = ntiles - 1;
        wq[d][q] = wload(wlane, (size_t)t * 256 + (size_t)lj * chunk_stride);
      }
      if (++lj == KC) { lj = 0; ++lr; }
    }
  }
}

template <int NTW, int DEPTH, int MT, bool PRE, typename WP, typename XL, typename XM, typename TOF, typename EPI>
__device__ __forceinline__ void stream_mfma_runs(f32x4 (&wq)[DEPTH][NTW], WP wlane, size_t chunk_stride, int ntiles, int nruns,
                                                 int KC, TOF tile_of, XL xload, XM xmake, EPI epilogue) {
  const int T = nruns * KC;
  if (T <= 0) return;
  int lr = 0, lj = 0;                                  // load cursor (run, chunk)
  if (PRE && T >= DEPTH) { lr = DEPTH / KC; lj = DEPTH - lr * KC; }
  auto load = [&](f32x4 (&wv)[NTW]) {
    const int t0 = tile_of(lr);
#pragma unroll
    for (int q = 0; q < NTW; ++q) {
      int t = t0 + q;
      if (t >= ntiles) t = ntiles - 1;
      wv[q] = wload(wlane, (size_t)t * 256 + (size_t)lj * chunk_stride);
    }
    if (++lj == KC) { lj = 0; ++lr; }
  };
  f32x4 acc[NTW][MT];
#pragma unroll
  for (int q = 0; q < NTW; ++q)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[q][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int cr = 0, cj = 0;                                  // compute cursor
  constexpr int XB = (DEPTH % 2 == 0) ? 2 : DEPTH;
  decltype(xload(0, 0)) xr[XB][MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) xr[0][m] = xload(0, m);
  auto compute = [&](int d, const f32x4 (&wv)[NTW]) {
    const int nj = (cj + 1 == KC) ? 0 : cj + 1;        // every run walks the same K chunks
#pragma unroll
    for (int m = 0; m < MT; ++m) xr[((d + 1) % DEPTH) % XB][m] = xload(nj, m);
    __builtin_amdgcn_sched_barrier(0);                 // next chunk's ds_reads before this chunk's MFMAs (see stream_mfma)
    f32x4 x[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) x[m] = xmake(xr[d % XB][m]);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int q = 0; q < NTW; ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[q][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[q][s], x[m][s], acc[q][m], 0, 0, 0);
    if (++cj == KC) {
      epilogue(tile_of(cr), acc);
#pragma unroll
      for (int q = 0; q < NTW; ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[q][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      cj = 0; ++cr;
    }
  };
  if (T >= DEPTH) {
    if (!PRE) {
#pragma unroll
      for (int d = 0; d < DEPTH; ++d) load(wq[d]);
    }
    int it = 0;
    for (; it + 2 * DEPTH <= T; it += DEPTH) {
#pragma unroll
      for (int d = 0; d < DEPTH; ++d) {
        compute(d, wq[d]);
        load(wq[d]);
        __builtin_amdgcn_sched_barrier(0);     // see stream_mfma
      }
    }
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      compute(d, wq[d]);
      if (it + DEPTH + d < T) load(wq[d]);
      __builtin_amdgcn_sched_barrier(0);
    }
    it += DEPTH;
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (it + d < T) compute(d, wq[d]);
  } else {
    // short stream (fewer chunks than ring slots): request everything (unless the prefetch already did), then compute
    if (!PRE) {
#pragma unroll
      for (int d = 0; d < DEPTH; ++d)
        if (d < T) load(wq[d]);
    }
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
      if (d < T) compute(d, wq[d]);
  }
}

// LDS carve of mbconv_block_kernel (floats), shared by the kernel and its launcher.
//   U: phase A: block input as B-operand fragments [KCe][MT][256];  later: SE means [G][Cexp] + gate [G][Cexp]
//      (the SE-reduce partials [NWAVES][48][G] borrow the gate space)
//   E: expanded activations [MT*16][Cexp + 4]
//   Z: phase A: expand BN scale/shift [2][Cexp];  later: r [16][52] + SE expand bias [Cexp]
struct BlockLds { int U, E, Z; };
__host__ __device__ inline BlockLds block_lds(int KCe, int Cexp, int MT, int G, int nwaves) {
  BlockLds l;
  const int xf = KCe * MT * 256;
  const int gp = (G * Cexp > nwaves * 48 * G) ? G * Cexp : nwaves * 48 * G;
  const int sg = G * Cexp + gp;
  l.U = xf > sg ? xf : sg;
  l.E = MT * 16 * (Cexp + 4);
  const int z2 = 16 * 52 + Cexp;
  l.Z = (2 * Cexp > z2) ? 2 * Cexp : z2;
  return l;
}

// MT = 16-row activation tiles per workgroup: 1 for 2x2 images (4 clips), 3 for 4x3 images (4 clips = 48 rows;
// every streamed weight fragment then feeds 3 MFMAs per n-tile instead of 1); 2 for 4x3 images in handles of at most 512
// clips (2 clips = 24 of 32 rows: twice the workgroups, so that every CU still gets one).
#ifndef MKWS_DW_CLIP_MINOR
#define MKWS_DW_CLIP_MINOR 1
#endif
template <int KS, int S, int HT, int WT, int MT, int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void mbconv_block_kernel(BlockArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_blk[];
  constexpr int NTHR = NWAVES * 64;
  constexpr int HW = HT * WT;
  constexpr int G = MT * 16 / HW;                              // clips per workgroup
  static_assert(G >= 1 && G * HW <= MT * 16, "G whole clips per workgroup; rows past G*HW of the last tile are padding (zeroed / never stored)");
  constexpr int HoT = (S == 1) ? HT : (HT == 4 ? 2 : 1), WoT = (S == 1) ? WT : (WT == 3 ? 2 : 1);
  constexpr int HoWo = HoT * WoT;
  constexpr int MTO = (G * HoWo + 15) / 16;                    // output row tiles (stride 2 shrinks them)
  constexpr int PT = (S == 1) ? KS / 2 : KS / 2 - (1 - HT % 2), PLF = (S == 1) ? KS / 2 : KS / 2 - (1 - WT % 2);
  const int Cexp = a.Cexp, LDE = Cexp + 4;
  const int KCx = Cexp / 16;                                   // K chunks of the SE-reduce and project GEMMs
  constexpr int LDR = 52;                                      // r rows: up to 48 SE units + pad
  const BlockLds L = block_lds(a.KCe, Cexp, MT, G, NWAVES);
  float* s_X = s_blk;                                          // U, phase A
  float* s_S = s_blk;                                          // U, phase B onwards: [G][Cexp] SE means
  float* s_G = s_S + G * Cexp;                                 //                     [G][Cexp] SE gate (phase C2 onwards)
  float* s_P = s_G;                                            //                     [NWAVES][48][G] SE-reduce partials (C1 only)
  float* s_E = s_blk + L.U;                                    // [MT*16][LDE]
  float* s_scE = s_E + L.E;                                    // Z, phase A: [Cexp] expand BN scale, shift
  float* s_shE = s_scE + Cexp;
  float* s_R = s_scE;                                          // Z, phase B onwards: [16][LDR], then SE expand bias [Cexp]
  float* s_be = s_R + 16 * LDR;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform: tile / chunk offsets of the weight streams stay on the scalar unit (WBuf)
  const int g = lane >> 4, c = lane & 15;
  const unsigned loff = (unsigned)(g * 64 + c * 4);                 // this lane's float4 inside a packed weight fragment
  const int b0 = blockIdx.x * G;
  const int gvalid = (a.B - b0 < G) ? (a.B - b0) : G;
  const int rows_in = gvalid * HW, rows_out = gvalid * HoWo;
  const size_t row0_in = (size_t)b0 * HW, row0_out = (size_t)b0 * HoWo;

#ifdef MKWS_FRONT_TIMING
  const long long dbg_c0 = clock64();
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 0] = wall_clock64();
#endif
  // phase A's weight stream does not depend on the input tile: its first fragments are requested before the staging, so that their L2
  // round trip runs under the tile's HBM round trip instead of after it
  constexpr int NTWA = (MT >= 3) ? 1 : 2;       // one weight fragment already feeds 4*MT MFMAs; finer runs balance the waves
  const int a_groups = (a.NTe + NTWA - 1) / NTWA;
  const int a_runs = (a_groups > wave) ? (a_groups - wave + NWAVES - 1) / NWAVES : 0;
  auto a_tile_of = [&](int r) { return (wave + NWAVES * r) * NTWA; };
  f32x4 wqa[4][NTWA];
  stream_mfma_runs_prefetch<NTWA, 4>(wqa, WBuf(a.WpE, loff), (size_t)a.NTe * 256, a.NTe, a_runs, a.KCe, a_tile_of);
  // ---- stage the input tiles as fragments: s_X[j][m][lane] = X[row = 16m + c][16j + 4g .. +3]; epilogue constants ----
  for (int jm = wave; jm < a.KCe * MT; jm += NWAVES) {
    const int j = jm / MT, m = jm - j * MT;
    const int r = m * 16 + c;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < rows_in && 16 * j + 4 * g < a.Cin) v = *reinterpret_cast<const f32x4*>(a.X + (row0_in + r) * a.Cin + 16 * j + 4 * g);
    *reinterpret_cast<f32x4*>(s_X + ((size_t)jm * 64 + lane) * 4) = v;
  }
  for (int i = tid; i < Cexp; i += NTHR) { s_scE[i] = a.scE[i]; s_shE[i] = a.shE[i]; }
  __syncthreads();

#ifdef MKWS_FRONT_TIMING
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 1] = wall_clock64();
#endif
  // ---- phase A: expand ----
  {
    constexpr int NTW = NTWA;
    const int nruns = a_runs;
    auto tile_of = a_tile_of;
    auto xload = [&](int j, int m) { return *reinterpret_cast<const f32x4*>(s_X + ((size_t)(j * MT + m) * 64 + lane) * 4); };
    auto xmake = [](const f32x4& v) { return v; };
    auto epi = [&](int t0, const f32x4 (&acc)[NTW][MT]) {
#pragma unroll
      for (int q = 0; q < NTW; ++q) {
        const int n = (t0 + q) * 16 + 4 * g;
        if (t0 + q < a.NTe) {
          const f32x4 sc = *reinterpret_cast<const f32x4*>(s_scE + n), sh = *reinterpret_cast<const f32x4*>(s_shE + n);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            f32x4 y = acc[q][m] * sc + sh;
            y = swish4_(y);
            if (m * 16 + c >= rows_in) y = (f32x4){0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(s_E + (size_t)(m * 16 + c) * LDE + n) = y;
          }
        }
      }
    };
    stream_mfma_runs<NTW, 4, MT, true>(wqa, WBuf(a.WpE, loff), (size_t)a.NTe * 256, a.NTe, nruns, a.KCe, tile_of, xload, xmake, epi);
  }
  __syncthreads();

#ifdef MKWS_FRONT_TIMING
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 2] = wall_clock64();
#endif
  // ---- phase B: depthwise (+BN+swish) + SE means.  Outputs overwrite the clip's own rows: row gi*HW + o
  //      (in place for stride 1; for stride 2 phase D maps output row r -> (r / HoWo)*HW + r % HoWo) ----
  for (int i = tid; i < Cexp; i += NTHR) s_be[i] = a.be[i];
  // the weight streams of the next phases are requested one phase early (their first fragments arrive while
  // this phase computes): C1's K slice of the SE-reduce weights here
  const int c1_per = (KCx + NWAVES - 1) / NWAVES;
  const int c1_j0 = wave * c1_per;
  const int c1_kc = (c1_j0 + c1_per <= KCx) ? c1_per : (KCx > c1_j0 ? KCx - c1_j0 : 0);
  const WBuf c1_w(a.WrP + (size_t)c1_j0 * a.NTR * 256, loff);
  f32x4 wq1[3][3];
  // 4x3 images: squeeze-excite on the 4x4x1 instruction when the block carries that packing (Se4 above; same calls as chain_block: bit-identical)
  constexpr bool kSe4 = (HW == 12);
  const bool se4 = kSe4 && a.WrQ != nullptr;
  constexpr bool kWq4Early = (KS == 3);                        // (5x5: behind the depthwise loop, whose 12 + 12 + 25 float4 leave no room for 11 more)
  f32x4 wq4[kSe4 ? kSe4MaxTQ : 1];
  if (se4) {
    if constexpr (kSe4 && kWq4Early) se4_request_c1(wq4, a.WrQ, wave, lane);
  } else {
    stream_mfma_prefetch<3, 3>(wq1, c1_w, (size_t)a.NTR * 256, 0, 1, a.NTR, c1_kc);
  }
  {
    const int Q = Cexp / 4;
    for (int task = tid; task < G * Q; task += NTHR) {
      // clip-minor task order: the G lanes that hold the G clips of one channel quad sit next to each other and ask for the SAME depthwise taps /
      // BN constants -- the texture unit fetches a line once per instruction, so the workgroup pulls the block's taps from L2 once instead of once
      // per clip (5b: 269 -> 67 KB per workgroup; chain 217.6 -> 216.7 us, the PAIRED kernels lose 2 us with it and keep clip-major; r06_notes.md section 12).  LDS: a 16-lane pass covers G clips x
      // 16 / G quads, and the clips' row offsets (12 LDE resp. 4 LDE floats) are multiples of 16 banks apart.  Same arithmetic per task: bit-identical.
      const int gi = MKWS_DW_CLIP_MINOR ? task % G : task / Q, q4 = (MKWS_DW_CLIP_MINOR ? task / G : task - gi * Q) * 4;
      float* Eg = s_E + (size_t)gi * HW * LDE + q4;
      f32x4 ein[HW];
#pragma unroll
      for (int pix = 0; pix < HW; ++pix) ein[pix] = *reinterpret_cast<const f32x4*>(Eg + (size_t)pix * LDE);
      f32x4 acc[HoWo];
#pragma unroll
      for (int o = 0; o < HoWo; ++o) acc[o] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < KS; ++i) {
#pragma unroll
        for (int jx = 0; jx < KS; ++jx) {
          bool used = false;
#pragma unroll
          for (int oh = 0; oh < HoT; ++oh)
#pragma unroll
            for (int ow = 0; ow < WoT; ++ow) {
              const int ih = oh * S - PT + i, iw = ow * S - PLF + jx;
              used |= (ih >= 0 && ih < HT && iw >= 0 && iw < WT);
            }
          if (!used) continue;
          const f32x4 wv = *reinterpret_cast<const f32x4*>(a.Wd + (size_t)(i * KS + jx) * Cexp + q4);
#pragma unroll
          for (int oh = 0; oh < HoT; ++oh)
#pragma unroll
            for (int ow = 0; ow < WoT; ++ow) {
              const int ih = oh * S - PT + i, iw = ow * S - PLF + jx;
              if (ih >= 0 && ih < HT && iw >= 0 && iw < WT) acc[oh * WoT + ow] += ein[ih * WT + iw] * wv;
            }
        }
      }
      const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scD + q4);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(a.shD + q4);
      f32x4 ssum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < HoWo; ++o) {
        f32x4 y = acc[o] * sc + sh;
        y = swish4_(y);
        if (gi >= gvalid) y = (f32x4){0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(Eg + (size_t)o * LDE) = y;
        ssum += y;
        if (a.dbg_dw && gi < gvalid) *reinterpret_cast<f32x4*>(a.dbg_dw + (row0_out + gi * HoWo + o) * Cexp + q4) = y;
      }
      *reinterpret_cast<f32x4*>(s_S + (size_t)gi * Cexp + q4) = ssum * (1.0f / (float)HoWo);
    }
  }
  if constexpr (kSe4 && !kWq4Early) {
    if (se4) se4_request_c1(wq4, a.WrQ, wave, lane);
  }
  __syncthreads();

#ifdef MKWS_FRONT_TIMING
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 3] = wall_clock64();
#endif
  // ---- phase C1: r^T[se, clips] = Wr^T . mean^T, K = Cexp split over the waves ----
  constexpr int NTW2 = 3;                                      // C2: gate tiles per run
  const int c2_groups = (KCx + NTW2 - 1) / NTW2;
  const int c2_runs = (c2_groups > wave) ? (c2_groups - wave + NWAVES - 1) / NWAVES : 0;
  auto c2_tile_of = [&](int r) { return (wave + NWAVES * r) * NTW2; };
  f32x4 wq2[3][NTW2];
  f32x4 wg4[kSe4 ? kSe4MaxGroups : 1][kSe4 ? kSe4MaxNQ : 1];
  if (se4) {
    if constexpr (kSe4) {
      se4_c1<G, NWAVES>(wq4, a.seT0, Cexp, s_S, s_P, wave, lane);
      se4_request_c2<NWAVES>(wg4, a.We2Q, Cexp, wave, lane);
      const float br4 = (tid < 32 * G && (tid & 31) < a.se) ? a.br[tid & 31] : 0.0f;
      __syncthreads();
      se4_fold<G, NWAVES, LDR>(s_P, s_R, a.se, br4, tid);
      __syncthreads();
    }
  } else {
    {
      f32x4 acc[3][1];
  #pragma unroll
      for (int q = 0; q < 3; ++q) acc[q][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* srow = s_S + (size_t)(c < G ? c : 0) * Cexp + 16 * c1_j0 + 4 * g;      // columns c >= G are don't-care
      auto xload = [&](int j, int) { return *reinterpret_cast<const f32x4*>(srow + 16 * j); };
      auto xmake = [](const f32x4& v) { return v; };
      if (c1_kc > 0) stream_mfma<3, 3, 1, true>(acc, wq1, c1_w, (size_t)a.NTR * 256, 0, 1, a.NTR, c1_kc, xload, xmake);
      stream_mfma_runs_prefetch<NTW2, 3>(wq2, WBuf(a.We2P, loff), (size_t)KCx * 256, KCx, c2_runs, a.NTR, c2_tile_of);   // C2's stream
      if (c < G) {
  #pragma unroll
        for (int q = 0; q < 3; ++q)
  #pragma unroll
          for (int r = 0; r < 4; ++r) s_P[((wave * 3 + q) * 16 + 4 * g + r) * G + c] = acc[q][0][r];
      }
    }
    const float br_pre = (tid < 48 * G && tid / G < a.se) ? a.br[tid / G] : 0.0f;     // requested before the barrier (48*G <= NTHR)
    __syncthreads();
    for (int t = tid; t < 48 * G; t += NTHR) {
      const int n = t / G, clip = t - n * G;
      float v = 0.0f;
      if (n < a.se) {
  #pragma unroll
        for (int w = 0; w < NWAVES; ++w) v += s_P[(w * 48 + n) * G + clip];
        v = swishf_(v + br_pre);
      }
      s_R[clip * LDR + n] = v;
    }
    __syncthreads();
  }
#ifdef MKWS_FRONT_TIMING
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 4] = wall_clock64();
#endif
  // ---- phase C2: gate^T[Cexp, clips] = We2^T . r^T, tiles over waves (columns c >= G are don't-care) ----
  // phase D's weight stream is requested first: this wave owns project tiles wave, wave + NWAVES, ...
  // NTp = NWAVES / 2 + 1 (blocks 4b / 4c: 5 projection tiles, 8 waves): waves 0 and 4 share SIMD 0, which would then run two whole
  // tiles while SIMDs 1..3 run one (14.2 us against a 6.4 us MFMA floor).  The last tile is therefore split by ROW tile over waves
  // NWAVES/2 .. NWAVES/2 + MTO - 1, one row tile each: every SIMD gets MTO + 1 (tile, row tile) units at most.
  const bool d_rowsplit = (a.NTp == NWAVES / 2 + 1) && (MTO > 1) && (MTO <= NWAVES / 2 - 1);
  const int d_ntw = d_rowsplit ? ((wave < NWAVES / 2) ? 1 : 0) : ((a.NTp > wave) ? (a.NTp - wave + NWAVES - 1) / NWAVES : 0);
  const int d_row = (d_rowsplit && wave >= NWAVES / 2 && wave < NWAVES / 2 + MTO) ? wave - NWAVES / 2 : -1;     // this wave's row tile of the last tile
  const WBuf d_w(a.WpP, loff);
  f32x4 wqd[4][3];
  if (d_ntw > 0 || d_row >= 0) stream_mfma_prefetch<3, 4>(wqd, d_w, (size_t)a.NTp * 256, wave, NWAVES, a.NTp, KCx);   // (tiles past NTp clamp to the last one)
  if (se4) {
    if constexpr (kSe4) {
      se4_c2_gate<G, HW, HoWo, NWAVES, LDR>(wg4, Cexp, s_R, s_be, s_E, wave, lane, a.dbg_gate ? a.dbg_gate + (size_t)b0 * Cexp : nullptr, gvalid);
      __syncthreads();
#ifdef MKWS_FRONT_TIMING
      if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 5] = wall_clock64();
#endif
    }
  } else {
    {
      const float* rrow = s_R + (c < G ? c : 0) * LDR + 4 * g;
      auto xload = [&](int j, int) { return *reinterpret_cast<const f32x4*>(rrow + 16 * j); };
      auto xmake = [](const f32x4& v) { return v; };
      auto epi = [&](int t0, const f32x4 (&acc)[NTW2][1]) {
  #pragma unroll
        for (int q = 0; q < NTW2; ++q) {
          const int n = (t0 + q) * 16 + 4 * g;
          if (t0 + q < KCx && c < G) {
            f32x4 y = acc[q][0] + *reinterpret_cast<const f32x4*>(s_be + n);
            y = sigmoid4_(y);
            *reinterpret_cast<f32x4*>(s_G + (size_t)c * Cexp + n) = y;
            if (a.dbg_gate && c < gvalid) *reinterpret_cast<f32x4*>(a.dbg_gate + (size_t)(b0 + c) * Cexp + n) = y;
          }
        }
      };
      stream_mfma_runs<NTW2, 3, 1, true>(wq2, WBuf(a.We2P, loff), (size_t)KCx * 256, KCx, c2_runs, a.NTR, c2_tile_of, xload, xmake, epi);
    }
    __syncthreads();

  #ifdef MKWS_FRONT_TIMING
    if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 5] = wall_clock64();
  #endif
    // ---- gate the depthwise output in place, once: phase D then reads ONE operand fragment per row tile and chunk
    //      (the gate as a second LDS operand plus a multiply per fragment cost the projection's MFMA issue) ----
    {
      const int Q = Cexp / 4;
      for (int i = tid; i < G * HoWo * Q; i += NTHR) {
        const int ro = i / Q, q4 = (i - ro * Q) * 4;
        const int clip = ro / HoWo;
        float* e = s_E + (size_t)(clip * HW + (ro - clip * HoWo)) * LDE + q4;
        *reinterpret_cast<f32x4*>(e) = *reinterpret_cast<const f32x4*>(e) * *reinterpret_cast<const f32x4*>(s_G + (size_t)clip * Cexp + q4);
      }
    }
    __syncthreads();
  }
  // ---- phase D: gated project (+ residual): output row r = 16m + c lives in E row (r / HoWo)*HW + r % HoWo ----
  {
    const size_t cstride = (size_t)a.NTp * 256;
    const float* erow[MTO];
#pragma unroll
    for (int m = 0; m < MTO; ++m) {
      int r = m * 16 + c;
      if (r >= G * HoWo) r = G * HoWo - 1;                   // padding rows of the last tile: any finite row
      const int clip = r / HoWo;
      erow[m] = s_E + (size_t)(clip * HW + (r - clip * HoWo)) * LDE + 4 * g;
    }
    auto xload = [&](int j, int m) { return *reinterpret_cast<const f32x4*>(erow[m] + 16 * j); };
    auto xmake = [](const f32x4& v) { return v; };
    auto run = [&](auto ntw_tag) {
      constexpr int NTW = decltype(ntw_tag)::value;
      f32x4 acc[NTW][MTO];
#pragma unroll
      for (int q = 0; q < NTW; ++q)
#pragma unroll
        for (int m = 0; m < MTO; ++m) acc[q][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      stream_mfma<NTW, 4, MTO, true>(acc, wqd, d_w, cstride, wave, NWAVES, a.NTp, KCx, xload, xmake);
#pragma unroll
      for (int q = 0; q < NTW; ++q) {
        const int t = wave + NWAVES * q;
        const int n = t * 16 + 4 * g;
        if (t < a.NTp) {
          const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scP + n), sh = *reinterpret_cast<const f32x4*>(a.shP + n);
#pragma unroll
          for (int m = 0; m < MTO; ++m) {
            const int r = m * 16 + c;
            if (r < rows_out) {
              f32x4 y = acc[q][m] * sc + sh;
              if (a.residual) y += *reinterpret_cast<const f32x4*>(a.X + (row0_in + r) * a.Cin + n);
              *reinterpret_cast<f32x4*>(a.Y + (row0_out + r) * a.Cout + n) = y;
            }
          }
        }
      }
    };
    // Cout/16 <= 20 tiles over NWAVES waves: each wave runs exactly the 0..3 tiles it owns
    if (d_row >= 0) {
      // one row tile of the last projection tile (see d_rowsplit above)
      const float* er = erow[0];
#pragma unroll
      for (int m = 1; m < MTO; ++m) er = (d_row == m) ? erow[m] : er;
      auto xload1 = [&](int j, int) { return *reinterpret_cast<const f32x4*>(er + 16 * j); };
      f32x4 acc1[1][1] = {{{0.f, 0.f, 0.f, 0.f}}};
      stream_mfma<1, 4, 1, true>(acc1, wqd, d_w, cstride, a.NTp - 1, NWAVES, a.NTp, KCx, xload1, xmake);
      const int n = (a.NTp - 1) * 16 + 4 * g, r = d_row * 16 + c;
      if (r < rows_out) {
        f32x4 y = acc1[0][0] * *reinterpret_cast<const f32x4*>(a.scP + n) + *reinterpret_cast<const f32x4*>(a.shP + n);
        if (a.residual) y += *reinterpret_cast<const f32x4*>(a.X + (row0_in + r) * a.Cin + n);
        *reinterpret_cast<f32x4*>(a.Y + (row0_out + r) * a.Cout + n) = y;
      }
    } else if (d_ntw == 1) run(std::integral_constant<int, 1>{});
    else if (d_ntw == 2) run(std::integral_constant<int, 2>{});
    else if (d_ntw >= 3) run(std::integral_constant<int, 3>{});
  }
#ifdef MKWS_FRONT_TIMING
  __syncthreads();
  if (threadIdx.x == 0) { a.dbg_t[(size_t)blockIdx.x * 8 + 6] = wall_clock64(); a.dbg_t[(size_t)blockIdx.x * 8 + 7] = (unsigned long long)(clock64() - dbg_c0); }
#endif
}

// ------------------------------------------------------------------------------------------------
// Depth-fused chain of whole-block kernels for the 4x3-image blocks (4b -> 4c -> 5a -> 5b -> 5c -> 6a): ONE launch.
// In mbconv_block_kernel a workgroup owns the same G clips in every one of these blocks and nothing crosses workgroups, so
// the launch boundaries between them were pure overhead: 2-3 us of start / end skew each, the input tile's HBM round trip
// and staging pass (~2 us), and a phase A that starts on an empty weight ring.  Here the workgroup walks the blocks itself:
//   * block k's projection epilogue writes its output tile straight into the U region as block k + 1's MFMA B-operand
//     fragments (the lane that holds output channels 16t + 4g .. +3 of row 16m + c IS lane (g, c) of fragment (j = t, m):
//     a lane-linear ds_write_b128, no transpose) -- the activations of the chain never leave the CU;
//   * the same lane finishes the same (tile, row tile) in the next block (Cin == Cout whenever a block has a residual), so
//     the residual rides in registers (carry) instead of being re-read;
//   * block k + 1's expand BN constants are requested while block k's SE phases run (its weight ring is requested at the top of the
//     block: see chain_block).
// Only the chain's input and its last block's output touch HBM (the launcher stops the chain at a tapped block, so the
// parity taps see the chain's own arithmetic).  Same operations in the same order as mbconv_block_kernel: bit-identical.
constexpr int kChainMax = 6;
// The per-block constants (weight pointers, sizes) live in a device table built once per handle (a by-value array indexed with the
// loop counter would be copied to scratch); the uniform loads below are scalar loads.
struct ChainArgs {
  const BlockArgs* tab;       // [kNumBlocks] in device memory: X / Y / dbg pointers null, B unused
  int i0, n;                  // blocks i0 .. i0 + n - 1 of the plan
  unsigned kinds;             // 2 bits per chain position: 0 = 3x3 stride 1, 1 = 5x5 stride 1, 2 = 5x5 stride 2 (last block only: the image shrinks to 2x2)
  const float* X; float* Y;   // the chain's input and its last block's output
  int B;
  int ldsU, ldsE;             // LDS carve in floats, the maximum over the chain's blocks (Z follows E)
  int se4;                    // 0: squeeze-excite on the 16x16x4 streams even where the table holds 4x4x1 weights (option "fuse_se4" = 0)
#ifdef MKWS_FRONT_TIMING
  unsigned long long* dbg_t;  // [workgroups][kChainMax][8] wall_clock64 stamps
#endif
};

// Values loaded from the block table arrive in VGPRs (a global load is a vector load unless the compiler can prove the memory is never
// written); used as a buffer descriptor or a scalar offset they would make hipcc wrap EVERY buffer_load of the weight rings in a
// waterfall loop (4 v_readfirstlane + compares + a branch per load).  The table entries are uniform by construction: pin them to SGPRs.
__device__ __forceinline__ int sgpr_(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <typename T>
__device__ __forceinline__ T* sgpr_(T* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  // rebuilt as a GLOBAL pointer: an integer cast to a generic pointer would turn every load through it into a flat_load, which hipcc
  // fences with s_waitcnt vmcnt(0) lgkmcnt(0) (it may alias LDS) -- the depthwise tap loads then ran one latency at a time
  typedef __attribute__((address_space(1))) T* gptr_t;
  return (T*)reinterpret_cast<gptr_t>(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ BlockArgs sgpr_block_args(const BlockArgs& t) {
  BlockArgs a;
  a.X = nullptr; a.Cin = sgpr_(t.Cin);
  a.WpE = sgpr_(t.WpE); a.scE = sgpr_(t.scE); a.shE = sgpr_(t.shE); a.KCe = sgpr_(t.KCe); a.NTe = sgpr_(t.NTe);
  a.Wd = sgpr_(t.Wd); a.scD = sgpr_(t.scD); a.shD = sgpr_(t.shD);
  a.WrP = sgpr_(t.WrP); a.br = sgpr_(t.br); a.NTR = sgpr_(t.NTR); a.We2P = sgpr_(t.We2P); a.be = sgpr_(t.be);
  a.WpP = sgpr_(t.WpP); a.scP = sgpr_(t.scP); a.shP = sgpr_(t.shP); a.NTp = sgpr_(t.NTp);
  a.Y = nullptr; a.Cout = sgpr_(t.Cout); a.residual = sgpr_(t.residual);
  a.dbg_dw = nullptr; a.dbg_gate = nullptr;
  a.B = 0; a.Cexp = sgpr_(t.Cexp); a.se = sgpr_(t.se);
  a.WrQ = sgpr_(t.WrQ); a.We2Q = sgpr_(t.We2Q); a.seT0 = sgpr_(t.seT0); a.seNQ = sgpr_(t.seNQ);
#ifdef MKWS_FRONT_TIMING
  a.dbg_t = nullptr;
#endif
  return a;
}

template <int KS, int S, int MT, int NWAVES>
__device__ __forceinline__ void chain_block(const BlockArgs& a, const BlockArgs* nxp, bool has_next, float* s_blk, int ldsU, int ldsE, bool first,
                                            f32x4 (&carry)[MT], unsigned long long* dbg_t) {
  constexpr int NTHR = NWAVES * 64;
  const BlockArgs* nx = has_next ? nxp : nullptr;      // nxp is always a valid table entry (the block itself when there is no next one)
  constexpr int HT = 4, WT = 3, HW = HT * WT;
  constexpr int G = MT * 16 / HW;
  constexpr int HoT = (S == 1) ? HT : 2, WoT = (S == 1) ? WT : 2;
  constexpr int HoWo = HoT * WoT;
  constexpr int MTO = (G * HoWo + 15) / 16;
  constexpr int PT = (S == 1) ? KS / 2 : KS / 2 - (1 - HT % 2), PLF = (S == 1) ? KS / 2 : KS / 2 - (1 - WT % 2);
  constexpr int LDR = 52;
  constexpr int NTWA = (MT >= 3) ? 1 : 2;
  const int Cexp = a.Cexp, LDE = Cexp + 4;
  const int KCx = Cexp / 16;
  float* s_X = s_blk;
  float* s_S = s_blk;
  float* s_G = s_S + G * Cexp;
  float* s_P = s_G;
  float* s_E = s_blk + ldsU;
  float* s_scE = s_E + ldsE;
  float* s_shE = s_scE + Cexp;
  float* s_R = s_scE;
  float* s_be = s_R + 16 * LDR;
  // opaque: per-thread index arithmetic must be recomputed in every block (hoisted out of the block loop it is spilled, and a scratch
  // reload inside a ring epilogue drains the in-order weight ring)
  const int tid = opaque_((int)threadIdx.x), lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const unsigned loff = (unsigned)(g * 64 + c * 4);
  const int b0 = blockIdx.x * G;
  const int gvalid = (a.B - b0 < G) ? (a.B - b0) : G;
  const int rows_in = gvalid * HW, rows_out = gvalid * HoWo;
  const size_t row0_in = (size_t)b0 * HW, row0_out = (size_t)b0 * HoWo;

#ifdef MKWS_FRONT_TIMING
  if (dbg_t && threadIdx.x == 0) dbg_t[0] = wall_clock64();
#endif
  // ---- phase A: expand.  The input fragments are in s_X and the first ring slots in flight (kernel prologue / previous block) ----
  const int a_groups = (a.NTe + NTWA - 1) / NTWA;
  const int a_runs = (a_groups > wave) ? (a_groups - wave + NWAVES - 1) / NWAVES : 0;
  auto a_tile_of = [&](int r) { return (wave + NWAVES * r) * NTWA; };
  {
    // The expand ring is requested HERE.  Requesting it during the previous block's projection (so that phase A never starts on an
    // empty ring) was measured and lost: carried across the block loop the ring's 16-32 registers cost the kernel ~30-50 (227 / 247
    // instead of 199 / 195 VGPRs) and 3 us per launch (profiles/r04_notes.md); its L2 round trip now runs once per block.
    f32x4 wqa[4][NTWA];
    stream_mfma_runs_prefetch<NTWA, 4>(wqa, WBuf(a.WpE, loff), (size_t)a.NTe * 256, a.NTe, a_runs, a.KCe, a_tile_of);
    auto xload = [&](int j, int m) { return *reinterpret_cast<const f32x4*>(s_X + ((size_t)(j * MT + m) * 64 + lane) * 4); };
    auto xmake = [](const f32x4& v) { return v; };
    auto epi = [&](int t0, const f32x4 (&acc)[NTWA][MT]) {
#pragma unroll
      for (int q = 0; q < NTWA; ++q) {
        const int n = (t0 + q) * 16 + 4 * g;
        if (t0 + q < a.NTe) {
          const f32x4 sc = *reinterpret_cast<const f32x4*>(s_scE + n), sh = *reinterpret_cast<const f32x4*>(s_shE + n);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            f32x4 y = acc[q][m] * sc + sh;
            y = swish4_(y);
            if (m * 16 + c >= rows_in) y = (f32x4){0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(s_E + (size_t)(m * 16 + c) * LDE + n) = y;
          }
        }
      }
    };
    stream_mfma_runs<NTWA, 4, MT, true>(wqa, WBuf(a.WpE, loff), (size_t)a.NTe * 256, a.NTe, a_runs, a.KCe, a_tile_of, xload, xmake, epi);
  }
  __syncthreads();

#ifdef MKWS_FRONT_TIMING
  if (dbg_t && threadIdx.x == 0) dbg_t[1] = wall_clock64();
#endif
  // ---- phase B: depthwise (+BN+swish) in place + SE means (see mbconv_block_kernel) ----
  for (int i = tid; i < Cexp; i += NTHR) s_be[i] = a.be[i];
  const int c1_per = (KCx + NWAVES - 1) / NWAVES;
  const int c1_j0 = wave * c1_per;
  const int c1_kc = (c1_j0 + c1_per <= KCx) ? c1_per : (KCx > c1_j0 ? KCx - c1_j0 : 0);
  const WBuf c1_w(a.WrP + (size_t)c1_j0 * a.NTR * 256, loff);
  f32x4 wq1[3][3];
  // (5x5: a thread holds 12 inputs + 12 outputs + 25 taps -- 196 registers; C1's ring is requested behind the depthwise loop there,
  // where waves that own one round of tasks wait for those that own two)
  constexpr bool kWq1Early = (KS == 3);                        // (requested in front of the 5x5 depthwise as well: measured, no difference)
  const bool se4 = a.WrQ != nullptr;                           // squeeze-excite on the 4x4x1 instruction (Se4 above); uniform
  f32x4 wq4[kSe4MaxTQ];
  if (kWq1Early) {
    if (se4) se4_request_c1(wq4, a.WrQ, wave, lane);
    else stream_mfma_prefetch<3, 3>(wq1, c1_w, (size_t)a.NTR * 256, 0, 1, a.NTR, c1_kc);
  }
  {
    const int Q = Cexp / 4;
    for (int task = tid; task < G * Q; task += NTHR) {
      // clip-minor task order: the G lanes that hold the G clips of one channel quad sit next to each other and ask for the SAME depthwise taps /
      // BN constants -- the texture unit fetches a line once per instruction, so the workgroup pulls the block's taps from L2 once instead of once
      // per clip (5b: 269 -> 67 KB per workgroup; chain 217.6 -> 216.7 us, the PAIRED kernels lose 2 us with it and keep clip-major; r06_notes.md section 12).  LDS: a 16-lane pass covers G clips x
      // 16 / G quads, and the clips' row offsets (12 LDE resp. 4 LDE floats) are multiples of 16 banks apart.  Same arithmetic per task: bit-identical.
      const int gi = MKWS_DW_CLIP_MINOR ? task % G : task / Q, q4 = (MKWS_DW_CLIP_MINOR ? task / G : task - gi * Q) * 4;
      float* Eg = s_E + (size_t)gi * HW * LDE + q4;
      // The taps are requested in SOURCE order ahead of their use (hipcc leaves this region in source order: with "load a tap, use it"
      // the phase ran one L2 latency per tap; mbconv_block_kernel's scheduler hoists all 25 loads by itself, but here 12 inputs + 12
      // outputs + 25 taps do not fit next to what the block loop keeps alive).  Kernel rows [0, PRE) first; row i + PRE goes into the
      // registers of row i once row i has been used, so at most PRE rows of taps are live.
      constexpr int PRE = (KS == 5) ? (MT >= 3 ? 3 : 2) : KS;      // (2-clip workgroups carry a wider expand ring: one row less in flight)
      auto tap_used = [](int i, int jx) {
        bool used = false;
        for (int oh = 0; oh < HoT; ++oh)
          for (int ow = 0; ow < WoT; ++ow) {
            const int ih = oh * S - PT + i, iw = ow * S - PLF + jx;
            used |= (ih >= 0 && ih < HT && iw >= 0 && iw < WT);
          }
        return used;
      };
      f32x4 wv[KS][KS];
      auto load_row = [&](int i) {
#pragma unroll
        for (int jx = 0; jx < KS; ++jx)
          if (tap_used(i, jx)) wv[i][jx] = *reinterpret_cast<const f32x4*>(a.Wd + (size_t)(i * KS + jx) * Cexp + q4);
      };
#pragma unroll
      for (int i = 0; i < PRE; ++i) load_row(i);
      const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scD + q4);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(a.shD + q4);
      f32x4 ein[HW];
#pragma unroll
      for (int pix = 0; pix < HW; ++pix) ein[pix] = *reinterpret_cast<const f32x4*>(Eg + (size_t)pix * LDE);
      __builtin_amdgcn_sched_barrier(0);
      f32x4 acc[HoWo];
#pragma unroll
      for (int o = 0; o < HoWo; ++o) acc[o] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < KS; ++i) {
#pragma unroll
        for (int jx = 0; jx < KS; ++jx) {
#pragma unroll
          for (int oh = 0; oh < HoT; ++oh)
#pragma unroll
            for (int ow = 0; ow < WoT; ++ow) {
              const int ih = oh * S - PT + i, iw = ow * S - PLF + jx;
              if (ih >= 0 && ih < HT && iw >= 0 && iw < WT) acc[oh * WoT + ow] += ein[ih * WT + iw] * wv[i][jx];
            }
        }
        if (i + PRE < KS) {
          __builtin_amdgcn_sched_barrier(0);
          load_row(i + PRE);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      f32x4 ssum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < HoWo; ++o) {
        f32x4 y = acc[o] * sc + sh;
        y = swish4_(y);
        if (gi >= gvalid) y = (f32x4){0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(Eg + (size_t)o * LDE) = y;
        ssum += y;
      }
      *reinterpret_cast<f32x4*>(s_S + (size_t)gi * Cexp + q4) = ssum * (1.0f / (float)HoWo);
    }
  }
  if (!kWq1Early) {
    if (se4) se4_request_c1(wq4, a.WrQ, wave, lane);
    else stream_mfma_prefetch<3, 3>(wq1, c1_w, (size_t)a.NTR * 256, 0, 1, a.NTR, c1_kc);
  }
  __syncthreads();

#ifdef MKWS_FRONT_TIMING
  if (dbg_t && threadIdx.x == 0) dbg_t[2] = wall_clock64();
#endif
  // ---- phase C1: r^T[se, clips] = Wr^T . mean^T, K = Cexp split over the waves ----
  // the NEXT block's expand BN constants are requested here (they go to Z under the gate pass, two phases later: nothing waits for them)
  constexpr int NCST = 3;                                       // Cexp <= NCST * NTHR (host-checked)
  float nsc[NCST], nsh[NCST];
  const int nxCexp = nx ? sgpr_(nx->Cexp) : 0;
  if (nx) {
    const float* nscE = sgpr_(nx->scE); const float* nshE = sgpr_(nx->shE);
#pragma unroll
    for (int k = 0; k < NCST; ++k) {
      const int i = tid + k * NTHR;
      if (i < nxCexp) { nsc[k] = nscE[i]; nsh[k] = nshE[i]; }
    }
  }
  constexpr int NTW2 = 3;
  const int c2_groups = (KCx + NTW2 - 1) / NTW2;
  const int c2_runs = (c2_groups > wave) ? (c2_groups - wave + NWAVES - 1) / NWAVES : 0;
  auto c2_tile_of = [&](int r) { return (wave + NWAVES * r) * NTW2; };
  f32x4 wq2[3][NTW2];
  f32x4 wg4[kSe4MaxGroups][kSe4MaxNQ];
  if (se4) {
    se4_c1<G, NWAVES>(wq4, a.seT0, Cexp, s_S, s_P, wave, lane);
    se4_request_c2<NWAVES>(wg4, a.We2Q, Cexp, wave, lane);                     // C2's weights: in flight across the fold
    const float br4 = (tid < 32 * G && (tid & 31) < a.se) ? a.br[tid & 31] : 0.0f;
    __syncthreads();
    se4_fold<G, NWAVES, LDR>(s_P, s_R, a.se, br4, tid);
    __syncthreads();
  } else {
    {
      f32x4 acc[3][1];
  #pragma unroll
      for (int q = 0; q < 3; ++q) acc[q][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* srow = s_S + (size_t)(c < G ? c : 0) * Cexp + 16 * c1_j0 + 4 * g;
      auto xload = [&](int j, int) { return *reinterpret_cast<const f32x4*>(srow + 16 * j); };
      auto xmake = [](const f32x4& v) { return v; };
      if (c1_kc > 0) stream_mfma<3, 3, 1, true>(acc, wq1, c1_w, (size_t)a.NTR * 256, 0, 1, a.NTR, c1_kc, xload, xmake);
      stream_mfma_runs_prefetch<NTW2, 3>(wq2, WBuf(a.We2P, loff), (size_t)KCx * 256, KCx, c2_runs, a.NTR, c2_tile_of);
      if (c < G) {
  #pragma unroll
        for (int q = 0; q < 3; ++q)
  #pragma unroll
          for (int r = 0; r < 4; ++r) s_P[((wave * 3 + q) * 16 + 4 * g + r) * G + c] = acc[q][0][r];
      }
    }
    const float br_pre = (tid < 48 * G && tid / G < a.se) ? a.br[tid / G] : 0.0f;
    __syncthreads();
    for (int t = tid; t < 48 * G; t += NTHR) {
      const int n = t / G, clip = t - n * G;
      float v = 0.0f;
      if (n < a.se) {
  #pragma unroll
        for (int w = 0; w < NWAVES; ++w) v += s_P[(w * 48 + n) * G + clip];
        v = swishf_(v + br_pre);
      }
      s_R[clip * LDR + n] = v;
    }
    __syncthreads();

  }
#ifdef MKWS_FRONT_TIMING
  if (dbg_t && threadIdx.x == 0) dbg_t[3] = wall_clock64();
#endif
  // ---- phase C2: gate; phase D's weight stream is requested first (see mbconv_block_kernel for the row split) ----
  const bool d_rowsplit = (a.NTp == NWAVES / 2 + 1) && (MTO > 1) && (MTO <= NWAVES / 2 - 1);
  const int d_ntw = d_rowsplit ? ((wave < NWAVES / 2) ? 1 : 0) : ((a.NTp > wave) ? (a.NTp - wave + NWAVES - 1) / NWAVES : 0);
  const int d_row = (d_rowsplit && wave >= NWAVES / 2 && wave < NWAVES / 2 + MTO) ? wave - NWAVES / 2 : -1;
  const WBuf d_w(a.WpP, loff);
  f32x4 wqd[4][3];
  if (d_ntw > 0 || d_row >= 0) stream_mfma_prefetch<3, 4>(wqd, d_w, (size_t)a.NTp * 256, wave, NWAVES, a.NTp, KCx);
  if (se4) {
    // gate computed and applied by the same lanes (no gate buffer, no gate pass); Z (r, be) is read until the barrier below, so the NEXT block's
    // expand BN constants go there behind it, in front of phase D's multiply-adds (phase A of the next block reads them behind D's closing barrier)
    se4_c2_gate<G, HW, HoWo, NWAVES, LDR>(wg4, Cexp, s_R, s_be, s_E, wave, lane, nullptr, gvalid);
    __syncthreads();
#ifdef MKWS_FRONT_TIMING
  if (dbg_t && threadIdx.x == 0) dbg_t[4] = wall_clock64();
#endif
    if (nx) {
  #pragma unroll
      for (int k = 0; k < NCST; ++k) {
        const int i = tid + k * NTHR;
        if (i < nxCexp) { s_scE[i] = nsc[k]; s_scE[nxCexp + i] = nsh[k]; }
      }
    }
  } else {
    {
      const float* rrow = s_R + (c < G ? c : 0) * LDR + 4 * g;
      auto xload = [&](int j, int) { return *reinterpret_cast<const f32x4*>(rrow + 16 * j); };
      auto xmake = [](const f32x4& v) { return v; };
      auto epi = [&](int t0, const f32x4 (&acc)[NTW2][1]) {
  #pragma unroll
        for (int q = 0; q < NTW2; ++q) {
          const int n = (t0 + q) * 16 + 4 * g;
          if (t0 + q < KCx && c < G) {
            f32x4 y = acc[q][0] + *reinterpret_cast<const f32x4*>(s_be + n);
            y = sigmoid4_(y);
            *reinterpret_cast<f32x4*>(s_G + (size_t)c * Cexp + n) = y;
          }
        }
      };
      stream_mfma_runs<NTW2, 3, 1, true>(wq2, WBuf(a.We2P, loff), (size_t)KCx * 256, KCx, c2_runs, a.NTR, c2_tile_of, xload, xmake, epi);
    }
    __syncthreads();

  #ifdef MKWS_FRONT_TIMING
    if (dbg_t && threadIdx.x == 0) dbg_t[4] = wall_clock64();
  #endif
    // ---- gate the depthwise output in place; the NEXT block's expand BN constants (requested in C1) go to Z, free from here on ----
    {
      const int Q = Cexp / 4;
      for (int i = tid; i < G * HoWo * Q; i += NTHR) {
        const int ro = i / Q, q4 = (i - ro * Q) * 4;
        const int clip = ro / HoWo;
        float* e = s_E + (size_t)(clip * HW + (ro - clip * HoWo)) * LDE + q4;
        *reinterpret_cast<f32x4*>(e) = *reinterpret_cast<const f32x4*>(e) * *reinterpret_cast<const f32x4*>(s_G + (size_t)clip * Cexp + q4);
      }
    }
    if (nx) {
  #pragma unroll
      for (int k = 0; k < NCST; ++k) {
        const int i = tid + k * NTHR;
        if (i < nxCexp) { s_scE[i] = nsc[k]; s_scE[nxCexp + i] = nsh[k]; }
      }
    }
    __syncthreads();
  }

#ifdef MKWS_FRONT_TIMING
  if (dbg_t && threadIdx.x == 0) dbg_t[5] = wall_clock64();
#endif
  // ---- phase D: gated project (+ residual).  The next block's expand ring is requested first; the output tile becomes the
  //      next block's input fragments in U (free since the gate was applied) and this lane's residual (carry) ----
  {
    const size_t cstride = (size_t)a.NTp * 256;
    const float* erow[MTO];
#pragma unroll
    for (int m = 0; m < MTO; ++m) {
      int r = m * 16 + c;
      if (r >= G * HoWo) r = G * HoWo - 1;
      const int clip = r / HoWo;
      erow[m] = s_E + (size_t)(clip * HW + (r - clip * HoWo)) * LDE + 4 * g;
    }
    auto xload = [&](int j, int m) { return *reinterpret_cast<const f32x4*>(erow[m] + 16 * j); };
    auto xmake = [](const f32x4& v) { return v; };
    // one finished output fragment: tile t, row tile m (slot = its index in carry)
    auto finish = [&](f32x4 y, int t, int m, int slot, const f32x4& sc, const f32x4& sh) {
      const int n = t * 16 + 4 * g, r = m * 16 + c;
      y = y * sc + sh;
      if (a.residual) {
        if (first) { if (r < rows_out) y += *reinterpret_cast<const f32x4*>(a.X + (row0_in + r) * a.Cin + n); }
        else y += carry[slot];
      }
      if (!nx && r < rows_out) *reinterpret_cast<f32x4*>(a.Y + (row0_out + r) * a.Cout + n) = y;
      if constexpr (S == 1) {
        if (r >= rows_out) y = (f32x4){0.f, 0.f, 0.f, 0.f};
        carry[slot] = y;                                           // (unconditional, like the ring above)
        if (nx) *reinterpret_cast<f32x4*>(s_X + ((size_t)(t * MT + m) * 64 + lane) * 4) = y;
      }
    };
    auto run = [&](auto ntw_tag) {
      constexpr int NTW = decltype(ntw_tag)::value;
      f32x4 acc[NTW][MTO];
#pragma unroll
      for (int q = 0; q < NTW; ++q)
#pragma unroll
        for (int m = 0; m < MTO; ++m) acc[q][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      stream_mfma<NTW, 4, MTO, true>(acc, wqd, d_w, cstride, wave, NWAVES, a.NTp, KCx, xload, xmake);
#pragma unroll
      for (int q = 0; q < NTW; ++q) {
        const int t = wave + NWAVES * q;
        if (t < a.NTp) {
          const int n = t * 16 + 4 * g;
          const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scP + n), sh = *reinterpret_cast<const f32x4*>(a.shP + n);
#pragma unroll
          for (int m = 0; m < MTO; ++m) finish(acc[q][m], t, m, (NTW == 1) ? m : 0, sc, sh);
        }
      }
    };
    if (d_row >= 0) {
      const float* er = erow[0];
#pragma unroll
      for (int m = 1; m < MTO; ++m) er = (d_row == m) ? erow[m] : er;
      auto xload1 = [&](int j, int) { return *reinterpret_cast<const f32x4*>(er + 16 * j); };
      f32x4 acc1[1][1] = {{{0.f, 0.f, 0.f, 0.f}}};
      stream_mfma<1, 4, 1, true>(acc1, wqd, d_w, cstride, a.NTp - 1, NWAVES, a.NTp, KCx, xload1, xmake);
      const int n = (a.NTp - 1) * 16 + 4 * g;
      finish(acc1[0][0], a.NTp - 1, d_row, 0, *reinterpret_cast<const f32x4*>(a.scP + n), *reinterpret_cast<const f32x4*>(a.shP + n));
    } else if (d_ntw == 1) run(std::integral_constant<int, 1>{});
    else if (d_ntw == 2) run(std::integral_constant<int, 2>{});
    else if (d_ntw >= 3) run(std::integral_constant<int, 3>{});
  }
#ifdef MKWS_FRONT_TIMING
  __syncthreads();
  if (dbg_t && threadIdx.x == 0) dbg_t[6] = wall_clock64();
#else
  if (nx) __syncthreads();
#endif
}

template <int MT, int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void mbconv_chain_kernel(ChainArgs ca) {
  extern __shared__ __attribute__((aligned(16))) float s_blk[];
  constexpr int NTHR = NWAVES * 64;
  constexpr int HW = 12, G = MT * 16 / HW;
  const BlockArgs* __restrict__ tab = ca.tab + ca.i0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
#ifdef MKWS_FRONT_TIMING
  if (ca.dbg_t && threadIdx.x == 0) ca.dbg_t[(size_t)gridDim.x * kChainMax * 8 + blockIdx.x] = wall_clock64();
#endif
  f32x4 carry[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) carry[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    // prologue = the head of mbconv_block_kernel: first block's expand ring, then its input tile and BN constants
    const int Cin = sgpr_(tab[0].Cin), KCe = sgpr_(tab[0].KCe), Cexp = sgpr_(tab[0].Cexp);
    const int b0 = blockIdx.x * G;
    const int gvalid = (ca.B - b0 < G) ? (ca.B - b0) : G;
    const int rows_in = gvalid * HW;
    const size_t row0_in = (size_t)b0 * HW;
    float* s_X = s_blk;
    float* s_scE = s_blk + ca.ldsU + ca.ldsE;
    for (int jm = wave; jm < KCe * MT; jm += NWAVES) {
      const int j = jm / MT, m = jm - j * MT;
      const int r = m * 16 + c;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < rows_in && 16 * j + 4 * g < Cin) v = *reinterpret_cast<const f32x4*>(ca.X + (row0_in + r) * Cin + 16 * j + 4 * g);
      *reinterpret_cast<f32x4*>(s_X + ((size_t)jm * 64 + lane) * 4) = v;
    }
    const float* scE = sgpr_(tab[0].scE); const float* shE = sgpr_(tab[0].shE);
    for (int i = tid; i < Cexp; i += NTHR) { s_scE[i] = scE[i]; s_scE[Cexp + i] = shE[i]; }
    __syncthreads();
  }
  for (int i = 0; i < ca.n; ++i) {
    BlockArgs a = sgpr_block_args(tab[i]);
    const bool last = (i + 1 == ca.n);
    if (!ca.se4) a.WrQ = nullptr;
    a.X = ca.X; a.Y = ca.Y; a.B = ca.B;                       // X is read by the first block only (residual), Y written by the last                // ("_dw" / "_gate" taps of a block run mbconv_block_kernel: the launcher ends the chain in front of it)
    const BlockArgs* nxp = last ? tab + i : tab + i + 1;
    const unsigned kind = (ca.kinds >> (2 * i)) & 3u;
#ifdef MKWS_FRONT_TIMING
    unsigned long long* dt = ca.dbg_t ? ca.dbg_t + ((size_t)blockIdx.x * kChainMax + i) * 8 : nullptr;
    if (dt && threadIdx.x == 0) dt[7] = wall_clock64();         // top of the block: before its constants are fetched
#else
    unsigned long long* dt = nullptr;
#endif
    if (kind == 0) chain_block<3, 1, MT, NWAVES>(a, nxp, !last, s_blk, ca.ldsU, ca.ldsE, i == 0, carry, dt);
    else if (kind == 1) chain_block<5, 1, MT, NWAVES>(a, nxp, !last, s_blk, ca.ldsU, ca.ldsE, i == 0, carry, dt);
    else chain_block<5, 2, MT, NWAVES>(a, nxp, !last, s_blk, ca.ldsU, ca.ldsE, i == 0, carry, dt);
  }
}

// ------------------------------------------------------------------------------------------------
// Paired whole-block kernel for the 2x2-image blocks (6b..7a).  mbconv_block_kernel gives every CU one 16-row tile and
// makes it pull the whole block's weights (2.2 MB) from L2, and a CU's L2 stream tops out at ~41 GB/s whatever is kept in
// flight (profiles/r02_notes.md): 54 us of the 59.  Here TWO workgroups on two CUs of one XCD share 8 clips (two row
// tiles) and split the block's CHANNELS: half h owns expanded channels [h*Cexp/2, (h+1)*Cexp/2).
//   A   expand: the half's n-tiles, both row tiles           -> each CU streams half of the expand weights, every
//   B   depthwise + SE sums on the half's channels              fragment feeds two row tiles
//   C1  SE reduce over the half's channels: PARTIAL r          -> exchange 1 (384 floats each way), r = swish(p0 + p1 + br)
//   C2  SE gate for the half's channels
//   D   projection over the half's K: PARTIAL output tiles     -> exchange 2: even tiles are finished by half 0, odd by
//       half 1 (partial of the other half + own, BN, residual)
// Exchanges go through a small global buffer (L2 of the shared XCD): plain stores, s_waitcnt vmcnt(0), barrier, a relaxed
// agent-scope flag; the consumer polls the flag, reads the data with agent-scope (L1-bypassing) loads and resets the flag
// (no epochs: hipGraph replay safe).  Measured with tools/microbench/pair_sync.hip: 1-3 us per exchange; the formal
// agent-scope fences cost 13 us (buffer_inv sc1) + 4-16 us (buffer_wbl2 sc1) EACH and are not needed inside one XCD.
// Workgroups are dealt round-robin over the XCDs, so blocks b and b ^ 8 share an XCD and are adjacent in its dispatch
// order (no deadlock: an XCD's resident set is a prefix of its sequence, complete pairs always finish); both halves publish
// their XCC id with the first flag.  If they differ, or a wait times out (CU masking, a partitioned device, another process
// holding CUs: the dispatch-order assumption is not a documented guarantee), the half poisons its output tiles with NaN AND
// records the failure (pair_report); every later launch of the handle then poisons without exchanging, and the next
// mkws_embed_forward moves the handle to mbconv_block_kernel for good and returns MKWS_ERR_EXCHANGE (check_pair_health).
// Reductions keep a fixed order (p0 + p1 commutes), so results are bit-identical across batch sizes.
// Store of an exchange partial (pair chain).  -DMKWS_PAIR_NT_STORES builds the A/B library whose exchange stores carry the non-temporal hint
// (round-5 PMC A/B of the chain's HBM write traffic, profiles/r05_notes.md: no gain, the plain store ships).
#ifdef MKWS_PAIR_NT_STORES
#define MKWS_XSTORE(ptr, val) __builtin_nontemporal_store((val), (ptr))
#else
#define MKWS_XSTORE(ptr, val) (*(ptr) = (val))
#endif

struct PairArgs {
  BlockArgs b;
  float* xc1;      // [pairs][2][384]
  float* xd;       // [pairs][2][10][2][256]
  int* flags;      // [pairs][2 exchanges][2 halves], zero between launches
  int* err_dev;    // device word, sticky: nonzero = an exchange of this handle has failed; later launches skip their exchanges and poison
  int* err_host;   // the same word in host-mapped memory: mkws_embed_forward reads it without synchronising (see check_pair_health)
  int fault;       // test hook ("pair_fault"): 1 = both halves expect the wrong XCC id, 2 = half 1 never shows up (timeout)
};
enum { kPairErrTimeout = 1, kPairErrXcc = 2 };
static constexpr int kPairXc1 = 384, kPairXdTiles = 10;

__device__ __forceinline__ f32x4 ld_agent_x4(const float* p) {
  f32x4 v;
  v.x = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); v.y = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  v.z = __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); v.w = __hip_atomic_load(p + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return v;
}

// Thread 0 of each half: publish `mine`, wait for the partner's flag, reset it.  Returns the partner's value (0 = timed out;
// the half then withdraws its own flag so that a partner arriving later times out too instead of consuming a stale signal).
__device__ __forceinline__ int pair_signal_wait(int* mine, int* theirs, int value) {
  __hip_atomic_store(mine, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int got = 0, spins = 0;
  while ((got = __hip_atomic_load(theirs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
    __builtin_amdgcn_s_sleep(1);
    if (++spins > (1 << 21)) { __hip_atomic_store(mine, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return 0; }
  }
  __hip_atomic_store(theirs, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return got;
}

// A failed exchange is recorded twice: in device memory (read by every later launch of the handle, which then skips its
// exchanges and poisons its output: stale flags can never be consumed silently) and in host-mapped memory (read by the
// next mkws_embed_forward without a synchronisation: the handle then leaves the paired kernel for good).
__device__ __forceinline__ void pair_report(int* err_dev, int* err_host, int code) {
  __hip_atomic_store(err_dev, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(err_host, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Probe for mkws_embed_create: every workgroup records the XCC it runs on (see pair_layout_ok).
__global__ void xcc_probe_kernel(int* out) {
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  if (threadIdx.x == 0) out[blockIdx.x] = (int)(xcc & 0xf);
}

struct PairLds { int U, E, Z; };
__host__ __device__ inline PairLds pair_lds(int KCe, int CH, int MT) {
  PairLds l;
  const int xf = KCe * MT * 256, sg = 4 * MT * CH * 2;
  l.U = xf > sg ? xf : sg;
  l.E = MT * 16 * (CH + 4);
  const int z2 = 16 * 52 + CH;             // A: scale / shift [2][CH];  later r [16][52] + bias [CH];  last 4 words: the error flag
  l.Z = ((2 * CH > z2) ? 2 * CH : z2) + 4;
  return l;
}

// MT = row tiles per pair: 2 (8 clips) at full batch; 1 (4 clips) for handles whose batch would otherwise leave half of the
// CUs without a workgroup (max_batch <= 512 on 256 CUs).
template <int KS, int MT, int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void mbconv_pair_kernel(PairArgs pa) {
  extern __shared__ __attribute__((aligned(16))) float s_blk[];
  const BlockArgs& a = pa.b;
  constexpr int NTHR = NWAVES * 64;
  constexpr int HT = 2, WT = 2, HW = 4, G = 4 * MT;
  constexpr int PT = KS / 2, PLF = KS / 2;
  constexpr int LDR = 52;
  const int h = (blockIdx.x >> 3) & 1, pair = (blockIdx.x >> 4) * 8 + (blockIdx.x & 7);
  const int b0 = pair * G;
  if (b0 >= a.B) return;                                        // both halves of a padding pair leave together
  const int Cexp = a.Cexp, CH = Cexp / 2, LDE = CH + 4;
  const int KH = CH / 16;                                       // this half's 16-channel tiles / K chunks
  const int KCx = Cexp / 16;
  const PairLds L = pair_lds(a.KCe, CH, MT);
  float* s_X = s_blk;                                           // U, phase A: [KCe][MT][256]
  float* s_S = s_blk;                                           // U, later: [8][CH] SE means
  float* s_G = s_S + G * CH;                                    //           [8][CH] gate; C1: [NWAVES][48][8] partials
  float* s_P = s_G;
  float* s_E = s_blk + L.U;                                     // [32][LDE]
  float* s_scE = s_E + L.E;                                     // Z, phase A: expand BN scale / shift of the half
  float* s_shE = s_scE + CH;
  float* s_R = s_scE;                                           // Z, later: r [8][LDR], SE expand bias [CH]
  float* s_be = s_R + 16 * LDR;
  volatile int* s_bad = reinterpret_cast<volatile int*>(s_scE + L.Z - 4);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform: wave-dependent tile / chunk offsets stay on the scalar unit
  const int g = lane >> 4, c = lane & 15;
  const int gvalid = (a.B - b0 < G) ? (a.B - b0) : G;
  const int rows = gvalid * HW;
  const size_t row0 = (size_t)b0 * HW;
  const int chan0 = h * CH;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  xcc &= 0xf;
  int* flag_mine = pa.flags + (size_t)pair * 4 + h;
  int* flag_theirs = pa.flags + (size_t)pair * 4 + (h ^ 1);
  if (pa.fault == 2 && h == 1) return;                            // test hook: the partner never arrives
  if (tid == 0) *s_bad = __hip_atomic_load(pa.err_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sticky: an earlier launch failed
  const int xcc_expect = 1 + (int)(pa.fault == 1 ? (xcc ^ 1u) : xcc);

#ifdef MKWS_FRONT_TIMING
  const long long dbg_c0 = clock64();
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 0] = wall_clock64();
#endif
  // phase A's weight ring is requested before the input is staged (its first fragments arrive during the staging)
  constexpr int RDA = 4, NTWA = 3;                               // 3 n-tiles x 2 row tiles per run: 24 MFMAs per 3 + 2 operand fragments
  const int a_groups = (KH + NTWA - 1) / NTWA;
  const int a_nruns = (a_groups > wave) ? (a_groups - wave + NWAVES - 1) / NWAVES : 0;
  auto a_tile_of = [&](int r) { return (wave + NWAVES * r) * NTWA; };
  const unsigned loff = (unsigned)(g * 64 + c * 4);                 // this lane's float4 inside a packed weight fragment
  const WBuf a_w(a.WpE + (size_t)(h * KH) * 256, loff);
  f32x4 wqa[RDA][NTWA];
  stream_mfma_runs_prefetch<NTWA, RDA>(wqa, a_w, (size_t)a.NTe * 256, KH, a_nruns, a.KCe, a_tile_of);
  for (int jm = wave; jm < a.KCe * MT; jm += NWAVES) {
    const int j = jm / MT, m = jm - j * MT;
    const int r = m * 16 + c;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < rows && 16 * j + 4 * g < a.Cin) v = *reinterpret_cast<const f32x4*>(a.X + (row0 + r) * a.Cin + 16 * j + 4 * g);
    *reinterpret_cast<f32x4*>(s_X + ((size_t)jm * 64 + lane) * 4) = v;
  }
  for (int i = tid; i < CH; i += NTHR) { s_scE[i] = a.scE[chan0 + i]; s_shE[i] = a.shE[chan0 + i]; }
  __syncthreads();
#ifdef MKWS_FRONT_TIMING
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 1] = wall_clock64();
#endif

  // ---- phase A: expand, this half's KH n-tiles; every weight fragment feeds both row tiles ----
  {
    auto xload = [&](int j, int m) { return *reinterpret_cast<const f32x4*>(s_X + ((size_t)(j * MT + m) * 64 + lane) * 4); };
    auto xmake = [](const f32x4& v) { return v; };
    auto epi = [&](int t0, const f32x4 (&acc)[NTWA][MT]) {
#pragma unroll
      for (int q = 0; q < NTWA; ++q) {
        const int n = (t0 + q) * 16 + 4 * g;
        if (t0 + q < KH) {
          const f32x4 sc = *reinterpret_cast<const f32x4*>(s_scE + n), sh = *reinterpret_cast<const f32x4*>(s_shE + n);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            f32x4 y = acc[q][m] * sc + sh;
            y = swish4_(y);
            if (m * 16 + c >= rows) y = (f32x4){0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(s_E + (size_t)(m * 16 + c) * LDE + n) = y;
          }
        }
      }
    };
    stream_mfma_runs<NTWA, RDA, MT, true>(wqa, a_w, (size_t)a.NTe * 256, KH, a_nruns, a.KCe, a_tile_of, xload, xmake, epi);
  }
  __syncthreads();
#ifdef MKWS_FRONT_TIMING
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 2] = wall_clock64();
#endif

  // ---- phase B: depthwise + BN + swish in place, SE means (thread = clip x channel quad of the half) ----
  for (int i = tid; i < CH; i += NTHR) s_be[i] = a.be[chan0 + i];
  const int c1_per = (KH + NWAVES - 1) / NWAVES;
  const int c1_j0 = wave * c1_per;
  const int c1_kc = (c1_j0 + c1_per <= KH) ? c1_per : (KH > c1_j0 ? KH - c1_j0 : 0);
  const WBuf c1_w(a.WrP + (size_t)(h * KH + c1_j0) * a.NTR * 256, loff);
  f32x4 wq1[3][3];
  stream_mfma_prefetch<3, 3>(wq1, c1_w, (size_t)a.NTR * 256, 0, 1, a.NTR, c1_kc);
  {
    const int Q = CH / 4;
    for (int task = tid; task < G * Q; task += NTHR) {
      const int gi = task / Q, q4 = (task - gi * Q) * 4;
      float* Eg = s_E + (size_t)gi * HW * LDE + q4;
      f32x4 ein[HW];
#pragma unroll
      for (int pix = 0; pix < HW; ++pix) ein[pix] = *reinterpret_cast<const f32x4*>(Eg + (size_t)pix * LDE);
      f32x4 acc[HW];
#pragma unroll
      for (int o = 0; o < HW; ++o) acc[o] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < KS; ++i) {
#pragma unroll
        for (int jx = 0; jx < KS; ++jx) {
          bool used = false;
#pragma unroll
          for (int oh = 0; oh < HT; ++oh)
#pragma unroll
            for (int ow = 0; ow < WT; ++ow) {
              const int ih = oh - PT + i, iw = ow - PLF + jx;
              used |= (ih >= 0 && ih < HT && iw >= 0 && iw < WT);
            }
          if (!used) continue;
          const f32x4 wv = *reinterpret_cast<const f32x4*>(a.Wd + (size_t)(i * KS + jx) * Cexp + chan0 + q4);
#pragma unroll
          for (int oh = 0; oh < HT; ++oh)
#pragma unroll
            for (int ow = 0; ow < WT; ++ow) {
              const int ih = oh - PT + i, iw = ow - PLF + jx;
              if (ih >= 0 && ih < HT && iw >= 0 && iw < WT) acc[oh * WT + ow] += ein[ih * WT + iw] * wv;
            }
        }
      }
      const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scD + chan0 + q4);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(a.shD + chan0 + q4);
      f32x4 ssum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < HW; ++o) {
        f32x4 y = acc[o] * sc + sh;
        y = swish4_(y);
        if (gi >= gvalid) y = (f32x4){0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(Eg + (size_t)o * LDE) = y;
        ssum += y;
        if (a.dbg_dw && gi < gvalid) *reinterpret_cast<f32x4*>(a.dbg_dw + (row0 + gi * HW + o) * Cexp + chan0 + q4) = y;
      }
      *reinterpret_cast<f32x4*>(s_S + (size_t)gi * CH + q4) = ssum * (1.0f / (float)HW);
    }
  }
  __syncthreads();
#ifdef MKWS_FRONT_TIMING
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 3] = wall_clock64();
#endif

  // ---- phase C1: partial r^T[se, clips] over the half's channels (K split over the waves), then exchange 1 ----
  constexpr int NTW2 = 3;
  const int c2_groups = (KH + NTW2 - 1) / NTW2;
  const int c2_runs = (c2_groups > wave) ? (c2_groups - wave + NWAVES - 1) / NWAVES : 0;
  auto c2_tile_of = [&](int r) { return (wave + NWAVES * r) * NTW2; };
  const WBuf c2_w(a.We2P + (size_t)(h * KH) * 256, loff);
  f32x4 wq2[3][NTW2];
  {
    f32x4 acc[3][1];
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* srow = s_S + (size_t)(c < G ? c : 0) * CH + 16 * c1_j0 + 4 * g;
    auto xload = [&](int j, int) { return *reinterpret_cast<const f32x4*>(srow + 16 * j); };
    auto xmake = [](const f32x4& v) { return v; };
    if (c1_kc > 0) stream_mfma<3, 3, 1, true>(acc, wq1, c1_w, (size_t)a.NTR * 256, 0, 1, a.NTR, c1_kc, xload, xmake);
    stream_mfma_runs_prefetch<NTW2, 3>(wq2, c2_w, (size_t)KCx * 256, KH, c2_runs, a.NTR, c2_tile_of);
    if (c < G) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_P[((wave * 3 + q) * 16 + 4 * g + r) * G + c] = acc[q][0][r];
    }
  }
  const float br_pre = (tid < 48 * G && tid / G < a.se) ? a.br[tid / G] : 0.0f;
  __syncthreads();
  float c1_part = 0.0f;
  float* xc1_mine = pa.xc1 + ((size_t)pair * 2 + h) * kPairXc1;
  const float* xc1_theirs = pa.xc1 + ((size_t)pair * 2 + (h ^ 1)) * kPairXc1;
  if (tid < 48 * G) {
    if (tid / G < a.se) {
#pragma unroll
      for (int w = 0; w < NWAVES; ++w) c1_part += s_P[(w * 48 + tid / G) * G + (tid % G)];
    }
    xc1_mine[tid] = c1_part;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0 && *s_bad == 0) {
    const int got = pair_signal_wait(flag_mine, flag_theirs, 1 + (int)xcc);
    if (got != xcc_expect) {                                     // timed out, or the halves sit on different XCDs
      *s_bad = 1;
      pair_report(pa.err_dev, pa.err_host, got == 0 ? kPairErrTimeout : kPairErrXcc);
    }
  }
  __syncthreads();
  if (tid < 48 * G) {
    const int n = tid / G, clip = tid - n * G;
    float v = 0.0f;
    if (n < a.se) {
      const float other = __hip_atomic_load(xc1_theirs + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v = swishf_((h == 0 ? c1_part + other : other + c1_part) + br_pre);
    }
    s_R[clip * LDR + n] = v;
  }
  __syncthreads();
#ifdef MKWS_FRONT_TIMING
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 4] = wall_clock64();
#endif

  // ---- phase C2: gate for the half's channels; phase D's weight stream is requested first ----
  const int d_ntw = (a.NTp > wave) ? (a.NTp - wave + NWAVES - 1) / NWAVES : 0;
  const WBuf d_w(a.WpP + (size_t)(h * KH) * a.NTp * 256, loff);
  f32x4 wqd[4][3];
  if (d_ntw > 0) stream_mfma_prefetch<3, 4>(wqd, d_w, (size_t)a.NTp * 256, wave, NWAVES, a.NTp, KH);
  {
    const float* rrow = s_R + (c < G ? c : 0) * LDR + 4 * g;
    auto xload = [&](int j, int) { return *reinterpret_cast<const f32x4*>(rrow + 16 * j); };
    auto xmake = [](const f32x4& v) { return v; };
    auto epi = [&](int t0, const f32x4 (&acc)[NTW2][1]) {
#pragma unroll
      for (int q = 0; q < NTW2; ++q) {
        const int n = (t0 + q) * 16 + 4 * g;
        if (t0 + q < KH && c < G) {
          f32x4 y = acc[q][0] + *reinterpret_cast<const f32x4*>(s_be + n);
          y = sigmoid4_(y);
          *reinterpret_cast<f32x4*>(s_G + (size_t)c * CH + n) = y;
          if (a.dbg_gate && c < gvalid) *reinterpret_cast<f32x4*>(a.dbg_gate + (size_t)(b0 + c) * Cexp + chan0 + n) = y;
        }
      }
    };
    stream_mfma_runs<NTW2, 3, 1, true>(wq2, c2_w, (size_t)KCx * 256, KH, c2_runs, a.NTR, c2_tile_of, xload, xmake, epi);
  }
  __syncthreads();
#ifdef MKWS_FRONT_TIMING
  if (threadIdx.x == 0) a.dbg_t[(size_t)blockIdx.x * 8 + 5] = wall_clock64();
#endif

  // ---- gate the depthwise output in place, once (see mbconv_block_kernel) ----
  {
    const int Q = CH / 4;
    for (int i = tid; i < G * HW * Q; i += NTHR) {
      const int r = i / Q, q4 = (i - r * Q) * 4;
      float* e = s_E + (size_t)r * LDE + q4;
      *reinterpret_cast<f32x4*>(e) = *reinterpret_cast<const f32x4*>(e) * *reinterpret_cast<const f32x4*>(s_G + (size_t)(r / HW) * CH + q4);
    }
  }
  __syncthreads();
  // ---- phase D: partial projection over the half's K; exchange 2; tiles of parity h are finished here ----
  {
    const size_t cstride = (size_t)a.NTp * 256;
    const float* erow[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) erow[m] = s_E + (size_t)(m * 16 + c) * LDE + 4 * g;
    auto xload = [&](int j, int m) { return *reinterpret_cast<const f32x4*>(erow[m] + 16 * j); };
    auto xmake = [](const f32x4& v) { return v; };
    const bool finisher = ((wave & 1) == h);                    // tiles wave + NWAVES*q share the wave's parity
    float* xd_mine = pa.xd + ((size_t)pair * 2 + h) * (kPairXdTiles * 2 * 256);
    const float* xd_theirs = pa.xd + ((size_t)pair * 2 + (h ^ 1)) * (kPairXdTiles * 2 * 256);
    auto run = [&](auto ntw_tag) {
      constexpr int NTW = decltype(ntw_tag)::value;
      f32x4 acc[NTW > 0 ? NTW : 1][MT];
#pragma unroll
      for (int q = 0; q < (NTW > 0 ? NTW : 1); ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[q][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (NTW > 0) {
        stream_mfma<NTW, 4, MT, true>(acc, wqd, d_w, cstride, wave, NWAVES, a.NTp, KH, xload, xmake);
        if (!finisher) {
#pragma unroll
          for (int q = 0; q < NTW; ++q) {
            const int t = wave + NWAVES * q;
            if (t < a.NTp) {
#pragma unroll
              for (int m = 0; m < MT; ++m) *reinterpret_cast<f32x4*>(xd_mine + ((size_t)((t >> 1) * 2 + m) * 64 + lane) * 4) = acc[q][m];
            }
          }
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0 && *s_bad == 0) {
        const int got = pair_signal_wait(flag_mine + 2, flag_theirs + 2, 1);
        if (got != 1) { *s_bad = 1; pair_report(pa.err_dev, pa.err_host, kPairErrTimeout); }
      }
      __syncthreads();
      if constexpr (NTW > 0) {
        if (finisher) {
          const bool bad = *s_bad != 0;
#pragma unroll
          for (int q = 0; q < NTW; ++q) {
            const int t = wave + NWAVES * q;
            const int n = t * 16 + 4 * g;
            if (t < a.NTp) {
              const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scP + n), sh = *reinterpret_cast<const f32x4*>(a.shP + n);
#pragma unroll
              for (int m = 0; m < MT; ++m) {
                const int r = m * 16 + c;
                const f32x4 other = ld_agent_x4(xd_theirs + ((size_t)((t >> 1) * 2 + m) * 64 + lane) * 4);
                if (r < rows) {
                  f32x4 y = ((h == 0) ? acc[q][m] + other : other + acc[q][m]) * sc + sh;
                  if (a.residual) y += *reinterpret_cast<const f32x4*>(a.X + (row0 + r) * a.Cin + n);
                  if (bad) y = (f32x4){__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                  *reinterpret_cast<f32x4*>(a.Y + (row0 + r) * a.Cout + n) = y;
                }
              }
            }
          }
        }
      }
    };
    if (d_ntw == 0) run(std::integral_constant<int, 0>{});
    else if (d_ntw == 1) run(std::integral_constant<int, 1>{});
    else if (d_ntw == 2) run(std::integral_constant<int, 2>{});
    else run(std::integral_constant<int, 3>{});
  }
#ifdef MKWS_FRONT_TIMING
  __syncthreads();
  if (threadIdx.x == 0) { a.dbg_t[(size_t)blockIdx.x * 8 + 6] = wall_clock64(); a.dbg_t[(size_t)blockIdx.x * 8 + 7] = (unsigned long long)(clock64() - dbg_c0); }
#endif
}

// ------------------------------------------------------------------------------------------------
// Depth-fused chain of PAIRED whole-block kernels: the stride-1 2x2-image blocks 6b -> 6c -> 6d -> 7a in ONE launch.  mbconv_pair_kernel's
// two halves (workgroups b and b ^ 8 of one XCD, sharing 4 * MT clips, each owning half of the expanded channels) walk the blocks
// themselves, like mbconv_chain_kernel's workgroups.  What changes against one launch per block:
//   * exchange 2 of a block that has a successor carries ALL projection tiles in both directions (not one parity each way), and BOTH
//     halves finish every tile (p0 + p1 in that order on both sides: identical bits): each half then holds the whole block output,
//     which it writes into U as the next block's input fragments; residual in registers (the same lane finishes the same tile);
//   * flags: one set per (block, exchange) -- a slot is published and reset once per launch, as in mbconv_pair_kernel (a reset that
//     lands after the next publish of the SAME slot would swallow it);
//   * the exchange buffers are reused from block to block: between two uses of a buffer lies the other exchange of the pair, which
//     orders the partner's reads before my next writes.
// The last block of the chain exchanges by parity and stores to HBM exactly like mbconv_pair_kernel.  Failure contract unchanged.
constexpr int kPairChainMax = 4;
struct PairChainArgs {
  const BlockArgs* tab;       // device table (see ChainArgs)
  int i0, n;
  unsigned kinds;             // 1 bit per chain position: 0 = 5x5, 1 = 3x3 (stride 1 both)
  const float* X; float* Y;
  int B;
  int ldsU, ldsE, ldsZ;       // LDS carve (floats): maxima over the chain's blocks; the last 4 words of Z hold the error flag
  float* xc1;                 // [pairs][2][kPairXc1]
  float* xd;                  // [pairs][2][kPairXdAll][2][256]
  int* flags;                 // [pairs][kPairChainMax][2 exchanges][2 halves], zero between launches
  int* err_dev; int* err_host; int fault;
  // top conv + BN + swish + global average pool as the chain's last phase (null = not fused): the halves split its n-tiles, no exchange
  const float* top_Wp; const float* top_sc; const float* top_sh; int top_KC, top_NT;
  float* gap;                 // [B, 16 * top_NT] pooled features
};
static constexpr int kPairXdAll = 20;

template <int KS, int MT, int NWAVES>
__device__ __forceinline__ void pair_chain_block(const BlockArgs& a, const BlockArgs* nxp, bool has_next, bool first, int blk, const PairChainArgs& pa,
                                                 float* s_blk, int h, int pair, int xcc_expect, unsigned xcc, f32x4 (&carry)[2][MT]) {
  constexpr int NTHR = NWAVES * 64;
  constexpr int HT = 2, WT = 2, HW = 4, G = 4 * MT;
  constexpr int PT = KS / 2, PLF = KS / 2;
  constexpr int LDR = 52;
  constexpr int RDA = 4, NTWA = 3;
  const BlockArgs* nx = has_next ? nxp : nullptr;
  const int b0 = pair * G;
  const int Cexp = a.Cexp, CH = Cexp / 2, LDE = CH + 4;
  const int KH = CH / 16;
  const int KCx = Cexp / 16;
  float* s_X = s_blk;
  float* s_S = s_blk;
  float* s_G = s_S + G * CH;
  float* s_P = s_G;
  float* s_E = s_blk + pa.ldsU;
  float* s_scE = s_E + pa.ldsE;
  float* s_shE = s_scE + CH;
  float* s_R = s_scE;
  float* s_be = s_R + 16 * LDR;
  volatile int* s_bad = reinterpret_cast<volatile int*>(s_scE + pa.ldsZ - 4);
  const int tid = opaque_((int)threadIdx.x), lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int gvalid = (a.B - b0 < G) ? (a.B - b0) : G;
  const int rows = gvalid * HW;
  const size_t row0 = (size_t)b0 * HW;
  const int chan0 = h * CH;
  const unsigned loff = (unsigned)(g * 64 + c * 4);
  int* fl = pa.flags + ((size_t)pair * kPairChainMax + blk) * 4;

  // ---- phase A: expand, this half's KH n-tiles (input fragments in s_X, ring in flight) ----
  const int a_groups = (KH + NTWA - 1) / NTWA;
  const int a_nruns = (a_groups > wave) ? (a_groups - wave + NWAVES - 1) / NWAVES : 0;
  auto a_tile_of = [&](int r) { return (wave + NWAVES * r) * NTWA; };
  {
    // the expand ring is requested HERE, not during the previous block's projection as in chain_block: carried across the block loop its 48
    // registers cost the kernel ~90 (165 -> 256 + spills); the price is one L2 round trip at the top of every block
    const WBuf a_w(a.WpE + (size_t)(h * KH) * 256, loff);
    f32x4 wqa[RDA][NTWA];
    stream_mfma_runs_prefetch<NTWA, RDA>(wqa, a_w, (size_t)a.NTe * 256, KH, a_nruns, a.KCe, a_tile_of);
    auto xload = [&](int j, int m) { return *reinterpret_cast<const f32x4*>(s_X + ((size_t)(j * MT + m) * 64 + lane) * 4); };
    auto xmake = [](const f32x4& v) { return v; };
    auto epi = [&](int t0, const f32x4 (&acc)[NTWA][MT]) {
#pragma unroll
      for (int q = 0; q < NTWA; ++q) {
        const int n = (t0 + q) * 16 + 4 * g;
        if (t0 + q < KH) {
          const f32x4 sc = *reinterpret_cast<const f32x4*>(s_scE + n), sh = *reinterpret_cast<const f32x4*>(s_shE + n);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            f32x4 y = acc[q][m] * sc + sh;
            y = swish4_(y);
            if (m * 16 + c >= rows) y = (f32x4){0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(s_E + (size_t)(m * 16 + c) * LDE + n) = y;
          }
        }
      }
    };
    stream_mfma_runs<NTWA, RDA, MT, true>(wqa, a_w, (size_t)a.NTe * 256, KH, a_nruns, a.KCe, a_tile_of, xload, xmake, epi);
  }
  __syncthreads();

  // ---- phase B: depthwise + BN + swish in place, SE means (thread = clip x channel quad of the half) ----
  for (int i = tid; i < CH; i += NTHR) s_be[i] = a.be[chan0 + i];
  const int c1_per = (KH + NWAVES - 1) / NWAVES;
  const int c1_j0 = wave * c1_per;
  const int c1_kc = (c1_j0 + c1_per <= KH) ? c1_per : (KH > c1_j0 ? KH - c1_j0 : 0);
  const WBuf c1_w(a.WrP + (size_t)(h * KH + c1_j0) * a.NTR * 256, loff);
  f32x4 wq1[3][3];
  stream_mfma_prefetch<3, 3>(wq1, c1_w, (size_t)a.NTR * 256, 0, 1, a.NTR, c1_kc);
  {
    const int Q = CH / 4;
    for (int task = tid; task < G * Q; task += NTHR) {
      const int gi = task / Q, q4 = (task - gi * Q) * 4;
      float* Eg = s_E + (size_t)gi * HW * LDE + q4;
      // taps and constants requested first, in source order (see chain_block)
      f32x4 wv[KS][KS];
#pragma unroll
      for (int i = 0; i < KS; ++i)
#pragma unroll
        for (int jx = 0; jx < KS; ++jx) {
          bool used = false;
#pragma unroll
          for (int oh = 0; oh < HT; ++oh)
#pragma unroll
            for (int ow = 0; ow < WT; ++ow) {
              const int ih = oh - PT + i, iw = ow - PLF + jx;
              used |= (ih >= 0 && ih < HT && iw >= 0 && iw < WT);
            }
          if (used) wv[i][jx] = *reinterpret_cast<const f32x4*>(a.Wd + (size_t)(i * KS + jx) * Cexp + chan0 + q4);
        }
      const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scD + chan0 + q4);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(a.shD + chan0 + q4);
      f32x4 ein[HW];
#pragma unroll
      for (int pix = 0; pix < HW; ++pix) ein[pix] = *reinterpret_cast<const f32x4*>(Eg + (size_t)pix * LDE);
      __builtin_amdgcn_sched_barrier(0);
      f32x4 acc[HW];
#pragma unroll
      for (int o = 0; o < HW; ++o) acc[o] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < KS; ++i)
#pragma unroll
        for (int jx = 0; jx < KS; ++jx)
#pragma unroll
          for (int oh = 0; oh < HT; ++oh)
#pragma unroll
            for (int ow = 0; ow < WT; ++ow) {
              const int ih = oh - PT + i, iw = ow - PLF + jx;
              if (ih >= 0 && ih < HT && iw >= 0 && iw < WT) acc[oh * WT + ow] += ein[ih * WT + iw] * wv[i][jx];
            }
      f32x4 ssum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < HW; ++o) {
        f32x4 y = acc[o] * sc + sh;
        y = swish4_(y);
        if (gi >= gvalid) y = (f32x4){0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(Eg + (size_t)o * LDE) = y;
        ssum += y;
      }
      *reinterpret_cast<f32x4*>(s_S + (size_t)gi * CH + q4) = ssum * (1.0f / (float)HW);
    }
  }
  __syncthreads();

  // ---- phase C1: partial r^T over the half's channels, then exchange 1 ----
  constexpr int NCST = 2;                                       // CH <= NCST * NTHR (host-checked)
  float nsc[NCST], nsh[NCST];
  const int nxCH = nx ? sgpr_(nx->Cexp) / 2 : 0;
  if (nx) {
    const float* nscE = sgpr_(nx->scE) + h * nxCH; const float* nshE = sgpr_(nx->shE) + h * nxCH;
#pragma unroll
    for (int k = 0; k < NCST; ++k) {
      const int i = tid + k * NTHR;
      if (i < nxCH) { nsc[k] = nscE[i]; nsh[k] = nshE[i]; }
    }
  }
  constexpr int NTW2 = 3;
  const int c2_groups = (KH + NTW2 - 1) / NTW2;
  const int c2_runs = (c2_groups > wave) ? (c2_groups - wave + NWAVES - 1) / NWAVES : 0;
  auto c2_tile_of = [&](int r) { return (wave + NWAVES * r) * NTW2; };
  const WBuf c2_w(a.We2P + (size_t)(h * KH) * 256, loff);
  f32x4 wq2[3][NTW2];
  {
    f32x4 acc[3][1];
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* srow = s_S + (size_t)(c < G ? c : 0) * CH + 16 * c1_j0 + 4 * g;
    auto xload = [&](int j, int) { return *reinterpret_cast<const f32x4*>(srow + 16 * j); };
    auto xmake = [](const f32x4& v) { return v; };
    if (c1_kc > 0) stream_mfma<3, 3, 1, true>(acc, wq1, c1_w, (size_t)a.NTR * 256, 0, 1, a.NTR, c1_kc, xload, xmake);
    stream_mfma_runs_prefetch<NTW2, 3>(wq2, c2_w, (size_t)KCx * 256, KH, c2_runs, a.NTR, c2_tile_of);
    if (c < G) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_P[((wave * 3 + q) * 16 + 4 * g + r) * G + c] = acc[q][0][r];
    }
  }
  const float br_pre = (tid < 48 * G && tid / G < a.se) ? a.br[tid / G] : 0.0f;
  __syncthreads();
  float c1_part = 0.0f;
  float* xc1_mine = pa.xc1 + ((size_t)pair * 2 + h) * kPairXc1;
  const float* xc1_theirs = pa.xc1 + ((size_t)pair * 2 + (h ^ 1)) * kPairXc1;
  if (tid < 48 * G) {
    if (tid / G < a.se) {
#pragma unroll
      for (int w = 0; w < NWAVES; ++w) c1_part += s_P[(w * 48 + tid / G) * G + (tid % G)];
    }
    xc1_mine[tid] = c1_part;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0 && *s_bad == 0) {
    const int got = pair_signal_wait(fl + h, fl + (h ^ 1), 1 + (int)xcc);
    if (got != xcc_expect) {
      *s_bad = 1;
      pair_report(pa.err_dev, pa.err_host, got == 0 ? kPairErrTimeout : kPairErrXcc);
    }
  }
  __syncthreads();
  if (tid < 48 * G) {
    const int n = tid / G, clip = tid - n * G;
    float v = 0.0f;
    if (n < a.se) {
      const float other = __hip_atomic_load(xc1_theirs + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v = swishf_((h == 0 ? c1_part + other : other + c1_part) + br_pre);
    }
    s_R[clip * LDR + n] = v;
  }
  __syncthreads();

  // ---- phase C2: gate for the half's channels; phase D's weight stream is requested first ----
  const int d_ntw = (a.NTp > wave) ? (a.NTp - wave + NWAVES - 1) / NWAVES : 0;
  const WBuf d_w(a.WpP + (size_t)(h * KH) * a.NTp * 256, loff);
  f32x4 wqd[4][3];
  if (d_ntw > 0) stream_mfma_prefetch<3, 4>(wqd, d_w, (size_t)a.NTp * 256, wave, NWAVES, a.NTp, KH);
  {
    const float* rrow = s_R + (c < G ? c : 0) * LDR + 4 * g;
    auto xload = [&](int j, int) { return *reinterpret_cast<const f32x4*>(rrow + 16 * j); };
    auto xmake = [](const f32x4& v) { return v; };
    auto epi = [&](int t0, const f32x4 (&acc)[NTW2][1]) {
#pragma unroll
      for (int q = 0; q < NTW2; ++q) {
        const int n = (t0 + q) * 16 + 4 * g;
        if (t0 + q < KH && c < G) {
          f32x4 y = acc[q][0] + *reinterpret_cast<const f32x4*>(s_be + n);
          y = sigmoid4_(y);
          *reinterpret_cast<f32x4*>(s_G + (size_t)c * CH + n) = y;
        }
      }
    };
    stream_mfma_runs<NTW2, 3, 1, true>(wq2, c2_w, (size_t)KCx * 256, KH, c2_runs, a.NTR, c2_tile_of, xload, xmake, epi);
  }
  __syncthreads();

  // ---- gate in place; the next block's expand BN constants (this half's) go to Z ----
  {
    const int Q = CH / 4;
    for (int i = tid; i < G * HW * Q; i += NTHR) {
      const int r = i / Q, q4 = (i - r * Q) * 4;
      float* e = s_E + (size_t)r * LDE + q4;
      *reinterpret_cast<f32x4*>(e) = *reinterpret_cast<const f32x4*>(e) * *reinterpret_cast<const f32x4*>(s_G + (size_t)(r / HW) * CH + q4);
    }
  }
  if (nx) {
#pragma unroll
    for (int k = 0; k < NCST; ++k) {
      const int i = tid + k * NTHR;
      if (i < nxCH) { s_scE[i] = nsc[k]; s_scE[nxCH + i] = nsh[k]; }
    }
  }
  __syncthreads();

  // ---- phase D: partial projection over the half's K; exchange 2; finish ----
  {
    const size_t cstride = (size_t)a.NTp * 256;
    const float* erow[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) erow[m] = s_E + (size_t)(m * 16 + c) * LDE + 4 * g;
    auto xload = [&](int j, int m) { return *reinterpret_cast<const f32x4*>(erow[m] + 16 * j); };
    auto xmake = [](const f32x4& v) { return v; };
    const bool all_tiles = has_next;                            // both halves finish every tile (the whole output becomes the next input)
    const bool my_parity = ((wave & 1) == h);                   // tiles wave + NWAVES*q share the wave's parity
    const bool sends = all_tiles || !my_parity, finishes = all_tiles || my_parity;
    float* xd_mine = pa.xd + ((size_t)pair * 2 + h) * (kPairXdAll * 2 * 256);
    const float* xd_theirs = pa.xd + ((size_t)pair * 2 + (h ^ 1)) * (kPairXdAll * 2 * 256);
    auto run = [&](auto ntw_tag) {
      constexpr int NTW = decltype(ntw_tag)::value;
      f32x4 acc[NTW > 0 ? NTW : 1][MT];
#pragma unroll
      for (int q = 0; q < (NTW > 0 ? NTW : 1); ++q)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[q][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (NTW > 0) {
        stream_mfma<NTW, 4, MT, true>(acc, wqd, d_w, cstride, wave, NWAVES, a.NTp, KH, xload, xmake);
        if (sends) {
#pragma unroll
          for (int q = 0; q < NTW; ++q) {
            const int t = wave + NWAVES * q;
            if (t < a.NTp) {
#pragma unroll
              for (int m = 0; m < MT; ++m) MKWS_XSTORE(reinterpret_cast<f32x4*>(xd_mine + ((size_t)(t * 2 + m) * 64 + lane) * 4), acc[q][m]);
            }
          }
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0 && *s_bad == 0) {
        const int got = pair_signal_wait(fl + 2 + h, fl + 2 + (h ^ 1), 1);
        if (got != 1) { *s_bad = 1; pair_report(pa.err_dev, pa.err_host, kPairErrTimeout); }
      }
      __syncthreads();
      if constexpr (NTW > 0) {
        if (finishes) {
          const bool bad = *s_bad != 0;
#pragma unroll
          for (int q = 0; q < NTW; ++q) {
            const int t = wave + NWAVES * q;
            const int n = t * 16 + 4 * g;
            if (t < a.NTp) {
              const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scP + n), sh = *reinterpret_cast<const f32x4*>(a.shP + n);
#pragma unroll
              for (int m = 0; m < MT; ++m) {
                const int r = m * 16 + c;
                const f32x4 other = ld_agent_x4(xd_theirs + ((size_t)(t * 2 + m) * 64 + lane) * 4);
                f32x4 y = ((h == 0) ? acc[q][m] + other : other + acc[q][m]) * sc + sh;
                if (a.residual) {
                  if (first) { if (r < rows) y += *reinterpret_cast<const f32x4*>(a.X + (row0 + r) * a.Cin + n); }
                  else if (q < 2) y += carry[q][m];            // (blocks inside a chain have at most 2 tiles per wave: host-checked)
                }
                if (bad) y = (f32x4){__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                if (!nx && r < rows) *reinterpret_cast<f32x4*>(a.Y + (row0 + r) * a.Cout + n) = y;
                if (r >= rows) y = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (q < 2) carry[q][m] = y;
                if (nx) *reinterpret_cast<f32x4*>(s_X + ((size_t)(t * MT + m) * 64 + lane) * 4) = y;
              }
            }
          }
        }
      }
    };
    if (d_ntw == 0) run(std::integral_constant<int, 0>{});
    else if (d_ntw == 1) run(std::integral_constant<int, 1>{});
    else if (d_ntw == 2) run(std::integral_constant<int, 2>{});
    else run(std::integral_constant<int, 3>{});
  }
  if (nx) __syncthreads();
}

// Last phase of the paired chain when the top conv is fused into it: [16 MT rows x K] . [K x 16 top_NT] + BN + swish + 2x2 average pool.
// Both halves hold block 7a's whole output as fragments in U; half h owns n-tiles [h * top_NT / 2, +top_NT / 2), wave w tiles w, w + 8, ...
// (five of them: one stream_mfma over five accumulator tiles x MT row tiles), so nothing is exchanged.  Same operations in the same order
// as pw_gemm_kernel<.., pool4>: chunk-ascending fp32 MFMA accumulation, acc * scale + shift, swish, (r0 + r1) + (r2 + r3) by two
// xor-shuffles, * 0.25 -- bit-identical pooled features.  Why it pays: the stand-alone top conv has K = 320, 20 chunks per wave: ring fill
// and epilogue are a third of its 38 us (0.55 of the MFMA roof); here its weights stream like another block's.
template <int MT, int NWAVES>
__device__ __forceinline__ void pair_top_phase(const PairChainArgs& pa, float* s_blk, int h, int pair) {
  constexpr int G = 4 * MT, NTW = 5;
  const int tid = opaque_((int)threadIdx.x), lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const unsigned loff = (unsigned)(g * 64 + c * 4);
  const int b0 = pair * G;
  const int NTh = pa.top_NT / 2;
  const float* s_X = s_blk;
  const WBuf w(pa.top_Wp, loff);
  f32x4 wq[4][NTW];
  f32x4 acc[NTW][MT];
#pragma unroll
  for (int q = 0; q < NTW; ++q)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[q][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto xload = [&](int j, int m) { return *reinterpret_cast<const f32x4*>(s_X + ((size_t)(j * MT + m) * 64 + lane) * 4); };
  auto xmake = [](const f32x4& v) { return v; };
  stream_mfma<NTW, 4, MT, false>(acc, wq, w, (size_t)pa.top_NT * 256, h * NTh + wave, NWAVES, (h + 1) * NTh, pa.top_KC, xload, xmake);
#pragma unroll
  for (int q = 0; q < NTW; ++q) {
    const int i = wave + NWAVES * q;                            // tile of this half
    const int n = (h * NTh + i) * 16 + 4 * g;
    const bool tok = i < NTh;                                   // (uniform)
    const f32x4 sc = *reinterpret_cast<const f32x4*>(pa.top_sc + (tok ? n : 0)), sh = *reinterpret_cast<const f32x4*>(pa.top_sh + (tok ? n : 0));
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      f32x4 y = acc[q][m] * sc + sh;                             // (one v_pk_fma, as in pw_gemm_kernel)
      y = swish4_(y);
      {
        // the pooling adds must NOT contract with swish's final multiply (fma(v, t, shuffled) would skip a rounding that pw_gemm_kernel,
        // whose activation sits behind a run-time switch, performs): 1-ulp differences in a fifth of the pooled features otherwise
#pragma clang fp contract(off)
        y.x += __shfl_xor(y.x, 1); y.y += __shfl_xor(y.y, 1); y.z += __shfl_xor(y.z, 1); y.w += __shfl_xor(y.w, 1);
        y.x += __shfl_xor(y.x, 2); y.y += __shfl_xor(y.y, 2); y.z += __shfl_xor(y.z, 2); y.w += __shfl_xor(y.w, 2);
      }
      const int clip = b0 + m * 4 + (c >> 2);
      if (tok && (c & 3) == 0 && clip < pa.B) *reinterpret_cast<f32x4*>(pa.gap + (size_t)clip * (16 * pa.top_NT) + n) = y * 0.25f;
    }
  }
}

template <int MT, int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void mbconv_pair_chain_kernel(PairChainArgs pa) {
  extern __shared__ __attribute__((aligned(16))) float s_blk[];
  constexpr int NTHR = NWAVES * 64;
  constexpr int HW = 4, G = 4 * MT;
  const BlockArgs* __restrict__ tab = pa.tab + pa.i0;
  const int h = (blockIdx.x >> 3) & 1, pair = (blockIdx.x >> 4) * 8 + (blockIdx.x & 7);
  const int b0 = pair * G;
  if (b0 >= pa.B) return;                                       // both halves of a padding pair leave together
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  xcc &= 0xf;
  if (pa.fault == 2 && h == 1) return;                          // test hook: the partner never arrives
  volatile int* s_bad = reinterpret_cast<volatile int*>(s_blk + pa.ldsU + pa.ldsE + pa.ldsZ - 4);
  if (tid == 0) *s_bad = __hip_atomic_load(pa.err_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int xcc_expect = 1 + (int)(pa.fault == 1 ? (xcc ^ 1u) : xcc);
  f32x4 carry[2][MT];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int m = 0; m < MT; ++m) carry[q][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    const int Cin = sgpr_(tab[0].Cin), KCe = sgpr_(tab[0].KCe), CH = sgpr_(tab[0].Cexp) / 2;
    const int gvalid = (pa.B - b0 < G) ? (pa.B - b0) : G;
    const int rows = gvalid * HW;
    const size_t row0 = (size_t)b0 * HW;
    float* s_X = s_blk;
    float* s_scE = s_blk + pa.ldsU + pa.ldsE;
    for (int jm = wave; jm < KCe * MT; jm += NWAVES) {
      const int j = jm / MT, m = jm - j * MT;
      const int r = m * 16 + c;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < rows && 16 * j + 4 * g < Cin) v = *reinterpret_cast<const f32x4*>(pa.X + (row0 + r) * Cin + 16 * j + 4 * g);
      *reinterpret_cast<f32x4*>(s_X + ((size_t)jm * 64 + lane) * 4) = v;
    }
    const float* scE = sgpr_(tab[0].scE) + h * CH; const float* shE = sgpr_(tab[0].shE) + h * CH;
    for (int i = tid; i < CH; i += NTHR) { s_scE[i] = scE[i]; s_scE[CH + i] = shE[i]; }
    __syncthreads();
  }
  for (int i = 0; i < pa.n; ++i) {
    BlockArgs a = sgpr_block_args(tab[i]);
    const bool last = (i + 1 == pa.n);
    a.X = pa.X; a.Y = pa.Y; a.B = pa.B;
    const BlockArgs* nxp = last ? tab + i : tab + i + 1;
    // with the top conv fused the last block hands its whole output to BOTH halves as fragments, like an inner block
    const bool hands_on = !last || pa.top_Wp != nullptr;
    if (((pa.kinds >> i) & 1u) == 0) pair_chain_block<5, MT, NWAVES>(a, nxp, hands_on, i == 0, i, pa, s_blk, h, pair, xcc_expect, xcc, carry);
    else pair_chain_block<3, MT, NWAVES>(a, nxp, hands_on, i == 0, i, pa, s_blk, h, pair, xcc_expect, xcc, carry);
  }
  if (pa.top_Wp != nullptr) pair_top_phase<MT, NWAVES>(pa, s_blk, h, pair);
}

// ------------------------------------------------------------------------------------------------
// Cluster kernel for the tiny-image blocks of SMALL-batch handles (live serving: one window at a time).  At batch 1 a whole-block
// kernel is one workgroup streaming the block's 0.75-2.2 MB of weights through ONE CU (~41 GB/s): 24-36 us per block, 11 blocks = 313
// of the 489 us a window costs (tools/latency_profile.py).  Here P workgroups on P CUs of one XCD share ONE 16-row tile (one clip of a
// 4x3 image, four clips of a 2x2 image) and split the block's expanded CHANNELS P ways -- P = 10 / 14 / 12 for Cexp = 480 / 672 / 1152,
// three or six 16-channel tiles per member: every CU pulls a tenth of the weights and the phases shrink towards their latencies.
//   A   expand: the member's KH = Cexp/(16 P) n-tiles            B   depthwise + SE means on its channels (local: depthwise is per channel)
//   C1  partial r over its channels -> exchange 1: all P partial r vectors are added in member order by everyone
//   C2  gate for its channels, applied in place                   D   partial projection over its K slice, ALL output tiles
//   exchange 2: output tile t is finished by member t % P (the P partials added in member order, BN, residual)
// Exchanges are the paired kernel's (plain stores, s_waitcnt vmcnt(0), barrier, relaxed agent-scope flag, L1-bypassing loads) with
// GENERATION flags instead of consumer resets (P - 1 readers per flag): a member reads its own flag g0 when it starts, publishes g0 + 1
// and waits for the others to show g0 + 1 -- all members took part in the same launches, so they agree on g0; nothing to reset, and a
// captured graph replays it.  Members of a cluster have linear workgroup ids that are congruent mod 8 (same XCD under the round-robin
// dispatch probed at create); every member checks the others' XCC ids and a poll limit, and a failure takes the paired kernel's
// exit: NaN output, sticky error words, handle moved to the plain whole-block kernels by the next mkws_embed_forward.
constexpr int kClusterPMax = 14, kClXc1 = 256, kClMaxTiles = 20, kClusterChMax = 192, kClFlagRow = 16;
constexpr int kClusterLdsFloats = 12 * 256 + 16 * (kClusterChMax + 4) + 4 * kClusterChMax + 4 * 52 + 2 * kClusterChMax + 48 * (kClusterChMax + 4) + 48 * kClusterChMax +
                                  27 * kClusterChMax;     // + depthwise taps [25][CH] and its BN scale / shift
struct ClusterArgs {
  BlockArgs b;
  const float* Wr;   // plain [Cexp][se]
  const float* We;   // plain [se][Cexp]
  float* xc1;        // [clusters][P][kClXc1]: 48 units x up to 4 clips of partial r; [255] = the member's XCC id
  float* xd;         // [clusters][P][kClMaxTiles][256]: partial projection tiles, lane-linear
  int* flags;        // [clusters][2 exchanges][kClFlagRow] generations
  int* err_dev; int* err_host; int fault;
  int P;             // members per cluster: 10 (Cexp 480), 14 (672), 12 (1152) -- Cexp / (16 P) whole tiles per member
};

// Wave 0 (all 64 lanes): lane p publishes generation `gen`, lanes q < P poll one member's flag each IN PARALLEL (one poll is an L2
// round trip of ~0.5 us: thirteen of them one after the other cost more than the phases they separate).  0 = ok, 1 = timed out.
__device__ __forceinline__ int cluster_signal_wait(int* row, int p, int P, int gen) {
  const int lane = threadIdx.x & 63;
  if (lane == p) __hip_atomic_store(row + p, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int spins = 0;
  while (true) {
    const int v = (lane < P && lane != p) ? __hip_atomic_load(row + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : gen;
    if (__builtin_amdgcn_ballot_w64(v != gen) == 0) return 0;
    __builtin_amdgcn_s_sleep(1);
    if (++spins > (1 << 21)) return 1;
  }
}

// Write-through (sc1) 16-byte accesses through a buffer descriptor: the hand-over of a block's output to the NEXT block's members inside one
// launch (mbconv_cluster_chain_kernel).  aux 16 = sc1: the store leaves the XCD's L2 for memory, the load bypasses the CU's L1 (Guideline 16, R1).
// The base must be wave-uniform.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
struct XBuf {
  __amdgpu_buffer_rsrc_t r;
  __device__ __forceinline__ explicit XBuf(const float* base) : r(__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, 0x7fffffff, 0x00020000)) {}
  __device__ __forceinline__ f32x4 ld(size_t idx) const { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (unsigned)(idx * 4u), 0, 16)); }
  __device__ __forceinline__ void st(size_t idx, const f32x4& v) const { __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (unsigned)(idx * 4u), 0, 16); }
};

// Wave 0 of a chained member: lanes q < P poll the previous block's `done` generations (one relaxed agent-scope load each).  0 = ok, 1 = timed out.
__device__ __forceinline__ int cluster_wait_done(int* row, int P, int gen) {
  const int lane = threadIdx.x & 63;
  int spins = 0;
  while (true) {
    const int v = (lane < P) ? __hip_atomic_load(row + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : gen;
    if (__builtin_amdgcn_ballot_w64(v != gen) == 0) return 0;
    __builtin_amdgcn_s_sleep(4);
    if (++spins > (1 << 20)) return 1;
  }
}

// One block of one cluster member.  CHAINED = false: the body of mbconv_cluster_kernel (one launch per block).  CHAINED = true: the body of
// mbconv_cluster_chain_kernel, where the members of ALL of a live window's tiny-image blocks start together: a member requests every weight it
// will need (expand ring, SE weights, taps, the whole projection ring) and parks the SE weights / taps in LDS BEFORE it waits for the previous
// block's `done` generations (wait_row, wait_P members), then reads the block input with L1-bypassing loads; its finishers store the output
// write-through (sc1) and every member publishes its `done` generation (done_row) -- Guideline 16's R1 form, valid for any XCD placement.
template <int KS, int S, int HT, int WT, bool CHAINED>
__device__ __forceinline__ void cluster_block(const ClusterArgs& ca, const int cl, const int p, float* s_cl, int& s_bad, int* wait_row, int wait_P, int* done_row) {
  constexpr int NTHR = 256, NW = 4;
  constexpr int HW = HT * WT, G = 16 / HW;                       // clips per cluster: 1 (4x3) or 4 (2x2)
  const int P = ca.P;
  constexpr int HoT = (S == 1) ? HT : (HT == 4 ? 2 : 1), WoT = (S == 1) ? WT : (WT == 3 ? 2 : 1), HoWo = HoT * WoT;
  constexpr int PT = (S == 1) ? KS / 2 : KS / 2 - (1 - HT % 2), PLF = (S == 1) ? KS / 2 : KS / 2 - (1 - WT % 2);
  constexpr int CHMAX = kClusterChMax, LDEMAX = CHMAX + 4, LDR = 52;
  float* s_X = s_cl;                                             // block input as B-operand fragments [KCe][64 lanes][4]
  float* s_E = s_X + 12 * 256;                                   // this member's expanded channels [16 rows][CH + 4]
  float* s_S = s_E + 16 * LDEMAX;                                // SE means [G][CH], later the gate
  float* s_R = s_S + 4 * CHMAX;                                  // r [G][52]
  float* s_sc = s_R + 4 * LDR;                                   // expand BN scale / shift of the member's channels
  float* s_sh = s_sc + CHMAX;
  float* s_Wr = s_sh + CHMAX;                                    // the member's rows of the SE-reduce weights, TRANSPOSED: [se][CH + 4]
  float* s_We = s_Wr + 48 * (CHMAX + 4);                         // its columns of the SE-expand weights [se][CH]
  float* s_Wd = s_We + 48 * CHMAX;                               // depthwise taps of its channels [KS*KS][CH], then BN scale [CH], shift [CH]
  const BlockArgs& a = ca.b;
  const int b0 = cl * G;
  if (b0 >= a.B) return;                                         // all members of a padding cluster leave together
  const int Cexp = a.Cexp, CH = Cexp / P, KH = CH / 16, chan0 = p * CH, LDE = CH + 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const unsigned loff = (unsigned)(g * 64 + c * 4);
  const int gvalid = (a.B - b0 < G) ? (a.B - b0) : G;
  const int rows_in = gvalid * HW, rows_out = gvalid * HoWo;
  const size_t row0_in = (size_t)b0 * HW, row0_out = (size_t)b0 * HoWo;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  xcc &= 0xf;
  int* frow = ca.flags + (size_t)cl * 2 * kClFlagRow;             // [2][kClFlagRow]
  float* xc1 = ca.xc1 + (size_t)cl * kClusterPMax * kClXc1;
  float* xd = ca.xd + (size_t)cl * kClusterPMax * kClMaxTiles * 256;
  if (ca.fault == 2 && p == 1) return;                           // test hook: a member never arrives
  if (tid == 0) s_bad = __hip_atomic_load(ca.err_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // sticky: an earlier launch failed
  // this launch's generations = the member's own last ones + 1 (uniform scalar loads; used by wave 0 at the exchanges)
  const int gen0 = __hip_atomic_load(frow + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
  const int gen1 = __hip_atomic_load(frow + kClFlagRow + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
  // chained: the hand-over generation.  Every chain launch runs every member of every block, so all `done` words of a handle agree between launches
  int genH = 0;
  if constexpr (CHAINED) genH = __hip_atomic_load(done_row + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
#ifdef MKWS_FRONT_TIMING
  const long long dbg_c0 = clock64();
  if (threadIdx.x == 0 && a.dbg_t) a.dbg_t[(size_t)blockIdx.x * 8 + 0] = wall_clock64();
#define MKWS_CL_STAMP(k) if (threadIdx.x == 0 && a.dbg_t) a.dbg_t[(size_t)blockIdx.x * 8 + (k)] = wall_clock64();
#else
#define MKWS_CL_STAMP(k)
#endif
  // ---- stage: input tile as fragments + expand BN constants (phase A needs them) -> LDS now; the SE weights and depthwise taps of
  //      the member's channels (phases B / C) are REQUESTED now and stored to LDS after phase A: they travel while the expand runs.
  //      Every global load is issued before the first LDS store (fixed trip counts, predicated): a load -> store loop pays one
  //      memory latency per iteration (9 iterations = 9 us measured) ----
  const int LDW = CH + 4;
  constexpr int NX = 3, NR = 9, NE = 9, ND = 6;                   // float4 per thread: X (12 chunks / 4 waves), Wr, We (48 * 192 / 4 / 256), taps (27 * 48 / 256)
  f32x4 rr[NR], re[NE], rd[ND];
  const int nWr = (a.se & 3) == 0 ? CH * a.se / 4 : 0, nWe = a.se * (CH / 4), nWd = (KS * KS + 2) * (CH / 4);
  constexpr int NTWA = (HW == 4) ? 2 : 1;                         // expand: KH = 6 tiles per member (2x2 images, 12 members) / 3 (4x3, 10 or 14): one run per wave
  const int a_ngroups = (KH + NTWA - 1) / NTWA;
  const int a_nruns = (a_ngroups > wave) ? (a_ngroups - wave + NW - 1) / NW : 0;
  auto a_tile_of = [&](int r) { return p * KH + (wave + NW * r) * NTWA; };
  f32x4 wqa[12][NTWA];                                             // the whole run (<= 12 chunks x NTWA fragments) in flight: one latency
  // phase D's weight ring: chained members hold their WHOLE K slice (KH = 3 chunks for Cexp / P = 48, 6 for 96) from before the wait
  constexpr int DD = CHAINED ? ((HW == 4) ? 6 : 3) : 4;
  f32x4 wqd[DD][5];
  const WBuf d_w(a.WpP + (size_t)(p * KH) * a.NTp * 256, loff);
  const int d_ntw = (a.NTp > wave) ? (a.NTp - wave + NW - 1) / NW : 0;
  // the SE weights / depthwise taps requested below go to LDS: after phase A (they travel under the expand), or -- chained -- before the wait
  auto park = [&]() {
#pragma unroll
    for (int k = 0; k < NR; ++k) {                                    // Wr [CH][se] -> transposed [se][CH + 4]; float4 = 4 units of one channel (se % 4 == 0)
      const int i = tid + NTHR * k;
      if (i < nWr) {
        const int ch = (4 * i) / a.se, n = 4 * i - ch * a.se;
#pragma unroll
        for (int q = 0; q < 4; ++q) s_Wr[(n + q) * LDW + ch] = rr[k][q];
      }
    }
    if ((a.se & 3) != 0)
      for (int i = tid; i < CH * a.se; i += NTHR) { const int ch = i / a.se, n = i - ch * a.se; s_Wr[n * LDW + ch] = ca.Wr[(size_t)chan0 * a.se + i]; }
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      const int i = tid + NTHR * k;
      if (i < nWe) { const int n = i / (CH / 4), q4 = (i - n * (CH / 4)) * 4; *reinterpret_cast<f32x4*>(s_We + (size_t)n * CH + q4) = re[k]; }
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) {
      const int i = tid + NTHR * k;
      if (i < nWd) { const int t = i / (CH / 4), q4 = (i - t * (CH / 4)) * 4; *reinterpret_cast<f32x4*>(s_Wd + (size_t)t * CH + q4) = rd[k]; }
    }
    // phase D's weight stream (K = the member's KH chunks, tiles wave, wave + 4, ...) is requested now: it lands under phases B and C
    if (d_ntw > 0) stream_mfma_prefetch<5, DD>(wqd, d_w, (size_t)a.NTp * 256, wave, NW, a.NTp, KH);
  };
  {
    f32x4 rx[NX];
    if constexpr (!CHAINED) {
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        const int j = wave + NW * k;
        rx[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (j < a.KCe && c < rows_in && 16 * j + 4 * g < a.Cin) rx[k] = *reinterpret_cast<const f32x4*>(a.X + (row0_in + c) * a.Cin + 16 * j + 4 * g);
      }
    }
    float sce = 0.0f, she = 0.0f;
    if (tid < CH) { sce = a.scE[chan0 + tid]; she = a.shE[chan0 + tid]; }       // CH <= 192 < NTHR
    // the expand's weight ring is requested BEFORE the SE weights / taps: loads return in order, so the other way round the first
    // expand fragment would arrive behind ~100 KB that nobody needs before phase B
    stream_mfma_runs_prefetch<NTWA, 12>(wqa, WBuf(a.WpE, loff), (size_t)a.NTe * 256, a.NTe, a_nruns, a.KCe, a_tile_of);
#pragma unroll
    for (int k = 0; k < NR; ++k) { const int i = tid + NTHR * k; if (i < nWr) rr[k] = *reinterpret_cast<const f32x4*>(ca.Wr + (size_t)chan0 * a.se + 4 * i); }
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      const int i = tid + NTHR * k;
      if (i < nWe) { const int n = i / (CH / 4), q4 = (i - n * (CH / 4)) * 4; re[k] = *reinterpret_cast<const f32x4*>(ca.We + (size_t)n * Cexp + chan0 + q4); }
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) {
      const int i = tid + NTHR * k;
      if (i < nWd) {
        const int t = i / (CH / 4), q4 = (i - t * (CH / 4)) * 4;
        const float* src = (t < KS * KS) ? a.Wd + (size_t)t * Cexp : (t == KS * KS ? a.scD : a.shD);
        rd[k] = *reinterpret_cast<const f32x4*>(src + chan0 + q4);
      }
    }
    if (tid < CH) { s_sc[tid] = sce; s_sh[tid] = she; }
    if constexpr (CHAINED) {
      // every weight of the block is requested; the SE weights / taps wait in LDS, the two rings in registers.  Now the block input: published by
      // ALL members of the previous block (its finishers stored the tiles write-through before their `done` word).  The chain's FIRST block has
      // nobody to wait for and its weights are on the critical path: it keeps the per-block kernel's order (input first, park behind the expand)
      if (wait_row != nullptr) park();
      __syncthreads();                                               // (s_bad is set)
      if (wait_row != nullptr) {
        if (wave == 0 && s_bad == 0) {
          const int to = cluster_wait_done(wait_row, wait_P, genH);
          if (to && lane == 0) { s_bad = 1; pair_report(ca.err_dev, ca.err_host, kPairErrTimeout); }
        }
        __syncthreads();
      }
      MKWS_CL_STAMP(7)
      const XBuf xin(a.X);
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        const int j = wave + NW * k;
        rx[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (j < a.KCe && c < rows_in && 16 * j + 4 * g < a.Cin) rx[k] = xin.ld((row0_in + c) * a.Cin + 16 * j + 4 * g);
      }
    }
#pragma unroll
    for (int k = 0; k < NX; ++k) { const int j = wave + NW * k; if (j < a.KCe) *reinterpret_cast<f32x4*>(s_X + ((size_t)j * 64 + lane) * 4) = rx[k]; }
  }
  __syncthreads();
  MKWS_CL_STAMP(1)
  // ---- A: expand: runs of NTWA tiles (independent accumulators: one accumulator per wave would wait out the MFMA's dependent
  //      latency on every k step) dealt over the four waves; the ring was requested during the staging ----
  {
    auto xload = [&](int j, int) { return *reinterpret_cast<const f32x4*>(s_X + ((size_t)j * 64 + lane) * 4); };
    auto xmake = [](const f32x4& v) { return v; };
    auto epi = [&](int t0, const f32x4 (&acc)[NTWA][1]) {
#pragma unroll
      for (int q = 0; q < NTWA; ++q) {
        const int tl = t0 + q - p * KH;                           // tile inside the member's slice (a run's tail may reach past it)
        if (tl < KH) {
          const int n = tl * 16 + 4 * g;
          f32x4 y = acc[q][0] * *reinterpret_cast<const f32x4*>(s_sc + n) + *reinterpret_cast<const f32x4*>(s_sh + n);
          y = swish4_(y);
          if (c >= rows_in) y = (f32x4){0.f, 0.f, 0.f, 0.f};
          *reinterpret_cast<f32x4*>(s_E + (size_t)c * LDE + n) = y;
        }
      }
    };
    if (HW == 4 && a.KCe == 12) {
      // 2x2 blocks (Cin = 192): ONE run per wave whose whole K sits in the ring -- straight-line code.  The general helper walks run-time
      // (run, chunk) cursors with a conditional epilogue behind every ring slot: ~30 scalar / accumulator-shuffle instructions per 8 MFMAs
      // (ISA, round 6), which a one-clip window cannot hide.  Same accumulation order per tile: bit-identical.
      if (a_nruns == 1) {
        f32x4 acc[NTWA][1];
#pragma unroll
        for (int q = 0; q < NTWA; ++q) acc[q][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 xr = xload(0, 0);
#pragma unroll
        for (int d = 0; d < 12; ++d) {
          const f32x4 xn = xload(d + 1 < 12 ? d + 1 : d, 0);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int q = 0; q < NTWA; ++q) acc[q][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wqa[d][q][s4], xr[s4], acc[q][0], 0, 0, 0);
          xr = xn;
        }
        epi(a_tile_of(0), acc);
      }
    } else {
      stream_mfma_runs<NTWA, 12, 1, true>(wqa, WBuf(a.WpE, loff), (size_t)a.NTe * 256, a.NTe, a_nruns, a.KCe, a_tile_of, xload, xmake, epi);
    }
  }
  // the SE weights / depthwise taps requested before phase A go to LDS now (chained members parked them before the wait)
  if (!CHAINED || wait_row == nullptr) park();
  __syncthreads();
  MKWS_CL_STAMP(2)
  // ---- B: depthwise + BN + swish in place, SE means (thread = clip x channel quad of the member's slice) ----
  {
    const int Q = CH / 4;
    for (int task = tid; task < G * Q; task += NTHR) {
      const int gi = task / Q, q4 = (task - gi * Q) * 4;
      float* Eg = s_E + (size_t)gi * HW * LDE + q4;
      f32x4 ein[HW];
#pragma unroll
      for (int pix = 0; pix < HW; ++pix) ein[pix] = *reinterpret_cast<const f32x4*>(Eg + (size_t)pix * LDE);
      f32x4 acc[HoWo];
#pragma unroll
      for (int o = 0; o < HoWo; ++o) acc[o] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < KS; ++i) {
#pragma unroll
        for (int jx = 0; jx < KS; ++jx) {
          bool used = false;
#pragma unroll
          for (int oh = 0; oh < HoT; ++oh)
#pragma unroll
            for (int ow = 0; ow < WoT; ++ow) {
              const int ih = oh * S - PT + i, iw = ow * S - PLF + jx;
              used |= (ih >= 0 && ih < HT && iw >= 0 && iw < WT);
            }
          if (!used) continue;
          const f32x4 wv = *reinterpret_cast<const f32x4*>(s_Wd + (size_t)(i * KS + jx) * CH + q4);
#pragma unroll
          for (int oh = 0; oh < HoT; ++oh)
#pragma unroll
            for (int ow = 0; ow < WoT; ++ow) {
              const int ih = oh * S - PT + i, iw = ow * S - PLF + jx;
              if (ih >= 0 && ih < HT && iw >= 0 && iw < WT) acc[oh * WoT + ow] += ein[ih * WT + iw] * wv;
            }
        }
      }
      const f32x4 sc = *reinterpret_cast<const f32x4*>(s_Wd + (size_t)(KS * KS) * CH + q4), sh = *reinterpret_cast<const f32x4*>(s_Wd + (size_t)(KS * KS + 1) * CH + q4);
      f32x4 ssum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < HoWo; ++o) {
        f32x4 y = acc[o] * sc + sh;
        y = swish4_(y);
        if (gi >= gvalid) y = (f32x4){0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(Eg + (size_t)o * LDE) = y;     // output o of clip gi lives in row gi*HW + o (in place)
        ssum += y;
        if (a.dbg_dw && gi < gvalid) *reinterpret_cast<f32x4*>(a.dbg_dw + (row0_out + gi * HoWo + o) * Cexp + chan0 + q4) = y;
      }
      *reinterpret_cast<f32x4*>(s_S + (size_t)gi * CH + q4) = ssum * (1.0f / (float)HoWo);
    }
  }
  __syncthreads();
  MKWS_CL_STAMP(3)
  // ---- C1: partial r[unit n][clip] over the member's channels (thread = (n, clip), a.se <= 48), published for exchange 1 ----
  if (tid < 48 * G) {
    const int n = tid / G, clip = tid - n * G;
    float v = 0.0f;
    if (n < a.se) {
      const float* wr = s_Wr + n * LDW;
      const float* mrow = s_S + (size_t)clip * CH;
      f32x4 acc4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int ch = 0; ch < CH; ch += 4) acc4 += *reinterpret_cast<const f32x4*>(mrow + ch) * *reinterpret_cast<const f32x4*>(wr + ch);
      v = (acc4.x + acc4.y) + (acc4.z + acc4.w);
    }
    xc1[(size_t)p * kClXc1 + tid] = v;
  }
  if (tid == 255) xc1[(size_t)p * kClXc1 + 255] = (float)(ca.fault == 1 && p == 1 ? (xcc ^ 1u) : xcc);
  const float br_pre = (tid < 48 * G && tid / G < a.se) ? a.br[tid / G] : 0.0f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (wave == 0 && s_bad == 0) {
    const int to = cluster_signal_wait(frow, p, P, gen0);
    if (to && lane == 0) { s_bad = 1; pair_report(ca.err_dev, ca.err_host, kPairErrTimeout); }
  }
  __syncthreads();
  if (tid < 48 * G) {
    const int n = tid / G, clip = tid - n * G;
    float v = 0.0f;
    if (n < a.se) {
      float part[kClusterPMax];                                     // all members' partials requested together, added in member order
#pragma unroll
      for (int q = 0; q < kClusterPMax; ++q) part[q] = (q < P) ? __hip_atomic_load(xc1 + (size_t)q * kClXc1 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
#pragma unroll
      for (int q = 0; q < kClusterPMax; ++q) v += part[q];
      v = swishf_(v + br_pre);
    }
    s_R[clip * LDR + n] = v;
  }
  if (wave == 3 && s_bad == 0) {                                     // lane q checks member q's XCC id
    const unsigned theirs = (lane < P) ? (unsigned)__hip_atomic_load(xc1 + (size_t)lane * kClXc1 + 255, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : xcc;
    if (__builtin_amdgcn_ballot_w64(theirs != xcc) != 0 && lane == 0) { s_bad = 1; pair_report(ca.err_dev, ca.err_host, kPairErrXcc); }
  }
  __syncthreads();
  MKWS_CL_STAMP(4)
  // ---- C2: gate of the member's channels (thread = (clip, channel)), applied to the depthwise output in place ----
  for (int t = tid; t < G * (CH / 4); t += NTHR) {                  // thread = (clip, channel quad)
    const int clip = t / (CH / 4), ch = (t - clip * (CH / 4)) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const float* we = s_We + ch;
    const float* rr = s_R + clip * LDR;
#pragma unroll 4
    for (int n = 0; n < a.se; ++n) v += *reinterpret_cast<const f32x4*>(we + n * CH) * rr[n];
    v = sigmoid4_(v + *reinterpret_cast<const f32x4*>(a.be + chan0 + ch));
    *reinterpret_cast<f32x4*>(s_S + (size_t)clip * CH + ch) = v;
    if (a.dbg_gate && clip < gvalid) *reinterpret_cast<f32x4*>(a.dbg_gate + (size_t)(b0 + clip) * Cexp + chan0 + ch) = v;
  }
  __syncthreads();
  {
    const int Q = CH / 4;
    for (int i = tid; i < G * HoWo * Q; i += NTHR) {
      const int ro = i / Q, q4 = (i - ro * Q) * 4;
      const int clip = ro / HoWo;
      float* e = s_E + (size_t)(clip * HW + (ro - clip * HoWo)) * LDE + q4;
      *reinterpret_cast<f32x4*>(e) = *reinterpret_cast<const f32x4*>(e) * *reinterpret_cast<const f32x4*>(s_S + (size_t)clip * CH + q4);
    }
  }
  __syncthreads();
  MKWS_CL_STAMP(5)
  // ---- D: partial projection over the member's K (KH chunks), every output tile; tiles wave, wave + 4, ... (at most 5 per wave) ----
  {
    int r = c;
    if (r >= G * HoWo) r = G * HoWo - 1;
    const int clip = r / HoWo;
    const float* erow = s_E + (size_t)(clip * HW + (r - clip * HoWo)) * LDE + 4 * g;
    auto xload = [&](int j, int) { return *reinterpret_cast<const f32x4*>(erow + 16 * j); };
    auto xmake = [](const f32x4& v) { return v; };
    const size_t cstride = (size_t)a.NTp * 256;
    auto run = [&](auto ntw_tag) {                                  // this wave's tiles wave, wave + 4, ...: one pass over K for all of them
      constexpr int NTW = decltype(ntw_tag)::value;
      f32x4 acc[NTW][1];
#pragma unroll
      for (int q = 0; q < NTW; ++q) acc[q][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
      stream_mfma<NTW, DD, 1, true>(acc, wqd, d_w, cstride, wave, NW, a.NTp, KH, xload, xmake);
#pragma unroll
      for (int q = 0; q < NTW; ++q) {
        const int t = wave + NW * q;
        if (t < a.NTp) *reinterpret_cast<f32x4*>(xd + ((size_t)(p * kClMaxTiles + t) * 64 + lane) * 4) = acc[q][0];
      }
    };
    if (d_ntw == 1) run(std::integral_constant<int, 1>{});
    else if (d_ntw == 2) run(std::integral_constant<int, 2>{});
    else if (d_ntw == 3) run(std::integral_constant<int, 3>{});
    else if (d_ntw == 4) run(std::integral_constant<int, 4>{});
    else if (d_ntw >= 5) run(std::integral_constant<int, 5>{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (wave == 0 && s_bad == 0) {
    const int to = cluster_signal_wait(frow + kClFlagRow, p, P, gen1);
    if (to && lane == 0) { s_bad = 1; pair_report(ca.err_dev, ca.err_host, kPairErrTimeout); }
  }
  __syncthreads();
  // ---- exchange 2: member t % P finishes output tile t (partials of all members in member order) ----
  {
    const bool bad = s_bad != 0;
    for (int k = wave; p + P * k < a.NTp; k += NW) {
      const int t = p + P * k;
      f32x4 v = {0.f, 0.f, 0.f, 0.f}, part[kClusterPMax];
#pragma unroll
      for (int q = 0; q < kClusterPMax; ++q) part[q] = (q < P) ? ld_agent_x4(xd + ((size_t)(q * kClMaxTiles + t) * 64 + lane) * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < kClusterPMax; ++q) v += part[q];
      const int n = t * 16 + 4 * g;
      if (c < rows_out) {
        f32x4 y = v * *reinterpret_cast<const f32x4*>(a.scP + n) + *reinterpret_cast<const f32x4*>(a.shP + n);
        if constexpr (CHAINED) {
          if (a.residual) y += XBuf(a.X).ld((row0_in + c) * a.Cin + n);
          if (bad) y = (f32x4){__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
          XBuf(a.Y).st((row0_out + c) * a.Cout + n, y);
        } else {
          if (a.residual) y += *reinterpret_cast<const f32x4*>(a.X + (row0_in + c) * a.Cin + n);
          if (bad) y = (f32x4){__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
          *reinterpret_cast<f32x4*>(a.Y + (row0_out + c) * a.Cout + n) = y;
        }
      }
    }
  }
  if constexpr (CHAINED) {
    // publish: every storing wave drains its write-through stores, then ONE lane shows this member's generation (members without a tile to
    // finish publish too: the next block waits for all P words, which also tells it that nobody still reads the exchange buffers)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(done_row + p, genH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#ifdef MKWS_FRONT_TIMING
  __syncthreads();
  if (threadIdx.x == 0 && a.dbg_t) { a.dbg_t[(size_t)blockIdx.x * 8 + 6] = wall_clock64(); if (!CHAINED) a.dbg_t[(size_t)blockIdx.x * 8 + 7] = (unsigned long long)(clock64() - dbg_c0); }
#endif
#undef MKWS_CL_STAMP
}

template <int KS, int S, int HT, int WT>
__global__ __launch_bounds__(256) void mbconv_cluster_kernel(ClusterArgs ca) {
  extern __shared__ __attribute__((aligned(16))) float s_cl[];    // kClusterLdsFloats, carved for the largest block (CH = 192, 12 K chunks)
  __shared__ int s_bad;
  const int P = ca.P;
  const int cl = (blockIdx.x / (8 * P)) * 8 + (blockIdx.x & 7), p = (blockIdx.x >> 3) % P;
  cluster_block<KS, S, HT, WT, false>(ca, cl, p, s_cl, s_bad, nullptr, 0, nullptr);
}

// ------------------------------------------------------------------------------------------------
// The tiny-image blocks 4b .. 7a of ONE live window as one launch (one-clip handles, option "fuse_cluster_chain").  Launch by launch, every
// block's 10-14 members spend the first 4-7 us of their 13-23 us waiting for ~200 KB of weights each (one CU pulls lines that miss L2 at
// ~13 GB/s, whatever the order), and only one block's members pull at a time.  Here the members of ALL ten blocks (120 workgroups on 120 CUs)
// start together and request everything they will need at once -- 12 MB arrive over 120 CUs while the first block computes -- and a block
// starts on resident operands the moment the previous one publishes its output (cluster_block<CHAINED>).
// Placement: block k's members sit on XCD k % 8 (ids base[k] + 8 m + k % 8 under the round-robin dispatch probed at create; the other ids
// of the range leave at once), so that a block's two exchanges stay inside one L2; the hand-over between blocks is write-through and
// placement-free.  A member only ever waits for workgroups with LOWER ids or of its own block: the in-order dispatch cannot deadlock a lone
// launch.  (Several chain launches at once on a crowded chip can starve each other; the waits are bounded and end in the exchange-failure
// contract of the paired kernels: NaN output, sticky error word, the handle leaves the cluster plan.)
constexpr int kClusterChainMax = 10;
struct ClusterChainArgs {
  const BlockArgs* tab;                // device table of the plan's block constants (see ChainArgs)
  int i0, n;                           // blocks i0 .. i0 + n - 1
  unsigned kinds;                      // 3 bits per position: 0 = <3,1,4,3>, 1 = <5,1,4,3>, 2 = <5,2,4,3>, 3 = <5,1,2,2>, 4 = <3,1,2,2>
  float* buf0; float* buf1;            // block j reads buf[j & 1] and writes buf[(j + 1) & 1]
  const float* Wr[kClusterChainMax];   // plain SE weights of every block
  const float* We[kClusterChainMax];
  int base[kClusterChainMax + 1];      // first workgroup id of every block (multiples of 8)
  signed char P[kClusterChainMax];
  float* xc1; float* xd;               // exchange buffers: block k uses cluster slot k -- NOT one slot for all: the blocks sit on different XCDs, and two
                                       // L2s holding dirty copies of one line write them back in any order (seen as silently wrong windows beside a second
                                       // handle's traffic, tools/chain_concurrency_probe.py)
  int* flags; int flag_stride;         // per-block flag region (ints): rows 0 / 1 of cluster slot 0 = the exchanges, row 0 of slot 1 = `done`
  int* err_dev; int* err_host; int fault;
#ifdef MKWS_FRONT_TIMING
  unsigned long long* dbg_t;
#endif
};

__global__ __launch_bounds__(256) void mbconv_cluster_chain_kernel(ClusterChainArgs cc) {
  extern __shared__ __attribute__((aligned(16))) float s_cl[];
  __shared__ int s_bad;
  int k = 0;
  while (k + 1 < cc.n && (int)blockIdx.x >= cc.base[k + 1]) ++k;
  const int r = (int)blockIdx.x - cc.base[k];
  if ((r & 7) != (k & 7)) return;                                  // not on this block's XCD
  const int p = r >> 3;
  ClusterArgs ca;
  ca.b = sgpr_block_args(cc.tab[cc.i0 + k]);
  ca.b.X = (k & 1) ? cc.buf1 : cc.buf0;
  ca.b.Y = (k & 1) ? cc.buf0 : cc.buf1;
  ca.b.B = 1;
  ca.b.dbg_dw = nullptr; ca.b.dbg_gate = nullptr;
#ifdef MKWS_FRONT_TIMING
  ca.b.dbg_t = cc.dbg_t;
#endif
  ca.Wr = cc.Wr[k]; ca.We = cc.We[k];
  ca.xc1 = cc.xc1 + (size_t)k * kClusterPMax * kClXc1; ca.xd = cc.xd + (size_t)k * kClusterPMax * kClMaxTiles * 256;
  ca.flags = cc.flags + (size_t)(cc.i0 + k) * cc.flag_stride;
  ca.err_dev = cc.err_dev; ca.err_host = cc.err_host; ca.fault = cc.fault;
  ca.P = cc.P[k];
  int* done = ca.flags + 2 * kClFlagRow;                           // cluster slot 1, row 0 (a one-clip handle only ever runs cluster 0)
  int* wait = (k > 0) ? cc.flags + (size_t)(cc.i0 + k - 1) * cc.flag_stride + 2 * kClFlagRow : nullptr;
  const int wait_P = (k > 0) ? cc.P[k - 1] : 0;
  switch ((cc.kinds >> (3 * k)) & 7u) {
    case 0: cluster_block<3, 1, 4, 3, true>(ca, 0, p, s_cl, s_bad, wait, wait_P, done); break;
    case 1: cluster_block<5, 1, 4, 3, true>(ca, 0, p, s_cl, s_bad, wait, wait_P, done); break;
    case 2: cluster_block<5, 2, 4, 3, true>(ca, 0, p, s_cl, s_bad, wait, wait_P, done); break;
    case 3: cluster_block<5, 1, 2, 2, true>(ca, 0, p, s_cl, s_bad, wait, wait_P, done); break;
    default: cluster_block<3, 1, 2, 2, true>(ca, 0, p, s_cl, s_bad, wait, wait_P, done); break;
  }
}

// ------------------------------------------------------------------------------------------------
// SE: mean = sums/HW; r = swish(mean @ Wr + br); gate = sigmoid(r @ We + be).
// Both FCs run on the fp32 MFMA as (weights x 16 clips) tiles with pack_gemm-packed weights, and both are
// spread over the whole chip (a single block per 16 clips would stream up to 442 KB of SE weights through
// one CU):
//   se_reduce_kernel  grid (B/16, nslices): K = C is split across blocks (and the 4 waves of a block);
//                     raw partial r^T[se, 16] tiles go to a small global buffer (fixed-order, no atomics)
//   se_expand_kernel  grid (B/16, nsplit):  sums the partials (+bias, swish), then computes its share of
//                     the C/16 output row tiles of gate^T[C, 16] = We^T[C, se] . r^T[se, 16]
template <int NTR>
__global__ __launch_bounds__(256) void se_reduce_kernel(const float* __restrict__ sums, float inv_hw, const float* __restrict__ WrP,
                                                        float* __restrict__ part, int B, int C, int KCr, int nslices) {
  __shared__ float s_part[4 * NTR * 256];
  const int b0 = blockIdx.x * 16, z = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform by construction: keeps wave-dependent offsets / branches on the scalar unit
  const int g = lane >> 4, c = lane & 15;
  const int per = (KCr + nslices - 1) / nslices;
  const int j0 = z * per;
  const int j1 = (j0 + per < KCr) ? j0 + per : KCr;
  const bool clip_ok = b0 + c < B;
  const float* srow = sums + (size_t)(clip_ok ? b0 + c : 0) * C + 4 * g;
  const float* wbase = WrP + (size_t)g * 64 + c * 4;
  f32x4 acc[NTR];
#pragma unroll
  for (int nt = 0; nt < NTR; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int U = 3;            // chunks per wave issued together (per <= 9 chunks, 4 waves)
  for (int jb = j0 + wave; jb < j1; jb += 4 * U) {
    f32x4 wv[U][NTR], xb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = jb + 4 * u;
      const bool ok = j < j1;
#pragma unroll
      for (int nt = 0; nt < NTR; ++nt)
        wv[u][nt] = ok ? *reinterpret_cast<const f32x4*>(wbase + ((size_t)j * NTR + nt) * 256) : (f32x4){0.f, 0.f, 0.f, 0.f};
      xb[u] = (ok && clip_ok && 16 * j + 4 * g < C) ? *reinterpret_cast<const f32x4*>(srow + 16 * j) * inv_hw : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int nt = 0; nt < NTR; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u][nt][s], xb[u][s], acc[nt], 0, 0, 0);
  }
#pragma unroll
  for (int nt = 0; nt < NTR; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) s_part[((wave * NTR + nt) * 16 + 4 * g + r) * 16 + c] = acc[nt][r];
  __syncthreads();
  float* dst = part + ((size_t)z * gridDim.x + blockIdx.x) * NTR * 256;
  for (int t = tid; t < NTR * 256; t += 256)
    dst[t] = (s_part[t] + s_part[NTR * 256 + t]) + (s_part[2 * NTR * 256 + t] + s_part[3 * NTR * 256 + t]);
}

template <int NTR>
__global__ __launch_bounds__(256) void se_expand_kernel(const float* __restrict__ part, int nslices, const float* __restrict__ br,
                                                        const float* __restrict__ WeP, const float* __restrict__ be,
                                                        float* __restrict__ gate, int B, int C, int se, int NTe, int nsplit) {
  constexpr int LDR = NTR * 16 + 4;
  __shared__ __attribute__((aligned(16))) float s_r[16 * LDR];
  const int b0 = blockIdx.x * 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform by construction: keeps wave-dependent offsets / branches on the scalar unit
  const int g = lane >> 4, c = lane & 15;
  for (int t = tid; t < NTR * 256; t += 256) {
    const int n = t >> 4, clip = t & 15;
    float v = 0.0f;
    if (n < se) {
      for (int z = 0; z < nslices; ++z) v += part[((size_t)z * gridDim.x + blockIdx.x) * NTR * 256 + t];
      v = swishf_(v + br[n]);
    }
    s_r[clip * LDR + n] = v;
  }
  __syncthreads();
  f32x4 rb[NTR];
#pragma unroll
  for (int jj = 0; jj < NTR; ++jj) rb[jj] = *reinterpret_cast<const f32x4*>(s_r + c * LDR + 16 * jj + 4 * g);
  const int tper = (NTe + nsplit - 1) / nsplit;
  const int t0 = blockIdx.y * tper;
  const int t1 = (t0 + tper < NTe) ? t0 + tper : NTe;
  constexpr int U = 3;
  for (int tb = t0 + wave; tb < t1; tb += 4 * U) {
    f32x4 wv[U][NTR], bias[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = tb + 4 * u;
      const bool ok = t < t1;
#pragma unroll
      for (int jj = 0; jj < NTR; ++jj)
        wv[u][jj] = ok ? *reinterpret_cast<const f32x4*>(WeP + (((size_t)jj * NTe + t) * 4 + g) * 64 + c * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
      bias[u] = (ok && t * 16 + 4 * g < C) ? *reinterpret_cast<const f32x4*>(be + t * 16 + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = tb + 4 * u;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int jj = 0; jj < NTR; ++jj)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u][jj][s], rb[jj][s], acc, 0, 0, 0);
      const int n = t * 16 + 4 * g;
      if (t < t1 && n < C && b0 + c < B) {
        f32x4 y = acc + bias[u];
        y = sigmoid4_(y);
        *reinterpret_cast<f32x4*>(gate + (size_t)(b0 + c) * C + n) = y;
      }
    }
  }
}

// global average pool: X [B, HW, C] -> Y [B, C]
__global__ __launch_bounds__(256) void mean_hw_kernel(const float* __restrict__ X, float* __restrict__ Y, int B, int HW, int C) {
  const int cq = C / 4;
  const long total = (long)B * cq;
  const float inv = 1.0f / (float)HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int b = (int)(i / cq), q = (int)(i % cq);
    const float* p = X + (size_t)b * HW * C + q * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < HW; ++k) s += *reinterpret_cast<const f32x4*>(p + (size_t)k * C);
    *reinterpret_cast<f32x4*>(Y + (size_t)b * C + q * 4) = s * inv;
  }
}

// ================================================================================================
// host side
// ================================================================================================
struct GemmLayer {   // device pointers into the weight blob
  const float* Wp = nullptr; const float* scale = nullptr; const float* shift = nullptr;
  int K = 0, N = 0, KC = 0, NTtot = 0;
};
struct DwLayer { const float* Wd = nullptr; const float* scale = nullptr; const float* shift = nullptr; };
struct SeLayer { const float* Wr = nullptr; const float* We = nullptr; const float* WrP = nullptr; const float* br = nullptr; const float* WeP = nullptr; const float* be = nullptr; int se = 0, KCr = 0, NTR = 0, NTe = 0;
                 const float* WrQ = nullptr; const float* WeQ = nullptr; int T0 = 0, NQ = 0; };   // 4x4x1-instruction packing (Se4), 4x3-image blocks only

struct BlockPlan {
  MBConvSpec spec;
  int ce, H, W, Ho, Wo, pt, pl;
  bool has_expand, residual;
  GemmLayer expand, project;
  DwLayer dw;
  SeLayer se;
};

}  // namespace mkws

using namespace mkws;

constexpr uint32_t kGuardCanary = 0x7FC00BADu;      // a quiet NaN with a recognisable payload

struct mkws_embed {
  int max_batch = 0;
  int plan_batch = 0;             // the batch size whose WORKGROUP SHAPES the tiny-image kernels of this handle use: max_batch, or -- option "plan_batch" -- the clips
                                  // that L handles running concurrently on L streams hold together (serving lanes: each of those launches then takes 1 / L of the chip)
  int device = 0;
  float* d_weights = nullptr;     // packed device weights
  float* d_ws = nullptr;          // workspace
  // guard-band mode (MKWS_EMBED_GUARD=<floats> in the environment at create; tests/test_guard_bands_gpu.py): the whole workspace starts as a NaN
  // canary pattern and every carved sub-buffer is followed (the first one also preceded) by `guard` floats that no kernel may touch
  size_t guard = 0;
  std::vector<std::pair<size_t, size_t>> guard_spans;   // (offset into d_ws, floats)
  // workspace carve (floats per clip in parentheses)
  float *bufA = nullptr, *bufB = nullptr;   // block in/out ping-pong (16000)
  float *bufE = nullptr;                    // expand output (48000)
  float *bufD = nullptr;                    // depthwise output (18720)
  float *sums = nullptr, *gate = nullptr;   // (1152 each)
  float *gap = nullptr, *d0 = nullptr, *d1 = nullptr;   // (1280, 2048, 2048)
  float* se_part = nullptr;                              // SE reduce partials (8 slices x 48 = 384, + tile padding)
  float* splitk_ws = nullptr; size_t splitk_floats = 0;  // per clip: 4 K slices x (4 rows x 1280 cols: the widest layer a small-batch plan may split) = 20480 floats
  // plan
  const float *stem_w = nullptr, *stem_scale = nullptr, *stem_shift = nullptr;
  float norm_mean = 0.f, norm_std = 1.f;
  bool fuse_front = true;          // expand + depthwise in one kernel (mbconv_front_kernel)
  int fuse_gap = 1;                // global average pool fused into the top conv's epilogue (2x2 image: 4 rows per clip)
  int fuse_stem = 1;               // 1: stem + whole block 1a in one kernel (stem_block1a_kernel); 0: separate kernels (parity taps)
  int fuse_back = 1;               // blocks that keep mbconv_front_kernel (2a, 2b, 3b): SE + gated projection in one launch (mbconv_back_kernel)
  int fuse_mid = 1;                // whole-block kernel for big-image blocks (mbconv_mid_kernel): 1 = 2b, 3a and 4a (where it measured faster), 2 = 2a..4a, 3 = 3a and 4a only, 0 = never
  int fuse_gemv = 1;               // handles of at most 4 planned rows (one clip): dense layers and top conv on gemv_kernel (one launch per layer, K split inside the workgroup); 0 = pw_gemm_kernel + split-K fold
  int fuse_se4 = 1;                // 4x3-image blocks: squeeze-excite FCs on the 4x4x1 matrix instruction + gate applied by the lanes that compute it (Se4); 0 = 16x16x4 streams + gate pass
  int fuse_walk = 1;               // block 2a's front kernel: one workgroup walks the clip's three channel blocks (input read from HBM once); 0 = three workgroups per clip
  int fuse_block = 2;              // whole MBConv block in one kernel (mbconv_block_kernel): 1 = 2x2 images only, 2 = 2x2 and 4x3
  int fuse_chain = 1;              // depth-fused chains: 1 = blocks 4b..6a in ONE launch (mbconv_chain_kernel) and 6b..7a in ONE paired launch (mbconv_pair_chain_kernel); 2 / 3 = only the first / second; 0 = one launch per block
  mkws::BlockArgs* d_chain_tab = nullptr;   // device copy of every block's constants (BlockArgs without X / Y / dbg) for the chain kernels
  int fuse_top = 1;                // top conv + pool as the last phase of the paired chain (needs fuse_chain 1 / 3 and fuse_gap)
  int fuse_pair = 1;               // stride-1 2x2 blocks on mbconv_pair_kernel: two workgroups share 8 clips and split the channels
  float* pair_xc1 = nullptr; float* pair_xd = nullptr; int* pair_flags = nullptr;   // exchange buffers of the paired kernel
  int* pair_err_dev = nullptr;     // sticky failure word of the paired kernel (device memory)
  int* pair_err_host = nullptr;    // the same in host-mapped memory (hipHostMalloc): read by the host without synchronising
  size_t pair_flag_count = 0;
  int* pair_chain_flags = nullptr;  // flags of the paired chain kernel (behind pair_flags, cleared with them)
  int pair_fault = 0;              // test hook, see PairArgs::fault
  int pair_degraded = 0;           // how many times this handle left the paired kernel because an exchange failed
  int fuse_cluster = 0;            // small-batch handles: tiny-image blocks on mbconv_cluster_kernel (6 workgroups per 16-row tile split the channels)
  float* cl_xc1 = nullptr; float* cl_xd = nullptr; int* cl_flags = nullptr; size_t cl_flag_count = 0;   // its exchange buffers / generation flags
  int fuse_cluster_chain = 0;      // one-clip handles: blocks 4b .. 7a as ONE launch (mbconv_cluster_chain_kernel: every member requests its weights at the start)
  int pair_mt = 2;                 // row tiles per pair (2 = 8 clips, 1 = 4 clips): pair_row_tiles(max_batch)
  int block_mt43 = 3;              // row tiles per workgroup of the 4x3 whole-block kernels (3 = 4 clips, 2 = 2 clips): same rule
  BlockPlan blocks[kNumBlocks];
  GemmLayer top, dense0, dense1, dense2;
  int topH = 0, topW = 0;
};

namespace {

// Optional per-launch timing (mkws_embed_profile): a hipEvent pair around every kernel launch.
struct LaunchProf {
  struct Rec { std::string stage, kernel; hipEvent_t e0, e1; double ms = 0.0; };
  std::vector<Rec> recs;
  size_t cursor = 0;
  bool first = true;
  hipStream_t stream = nullptr;
  void begin(const std::string& stage, const std::string& kernel) {
    if (first) {
      Rec r; r.stage = stage; r.kernel = kernel;
      (void)hipEventCreate(&r.e0); (void)hipEventCreate(&r.e1);
      recs.push_back(r);
    }
    (void)hipEventRecord(recs[cursor].e0, stream);
  }
  void end() { (void)hipEventRecord(recs[cursor].e1, stream); ++cursor; }
  void finish_pass() {
    (void)hipStreamSynchronize(stream);
    for (auto& r : recs) { float ms = 0.f; (void)hipEventElapsedTime(&ms, r.e0, r.e1); r.ms += ms; }
    cursor = 0; first = false;
  }
  ~LaunchProf() { for (auto& r : recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); } }
};
static thread_local LaunchProf* g_prof = nullptr;
struct ProfScope {
  ProfScope(const std::string& stage, const std::string& kernel) { if (g_prof) g_prof->begin(stage, kernel); }
  ~ProfScope() { if (g_prof) g_prof->end(); }
};

// Development-build reporting (`make timing`): timing_arm / timing_report_* / wg_trace_*, empty stubs in the product build
#include "mkws_embed_timing.h"

// Kernels launched with more than 64 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize raised once per
// (kernel, device): a process-wide flag would leave the second GPU of a multi-device process at the default.
int ensure_dynamic_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(MKWS_ERR_HIP, "hipGetDevice failed");
  std::lock_guard<std::mutex> lk(mu);
  if (done.count({fn, dev})) return MKWS_OK;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return fail(MKWS_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize=%d) failed: %s", bytes, hipGetErrorString(e));
  done.insert({fn, dev});
  return MKWS_OK;
}

// One launch of a kernel that takes its arguments as one struct and may need more than 64 KB of dynamic LDS (limit raised to `lds_cap`).
// A launcher's ladder picks the instantiation; this is the only place that raises the limit and launches it.
template <class Args>
int launch_big_lds(void (*kernel)(Args), int lds_cap, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args& a) {
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds_cap)) return rc;
  hipLaunchKernelGGL(kernel, grid, block, lds, s, a);
  return MKWS_OK;
}

int device_cu_count() {
  static thread_local int cached_dev = -1, cached_cus = 256;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return cached_cus;
  if (dev != cached_dev) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) { cached_cus = n; cached_dev = dev; }
  }
  return cached_cus;
}

// ---- host-side packing -------------------------------------------------------------------------------
struct Packer {
  std::vector<float> buf;
  size_t add(const float* p, size_t n) {
    size_t off = (buf.size() + 3) & ~size_t(3);
    buf.resize(off + n, 0.0f);
    if (p) memcpy(buf.data() + off, p, n * sizeof(float));
    return off;
  }
  size_t reserve(size_t n) { return add(nullptr, n); }
};

struct GemmOff { size_t Wp, scale, shift; int K, N, KC, NTtot; };

// W: Keras [K, N] row-major.  scale/shift: per output channel (already folded).
GemmOff pack_gemm(Packer& pk, const float* W, int K, int N, const std::vector<float>& scale, const std::vector<float>& shift) {
  GemmOff o;
  o.K = K; o.N = N; o.KC = (K + 15) / 16; o.NTtot = (N + 15) / 16;
  const size_t n = (size_t)o.NTtot * o.KC * 256;
  o.Wp = pk.reserve(n);
  float* dst = pk.buf.data() + o.Wp;
  for (int nt = 0; nt < o.NTtot; ++nt)
    for (int j = 0; j < o.KC; ++j)
      for (int g = 0; g < 4; ++g)
        for (int c = 0; c < 16; ++c)
          for (int s = 0; s < 4; ++s) {
            const int k = 16 * j + 4 * g + s, col = 16 * nt + c;
            dst[(((size_t)j * o.NTtot + nt) * 4 + g) * 64 + c * 4 + s] = (k < K && col < N) ? W[(size_t)k * N + col] : 0.0f;
          }
  const int Np = o.NTtot * 16;
  std::vector<float> sc(Np, 0.0f), sh(Np, 0.0f);
  for (int i = 0; i < N; ++i) { sc[i] = scale[i]; sh[i] = shift[i]; }
  o.scale = pk.add(sc.data(), Np);
  o.shift = pk.add(sh.data(), Np);
  return o;
}

// 4x4x1-instruction packing of both squeeze-excite FCs of a 4x3-image block (Se4 in the kernel section: lane l of instruction 4 q + e reads
// float e of dwordx4 (q, l)).  wr: Keras [C][se], we: [se][C].  Reduce: wave w, half kh = l / 32, unit l % 32; channel w cpw + t (half 0,
// t < cpw - T0) or w cpw + cpw - T0 + t (half 1).  Expand: group of 64 channels, channel 64 group + l, unit 4 q + e.  Zero where a channel /
// unit does not exist, and zero padded to the kernels' fixed step counts.  T0 == 0 in the result: the block does not fit the packing.
struct Se4Off { size_t r = 0, e = 0; int T0 = 0, NQ = 0; };
Se4Off pack_se4(Packer& pk, const float* wr, const float* we, int ce, int se, int waves) {
  Se4Off o;
  const int cpw = ce / waves, T0 = 4 * ((cpw + 7) / 8), NQ = (se + 3) / 4, NG = (ce + 63) / 64;
  if (ce % (4 * waves) != 0 || se > 32 || T0 / 4 > kSe4MaxTQ || NQ > kSe4MaxNQ || NG > kSe4MaxGroups * waves ||
      waves * 4 * 32 > 4 * ce) return o;      // (the wave partials [8][G][32] live where the gate used to: G * Cexp floats)
  std::vector<float> qr((size_t)waves * kSe4MaxTQ * 256, 0.0f), qe((size_t)NG * kSe4MaxNQ * 256, 0.0f);
  for (int w = 0; w < waves; ++w)
    for (int t = 0; t < T0; ++t)
      for (int l = 0; l < 64; ++l) {
        const int kh = l / 32, n = l % 32;
        const int ch = w * cpw + (kh ? cpw - T0 + t : t);
        const bool ok = n < se && (kh || t < cpw - T0);
        qr[(((size_t)w * kSe4MaxTQ + t / 4) * 64 + l) * 4 + t % 4] = ok ? wr[(size_t)ch * se + n] : 0.0f;
      }
  for (int gq = 0; gq < NG; ++gq)
    for (int n = 0; n < 4 * NQ; ++n)
      for (int l = 0; l < 64; ++l) {
        const int ch = 64 * gq + l;
        qe[(((size_t)gq * kSe4MaxNQ + n / 4) * 64 + l) * 4 + n % 4] = (n < se && ch < ce) ? we[(size_t)n * ce + ch] : 0.0f;
      }
  o.r = pk.add(qr.data(), qr.size()); o.e = pk.add(qe.data(), qe.size());
  o.T0 = T0; o.NQ = NQ;
  return o;
}

void fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, int C, std::vector<float>* scale, std::vector<float>* shift) {
  scale->resize(C); shift->resize(C);
  for (int i = 0; i < C; ++i) {
    const float s = gamma[i] / std::sqrt(var[i] + kBnEps);
    (*scale)[i] = s;
    (*shift)[i] = beta[i] - mean[i] * s;
  }
}

void correct_pad(int H, int W, int k, int* pt, int* pb, int* pl, int* pr) {
  const int c = k / 2;
  *pt = c - (1 - H % 2); *pb = c; *pl = c - (1 - W % 2); *pr = c;
}

int pick_cqb(int cq) {   // largest divisor of cq that is <= 64
  for (int d = (cq < 64 ? cq : 64); d >= 1; --d) if (cq % d == 0) return d;
  return 1;
}

// split-K workspace: part of the handle's own workspace, handed to every launch_gemm of its forward
struct SplitWs { float* p = nullptr; size_t floats = 0; const int* poison = nullptr; int gemv = 0; };   // poison: see GemmArgs (set for the LAST layer only)

template <int MT, bool GATE>
void launch_gemm_nt(int NT, dim3 grid, hipStream_t s, const GemmArgs& a) {
  switch (NT) {
    case 1: hipLaunchKernelGGL((pw_gemm_kernel<MT, 1, GATE>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((pw_gemm_kernel<MT, 2, GATE>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((pw_gemm_kernel<MT, 3, GATE>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((pw_gemm_kernel<MT, 4, GATE>), grid, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL((pw_gemm_kernel<MT, 5, GATE>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((pw_gemm_kernel<MT, 6, GATE>), grid, dim3(256), 0, s, a); break;
  }
}

// Tile / split-K choice, from a sweep on MI355X (profiles/r01_gemm_sweep.txt): no (MT,NT) gets past ~60 % of
// the fp32 MFMA peak with operands fetched straight into registers, and what matters most is having >= 2
// waves per SIMD.  NT = 3, 5, 6 tiles were consistently slower than 2 / 4.  Rule:
//   wide, long-K layers with few rows (the dense layers): 2x4 tiles if that still gives 1 wave per SIMD;
//   otherwise NT = 2, MT = 2 if that reaches kWantWaves, else MT = 1, else split K (2, then 4).
constexpr int kWantWaves = 2048;
struct TileChoice { int MT, NT, splitk; };
TileChoice pick_tile(int M, int NTtot, int KC) {
  if (NTtot == 1) return {2, 1, 1};
  auto waves = [&](int mt, int nt, int sk) { return (long)((M + 16 * mt - 1) / (16 * mt)) * ((NTtot + nt - 1) / nt) * sk; };
  // dense layers of a 1024-clip handle: 1 x 4 tiles put two waves on every SIMD (N = 2048) and measured 154 us for the three
  // layers against 170 us with 2 x 4 (+ 1 x 2 for dense_2) once the K loop was free of VALU instructions (tools/gpu/sweep1024.sh)
  if (NTtot >= 64 && KC >= 64 && M >= 1024 && M < 2048 && waves(1, 4, 1) >= 1024) return {1, 4, 1};
  if (NTtot >= 64 && KC >= 64 && waves(2, 4, 1) >= 1024) return {2, 4, 1};
  // dense layers of 129..1023-clip handles (round 6, `tools/gpu/r6_gemm256.sh`: eleven forced shapes per layer at 256 and 512 clips): the winner is
  // the widest 1 x NT tile that still puts ONE wave on every SIMD (1 024 waves) WITHOUT splitting K -- 256 clips: 1 x 2 (20.3 / 27.6 us against
  // 26.0 / 33.6 for 1 x 2 over two K slices + the fold launch), 512 clips: 1 x 4 (28.7 / 38.2 against 33.1 / 48.0) and 1 x 2 for dense_2 (27.5
  // against 32.7) -- and two K slices only where even 1 x 2 leaves half the SIMDs empty (dense_2 at 256 clips: 22.3 against 27.3 unsplit)
  if (NTtot >= 64 && KC >= 64 && M > 128) {
    if (waves(1, 4, 1) >= 1024) return {1, 4, 1};
    if (waves(1, 2, 1) >= 1024) return {1, 2, 1};
    if (waves(1, 2, 2) >= 1024) return {1, 2, 2};
  }
  if (waves(2, 2, 1) >= kWantWaves) return {2, 2, 1};
  if (waves(1, 2, 1) >= kWantWaves) return {1, 2, 1};
  if (KC >= 32 && waves(1, 2, 2) >= kWantWaves) return {1, 2, 2};
  if (KC >= 64) return {1, 2, 4};
  return {1, 2, 1};
}

void launch_gemm(hipStream_t s, const SplitWs& sw, const char* stage, const GemmLayer& L, const float* X, int ldx, int M, int Mplan, int act, const float* gate, int HW,
                 const float* R, int ldr, float* Y, int ldy, int pool4 = 0) {
  GemmArgs a = {};
  a.pool4 = pool4;
  a.poison = sw.poison;
  a.X = X; a.ldx = ldx; a.Wp = L.Wp; a.scale = L.scale; a.shift = L.shift; a.gate = gate; a.HW = HW > 0 ? HW : 1;
  a.R = R; a.ldr = ldr; a.Y = Y; a.ldy = ldy; a.M = M; a.K = L.K; a.N = L.N; a.KC = L.KC; a.NTtot = L.NTtot; a.act = act;
  // live-serving handles (planned for at most 4 rows): the matrix-vector kernel, one launch per layer (decided on the planned rows: every batch
  // size of a handle takes the same path)
  if (sw.gemv && Mplan <= 4 && !gate && !R && L.KC <= 128 && L.NTtot >= 32 && L.K % 4 == 0 && (!pool4 || (Mplan == 4 && M == 4))) {
    a.splitk = 1; a.part = nullptr; a.ldp = 0;
    const int rows = Mplan <= 1 ? 1 : 4, nj = (L.KC + 15) / 16;
    ProfScope ps(stage, std::string("gemv_kernel<") + std::to_string(rows) + "," + std::to_string(nj <= 2 ? 2 : nj <= 5 ? 5 : 8) + ">");
    const dim3 grid(L.NTtot), block(1024);     // (two / four workgroups per tile, by columns, so that every CU streams: measured, no faster -- a launch of this size is ~6 us whatever it does)
    if (rows == 1) {
      if (nj <= 2) hipLaunchKernelGGL((gemv_kernel<1, 2>), grid, block, 0, s, a);
      else if (nj <= 5) hipLaunchKernelGGL((gemv_kernel<1, 5>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((gemv_kernel<1, 8>), grid, block, 0, s, a);
    } else {
      if (nj <= 2) hipLaunchKernelGGL((gemv_kernel<4, 2>), grid, block, 0, s, a);
      else if (nj <= 5) hipLaunchKernelGGL((gemv_kernel<4, 5>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((gemv_kernel<4, 8>), grid, block, 0, s, a);
    }
    return;
  }
  TileChoice tc = pick_tile(Mplan, L.NTtot, L.KC);
  if (pool4) tc.splitk = 1;                 // the fused average pool lives in the direct epilogue only
  if (const char* f = getenv("MKWS_GEMM_FORCE")) {       // experiment hook: "Mmax,MT,NT,SK" applies to layers with Mplan <= Mmax
    int mmax = 0, fmt = 0, fnt = 0, fsk = 0;
    const int mmin = getenv("MKWS_GEMM_FORCE_MIN") ? atoi(getenv("MKWS_GEMM_FORCE_MIN")) : 0;
    if (sscanf(f, "%d,%d,%d,%d", &mmax, &fmt, &fnt, &fsk) == 4 && Mplan <= mmax && Mplan >= mmin && fnt <= L.NTtot) tc = {fmt, fnt, fsk};
  }
  const int MT = tc.MT, NT = tc.NT;
  a.splitk = tc.splitk; a.part = nullptr; a.ldp = L.NTtot * 16;
  if (tc.splitk > 1) {
    if (!sw.p || (size_t)tc.splitk * Mplan * a.ldp > sw.floats) a.splitk = 1;   // no workspace: plain path (decided on the planned M, so every batch size of a handle takes the same path)
    else a.part = sw.p;
  }
  dim3 grid((M + 64 * MT - 1) / (64 * MT), (L.NTtot + NT - 1) / NT, a.splitk);
  timing_arm(a, grid);
  {
    ProfScope ps(stage, std::string("pw_gemm_kernel<") + std::to_string(MT) + "," + std::to_string(NT) + (gate ? ",true>" : ",false>"));
    if (MT == 2) { if (gate) launch_gemm_nt<2, true>(NT, grid, s, a); else launch_gemm_nt<2, false>(NT, grid, s, a); }
    else { if (gate) launch_gemm_nt<1, true>(NT, grid, s, a); else launch_gemm_nt<1, false>(NT, grid, s, a); }
  }
  timing_report_gemm(s, stage, MT, NT, grid, a);
  if (a.splitk > 1) {
    ProfScope ps(std::string(stage) + "#reduce", "splitk_reduce_kernel");
    const long total = (long)M * (L.N / 4);
    int rg = (int)((total + 255) / 256); if (rg > 4096) rg = 4096;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(rg), dim3(256), 0, s, a.part, a.splitk, M, L.N, a.ldp, L.scale, L.shift, act, R, ldr, Y, ldy, a.poison);
  }
}

void launch_dw(hipStream_t s, const char* stage, const BlockPlan& b, const float* X, float* Y, float* sums, int B) {
  ProfScope ps(stage, std::string("dw_kernel<") + std::to_string(b.spec.kernel) + "," + std::to_string(b.spec.stride) + ">");
  const int cq = b.ce / 4;
  const int CQB = pick_cqb(cq);
  int P = 256 / CQB;
  const int npix = b.Ho * b.Wo;
  if (P > npix) P = npix;
  dim3 grid(B, cq / CQB);
#define MKWS_DW(KS, S) hipLaunchKernelGGL((dw_kernel<KS, S>), grid, dim3(256), 0, s, X, b.dw.Wd, b.dw.scale, b.dw.shift, Y, sums, \
                                          b.H, b.W, b.ce, b.Ho, b.Wo, b.pt, b.pl, CQB, P)
  if (b.spec.kernel == 3 && b.spec.stride == 1) MKWS_DW(3, 1);
  else if (b.spec.kernel == 3) MKWS_DW(3, 2);
  else if (b.spec.stride == 1) MKWS_DW(5, 1);
  else MKWS_DW(5, 2);
#undef MKWS_DW
}

// Fused expand + depthwise (mbconv_front_kernel): geometry per layer.
bool front_supported(const BlockPlan& b) {
  const int ks = b.spec.kernel, st = b.spec.stride, kc = (b.spec.in_ch + 15) / 16;
  const int HW = b.H * b.W;
  if (HW > 16) {       // one instance per layer geometry of the 49x40 network (image size is a template constant)
    return (b.H == 25 && b.W == 20 && ks == 3 && st == 2 && kc == 1) || (b.H == 13 && b.W == 10 && ks == 3 && st == 1 && kc == 2) ||
           (b.H == 13 && b.W == 10 && ks == 5 && st == 2 && kc == 2) || (b.H == 7 && b.W == 5 && ks == 5 && st == 1 && kc == 3) ||
           (b.H == 7 && b.W == 5 && ks == 3 && st == 2 && kc == 3);
  }
  if (b.H == 4 && b.W == 3) return (ks == 3 && st == 1) || (ks == 5 && st == 1) || (ks == 5 && st == 2);
  if (b.H == 2 && b.W == 2) return (ks == 5 && st == 1) || (ks == 3 && st == 1);
  return false;
}

void launch_front(hipStream_t s, const char* stage, const BlockPlan& b, const float* X, float* Y, float* sums, int B, int walk) {
  FrontArgs a = {};
  a.X = X; a.Cin = b.spec.in_ch; a.WpE = b.expand.Wp; a.scE = b.expand.scale; a.shE = b.expand.shift; a.KC = b.expand.KC;
  a.NTtotE = b.expand.NTtot;
  a.Wd = b.dw.Wd; a.scD = b.dw.scale; a.shD = b.dw.shift; a.Y = Y; a.sums = sums;
  a.B = B; a.H = b.H; a.W = b.W; a.Ho = b.Ho; a.Wo = b.Wo; a.pt = b.pt; a.pl = b.pl; a.Cexp = b.ce;
  const int HW = b.H * b.W;
  const bool tiny = HW <= 16;
  const int ks = b.spec.kernel, st = b.spec.stride, kc = b.expand.KC;
  int CC, G;
  if (tiny) {                       // 4x3 and 2x2 images: wide channel chunks, 128 LDS rows per block
    CC = 128;
    G = 128 / HW;
  } else {                          // big images: 32 channels; clips per block so that the row strips fill 256 threads
    CC = 32;
    G = (b.H == 25) ? 1 : (b.H == 13 ? (st == 1 ? 1 : 3) : (st == 1 ? 4 : 8));    // 2a | 2b, 3a | 3b, 4a (LDS: 2+ blocks per CU)
  }
  if (G > B) G = B;
  a.G = G;
  const size_t lds = (((size_t)G * HW + 1) * (CC + 4) + 256 * 4 + (size_t)G * CC + (tiny ? 0 : (size_t)ks * ks * CC)) * sizeof(float);
  const int nblk_c = (b.ce + CC - 1) / CC;
  a.ncb = (!tiny && walk && b.H == 25) ? nblk_c : 1;      // 2a: one workgroup walks the clip's three channel blocks (fuse_walk)
  const dim3 grid((B + G - 1) / G, nblk_c / a.ncb);
  ProfScope ps(stage, std::string("mbconv_front_kernel<") + std::to_string(ks) + "," + std::to_string(st) + "," + std::to_string(CC) + "," +
                          (tiny ? "0," : std::to_string(kc) + ",") + std::to_string(b.H) + "," + std::to_string(b.W) + ">");
  const size_t nblk = (size_t)grid.x * grid.y;
  timing_arm(a);
  wg_trace_arm();
#define MKWS_FRONT(KS, S, C_, KC_, H_, W_) \
  hipLaunchKernelGGL((mbconv_front_kernel<KS, S, C_, KC_, H_, W_>), grid, dim3((KC_) > 0 ? 256 : 512), lds, s, a)
  if (!tiny) {
    if (ks == 3 && st == 2 && kc == 1) MKWS_FRONT(3, 2, 32, 1, 25, 20);        // 2a
    else if (ks == 3 && st == 1 && kc == 2) MKWS_FRONT(3, 1, 32, 2, 13, 10);   // 2b
    else if (ks == 5 && st == 2 && kc == 2) MKWS_FRONT(5, 2, 32, 2, 13, 10);   // 3a
    else if (ks == 5 && st == 1 && kc == 3) MKWS_FRONT(5, 1, 32, 3, 7, 5);     // 3b
    else if (ks == 3 && st == 2 && kc == 3) MKWS_FRONT(3, 2, 32, 3, 7, 5);     // 4a
  } else if (b.H == 4 && b.W == 3) {
    if (ks == 3 && st == 1) MKWS_FRONT(3, 1, 128, 0, 4, 3);                  // 4b, 4c
    else if (ks == 5 && st == 1) MKWS_FRONT(5, 1, 128, 0, 4, 3);             // 5a, 5b, 5c
    else if (ks == 5 && st == 2) MKWS_FRONT(5, 2, 128, 0, 4, 3);             // 6a
  } else if (b.H == 2 && b.W == 2) {
    if (ks == 5 && st == 1) MKWS_FRONT(5, 1, 128, 0, 2, 2);                  // 6b, 6c, 6d
    else if (ks == 3 && st == 1) MKWS_FRONT(3, 1, 128, 0, 2, 2);             // 7a
  }
#undef MKWS_FRONT
  timing_report_front(s, stage, ks, st, nblk);
  wg_trace_report(s, stage, "front", nblk);
}

// Whole-block kernel for 4x3 / 2x2 images (blocks 4b..7a): 4 clips per workgroup either way.
static constexpr int kBlockWaves = 8;
static int block_row_tiles(const BlockPlan& b, int mt43) { return (b.H * b.W == 4) ? 1 : mt43; }
static size_t block_lds_bytes(const BlockPlan& b, int mt43 = 3) {
  const int HW = b.H * b.W, MT = block_row_tiles(b, mt43), G = MT * 16 / HW;
  const BlockLds L = block_lds(b.expand.KC, b.ce, MT, G, kBlockWaves);
  return ((size_t)L.U + L.E + L.Z) * sizeof(float);
}
bool block_supported(const BlockPlan& b, int mode) {
  const int ks = b.spec.kernel, st = b.spec.stride;
  if (!b.has_expand || b.ce % 16 != 0 || b.spec.out_ch % 16 != 0 || b.spec.out_ch > 320 || b.se.NTR > 3) return false;
  if (!((b.H == 4 && b.W == 3) || (b.H == 2 && b.W == 2))) return false;
  if (block_lds_bytes(b) > 160 * 1024) return false;
  if (b.H == 4 && b.W == 3) return mode >= 2 && ((ks == 3 && st == 1) || (ks == 5 && st == 1) || (ks == 5 && st == 2));
  return (ks == 5 && st == 1) || (ks == 3 && st == 1);
}

// The constants of one block as the whole-block kernels (block, pair, cluster, and the chain kernels through the device table) read them.
// Everything else is zero: a launcher sets X, Y, B and the debug pointers, and clears WrQ where the 4x4x1 squeeze-excite is switched off.
static BlockArgs block_args(const BlockPlan& b) {
  BlockArgs a;
  memset(static_cast<void*>(&a), 0, sizeof(a));
  a.Cin = b.spec.in_ch;
  a.WpE = b.expand.Wp; a.scE = b.expand.scale; a.shE = b.expand.shift; a.KCe = b.expand.KC; a.NTe = b.expand.NTtot;
  a.Wd = b.dw.Wd; a.scD = b.dw.scale; a.shD = b.dw.shift;
  a.WrP = b.se.WrP; a.br = b.se.br; a.NTR = b.se.NTR; a.We2P = b.se.WeP; a.be = b.se.be;
  a.WpP = b.project.Wp; a.scP = b.project.scale; a.shP = b.project.shift; a.NTp = b.project.NTtot;
  a.Cout = b.spec.out_ch; a.residual = b.residual ? 1 : 0;
  a.Cexp = b.ce; a.se = b.se.se;
  a.WrQ = b.se.WrQ; a.We2Q = b.se.WeQ; a.seT0 = b.se.T0; a.seNQ = b.se.NQ;
  return a;
}
// ... with the pointers of one launch
static BlockArgs block_args(const BlockPlan& b, const float* X, float* Y, float* dbg_dw, float* dbg_gate, int B) {
  BlockArgs a = block_args(b);
  a.X = X; a.Y = Y; a.dbg_dw = dbg_dw; a.dbg_gate = dbg_gate; a.B = B;
  return a;
}

int launch_block(hipStream_t s, const char* stage, const BlockPlan& b, int mt43, const float* X, float* Y, float* dbg_dw, float* dbg_gate, int B, bool se4 = true) {
  BlockArgs a = block_args(b, X, Y, dbg_dw, dbg_gate, B);
  if (!se4) a.WrQ = nullptr;
  const int HW = b.H * b.W, MT = block_row_tiles(b, mt43), G = MT * 16 / HW;
  const size_t lds = block_lds_bytes(b, mt43);
  const dim3 grid((B + G - 1) / G);
  const int ks = b.spec.kernel, st = b.spec.stride;
  ProfScope ps(stage, std::string("mbconv_block_kernel<") + std::to_string(ks) + "," + std::to_string(st) + "," + std::to_string(b.H) + "," +
                          std::to_string(b.W) + "," + std::to_string(MT) + "," + std::to_string(kBlockWaves) + ">");
  void (*k)(BlockArgs);
  if (b.H == 4 && b.W == 3 && MT == 3) {
    if (ks == 3 && st == 1) k = &mbconv_block_kernel<3, 1, 4, 3, 3, kBlockWaves>;
    else if (ks == 5 && st == 1) k = &mbconv_block_kernel<5, 1, 4, 3, 3, kBlockWaves>;
    else k = &mbconv_block_kernel<5, 2, 4, 3, 3, kBlockWaves>;
  } else if (b.H == 4 && b.W == 3 && MT == 2) {
    if (ks == 3 && st == 1) k = &mbconv_block_kernel<3, 1, 4, 3, 2, kBlockWaves>;
    else if (ks == 5 && st == 1) k = &mbconv_block_kernel<5, 1, 4, 3, 2, kBlockWaves>;
    else k = &mbconv_block_kernel<5, 2, 4, 3, 2, kBlockWaves>;
  } else if (b.H == 4 && b.W == 3) {                     // one clip per workgroup (handles of <= 256 clips: a workgroup for every CU)
    if (ks == 3 && st == 1) k = &mbconv_block_kernel<3, 1, 4, 3, 1, kBlockWaves>;
    else if (ks == 5 && st == 1) k = &mbconv_block_kernel<5, 1, 4, 3, 1, kBlockWaves>;
    else k = &mbconv_block_kernel<5, 2, 4, 3, 1, kBlockWaves>;
  } else {
    if (ks == 5) k = &mbconv_block_kernel<5, 1, 2, 2, 1, kBlockWaves>;
    else k = &mbconv_block_kernel<3, 1, 2, 2, 1, kBlockWaves>;
  }
  timing_arm(a);
  if (int rc = launch_big_lds(k, 160 * 1024, grid, dim3(kBlockWaves * 64), lds, s, a)) return rc;
  timing_report_block(s, stage, grid.x);
  return MKWS_OK;
}

// Depth-fused chain (mbconv_chain_kernel): consecutive 4x3-image blocks [i0, i1] of the plan in one launch.
// May block i+1 follow block i inside one chain launch?  (The chain keeps activations in LDS and the residual in registers.)
static bool chain_link_ok(const BlockPlan& b, const BlockPlan& next) {
  if (b.spec.stride != 1) return false;                                  // a stride-2 block ends the chain (the image shrinks)
  if (b.project.NTtot > kBlockWaves) return false;                       // one output tile per wave: the residual carry is one fragment per row tile
  if (next.spec.in_ch != b.spec.out_ch || next.expand.KC != b.project.NTtot) return false;
  return next.ce <= 3 * kBlockWaves * 64;
}
bool cluster_supported(const BlockPlan& b);
bool pair_supported(const BlockPlan& b);
// Does this handle run block b on the cluster kernel?  (Its blocks are members of no other chain.)
static bool cluster_enabled(const mkws_embed* em, const BlockPlan& b) { return em->fuse_cluster && cluster_supported(b) && em->cl_flags; }
static bool chain_member(const mkws_embed* em, const BlockPlan& b) {
  if (!(em->fuse_chain == 1 || em->fuse_chain == 2) || !em->fuse_block || !block_supported(b, em->fuse_block)) return false;
  if (!(b.H == 4 && b.W == 3)) return false;
  return !cluster_enabled(em, b);
}
int launch_chain(hipStream_t s, const mkws_embed* em, int i0, int i1, const float* X, float* Y, int B) {
  ChainArgs ca = {};
  const int n = i1 - i0 + 1, mt43 = em->block_mt43;
  if (!em->d_chain_tab) return fail(MKWS_ERR_UNSUPPORTED, "chain: no block table");
  ca.tab = em->d_chain_tab; ca.i0 = i0; ca.n = n; ca.kinds = 0; ca.ldsU = ca.ldsE = 0;
  ca.X = X; ca.Y = Y; ca.B = B; ca.se4 = em->fuse_se4;
  int ldsZ = 0;
  std::string names;
  for (int k = 0; k < n; ++k) {
    const BlockPlan& b = em->blocks[i0 + k];
    const int ks = b.spec.kernel, st = b.spec.stride;
    if (ks == 3 && st != 1) return fail(MKWS_ERR_UNSUPPORTED, "chain: 3x3 stride-2 block");
    ca.kinds |= (unsigned)((ks == 3 && st == 1) ? 0 : (ks == 5 && st == 1) ? 1 : 2) << (2 * k);
    const int MT = block_row_tiles(b, mt43), G = MT * 16 / (b.H * b.W);
    const BlockLds L = block_lds(b.expand.KC, b.ce, MT, G, kBlockWaves);
    ca.ldsU = std::max(ca.ldsU, L.U); ca.ldsE = std::max(ca.ldsE, L.E); ldsZ = std::max(ldsZ, L.Z);
    names += (k ? "," : "") + std::string(b.spec.name);
  }
  const size_t lds = ((size_t)ca.ldsU + ca.ldsE + ldsZ) * sizeof(float);
  if (lds > 160 * 1024) return fail(MKWS_ERR_UNSUPPORTED, "chain: LDS carve %zu bytes", lds);
  const int G = mt43 * 16 / 12;
  const dim3 grid((B + G - 1) / G);
  ProfScope ps("chain:" + names, std::string("mbconv_chain_kernel<") + std::to_string(mt43) + "," + std::to_string(kBlockWaves) + ">");
  void (*k)(ChainArgs);
  if (mt43 == 3) k = &mbconv_chain_kernel<3, kBlockWaves>;
  else if (mt43 == 2) k = &mbconv_chain_kernel<2, kBlockWaves>;
  else k = &mbconv_chain_kernel<1, kBlockWaves>;
  timing_arm(ca, grid.x);
  if (int rc = launch_big_lds(k, 160 * 1024, grid, dim3(kBlockWaves * 64), lds, s, ca)) return rc;
  timing_report_chain(s, em->blocks + i0, n, names, grid.x, ca);
  return MKWS_OK;
}

// Paired whole-block kernel (mbconv_pair_kernel): the stride-1 2x2-image blocks (6b, 6c, 6d, 7a).
struct PairWs { float* xc1 = nullptr; float* xd = nullptr; int* flags = nullptr; int* err_dev = nullptr; int* err_host = nullptr; int fault = 0; int mt = 2; };
static int pair_count(int B, int mt) { const int G = 4 * mt; return ((B + G - 1) / G + 7) / 8 * 8; }   // padded to whole groups of 8 pairs (16 workgroups)
// Row tiles per pair for a handle: 8 clips per pair fill the chip from ~1024 clips up; smaller handles use 4-clip pairs so
// that twice as many workgroups exist (512 clips: 256 instead of 128).  Per handle, like every other plan decision.
// Row tiles per workgroup of the 4x3-image whole-block / chain kernels: 3 (4 clips), 2 (2 clips) or 1 (1 clip) -- the largest that still gives
// every CU a workgroup (round 6: a 256-clip serving handle used to run 128 two-clip workgroups on 256 CUs).
static int block43_row_tiles(int max_batch) {
  const int cus = device_cu_count();
  if ((max_batch + 3) / 4 >= cus) return 3;
  if ((max_batch + 1) / 2 >= cus) return 2;
  return (max_batch > cus / 2 && max_batch <= cus) ? 1 : 2;      // one clip per workgroup while that is still ONE round of workgroups and more than half a chip of them
}
static int pair_row_tiles(int max_batch) { return (2 * ((max_batch + 3) / 4) <= device_cu_count()) ? 1 : 2; }   // 4-clip pairs while they still fit in one round
// The paired kernel wants blocks b and b ^ 8 on ONE XCD (their exchange goes through that XCD's L2 without agent-scope
// cache maintenance).  True for the round-robin dispatch of an 8-XCD device in SPX mode; checked once per device instead of
// assumed (other partition modes / future parts), and the kernel re-checks every pair at run time.
static bool pair_layout_ok() {
  static std::mutex mu;
  static std::map<int, bool> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(dev);
  if (it != cache.end()) return it->second;
  bool ok = false;
  const int n = 4 * device_cu_count() / 16 * 16;
  int* d = nullptr;
  if (n >= 16 && hipMalloc(reinterpret_cast<void**>(&d), n * sizeof(int)) == hipSuccess) {
    std::vector<int> h(n, -1);
    hipLaunchKernelGGL(xcc_probe_kernel, dim3(n), dim3(64), 0, nullptr, d);
    if (hipMemcpy(h.data(), d, n * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) {
      ok = true;
      for (int b = 0; b < n; ++b) ok = ok && h[b] >= 0 && h[b] == h[b & 7];    // the XCD is a function of (linear id mod 8) only
    }
    (void)hipFree(d);
  }
  cache[dev] = ok;
  return ok;
}

bool pair_supported(const BlockPlan& b) {
  if (!b.has_expand || b.H != 2 || b.W != 2 || b.spec.stride != 1 || (b.spec.kernel != 3 && b.spec.kernel != 5)) return false;
  if (b.ce % 32 != 0 || b.spec.out_ch % 16 != 0 || b.project.NTtot > 2 * kPairXdTiles || b.se.NTR > 3 || b.se.se > 48) return false;
  const PairLds L = pair_lds(b.expand.KC, b.ce / 2, 2);
  return ((size_t)L.U + L.E + L.Z) * sizeof(float) <= 160 * 1024;
}

int launch_pair(hipStream_t s, const char* stage, const BlockPlan& b, const PairWs& ws, const float* X, float* Y, float* dbg_dw, float* dbg_gate, int B) {
  PairArgs pa = {};
  pa.b = block_args(b, X, Y, dbg_dw, dbg_gate, B);
  pa.xc1 = ws.xc1; pa.xd = ws.xd; pa.flags = ws.flags; pa.err_dev = ws.err_dev; pa.err_host = ws.err_host; pa.fault = ws.fault;
  const PairLds L = pair_lds(b.expand.KC, b.ce / 2, ws.mt);
  const size_t lds = ((size_t)L.U + L.E + L.Z) * sizeof(float);
  const dim3 grid(2 * pair_count(B, ws.mt));
  const int ks = b.spec.kernel;
  ProfScope ps(stage, std::string("mbconv_pair_kernel<") + std::to_string(ks) + "," + std::to_string(ws.mt) + "," + std::to_string(kBlockWaves) + ">");
  void (*k)(PairArgs);
  if (ks == 5) k = (ws.mt == 2) ? &mbconv_pair_kernel<5, 2, kBlockWaves> : &mbconv_pair_kernel<5, 1, kBlockWaves>;
  else         k = (ws.mt == 2) ? &mbconv_pair_kernel<3, 2, kBlockWaves> : &mbconv_pair_kernel<3, 1, kBlockWaves>;
  timing_arm(pa.b);
  if (int rc = launch_big_lds(k, 160 * 1024, grid, dim3(kBlockWaves * 64), lds, s, pa)) return rc;
  timing_report_block(s, stage, grid.x);
  return MKWS_OK;
}

// Paired chain (mbconv_pair_chain_kernel): consecutive stride-1 2x2-image blocks [i0, i1] in one paired launch.
static bool pair_chain_member(const mkws_embed* em, const BlockPlan& b) {
  if (!(em->fuse_chain == 1 || em->fuse_chain == 3) || !em->fuse_block || !em->fuse_pair || !block_supported(b, em->fuse_block) || !pair_supported(b)) return false;
  if (cluster_enabled(em, b)) return false;
  return b.ce / 2 <= 2 * kBlockWaves * 64 && b.project.NTtot <= kPairXdAll && b.project.NTtot <= 3 * kBlockWaves;
}
static bool pair_chain_link_ok(const BlockPlan& b, const BlockPlan& next) {
  if (b.project.NTtot > 2 * kBlockWaves) return false;                   // the residual carry holds two tiles per wave
  return b.spec.stride == 1 && next.spec.in_ch == b.spec.out_ch && next.expand.KC == b.project.NTtot;
}
int launch_pair_chain(hipStream_t s, const mkws_embed* em, int i0, int i1, const float* X, float* Y, int B, bool with_top) {
  PairChainArgs pa = {};
  const int n = i1 - i0 + 1, mt = em->pair_mt;
  if (!em->d_chain_tab || n > kPairChainMax) return fail(MKWS_ERR_UNSUPPORTED, "pair chain: no block table / too many blocks");
  pa.tab = em->d_chain_tab; pa.i0 = i0; pa.n = n; pa.kinds = 0; pa.ldsU = pa.ldsE = pa.ldsZ = 0;
  pa.X = X; pa.Y = Y; pa.B = B;
  pa.xc1 = em->pair_xc1; pa.xd = em->pair_xd; pa.flags = em->pair_chain_flags; pa.err_dev = em->pair_err_dev; pa.err_host = em->pair_err_host; pa.fault = em->pair_fault;
  std::string names;
  for (int k = 0; k < n; ++k) {
    const BlockPlan& b = em->blocks[i0 + k];
    if (b.spec.kernel == 3) pa.kinds |= 1u << k;
    const PairLds L = pair_lds(b.expand.KC, b.ce / 2, mt);
    pa.ldsU = std::max(pa.ldsU, L.U); pa.ldsE = std::max(pa.ldsE, L.E); pa.ldsZ = std::max(pa.ldsZ, L.Z);
    names += (k ? "," : "") + std::string(b.spec.name);
  }
  pa.top_Wp = nullptr; pa.top_sc = pa.top_sh = nullptr; pa.top_KC = pa.top_NT = 0; pa.gap = nullptr;
  if (with_top) {
    const GemmLayer& T = em->top;
    if (T.NTtot != 2 * 5 * kBlockWaves || T.KC < 4 || T.KC != em->blocks[i1].project.NTtot) return fail(MKWS_ERR_UNSUPPORTED, "pair chain: top conv shape");
    pa.top_Wp = T.Wp; pa.top_sc = T.scale; pa.top_sh = T.shift; pa.top_KC = T.KC; pa.top_NT = T.NTtot; pa.gap = em->gap;
    pa.ldsU = std::max(pa.ldsU, T.KC * mt * 256);
    names += ",top";
  }
  const size_t lds = ((size_t)pa.ldsU + pa.ldsE + pa.ldsZ) * sizeof(float);
  if (lds > 160 * 1024) return fail(MKWS_ERR_UNSUPPORTED, "pair chain: LDS carve %zu bytes", lds);
  const dim3 grid(2 * pair_count(B, mt));
  ProfScope ps("chain:" + names, std::string("mbconv_pair_chain_kernel<") + std::to_string(mt) + "," + std::to_string(kBlockWaves) + ">");
  void (*k)(PairChainArgs) = (mt == 2) ? &mbconv_pair_chain_kernel<2, kBlockWaves> : &mbconv_pair_chain_kernel<1, kBlockWaves>;
  return launch_big_lds(k, 160 * 1024, grid, dim3(kBlockWaves * 64), lds, s, pa);
}

// Cluster kernel (mbconv_cluster_kernel): tiny-image blocks of small-batch handles.
constexpr int kClusterMaxBatch = 32;                 // handles up to this size plan the cluster kernel (tools/plan_sweep.py)
static int cluster_count(int B, int clips_per_cluster) { return (((B + clips_per_cluster - 1) / clips_per_cluster) + 7) / 8 * 8; }   // whole groups of 8 clusters
// Members per cluster: as many as leave every member whole 16-channel tiles (3 to 6 of them) -- the members pull their weights from
// the Infinity Cache / HBM at a latency-bound ~13 GB/s per CU (measured: 100 KB in 7.5 us), so the split is what shortens the phases.
static int cluster_members(int ce) {
  for (int P = kClusterPMax; P >= 2; --P)
    if (ce % (16 * P) == 0 && ce / P >= 48 && ce / P <= kClusterChMax) return P;
  return 0;
}
bool cluster_supported(const BlockPlan& b) {
  const int ks = b.spec.kernel, st = b.spec.stride;
  if (!b.has_expand || cluster_members(b.ce) == 0 || b.expand.KC > 12) return false;
  if (b.project.NTtot > kClMaxTiles || b.se.se > 48 || b.spec.out_ch % 16 != 0) return false;
  if (b.H == 4 && b.W == 3) return (ks == 3 && st == 1) || (ks == 5 && st == 1) || (ks == 5 && st == 2);
  if (b.H == 2 && b.W == 2) return (ks == 5 && st == 1) || (ks == 3 && st == 1);
  return false;
}

int launch_cluster(hipStream_t s, const char* stage, const BlockPlan& b, int block_index, const mkws_embed* em, const float* X, float* Y, float* dbg_dw, float* dbg_gate, int B) {
  ClusterArgs ca = {};
  ca.b = block_args(b, X, Y, dbg_dw, dbg_gate, B);
  ca.Wr = b.se.Wr; ca.We = b.se.We;
  // generation flags are PER BLOCK: a member's generation counts the launches it took part in, and blocks differ in their member count
  ca.xc1 = em->cl_xc1; ca.xd = em->cl_xd; ca.flags = em->cl_flags + (size_t)block_index * (em->cl_flag_count / kNumBlocks);
  ca.err_dev = em->pair_err_dev; ca.err_host = em->pair_err_host; ca.fault = em->pair_fault;
  ca.P = cluster_members(b.ce);
  const int G = 16 / (b.H * b.W);
  const dim3 grid(cluster_count(B, G) * ca.P);
  const size_t lds = (size_t)kClusterLdsFloats * sizeof(float);      // (+ 16 B static)
  const int ks = b.spec.kernel, st = b.spec.stride;
  ProfScope ps(stage, std::string("mbconv_cluster_kernel<") + std::to_string(ks) + "," + std::to_string(st) + "," + std::to_string(b.H) + "," + std::to_string(b.W) + ">");
  void (*k)(ClusterArgs);
  if (b.H == 4) {
    if (ks == 3) k = &mbconv_cluster_kernel<3, 1, 4, 3>;
    else if (st == 1) k = &mbconv_cluster_kernel<5, 1, 4, 3>;
    else k = &mbconv_cluster_kernel<5, 2, 4, 3>;
  } else {
    if (ks == 5) k = &mbconv_cluster_kernel<5, 1, 2, 2>;
    else k = &mbconv_cluster_kernel<3, 1, 2, 2>;
  }
  auto launch = [&] { return launch_big_lds(k, (int)lds, grid, dim3(256), lds, s, ca); };
  timing_arm(ca.b, s);
  if (int rc = launch()) return rc;
  timing_report_cluster(s, stage, grid.x, launch);
  return MKWS_OK;
}

// Blocks i0 .. i1 (all cluster_supported, one clip) as ONE launch: see mbconv_cluster_chain_kernel.  The last block's output lands in
// buf0 when the chain has an even number of blocks, in buf1 otherwise (the blocks ping-pong like the launch-by-launch plan).
int cluster_chain_kind(const BlockPlan& b) {
  const int ks = b.spec.kernel, st = b.spec.stride;
  if (b.H == 4 && b.W == 3) return (ks == 3 && st == 1) ? 0 : (ks == 5 && st == 1) ? 1 : (ks == 5 && st == 2) ? 2 : -1;
  if (b.H == 2 && b.W == 2) return (ks == 5 && st == 1) ? 3 : (ks == 3 && st == 1) ? 4 : -1;
  return -1;
}
bool cluster_chain_ok(const mkws_embed* em, int i0, int i1) {
  if (!em->fuse_cluster_chain || !em->fuse_cluster || !em->cl_flags || !em->d_chain_tab || em->max_batch != 1) return false;
  if (i1 - i0 + 1 > kClusterChainMax || i1 - i0 + 1 < 2 || em->cl_flag_count / kNumBlocks < 4 * (size_t)kClFlagRow) return false;
  if (em->cl_flag_count / ((size_t)2 * kClFlagRow * kNumBlocks) < (size_t)(i1 - i0 + 1)) return false;      // an exchange slot per block
  for (int i = i0; i <= i1; ++i) {
    const BlockPlan& b = em->blocks[i];
    if (!cluster_supported(b) || cluster_chain_kind(b) < 0 || (b.se.se & 3) != 0) return false;
    const int P = cluster_members(b.ce), KH = b.ce / P / 16;
    if (KH != ((b.H * b.W == 4) ? 6 : 3)) return false;              // the chained members hold their whole projection slice in a ring of that depth
    if (i > i0 && (em->blocks[i - 1].spec.out_ch != b.spec.in_ch || em->blocks[i - 1].Ho != b.H || em->blocks[i - 1].Wo != b.W)) return false;
  }
  return true;
}
int launch_cluster_chain(hipStream_t s, const mkws_embed* em, int i0, int i1, float* buf0, float* buf1) {
  ClusterChainArgs cc;
  memset(static_cast<void*>(&cc), 0, sizeof(cc));
  cc.tab = em->d_chain_tab; cc.i0 = i0; cc.n = i1 - i0 + 1; cc.kinds = 0;
  cc.buf0 = buf0; cc.buf1 = buf1;
  std::string names;
  int base = 0;
  for (int k = 0; k < cc.n; ++k) {
    const BlockPlan& b = em->blocks[i0 + k];
    cc.kinds |= (unsigned)cluster_chain_kind(b) << (3 * k);
    cc.Wr[k] = b.se.Wr; cc.We[k] = b.se.We;
    cc.P[k] = (signed char)cluster_members(b.ce);
    cc.base[k] = base;
    base += 8 * cc.P[k];
    names += (k ? "," : "") + std::string(b.spec.name);
  }
  cc.base[cc.n] = base;
  cc.xc1 = em->cl_xc1; cc.xd = em->cl_xd;
  cc.flags = em->cl_flags; cc.flag_stride = (int)(em->cl_flag_count / kNumBlocks);
  cc.err_dev = em->pair_err_dev; cc.err_host = em->pair_err_host; cc.fault = em->pair_fault;
  const size_t lds = (size_t)kClusterLdsFloats * sizeof(float);
  ProfScope ps("chain:" + names, "mbconv_cluster_chain_kernel");
  timing_arm(cc, s);
  if (int rc = launch_big_lds(&mbconv_cluster_chain_kernel, (int)lds, dim3(base), dim3(256), lds, s, cc)) return rc;
  timing_report_cluster_chain(s, em->blocks + i0, cc);
  return MKWS_OK;
}

// Whole-block kernel for the big-image blocks 2a..4a (mbconv_mid_kernel): one instance per layer geometry.
bool mid_supported(const BlockPlan& b) {
  if (!b.has_expand || b.se.se > 10) return false;
  const int ks = b.spec.kernel, st = b.spec.stride, ci = b.spec.in_ch, co = b.spec.out_ch;
  return (b.H == 25 && b.W == 20 && ks == 3 && st == 2 && ci == 16 && co == 24) || (b.H == 13 && b.W == 10 && ks == 3 && st == 1 && ci == 24 && co == 24) ||
         (b.H == 13 && b.W == 10 && ks == 5 && st == 2 && ci == 24 && co == 40) || (b.H == 7 && b.W == 5 && ks == 5 && st == 1 && ci == 40 && co == 40) ||
         (b.H == 7 && b.W == 5 && ks == 3 && st == 2 && ci == 40 && co == 80);
}

template <int KS, int S, int KCT, int HT, int WT, int CEXP, int CC, int NTP, int G, int SEG, int NTHR, int WPE, bool PAIR = false>
int launch_mid_inst(hipStream_t s, const char* stage, MidArgs a) {
  using GM = MidGeom<KS, S, KCT, HT, WT, CEXP, CC, G, SEG>;
  constexpr size_t lds = (size_t)(GM::lds_floats + kMidStampFloats) * sizeof(float);
  static_assert(lds <= 160 * 1024, "LDS carve exceeds one CU");
  ProfScope ps(stage, std::string("mbconv_mid_kernel<") + std::to_string(KS) + "," + std::to_string(S) + "," + std::to_string(HT) + "," + std::to_string(WT) +
                          "," + std::to_string(CEXP) + "," + std::to_string(CC) + "," + std::to_string(G) + "," + std::to_string(NTHR) + ">");
  const dim3 grid((a.B + G - 1) / G);
  timing_arm(a, grid.x);
  wg_trace_arm();
  if (int rc = launch_big_lds(&mbconv_mid_kernel<KS, S, KCT, HT, WT, CEXP, CC, NTP, G, SEG, NTHR, WPE, PAIR>, 160 * 1024, grid, dim3(NTHR), lds, s, a)) return rc;
  timing_report_mid(s, stage, CC, G, GM::NCH, grid.x, NTHR, lds);
  wg_trace_report(s, stage, "mid", (size_t)grid.x);
  return MKWS_OK;
}

// fuse_mid: 1 = the blocks where the whole-block kernel measured faster (2b, 3a, 4a); 3 = 3a and 4a only (rounds 2-3); 2 = all five big-image blocks
// (A/B and parity runs); 0 = the three-kernel path everywhere.
bool mid_enabled(const BlockPlan& b, int fuse_mid) {
  if (!fuse_mid || !mid_supported(b)) return false;
  if (fuse_mid == 2) return true;
  if (b.H == 13 && b.spec.kernel == 3) return fuse_mid == 1;           // 2b: 67.9 us against 40.4 + 31.8 for the front / back pair (round 4; before the round-3 mid-kernel work it tied)
  return (b.H == 13 && b.spec.kernel == 5) || (b.H == 7 && b.spec.stride == 2);
}

// One launch's arguments for the big-image whole-block kernel (mbconv_mid_kernel); what is not set here is zero
static MidArgs mid_args(const BlockPlan& b, const float* X, float* Y, float* dbg_dw, float* dbg_gate, int B) {
  MidArgs a;
  memset(static_cast<void*>(&a), 0, sizeof(a));
  a.X = X; a.Cin = b.spec.in_ch;
  a.WpE = b.expand.Wp; a.scE = b.expand.scale; a.shE = b.expand.shift; a.NTtotE = b.expand.NTtot;
  a.Wd = b.dw.Wd; a.scD = b.dw.scale; a.shD = b.dw.shift;
  a.Wr = b.se.Wr; a.br = b.se.br; a.We = b.se.We; a.be = b.se.be; a.se = b.se.se;
  a.WpP = b.project.Wp; a.scP = b.project.scale; a.shP = b.project.shift;
  a.Y = Y; a.Cout = b.spec.out_ch; a.residual = b.residual ? 1 : 0;
  a.dbg_dw = dbg_dw; a.dbg_gate = dbg_gate; a.B = B;
  return a;
}

int launch_mid(hipStream_t s, const char* stage, const BlockPlan& b, int one_clip, const float* X, float* Y, float* dbg_dw, float* dbg_gate, int B) {
  const MidArgs a = mid_args(b, X, Y, dbg_dw, dbg_gate, B);
  const int ks = b.spec.kernel, st = b.spec.stride;
  //                              KS S KCT  H   W  CEXP CC NTP G SEG NTHR WPE
  if (b.H == 25) return launch_mid_inst<3, 2, 1, 25, 20, 96, 16, 2, 1, 1, 1024, 4>(s, stage, a);                  // 2a
  if (b.H == 13 && ks == 3) return launch_mid_inst<3, 1, 2, 13, 10, 144, 48, 2, 1, 5, 1024, 4, true>(s, stage, a);     // 2b: pair strips of half an output row (67.1 vs 67.8 us with quad items; 512 threads: 71-74 us)
  if (b.H == 13) return launch_mid_inst<5, 2, 2, 13, 10, 144, 48, 3, 1, 5, 512, 4, true>(s, stage, a);            // 3a: pair strips of a whole output row
  if (st == 1) return launch_mid_inst<5, 1, 3, 7, 5, 240, 48, 3, 1, 1, 512, 4>(s, stage, a);                      // 3b
  if (one_clip) return launch_mid_inst<3, 2, 3, 7, 5, 240, 48, 5, 1, 3, 512, 4, true>(s, stage, a);                // 4a on handles of <= 256 clips: a workgroup per clip (two-clip workgroups leave half the CUs idle there)
  return launch_mid_inst<3, 2, 3, 7, 5, 240, 48, 5, 2, 3, 512, 4, true>(s, stage, a);                             // 4a: the same
}

// Back half (SE + gated projection in one launch) for the blocks that keep mbconv_front_kernel: 2a, 2b, 3b -- and 3a / 4a where the whole-block
// (mid) kernel is not taken: one-clip serving handles split those blocks into front + back so that several CUs work on the window, and the back
// launch replaces se_reduce + se_expand + the gated projection GEMM (three dependent launches, 14.5 us of a live window, by one of ~7).
bool back_supported(const BlockPlan& b) {
  if (!b.has_expand || b.se.se > 10) return false;
  const int hw = b.Ho * b.Wo;
  return (hw == 130 && b.ce == 96 && b.spec.out_ch == 24) || (hw == 130 && b.ce == 144 && b.spec.out_ch == 24) || (hw == 35 && b.ce == 240 && b.spec.out_ch == 40) ||
         (hw == 35 && b.ce == 144 && b.spec.out_ch == 40) || (hw == 12 && b.ce == 240 && b.spec.out_ch == 80);
}

template <int HOWO, int CEXP, int NTP, int RS, int NTHR, int WPE>
int launch_back_inst(hipStream_t s, const char* stage, const BackArgs& a) {
  constexpr int SCR = (RS * CEXP > NTHR) ? RS * CEXP : NTHR;
  constexpr size_t lds = ((size_t)HOWO * (CEXP + 4) + 2 * CEXP + 16 + SCR) * sizeof(float);
  ProfScope ps(stage, std::string("mbconv_back_kernel<") + std::to_string(HOWO) + "," + std::to_string(CEXP) + "," + std::to_string(NTP) + "," + std::to_string(NTHR) + ">");
  wg_trace_arm();
  if (int rc = launch_big_lds(&mbconv_back_kernel<HOWO, CEXP, NTP, RS, NTHR, WPE>, 160 * 1024, dim3(a.B), dim3(NTHR), lds, s, a)) return rc;
  wg_trace_report(s, stage, "back", (size_t)a.B);
  return MKWS_OK;
}

int launch_back(hipStream_t s, const char* stage, const BlockPlan& b, const float* D, const float* X, float* Y, float* dbg_gate, int B) {
  BackArgs a = {};
  a.D = D; a.X = X; a.Cin = b.spec.in_ch;
  a.Wr = b.se.Wr; a.br = b.se.br; a.We = b.se.We; a.be = b.se.be; a.se = b.se.se;
  a.WpP = b.project.Wp; a.scP = b.project.scale; a.shP = b.project.shift;
  a.Y = Y; a.Cout = b.spec.out_ch; a.residual = b.residual ? 1 : 0; a.dbg_gate = dbg_gate; a.B = B;
  //                          HOWO CEXP NTP RS NTHR WPE
  const int hw = b.Ho * b.Wo;
  if (b.ce == 96) return launch_back_inst<130, 96, 2, 8, 512, 4>(s, stage, a);   // 2a: 52 KB of LDS -> 3 workgroups per CU
  if (b.ce == 144 && hw == 130) return launch_back_inst<130, 144, 2, 4, 512, 4>(s, stage, a);  // 2b: 80.5 KB -> 2 per CU
  if (b.ce == 144) return launch_back_inst<35, 144, 3, 4, 512, 4>(s, stage, a);   // 3a (handles without the mid kernel): 22 KB
  if (hw == 12) return launch_back_inst<12, 240, 5, 4, 512, 4>(s, stage, a);      // 4a (the same): 15 KB; five n-tiles on five of the eight waves
  return launch_back_inst<35, 240, 3, 4, 512, 4>(s, stage, a);                    // 3b: 39 KB -> 4 per CU by LDS; 91 VGPRs keep it at 2 (6 waves per SIMD spills 37 registers: tried in round 4)
}

void launch_se(hipStream_t s, const char* stage, const BlockPlan& b, const float* sums, float* part, float* gate, int B) {
  const SeLayer& L = b.se;
  int nsl = L.KCr / 4; if (nsl < 1) nsl = 1; if (nsl > 8) nsl = 8;       // K slices of the reduce FC
  int nsp = L.NTe / 4; if (nsp < 1) nsp = 1; if (nsp > 8) nsp = 8;       // column slices of the expand FC
  const int nb = (B + 15) / 16;
  const float inv = 1.0f / (float)(b.Ho * b.Wo);
#define MKWS_SE(N)                                                                                                            \
  do {                                                                                                                        \
    {                                                                                                                         \
      ProfScope ps(std::string(stage) + "#reduce", std::string("se_reduce_kernel<") + std::to_string(N) + ">");             \
      hipLaunchKernelGGL((se_reduce_kernel<N>), dim3(nb, nsl), dim3(256), 0, s, sums, inv, L.WrP, part, B, b.ce, L.KCr, nsl);  \
    }                                                                                                                         \
    {                                                                                                                         \
      ProfScope ps(stage, std::string("se_expand_kernel<") + std::to_string(N) + ">");                                      \
      hipLaunchKernelGGL((se_expand_kernel<N>), dim3(nb, nsp), dim3(256), 0, s, part, nsl, L.br, L.WeP, L.be, gate, B, b.ce, \
                         L.se, L.NTe, nsp);                                                                                  \
    }                                                                                                                         \
  } while (0)
  switch (L.NTR) {
    case 1: MKWS_SE(1); break;
    case 2: MKWS_SE(2); break;
    default: MKWS_SE(3); break;
  }
#undef MKWS_SE
}

// Paired-kernel health: a failed exchange (see mbconv_pair_kernel) left a nonzero word in host-mapped memory.  Read here without
// synchronising, at the top of every entry point that runs the network: the handle leaves the paired kernel for good
// (mbconv_block_kernel computes the same blocks), flags and error words are cleared in stream order, and the CALL FAILS with
// MKWS_ERR_EXCHANGE because a result the caller already holds (the failing forward was asynchronous) is poisoned with NaN.
// The caller repeats the call; it then runs on the single-workgroup plan.
int check_pair_health(mkws_embed* em, hipStream_t s) {
  if (!em->pair_err_host) return MKWS_OK;
  const int code = *reinterpret_cast<volatile int*>(em->pair_err_host);
  if (code == 0) return MKWS_OK;
  em->fuse_pair = 0;
  em->fuse_cluster = 0;
  em->fuse_cluster_chain = 0;
  em->pair_fault = 0;
  ++em->pair_degraded;
  *reinterpret_cast<volatile int*>(em->pair_err_host) = 0;
  MKWS_HIP(hipMemsetAsync(em->pair_flags, 0, em->pair_flag_count * sizeof(int), s));
  MKWS_HIP(hipMemsetAsync(em->pair_err_dev, 0, sizeof(int), s));
  if (em->cl_flags) MKWS_HIP(hipMemsetAsync(em->cl_flags, 0, em->cl_flag_count * sizeof(int), s));
  return fail(MKWS_ERR_EXCHANGE, "paired whole-block kernel: %s in an earlier forward of this handle -- that forward's embeddings are NaN-poisoned; "
              "the handle now uses one workgroup per 4 clips (fuse_pair = 0): repeat the call",
              code == kPairErrXcc ? "the two halves of a pair ran on different XCDs" : "a half timed out waiting for its partner");
}

// ---- routing: which launch path a block takes ----------------------------------------------------------------------------------
// In order of precedence.  The three chain paths run blocks i .. last in one launch; every other path runs block i alone.
enum class Path {
  Fused1a,        // block 1a inside stem_block1a_kernel (already launched with the stem)
  Mid,            // mbconv_mid_kernel (big-image blocks)
  Chain,          // mbconv_chain_kernel (4x3-image blocks)
  PairChain,      // mbconv_pair_chain_kernel (stride-1 2x2-image blocks, + top conv and pool when with_top)
  ClusterChain,   // mbconv_cluster_chain_kernel (one-clip handles: every tiny-image block)
  Cluster,        // mbconv_cluster_kernel
  Pair,           // mbconv_pair_kernel
  Block,          // mbconv_block_kernel
  Split           // front (or expand GEMM + depthwise) then back (or SE FCs + gated projection GEMM)
};
struct Route { Path path; int last; bool with_top; };

static bool tap_is(const char* stop, const BlockPlan& b, const char* suffix) { return stop && std::string("block") + b.spec.name + suffix == stop; }
// "_expand" / "_dw" / "_gate" of a block: a chain stops in front of such a block and leaves it to the single-block paths
static bool inner_tap(const char* stop, const BlockPlan& b) { return tap_is(stop, b, "_expand") || tap_is(stop, b, "_dw") || tap_is(stop, b, "_gate"); }
// whole block 1a with the stem (its inner taps come from the separate kernels); SE is at most 8 units wide there
static bool fused_1a(const mkws_embed* em, const char* stop) {
  const BlockPlan& b = em->blocks[0];
  return em->fuse_stem && !(stop && strcmp(stop, "stem") == 0) && b.se.se <= 8 && !b.has_expand && b.spec.out_ch == 16 && !tap_is(stop, b, "_dw") && !tap_is(stop, b, "_gate");
}

Route route_block(const mkws_embed* em, int i, int B, const char* stop) {
  const BlockPlan& b = em->blocks[i];
  if (i == 0 && fused_1a(em, stop)) return {Path::Fused1a, i, false};
  const bool want_expand_tap = tap_is(stop, b, "_expand");      // only the unfused path materialises the expand output
  if (mid_enabled(b, em->fuse_mid) && !want_expand_tap) return {Path::Mid, i, false};
  // depth-fused chains: a block whose output is tapped ends the chain, a block whose inner taps are wanted is not entered
  auto extend = [&](int max_len, bool (*member)(const mkws_embed*, const BlockPlan&), bool (*link_ok)(const BlockPlan&, const BlockPlan&)) {
    int e = i;
    while (e + 1 < kNumBlocks && e + 1 - i < max_len && !tap_is(stop, em->blocks[e], "") && member(em, em->blocks[e + 1]) &&
           link_ok(em->blocks[e], em->blocks[e + 1]) && !inner_tap(stop, em->blocks[e + 1])) ++e;
    return e;
  };
  if (chain_member(em, b) && !inner_tap(stop, b)) return {Path::Chain, extend(kChainMax, chain_member, chain_link_ok), false};
  if (pair_chain_member(em, b) && !inner_tap(stop, b)) {
    const int e = extend(kPairChainMax, pair_chain_member, pair_chain_link_ok);
    // the top conv (+ BN + swish + global average pool) rides as the chain's last phase when nothing between here and the pooled
    // features is tapped
    const bool with_top = em->fuse_top && em->fuse_gap && (!stop || strcmp(stop, "gap") == 0 || strncmp(stop, "dense", 5) == 0) && e == kNumBlocks - 1 && em->topH * em->topW == 4;
    return {Path::PairChain, e, with_top};
  }
  if (B == 1 && em->fuse_block && em->fuse_cluster_chain && cluster_supported(b) && !stop) {
    // a live window's tiny-image blocks from here to the top conv as ONE launch (no taps inside: those run launch by launch)
    int e = i;
    while (e + 1 < kNumBlocks && e + 1 - i < kClusterChainMax && cluster_supported(em->blocks[e + 1])) ++e;
    if (cluster_chain_ok(em, i, e)) return {Path::ClusterChain, e, false};
  }
  if (em->fuse_block && block_supported(b, em->fuse_block) && !want_expand_tap) {
    if (cluster_enabled(em, b)) return {Path::Cluster, i, false};
    if (em->fuse_pair && pair_supported(b)) return {Path::Pair, i, false};
    return {Path::Block, i, false};
  }
  return {Path::Split, i, false};
}

// Runs the network; stops after `stop` (nullptr = run everything).  On stop, *tap_src/*tap_count describe
// the buffer holding that stage's output.
int run_forward(mkws_embed* em, const float* d_spec, int B, float* d_emb, hipStream_t s, const char* stop,
                const float** tap_src, size_t* tap_count) {
  SplitWs sw; sw.p = em->splitk_ws; sw.floats = em->splitk_floats; sw.gemv = em->fuse_gemv;
  auto hit = [&](const std::string& name, const float* p, size_t n) {
    if (stop && name == stop) { *tap_src = p; *tap_count = n; return true; }
    return false;
  };
  const BlockPlan& blk1a = em->blocks[0];
  if (fused_1a(em, stop)) {
    ProfScope ps("block1a", "stem_block1a_kernel");
    const size_t lds = ((size_t)((51 * 41 + 3) & ~3) + 27 * 22 * 32 + 500 * 36 + 64 * 4 + 32 + 16 + 32) * sizeof(float);
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&stem_block1a_kernel), 160 * 1024)) return rc;
    const int nwg = B < device_cu_count() ? B : device_cu_count();
    wg_trace_arm();
    hipLaunchKernelGGL(stem_block1a_kernel, dim3(nwg), dim3(512), lds, s, d_spec, em->stem_w, em->stem_scale, em->stem_shift, em->norm_mean,
                       em->norm_std, blk1a.dw.Wd, blk1a.dw.scale, blk1a.dw.shift, blk1a.se.Wr, blk1a.se.br, blk1a.se.We, blk1a.se.be,
                       blk1a.se.se, blk1a.project.Wp, blk1a.project.scale, blk1a.project.shift, em->bufB, B);
    wg_trace_report(s, "block1a", "stem_block1a", (size_t)nwg);
    wg_phase_report("block1a: prologue / stem / depthwise + next stage / SE / projection", (size_t)nwg, 5);
  } else {
    const long pix = (long)B * 500;
    int grid = (int)((pix + 31) / 32);
    if (grid > 8192) grid = 8192;
    ProfScope ps("stem", "stem_kernel");
    hipLaunchKernelGGL(stem_kernel, dim3(grid), dim3(256), 0, s, d_spec, em->stem_w, em->stem_scale, em->stem_shift,
                       em->norm_mean, em->norm_std, em->bufA, B);
    if (hit("stem", em->bufA, (size_t)B * 500 * kStemCh)) return MKWS_OK;
  }
  float* cur = em->bufA;
  float* nxt = em->bufB;
  bool top_done = false;
  for (int i = 0; i < kNumBlocks; ++i) {
    const BlockPlan& b = em->blocks[i];
    const std::string p = std::string("block") + b.spec.name;
    const int Min = B * b.H * b.W, Mout = B * b.Ho * b.Wo;
    const Route r = route_block(em, i, B, stop);
    // the single-block kernels serve the "_dw" / "_gate" taps from their debug stores
    float* const dbg_dw = tap_is(stop, b, "_dw") ? em->bufD : nullptr;
    float* const dbg_gate = tap_is(stop, b, "_gate") ? em->gate : nullptr;
    bool swap = true;       // the path leaves its output in nxt
    int rc = MKWS_OK;
    switch (r.path) {
      case Path::Fused1a: break;          // already computed into nxt (= bufB) by stem_block1a_kernel
      case Path::Mid: rc = launch_mid(s, p.c_str(), b, em->block_mt43 == 1, cur, nxt, dbg_dw, dbg_gate, B); break;
      case Path::Chain: rc = launch_chain(s, em, i, r.last, cur, nxt, B); break;
      case Path::PairChain:
        rc = launch_pair_chain(s, em, i, r.last, cur, nxt, B, r.with_top);
        top_done = r.with_top;
        break;
      case Path::ClusterChain:
        rc = launch_cluster_chain(s, em, i, r.last, cur, nxt);
        swap = ((r.last - i + 1) & 1) != 0;       // (an even number of blocks ends in the buffer it started from)
        break;
      case Path::Cluster: rc = launch_cluster(s, p.c_str(), b, i, em, cur, nxt, dbg_dw, dbg_gate, B); break;
      case Path::Pair: {
        PairWs pw; pw.xc1 = em->pair_xc1; pw.xd = em->pair_xd; pw.flags = em->pair_flags; pw.mt = em->pair_mt;
        pw.err_dev = em->pair_err_dev; pw.err_host = em->pair_err_host; pw.fault = em->pair_fault;
        rc = launch_pair(s, p.c_str(), b, pw, cur, nxt, dbg_dw, dbg_gate, B);
        break;
      }
      case Path::Block: rc = launch_block(s, p.c_str(), b, em->block_mt43, cur, nxt, dbg_dw, dbg_gate, B, em->fuse_se4 != 0); break;
      case Path::Split:
        if (b.has_expand && (tap_is(stop, b, "_expand") || !em->fuse_front)) {
          // unfused path: kept for the "<block>_expand" parity tap and as an A/B switch (mkws_embed_set_option)
          launch_gemm(s, sw, (p + "_expand").c_str(), b.expand, cur, b.spec.in_ch, Min, em->max_batch * b.H * b.W, ACT_SWISH, nullptr, 0, nullptr, 0, em->bufE, b.ce);
          if (hit(p + "_expand", em->bufE, (size_t)Min * b.ce)) return MKWS_OK;
          launch_dw(s, (p + "_dw").c_str(), b, em->bufE, em->bufD, em->sums, B);
        } else if (b.has_expand && front_supported(b)) {
          launch_front(s, (p + "_dw").c_str(), b, cur, em->bufD, em->sums, B, em->fuse_walk && em->max_batch >= 128);   // (small handles keep one workgroup per channel block: three CUs per clip instead of one)
        } else if (b.has_expand) {
          launch_gemm(s, sw, (p + "_expand").c_str(), b.expand, cur, b.spec.in_ch, Min, em->max_batch * b.H * b.W, ACT_SWISH, nullptr, 0, nullptr, 0, em->bufE, b.ce);
          launch_dw(s, (p + "_dw").c_str(), b, em->bufE, em->bufD, em->sums, B);
        } else {
          launch_dw(s, (p + "_dw").c_str(), b, cur, em->bufD, em->sums, B);
        }
        if (hit(p + "_dw", em->bufD, (size_t)Mout * b.ce)) return MKWS_OK;       // (here and below: a tap returns before the launches behind it)
        if (em->fuse_back && back_supported(b)) {
          // SE + gated projection of this block in one launch, the clip's depthwise output staged in LDS once
          rc = launch_back(s, p.c_str(), b, em->bufD, cur, nxt, dbg_gate, B);
          break;
        }
        launch_se(s, (p + "_gate").c_str(), b, em->sums, em->se_part, em->gate, B);
        if (hit(p + "_gate", em->gate, (size_t)B * b.ce)) return MKWS_OK;
        launch_gemm(s, sw, p.c_str(), b.project, em->bufD, b.ce, Mout, em->max_batch * b.Ho * b.Wo, ACT_NONE, em->gate, b.Ho * b.Wo, b.residual ? cur : nullptr,
                    b.spec.out_ch, nxt, b.spec.out_ch);
        break;
    }
    if (rc) return rc;
    // taps of the block(s) just run (a chain never holds block i's inner taps, and its output tap is its last block's), then on to the next
    const BlockPlan& bl = em->blocks[r.last];
    if (hit(p + "_dw", em->bufD, (size_t)Mout * b.ce)) return MKWS_OK;
    if (hit(p + "_gate", em->gate, (size_t)B * b.ce)) return MKWS_OK;
    if (hit(std::string("block") + bl.spec.name, nxt, (size_t)B * bl.Ho * bl.Wo * bl.spec.out_ch)) return MKWS_OK;
    if (swap) { float* t = cur; cur = nxt; nxt = t; }
    i = r.last;
  }
  const int HWt = em->topH * em->topW;
  const bool fuse_gap = em->fuse_gap && HWt == 4 && !(stop && strcmp(stop, "top") == 0);
  if (top_done) {
    // (already computed by the paired chain's last phase)
  } else if (fuse_gap) {
    // top conv + BN + swish + global average pool in one launch: the [B*4, 1280] tensor never reaches HBM
    launch_gemm(s, sw, "top", em->top, cur, em->top.K, B * HWt, em->max_batch * HWt, ACT_SWISH, nullptr, 0, nullptr, 0, em->gap, kTopCh, 1);
  } else {
    launch_gemm(s, sw, "top", em->top, cur, em->top.K, B * HWt, em->max_batch * HWt, ACT_SWISH, nullptr, 0, nullptr, 0, em->bufE, kTopCh);
    if (hit("top", em->bufE, (size_t)B * HWt * kTopCh)) return MKWS_OK;
  }
  if (!fuse_gap && !top_done) {
    const long total = (long)B * (kTopCh / 4);
    ProfScope ps("gap", "mean_hw_kernel");
    hipLaunchKernelGGL(mean_hw_kernel, dim3((int)((total + 255) / 256)), dim3(256), 0, s, em->bufE, em->gap, B, HWt, kTopCh);
  }
  if (hit("gap", em->gap, (size_t)B * kTopCh)) return MKWS_OK;
  launch_gemm(s, sw, "dense", em->dense0, em->gap, kTopCh, B, em->max_batch, ACT_RELU, nullptr, 0, nullptr, 0, em->d0, kDense0);
  if (hit("dense", em->d0, (size_t)B * kDense0)) return MKWS_OK;
  launch_gemm(s, sw, "dense_1", em->dense1, em->d0, kDense0, B, em->max_batch, ACT_RELU, nullptr, 0, nullptr, 0, em->d1, kDense1);
  if (hit("dense_1", em->d1, (size_t)B * kDense1)) return MKWS_OK;
  float* out = d_emb ? d_emb : em->d0;
  // NaN from a failed pair exchange does not survive the ReLUs above (max(NaN, 0) = 0), so the LAST layer reads the sticky error
  // word itself: a forward that ran a failed exchange returns all-NaN embeddings, never plausible numbers
  sw.poison = em->pair_err_dev;
  launch_gemm(s, sw, "dense_2", em->dense2, em->d1, kDense1, B, em->max_batch, ACT_SELU, nullptr, 0, nullptr, 0, out, kEmbDim);
  if (hit("dense_2", out, (size_t)B * kEmbDim)) return MKWS_OK;
  if (stop) return fail(MKWS_ERR_INVALID_ARG, "unknown stage '%s'", stop);
  return MKWS_OK;
}

}  // namespace

extern "C" {

size_t mkws_embed_weight_count(void) {
  const auto v = enumerate_tensors();
  return v.back().offset + v.back().count;
}

int mkws_embed_weight_manifest(char* dst, size_t cap) {
  const auto v = enumerate_tensors();
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

int mkws_embed_create(const float* h, size_t n_floats, int max_batch, mkws_embed** out) {
  if (!h || !out) return fail(MKWS_ERR_INVALID_ARG, "weights/out is NULL");
  *out = nullptr;
  if (max_batch <= 0) return fail(MKWS_ERR_INVALID_ARG, "max_batch must be positive");
  if (n_floats != mkws_embed_weight_count())
    return fail(MKWS_ERR_BAD_WEIGHTS, "weight blob has %zu floats, architecture needs %zu", n_floats, mkws_embed_weight_count());
  int rc = require_device();
  if (rc != MKWS_OK) return rc;
  const auto tens = enumerate_tensors();
  auto T = [&](const std::string& name) -> const float* {
    for (const auto& t : tens) if (t.name == name) return h + t.offset;
    return nullptr;
  };
  for (size_t i = 0; i < n_floats; ++i)
    if (!std::isfinite(h[i])) return fail(MKWS_ERR_BAD_WEIGHTS, "weight blob has a non-finite value at %zu", i);

  mkws_embed* em = new (std::nothrow) mkws_embed();
  if (!em) return fail(MKWS_ERR_ALLOC, "out of host memory");
  em->max_batch = max_batch;
  em->plan_batch = max_batch;
  // Plan: whole-block kernels (+ the paired kernel where the device's dispatch order passed the probe) for EVERY handle size.
  // Round 2 gave handles below 384 clips the multi-kernel path (a whole-block kernel re-streams a block's weights once per 4
  // clips, and with launch-by-launch calls that lost below ~300 clips).  Since the serving paths replay hipGraphs the count of
  // dependent launches is what a small batch pays for (23 instead of ~65): tools/plan_sweep.py, graph replay, clips/s multi-kernel
  // vs whole-block + pair: batch 1 2243 / 2289, 16 31.9 k / 34.7 k, 64 122 k / 136 k, 256 396 k / 479 k, 384 511 k / 630 k.
  // The multi-kernel path stays behind mkws_embed_set_option (A/B, parity taps).  Per handle, so results stay bit-identical
  // across the batch sizes one handle sees.
  em->fuse_block = 2;
  // (one-clip handles = live windows: the split front / back kernels put a clip's channel blocks on several CUs where the whole-block
  //  kernel is ONE workgroup: 0.3056 -> 0.3023-0.3041 ms per window, tools/latency_ab.py fuse_mid, two rounds)
  em->fuse_mid = (max_batch == 1) ? 0 : 1;
  em->fuse_back = 1;
  em->fuse_pair = pair_layout_ok() ? 1 : 0;
  // small-batch (live serving) handles: the tiny-image blocks on the 6-way cluster kernel, same dispatch-order premise as the pairs
  em->fuse_cluster = (max_batch <= kClusterMaxBatch && em->fuse_pair) ? 1 : 0;
  em->fuse_cluster_chain = (max_batch == 1 && em->fuse_cluster) ? 1 : 0;
  em->pair_mt = pair_row_tiles(max_batch);
  em->block_mt43 = block43_row_tiles(max_batch);
  (void)hipGetDevice(&em->device);
  Packer pk;
  std::vector<float> sc, sh;

  // stem
  em->norm_mean = *T("normalization/mean");
  {
    const float sd = std::sqrt(*T("normalization/variance"));
    em->norm_std = sd > 1e-7f ? sd : 1e-7f;
  }
  const size_t o_stem_w = pk.add(T("stem_conv/kernel"), 9 * kStemCh);
  fold_bn(T("stem_bn/gamma"), T("stem_bn/beta"), T("stem_bn/moving_mean"), T("stem_bn/moving_variance"), kStemCh, &sc, &sh);
  const size_t o_stem_sc = pk.add(sc.data(), kStemCh), o_stem_sh = pk.add(sh.data(), kStemCh);

  struct BlockOff { GemmOff expand, project, se_r, se_e; size_t dw_w, dw_sc, dw_sh, se_wr, se_we; Se4Off se4; } bo[kNumBlocks];
  int H = 25, W = 20;
  for (int i = 0; i < kNumBlocks; ++i) {
    BlockPlan& b = em->blocks[i];
    b.spec = kBlocks[i];
    const std::string p = std::string("block") + b.spec.name;
    b.ce = b.spec.in_ch * b.spec.expand;
    b.has_expand = b.spec.expand != 1;
    b.residual = (b.spec.stride == 1 && b.spec.in_ch == b.spec.out_ch);
    b.H = H; b.W = W;
    if (b.spec.stride == 2) {
      int pt, pb, pl, pr;
      correct_pad(H, W, b.spec.kernel, &pt, &pb, &pl, &pr);
      b.pt = pt; b.pl = pl;
      b.Ho = (H + pt + pb - b.spec.kernel) / 2 + 1;
      b.Wo = (W + pl + pr - b.spec.kernel) / 2 + 1;
    } else {
      b.pt = b.pl = b.spec.kernel / 2;
      b.Ho = H; b.Wo = W;
    }
    const int se = se_channels(b.spec);
    b.se.se = se;
    std::vector<float> ones;
    if (b.has_expand) {
      fold_bn(T(p + "_expand_bn/gamma"), T(p + "_expand_bn/beta"), T(p + "_expand_bn/moving_mean"), T(p + "_expand_bn/moving_variance"), b.ce, &sc, &sh);
      bo[i].expand = pack_gemm(pk, T(p + "_expand_conv/kernel"), b.spec.in_ch, b.ce, sc, sh);
    }
    bo[i].dw_w = pk.add(T(p + "_dwconv/depthwise_kernel"), (size_t)b.spec.kernel * b.spec.kernel * b.ce);
    fold_bn(T(p + "_bn/gamma"), T(p + "_bn/beta"), T(p + "_bn/moving_mean"), T(p + "_bn/moving_variance"), b.ce, &sc, &sh);
    bo[i].dw_sc = pk.add(sc.data(), b.ce); bo[i].dw_sh = pk.add(sh.data(), b.ce);
    {
      std::vector<float> one_r(se, 1.0f), bias_r(T(p + "_se_reduce/bias"), T(p + "_se_reduce/bias") + se);
      bo[i].se_r = pack_gemm(pk, T(p + "_se_reduce/kernel"), b.ce, se, one_r, bias_r);
      bo[i].se_wr = pk.add(T(p + "_se_reduce/kernel"), (size_t)b.ce * se);     // plain [C][se] for the fused partials
      bo[i].se_we = pk.add(T(p + "_se_expand/kernel"), (size_t)se * b.ce);     // plain [se][C] (stem_block1a_kernel)
      std::vector<float> one_e(b.ce, 1.0f), bias_e(T(p + "_se_expand/bias"), T(p + "_se_expand/bias") + b.ce);
      bo[i].se_e = pack_gemm(pk, T(p + "_se_expand/kernel"), se, b.ce, one_e, bias_e);
      if (bo[i].se_r.NTtot > 3) { mkws_embed_destroy(em); return fail(MKWS_ERR_UNSUPPORTED, "SE width %d > 48", se); }
      if (H == 4 && W == 3 && b.has_expand) bo[i].se4 = pack_se4(pk, T(p + "_se_reduce/kernel"), T(p + "_se_expand/kernel"), b.ce, se, kBlockWaves);
    }
    fold_bn(T(p + "_project_bn/gamma"), T(p + "_project_bn/beta"), T(p + "_project_bn/moving_mean"), T(p + "_project_bn/moving_variance"), b.spec.out_ch, &sc, &sh);
    bo[i].project = pack_gemm(pk, T(p + "_project_conv/kernel"), b.ce, b.spec.out_ch, sc, sh);
    H = b.Ho; W = b.Wo;
  }
  em->topH = H; em->topW = W;
  fold_bn(T("top_bn/gamma"), T("top_bn/beta"), T("top_bn/moving_mean"), T("top_bn/moving_variance"), kTopCh, &sc, &sh);
  const GemmOff o_top = pack_gemm(pk, T("top_conv/kernel"), kBlocks[kNumBlocks - 1].out_ch, kTopCh, sc, sh);
  auto dense = [&](const char* name, int K, int N) {
    std::vector<float> one(N, 1.0f), bias(T(std::string(name) + "/bias"), T(std::string(name) + "/bias") + N);
    return pack_gemm(pk, T(std::string(name) + "/kernel"), K, N, one, bias);
  };
  const GemmOff o_d0 = dense("dense", kTopCh, kDense0);
  const GemmOff o_d1 = dense("dense_1", kDense0, kDense1);
  const GemmOff o_d2 = dense("dense_2", kDense1, kEmbDim);

  // upload
  const size_t wbytes = pk.buf.size() * sizeof(float);
  // every failure exit from here on leaves through mkws_embed_destroy, which frees what has been allocated so far
  auto give_up = [&](int code, const char* what) { mkws_embed_destroy(em); return fail(code, "%s", what); };
  if (hipMalloc(reinterpret_cast<void**>(&em->d_weights), wbytes) != hipSuccess) { mkws_embed_destroy(em); return fail(MKWS_ERR_ALLOC, "hipMalloc(%zu) for weights failed", wbytes); }
  if (hipMemcpy(em->d_weights, pk.buf.data(), wbytes, hipMemcpyHostToDevice) != hipSuccess) return give_up(MKWS_ERR_HIP, "weight upload failed");
  const float* d = em->d_weights;
  auto G = [&](const GemmOff& o) { GemmLayer L; L.Wp = d + o.Wp; L.scale = d + o.scale; L.shift = d + o.shift; L.K = o.K; L.N = o.N; L.KC = o.KC; L.NTtot = o.NTtot; return L; };
  em->stem_w = d + o_stem_w; em->stem_scale = d + o_stem_sc; em->stem_shift = d + o_stem_sh;
  for (int i = 0; i < kNumBlocks; ++i) {
    BlockPlan& b = em->blocks[i];
    if (b.has_expand) b.expand = G(bo[i].expand);
    b.project = G(bo[i].project);
    b.dw.Wd = d + bo[i].dw_w; b.dw.scale = d + bo[i].dw_sc; b.dw.shift = d + bo[i].dw_sh;
    b.se.Wr = d + bo[i].se_wr; b.se.We = d + bo[i].se_we; b.se.WrP = d + bo[i].se_r.Wp; b.se.br = d + bo[i].se_r.shift; b.se.WeP = d + bo[i].se_e.Wp; b.se.be = d + bo[i].se_e.shift;
    b.se.KCr = bo[i].se_r.KC; b.se.NTR = bo[i].se_r.NTtot; b.se.NTe = bo[i].se_e.NTtot;
    if (bo[i].se4.T0) { b.se.WrQ = d + bo[i].se4.r; b.se.WeQ = d + bo[i].se4.e; b.se.T0 = bo[i].se4.T0; b.se.NQ = bo[i].se4.NQ; }
    // the expand FC's K (= se) is padded to NTR*16 by pack_gemm: KC of se_e == NTR by construction
  }
  em->top = G(o_top); em->dense0 = G(o_d0); em->dense1 = G(o_d1); em->dense2 = G(o_d2);
  {
    // constants of every block for the chain kernels (blocks without an expand conv are never chained: their entries stay zero)
    std::vector<BlockArgs> tab(kNumBlocks);
    memset(static_cast<void*>(tab.data()), 0, sizeof(BlockArgs) * kNumBlocks);
    for (int i = 0; i < kNumBlocks; ++i)
      if (em->blocks[i].has_expand) tab[i] = block_args(em->blocks[i]);
    if (hipMalloc(reinterpret_cast<void**>(&em->d_chain_tab), sizeof(BlockArgs) * kNumBlocks) != hipSuccess ||
        hipMemcpy(em->d_chain_tab, tab.data(), sizeof(BlockArgs) * kNumBlocks, hipMemcpyHostToDevice) != hipSuccess) return give_up(MKWS_ERR_ALLOC, "block table upload failed");
  }

  // workspace: ONE list of (buffer, floats), in carve order -- the allocation is its sum, the carve walks it, and in guard-band mode a band
  // follows every entry (and precedes the first)
  const size_t mb = (size_t)max_batch, np = (size_t)pair_count(max_batch, em->pair_mt);
  // cluster exchange buffers exist for handles that may ever use the kernel (the option can be set after create up to 64 clips)
  // (a one-clip handle's chain launch gives every block an exchange slot of its own: blocks on different XCDs must never hold dirty copies of one line)
  const size_t ncl = (max_batch == 1) ? 16 : (max_batch <= 64) ? (size_t)cluster_count(max_batch, 1) : 0;
  em->splitk_floats = 20480 * mb;
  // mbconv_pair_kernel: [pairs][2 exchanges][2 halves] | mbconv_pair_chain_kernel: [pairs][blocks][2][2] | the error word (cleared with the flags)
  em->pair_flag_count = np * 4 + np * 4 * kPairChainMax;
  em->cl_flag_count = ncl * 2 * kClFlagRow * kNumBlocks;
  float *pair_flags = nullptr, *cl_flags = nullptr;        // (carved like the rest, used as ints)
  std::vector<std::pair<float**, size_t>> carves = {
      {&em->bufA, 16000 * mb}, {&em->bufB, 16000 * mb}, {&em->bufE, 48000 * mb}, {&em->bufD, 18720 * mb},
      {&em->sums, 1152 * mb}, {&em->gate, 1152 * mb}, {&em->gap, 1280 * mb}, {&em->d0, 2048 * mb}, {&em->d1, 2048 * mb},
      {&em->splitk_ws, em->splitk_floats},
      {&em->se_part, 9 * 48 * mb + 8 * 768},      // 8 slices x ceil(mb/16) groups x 768 floats <= 384*mb + 6144
      {&em->pair_xc1, np * 2 * kPairXc1}, {&em->pair_xd, np * 2 * kPairXdAll * 2 * 256}, {&pair_flags, em->pair_flag_count + 4}};
  if (ncl > 0) {
    carves.push_back({&em->cl_xc1, ncl * kClusterPMax * kClXc1});
    carves.push_back({&em->cl_xd, ncl * kClusterPMax * kClMaxTiles * 256});
    carves.push_back({&cl_flags, em->cl_flag_count});
  }
  {
    const char* g = getenv("MKWS_EMBED_GUARD");
    const long gv = g ? atol(g) : 0;
    em->guard = gv > 0 ? (size_t)((gv + 63) / 64 * 64) : 0;      // whole 256-byte lines: the carve keeps its alignment
  }
  // one 256-byte line behind the last carve: the kernels read the workspace with 16-byte vector loads, and the end of the last buffer is
  // then never the end of the allocation
  constexpr size_t kWsTailPad = 64;
  size_t ws = em->guard + kWsTailPad;
  for (const auto& c : carves) ws += c.second + em->guard;
  if (hipMalloc(reinterpret_cast<void**>(&em->d_ws), ws * sizeof(float)) != hipSuccess) { mkws_embed_destroy(em); return fail(MKWS_ERR_ALLOC, "hipMalloc(%zu) for workspace failed", ws * sizeof(float)); }
  if (em->guard && hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(em->d_ws), (int)kGuardCanary, ws) != hipSuccess) return give_up(MKWS_ERR_HIP, "filling the guarded workspace failed");
  float* w = em->d_ws;
  if (em->guard) { em->guard_spans.emplace_back(0, em->guard); w += em->guard; }
  for (const auto& c : carves) {
    *c.first = w;
    w += c.second;
    if (em->guard) { em->guard_spans.emplace_back((size_t)(w - em->d_ws), em->guard); w += em->guard; }
  }
  em->pair_flags = reinterpret_cast<int*>(pair_flags);
  em->pair_chain_flags = em->pair_flags + np * 4;
  em->pair_err_dev = em->pair_flags + em->pair_flag_count;
  if (hipMemset(em->pair_flags, 0, (em->pair_flag_count + 4) * sizeof(int)) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&em->pair_err_host), 64, hipHostMallocMapped) != hipSuccess) return give_up(MKWS_ERR_HIP, "setting up the pair flags failed");
  *em->pair_err_host = 0;
  if (ncl > 0) {
    em->cl_flags = reinterpret_cast<int*>(cl_flags);
    if (hipMemset(em->cl_flags, 0, em->cl_flag_count * sizeof(int)) != hipSuccess) return give_up(MKWS_ERR_HIP, "clearing the cluster flags failed");
  }
  *out = em;
  return MKWS_OK;
}

// Guard-band mode: how many guard words no longer hold the canary (synchronises the device; 0 when the mode is off)
static int guard_violations(const mkws_embed* em) {
  if (!em->guard) return 0;
  if (hipDeviceSynchronize() != hipSuccess) return fail(MKWS_ERR_HIP, "device synchronisation failed");
  std::vector<uint32_t> host(em->guard);
  long bad = 0;
  for (const auto& sp : em->guard_spans) {
    if (hipMemcpy(host.data(), em->d_ws + sp.first, sp.second * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return fail(MKWS_ERR_HIP, "reading a guard band failed");
    for (size_t i = 0; i < sp.second; ++i) bad += host[i] != kGuardCanary;
  }
  return bad > 0x7fffffff ? 0x7fffffff : (int)bad;
}

void mkws_embed_destroy(mkws_embed* em) {
  if (!em) return;
  if (em->d_weights) (void)hipFree(em->d_weights);
  if (em->d_ws) (void)hipFree(em->d_ws);
  if (em->d_chain_tab) (void)hipFree(em->d_chain_tab);
  if (em->pair_err_host) (void)hipHostFree(em->pair_err_host);
  delete em;
}

int mkws_embed_forward(mkws_embed* em, const float* d_spec, int B, float* d_emb, void* stream) {
  if (!em) return fail(MKWS_ERR_INVALID_ARG, "embed handle is NULL");
  if (B < 0 || B > em->max_batch) return fail(MKWS_ERR_INVALID_ARG, "batch %d outside [0, max_batch=%d]", B, em->max_batch);
  if (B == 0) return MKWS_OK;
  if (!d_spec || !d_emb) return fail(MKWS_ERR_INVALID_ARG, "d_spec/d_emb is NULL");
  const float* src; size_t cnt;
  int rc = check_pair_health(em, static_cast<hipStream_t>(stream));
  if (rc != MKWS_OK) return rc;
  rc = run_forward(em, d_spec, B, d_emb, static_cast<hipStream_t>(stream), nullptr, &src, &cnt);
  if (rc != MKWS_OK) return rc;
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

// ---- options: ONE table for mkws_embed_set_option and mkws_embed_get_option --------------------------------------------------------
// (what an option means is said once, at its member of struct mkws_embed).  `member`: a plain integer, written and read as it is.
// Otherwise `set` / `get`, either of which may be missing: the option is then read-only / write-only ("unknown option" the other way).
namespace {
struct EmbedOption {
  const char* name;
  int mkws_embed::* member;
  int (*set)(mkws_embed*, int);
  int (*get)(const mkws_embed*);
};
void plan_tiles(mkws_embed* em) { em->pair_mt = pair_row_tiles(em->plan_batch); em->block_mt43 = block43_row_tiles(em->plan_batch); }
const EmbedOption kEmbedOptions[] = {
    {"fuse_front", nullptr, [](mkws_embed* em, int v) { em->fuse_front = v != 0; return (int)MKWS_OK; }, [](const mkws_embed* em) { return em->fuse_front ? 1 : 0; }},
    {"fuse_block", &mkws_embed::fuse_block, nullptr, nullptr},
    {"fuse_mid", &mkws_embed::fuse_mid, nullptr, nullptr},
    {"fuse_walk", &mkws_embed::fuse_walk, nullptr, nullptr},
    {"fuse_se4", nullptr, [](mkws_embed* em, int v) { em->fuse_se4 = v ? 1 : 0; return (int)MKWS_OK; }, [](const mkws_embed* em) { return em->fuse_se4; }},
    {"fuse_gemv", &mkws_embed::fuse_gemv, nullptr, nullptr},
    {"fuse_back", &mkws_embed::fuse_back, nullptr, nullptr},
    {"fuse_pair", &mkws_embed::fuse_pair, nullptr, nullptr},
    {"fuse_chain", &mkws_embed::fuse_chain, nullptr, nullptr},
    {"fuse_top", &mkws_embed::fuse_top, nullptr, nullptr},
    {"fuse_cluster", nullptr,
     [](mkws_embed* em, int v) {
       if (v && !em->cl_flags) return fail(MKWS_ERR_UNSUPPORTED, "fuse_cluster needs a handle of at most 64 clips (max_batch = %d)", em->max_batch);
       em->fuse_cluster = v; return (int)MKWS_OK;
     },
     [](const mkws_embed* em) { return em->fuse_cluster; }},
    {"fuse_cluster_chain", nullptr,
     [](mkws_embed* em, int v) {
       if (v && (em->max_batch != 1 || !em->cl_flags)) return fail(MKWS_ERR_UNSUPPORTED, "fuse_cluster_chain is the plan of one-clip handles (max_batch = %d)", em->max_batch);
       em->fuse_cluster_chain = v; return (int)MKWS_OK;
     },
     [](const mkws_embed* em) { return em->fuse_cluster_chain; }},
    {"fuse_stem", &mkws_embed::fuse_stem, nullptr, nullptr},
    {"fuse_gap", &mkws_embed::fuse_gap, nullptr, nullptr},
    // A/B: 8-clip pairs and 4-clip 4x3 workgroups whatever max_batch is (fewer, larger workgroups: the workspaces still fit)
    {"big_tiles", nullptr,
     [](mkws_embed* em, int v) {
       if (v) { em->pair_mt = 2; em->block_mt43 = 3; } else plan_tiles(em);
       return (int)MKWS_OK;
     },
     nullptr},
    // Plan for `value` clips (0 = back to max_batch): the caller runs several handles CONCURRENTLY on separate streams (serving lanes) and passes
    // the clips they hold together, so that the tiny-image launches (blocks 4a..7a: 60 % of a forward pass) of a 256-clip lane take a quarter of the
    // chip each -- the 1024-clip plan's workgroup shapes: 4-clip workgroups, 8-clip pairs -- instead of spreading one clip per CU and queueing behind the
    // other lanes.  The GEMM tiles stay those of max_batch (measured: the 1024-clip tiles on 256 rows are a few long workgroups, 1.58 vs 0.99 ms per
    // 4 x 256 clips, profiles/r06_notes.md section 8).  Per-clip arithmetic does not depend on the shapes beyond the documented round-off between them;
    // workspaces are sized by max_batch and larger shapes need less of them.
    {"plan_batch", nullptr,
     [](mkws_embed* em, int v) {
       if (v != 0 && v < em->max_batch) return fail(MKWS_ERR_INVALID_ARG, "plan_batch %d is below the handle's max_batch %d", v, em->max_batch);
       em->plan_batch = v ? v : em->max_batch;
       plan_tiles(em);
       return (int)MKWS_OK;
     },
     [](const mkws_embed* em) { return em->plan_batch; }},
    // A/B: row tiles (3 / 2 / 1 = 4 / 2 / 1 clips) per workgroup of the 4x3-image kernels; 0 = the rule of the handle's plan_batch.  Reads back the tiles in use
    {"block_tiles", nullptr,
     [](mkws_embed* em, int v) {
       if (v < 0 || v > 3) return fail(MKWS_ERR_INVALID_ARG, "block_tiles is 0 (rule), 1, 2 or 3");
       em->block_mt43 = v ? v : block43_row_tiles(em->plan_batch);
       return (int)MKWS_OK;
     },
     [](const mkws_embed* em) { return em->block_mt43; }},
    {"pair_fault", nullptr, [](mkws_embed* em, int v) { em->pair_fault = v; return (int)MKWS_OK; }, nullptr},     // test hook: forces the paired kernel's failure paths
    // test hook: the state a failed exchange of an EARLIER launch leaves behind (sticky device word + host-mapped word), without running
    // one -- what a captured graph meets when a replay before it failed.  Synchronous.
    {"inject_exchange_error", nullptr,
     [](mkws_embed* em, int v) {
       if (!em->pair_err_host || !em->pair_err_dev) return fail(MKWS_ERR_UNSUPPORTED, "handle has no exchange kernels");
       const int code = v ? kPairErrTimeout : 0;
       MKWS_HIP(hipDeviceSynchronize());
       MKWS_HIP(hipMemcpy(em->pair_err_dev, &code, sizeof(int), hipMemcpyHostToDevice));
       *reinterpret_cast<volatile int*>(em->pair_err_host) = code;
       return (int)MKWS_OK;
     },
     nullptr},
    {"pair_degraded", nullptr, nullptr, [](const mkws_embed* em) { return em->pair_degraded; }},
    {"guard_floats", nullptr, nullptr, [](const mkws_embed* em) { return (int)em->guard; }},
    {"guard_bands", nullptr, nullptr, [](const mkws_embed* em) { return (int)em->guard_spans.size(); }},
    {"guard_violations", nullptr, nullptr, guard_violations},
    // nonzero: a launch that has ALREADY EXECUTED recorded a failed exchange and the handle has not been healed yet (the next forward /
    // tap / profile call heals it and returns MKWS_ERR_EXCHANGE).  A host-mapped word: no synchronisation.  This is what hipGraph users
    // poll -- a replay does not pass through mkws_embed_forward, so "pair_degraded" cannot move under it.
    {"exchange_error", nullptr, nullptr, [](const mkws_embed* em) { return em->pair_err_host ? *reinterpret_cast<volatile int*>(em->pair_err_host) : 0; }},
    {"max_batch", nullptr, nullptr, [](const mkws_embed* em) { return em->max_batch; }},
};
const EmbedOption* find_option(const char* name) {
  for (const EmbedOption& o : kEmbedOptions) if (strcmp(name, o.name) == 0) return &o;
  return nullptr;
}
}  // namespace

int mkws_embed_set_option(mkws_embed* em, const char* name, int value) {
  if (!em || !name) return fail(MKWS_ERR_INVALID_ARG, "NULL argument");
  const EmbedOption* o = find_option(name);
  if (o && o->member) { em->*(o->member) = value; return MKWS_OK; }
  if (o && o->set) return o->set(em, value);
  return fail(MKWS_ERR_INVALID_ARG, "unknown option '%s'", name);
}

int mkws_embed_get_option(const mkws_embed* em, const char* name) {
  if (!em || !name) return fail(MKWS_ERR_INVALID_ARG, "NULL argument");
  const EmbedOption* o = find_option(name);
  if (o && o->member) return em->*(o->member);
  if (o && o->get) return o->get(em);
  return fail(MKWS_ERR_INVALID_ARG, "unknown option '%s'", name);
}

int mkws_embed_profile(mkws_embed* em, const float* d_spec, int B, int reps, float* d_emb, char* dst, size_t cap, void* stream) {
  if (!em) return fail(MKWS_ERR_INVALID_ARG, "embed handle is NULL");
  if (B <= 0 || B > em->max_batch || reps <= 0) return fail(MKWS_ERR_INVALID_ARG, "bad batch/reps");
  if (!d_spec || !d_emb) return fail(MKWS_ERR_INVALID_ARG, "d_spec/d_emb is NULL");
  LaunchProf prof;
  prof.stream = static_cast<hipStream_t>(stream);
  int rc = check_pair_health(em, prof.stream);
  if (rc != MKWS_OK) return rc;
  g_prof = &prof;
  for (int r = 0; r < reps && rc == MKWS_OK; ++r) {
    const float* src; size_t cnt;
    rc = run_forward(em, d_spec, B, d_emb, prof.stream, nullptr, &src, &cnt);
    prof.finish_pass();
  }
  g_prof = nullptr;
  if (rc != MKWS_OK) return rc;
  MKWS_HIP(hipGetLastError());
  std::string out;
  char line[256];
  for (const auto& r : prof.recs) {
    snprintf(line, sizeof(line), "%s\t%s\t%.6f\n", r.stage.c_str(), r.kernel.c_str(), r.ms / reps);
    out += line;
  }
  if (dst && cap > 0) {
    const size_t n = out.size() < cap - 1 ? out.size() : cap - 1;
    memcpy(dst, out.data(), n);
    dst[n] = 0;
  }
  return (int)out.size();
}

int mkws_embed_forward_tap(mkws_embed* em, const float* d_spec, int B, const char* stage, float* d_dst, size_t cap_floats, void* stream) {
  if (!em || !stage) return fail(MKWS_ERR_INVALID_ARG, "embed handle/stage is NULL");
  if (B <= 0 || B > em->max_batch) return fail(MKWS_ERR_INVALID_ARG, "batch %d outside [1, max_batch=%d]", B, em->max_batch);
  if (!d_spec || !d_dst) return fail(MKWS_ERR_INVALID_ARG, "d_spec/d_dst is NULL");
  const float* src = nullptr; size_t cnt = 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = check_pair_health(em, s);
  if (rc != MKWS_OK) return rc;
  rc = run_forward(em, d_spec, B, nullptr, s, stage, &src, &cnt);
  if (rc != MKWS_OK) return rc;
  MKWS_HIP(hipGetLastError());
  if (cnt > cap_floats) return fail(MKWS_ERR_INVALID_ARG, "stage '%s' has %zu floats, destination holds %zu", stage, cnt, cap_floats);
  MKWS_HIP(hipMemcpyAsync(d_dst, src, cnt * sizeof(float), hipMemcpyDeviceToDevice, s));
  return (int)cnt;
}

}  // extern "C"
