// DS-CNN baseline, inference (include/mkws.h "DS-CNN baseline").
//
// One launch per forward.  A workgroup of eight waves owns one clip at a time and walks all nine layers with the activation
// [25][20][64] fp32 in LDS; nothing but the spectrogram, the weights and the [label_count] results cross HBM.
//
//   stem     im2col on the fly from a zero-padded copy of the spectrogram in LDS: [500 pixels] x [K = 10*4] x [64] through
//            v_mfma_f32_16x16x4_f32, one k-step per kernel row (the four lane groups are the four kernel columns).
//   blocks   two output rows per step, 13 steps per block, 52 steps in one pipeline.  Waves 0..3 are the depthwise half: 3x3 vector code
//            of rows r, r+1 into one of two [40 pixel][64] staging tiles.  Waves 4..7 are the pointwise half, one step behind: 64x64 on
//            the matrix cores from the other tile (wave w owns output channels 16w..16w+15 and keeps its share of the weights in 16
//            registers).  Every SIMD holds one wave of each half, so its vector and matrix work overlap, and a step costs ONE barrier.
//            The pointwise result of rows r, r+1 goes into the ring slots of input rows r-2 and r-1 -- dead once the depthwise of that
//            step has been read, which the barrier in between guarantees.  The activation therefore lives in a ring of 25 + 2 rows
//            and each block moves the ring's base back by two slots.
//   pool     rows 0..23 only; dense and softmax by the first label_count threads.
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "mkws_common.h"

using mkws::fail;

namespace {

constexpr int kInH = 49, kInW = 40;
constexpr int kH = 25, kW = 20, kC = 64;
constexpr int kPoolRows = 24;                       // int(49 / 2): row 24 is computed and not pooled
constexpr int kBlocks = 4;
constexpr int kStemKH = 10, kStemKW = 4;
constexpr int kMinLabels = 2, kMaxLabels = 64;
constexpr float kBnEps = 1e-3f;

// ---- parameter blob (Keras order) and folded device layout, in floats ---------------------------------------------------------------
constexpr int kRawStem = kStemKH * kStemKW * kC + kC + 4 * kC;                       // 2880
constexpr int kRawBlock = (9 * kC + kC + 4 * kC) + (kC * kC + kC + 4 * kC);          // 5312
constexpr int kRawTrunk = kRawStem + kBlocks * kRawBlock;                            // 24128

constexpr int kFStemW = 0, kFStemB = kFStemW + kStemKH * kStemKW * kC;               // [40][64], [64]
constexpr int kFBlock0 = kFStemB + kC;
constexpr int kFDwW = 0, kFDwB = 9 * kC, kFPwW = kFDwB + kC, kFPwB = kFPwW + kC * kC, kFBlockSize = kFPwB + kC;   // per block
constexpr int kFDenseW = kFBlock0 + kBlocks * kFBlockSize;                           // [64][L], then [L]

// ---- LDS layout, in floats ---------------------------------------------------------------------------------------------------------
constexpr int kThreads = 512;
constexpr int kRowF = kW * kC;                      // 1280 floats per activation row
constexpr int kRing = kH + 2;                       // 27 row slots
constexpr int kStepRows = 2, kSteps = (kH + kStepRows - 1) / kStepRows;              // 13 steps per block, the last one row
constexpr int kTileP = kStepRows * kW, kTileS = 68; // a staging tile: 40 pixels; stride 68 keeps the depthwise stores (lanes = channels)
                                                    // and the A-operand loads (bank 4*pixel + k) conflict-free
constexpr int kSpecH = 58, kSpecW = 44;             // spectrogram rows -4..53, columns -1..42 (zero outside the 49 x 40)
constexpr int kLdsAct = 0, kLdsTile = kLdsAct + kRing * kRowF;
constexpr int kLdsFloats = kLdsTile + 2 * kTileP * kTileS;                           // (the padded spectrogram lies over the tiles: the
constexpr size_t kLdsBytes = sizeof(float) * kLdsFloats;                             //  stem is done before the first depthwise) 160 000 B
static_assert(kLdsBytes <= 160 * 1024, "the DS-CNN workgroup must fit one CU's LDS");
static_assert(2 * (kH - 1) + kStemKH <= kSpecH && 2 * (kW - 1) + kStemKW <= kSpecW, "padded spectrogram too small for the stem's reach");
static_assert(kSpecH * kSpecW <= 2 * kTileP * kTileS && 33 * kC + kMaxLabels <= 2 * kTileP * kTileS, "the tiles are too small for what lies over them");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct DscnnArgs {
  const float* w;        // folded weights
  const float* spec;     // [B][49][40]
  float* probs;          // [B][L] or NULL
  float* logits;         // [B][L] or NULL
  float* tap;            // stage 0..4: [B][25][20][64]; stage 5: [B][64]; NULL without a tap
  int B, L, tap_stage;
};

__device__ inline int ring_slot(int base, int row) {             // base in [0, kRing), row in [-2, kH]
  int s = base + row;
  s = s < 0 ? s + kRing : s;
  return s >= kRing ? s - kRing : s;
}

__device__ inline void store_stage(const float* s_act, int base, float* dst, int tid) {
  const float4* src4 = reinterpret_cast<const float4*>(s_act);
  float4* dst4 = reinterpret_cast<float4*>(dst);
#pragma unroll 1
  for (int i = tid; i < kH * kRowF / 4; i += kThreads) {
    const int r = i / (kRowF / 4), x = i - r * (kRowF / 4);
    dst4[i] = src4[ring_slot(base, r) * (kRowF / 4) + x];
  }
}

__global__ __launch_bounds__(kThreads) void dscnn_kernel(DscnnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_lds[];
  float* s_act = s_lds + kLdsAct;
  float* s_T = s_lds + kLdsTile;                                 // two staging tiles
  float* s_spec = s_T;                                           // before the blocks: the padded spectrogram
  double* s_part = reinterpret_cast<double*>(s_T);               // after them: the pool's partial sums [8][64],
  double* s_dot = s_part + 8 * kC;                               // the dense layer's partial dot products [64][8],
  float* s_pool = s_T + 32 * kC;                                 // the pooled [64] and the logits [<= 64]
  float* s_logit = s_pool + kC;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i16 = lane & 15;
  const int half = wave >> 2;                                    // blocks: 0 = depthwise, 1 = pointwise
  const int ch = 16 * (wave & 3) + i16;                          // the output channel this lane holds in every MFMA result
  const int L = a.L;
  // (the loops outside the blocks are kept rolled: unrolled, their addresses are hoisted over the whole kernel -- the dense layer's alone
  //  were 128 registers -- and the pointwise half's operands no longer fit)

  for (int clip = blockIdx.x; clip < a.B; clip += gridDim.x) {
    // ---- the spectrogram, zero-padded -------------------------------------------------------------------------------------------
    const float* spec = a.spec + (size_t)clip * (kInH * kInW);
#pragma unroll
    for (int k = 0; k < (kSpecH * kSpecW + kThreads - 1) / kThreads; ++k) {     // (a constant trip count: the five reads are in flight together)
      const int i = tid + k * kThreads;
      const int r = i / kSpecW - 4, c = i % kSpecW - 1;
      const bool inside = r >= 0 && r < kInH && c >= 0 && c < kInW;
      const float v = spec[inside ? r * kInW + c : 0];
      if (i < kSpecH * kSpecW) s_spec[i] = inside ? v : 0.0f;
    }
    float wd_next[9], wp_next[16], bd_next = 0.0f, bp_next = 0.0f;
    if (half == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) wd_next[k] = a.w[kFBlock0 + kFDwW + k * kC + lane];
      bd_next = a.w[kFBlock0 + kFDwB + lane];
    } else {
#pragma unroll
      for (int t = 0; t < 16; ++t) wp_next[t] = a.w[kFBlock0 + kFPwW + (8 * (t >> 1) + 2 * g + (t & 1)) * kC + ch];
      bp_next = a.w[kFBlock0 + kFPwB + ch];
    }
    __syncthreads();

    // ---- stem: out[p][co] = sum_{ky,kx} spec[2 oy + ky - 4][2 ox + kx - 1] * w[ky][kx][co] ------------------------------------------
    {
      float bw[kStemKH];
#pragma unroll
      for (int ky = 0; ky < kStemKH; ++ky) bw[ky] = a.w[kFStemW + (ky * kStemKW + g) * kC + ch];
      const float bias = a.w[kFStemB + ch];
#pragma unroll 1
      for (int mt = half; mt < (kH * kW + 31) / 32; mt += 2) {   // 16 pairs of 16-pixel tiles; pixels 500..511 are clamped and not stored
        f32x4 acc[2];
        const float* sp[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          int p = 32 * mt + 16 * u + i16;
          p = p < kH * kW ? p : kH * kW - 1;
          const int oy = p / kW, ox = p - oy * kW;
          sp[u] = s_spec + (2 * oy) * kSpecW + 2 * ox + g;
          acc[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int ky = 0; ky < kStemKH; ++ky) {
#pragma unroll
          for (int u = 0; u < 2; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(sp[u][ky * kSpecW], bw[ky], acc[u], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int q = 32 * mt + 16 * u + 4 * g + r;
            if (q < kH * kW) s_act[q * kC + ch] = fmaxf(acc[u][r] + bias, 0.0f);
          }
        }
      }
    }
    __syncthreads();
    if (a.tap_stage == 0) store_stage(s_act, 0, a.tap + (size_t)clip * (kH * kRowF), tid);

    // ---- four depthwise + pointwise blocks: iteration `it` runs the depthwise of step `it` and the pointwise of step `it - 1` ------------
    // Row r of block blk's input is ring slot (base + r) mod 27 with base = -2 blk mod 27; its output row r goes to slot base + r - 2.
    // What the one barrier per iteration orders:
    //  - within a block, the depthwise of step k reads input rows 2k-1 .. 2k+2 while the pointwise of step k-1 writes the slots of input
    //    rows 2k-4, 2k-3: disjoint.  Those slots were last read by the depthwise of step k-1, an iteration (a barrier) earlier.
    //  - across blocks, the depthwise of step 0 of block blk+1 reads the new rows 0..2, written by the pointwise of steps 0, 1 of block blk,
    //    while that block's last pointwise step writes row 24 only; every later depthwise step comes after the barrier that completes row 24.
    //  - the two staging tiles alternate: tile it & 1 is written in iteration it and read in iteration it + 1.
    // A half's weights of block blk + 1 are requested during step 1 of block blk and taken over at step 0 of blk + 1, so that no step waits
    // for global memory; block 0's were requested before the stem.
    float wd[9], wp[16], bd = 0.0f, bp = 0.0f;
#pragma unroll 1
    for (int it = 0; it <= kBlocks * kSteps; ++it) {
      if (half == 0 && it < kBlocks * kSteps) {
        const int blk = it / kSteps, r0 = kStepRows * (it - blk * kSteps), base = (kRing - kStepRows * blk) % kRing;
        const int c = lane, col0 = 5 * wave;                     // this thread's channel and its five output columns
        if (r0 == 0) {                                           // (requested a block ago, or before the stem)
#pragma unroll
          for (int k = 0; k < 9; ++k) wd[k] = wd_next[k];
          bd = bd_next;
        } else if (r0 == kStepRows && blk + 1 < kBlocks) {
          const float* wb = a.w + kFBlock0 + (blk + 1) * kFBlockSize;
#pragma unroll
          for (int k = 0; k < 9; ++k) wd_next[k] = wb[kFDwW + k * kC + c];
          bd_next = wb[kFDwB + c];
        }
        // rows r0, r0+1 from input rows r0-1 .. r0+2, columns col0-1 .. col0+5
        float in[4][7];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int row = r0 - 1 + rr;
          const bool row_ok = row >= 0 && row < kH;
          const float* src = s_act + ring_slot(base, row_ok ? row : 0) * kRowF + c;
#pragma unroll
          for (int cc = 0; cc < 7; ++cc) {
            const int col = col0 - 1 + cc, colc = col < 0 ? 0 : (col >= kW ? kW - 1 : col);
            const float v = src[colc * kC];                      // read unconditionally from a clamped address, so that the 28 reads
            in[rr][cc] = (row_ok && col == colc) ? v : 0.0f;     // issue together: a guarded read is a branch that waits out its own latency
          }
        }
        float* tile = s_T + (it & 1) * (kTileP * kTileS);
#pragma unroll
        for (int orow = 0; orow < 2; ++orow) {
#pragma unroll
          for (int oc = 0; oc < 5; ++oc) {
            float acc = bd;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
              for (int kx = 0; kx < 3; ++kx) acc = fmaf(in[orow + ky][oc + kx], wd[ky * 3 + kx], acc);
            }
            tile[(orow * kW + col0 + oc) * kTileS + c] = fmaxf(acc, 0.0f);     // (row r0+1 = 25 of a block's last step: computed, never stored below)
          }
        }
      } else if (half == 1 && it > 0) {
        const int st = it - 1, blk = st / kSteps, r0 = kStepRows * (st - blk * kSteps), base = (kRing - kStepRows * blk) % kRing;
        if (r0 == 0) {
#pragma unroll
          for (int t = 0; t < 16; ++t) wp[t] = wp_next[t];
          bp = bp_next;
        } else if (r0 == kStepRows && blk + 1 < kBlocks) {
          const float* wb = a.w + kFBlock0 + (blk + 1) * kFBlockSize;
#pragma unroll
          for (int t = 0; t < 16; ++t) wp_next[t] = wb[kFPwW + (8 * (t >> 1) + 2 * g + (t & 1)) * kC + ch];
          bp_next = wb[kFPwB + ch];
        }
        // [40 (+ 8 clamped)][64] x [64][16 of this wave]
        const float* tile = s_T + (st & 1) * (kTileP * kTileS);
        // The sum over k may run in any order, so k-step t = 2 q + e pairs lane group g with k = 8 q + 2 g + e (the weights above follow): a lane's
        // operands of two k-steps are then one 8-byte read, conflict-free at stride 68 (bank (4 pixel + 2 g) mod 64 over 32 lanes), where 4-byte
        // reads are two-way conflicts (banks mod 32) and far from their rate at one wave per SIMD.  Reads run one group of four k-steps ahead of
        // the MFMAs, and the MFMAs of a group go round the three accumulators (a dependent v_mfma_f32_16x16x4_f32 waits 40 cycles, an
        // independent one 32); the scheduling barriers keep that order, which the compiler otherwise undoes.
        const float2* ap[3];
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) {
          const int p = 16 * mt + i16;
          ap[mt] = reinterpret_cast<const float2*>(tile + (p < kTileP ? p : kTileP - 1) * kTileS + 2 * g);
        }
        f32x4 acc[3];
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        float2 av[2][6];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
          for (int mt = 0; mt < 3; ++mt) av[0][3 * q + mt] = ap[mt][4 * q];
        }
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
          if (c4 < 3) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
#pragma unroll
              for (int mt = 0; mt < 3; ++mt) av[(c4 + 1) & 1][3 * q + mt] = ap[mt][4 * (2 * (c4 + 1) + q)];
            }
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int mt = 0; mt < 3; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c4 & 1][3 * q + mt].x, wp[4 * c4 + 2 * q], acc[mt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < 3; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c4 & 1][3 * q + mt].y, wp[4 * c4 + 2 * q + 1], acc[mt], 0, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int q = 16 * mt + 4 * g + r;
            const int orow = q >= kW ? 1 : 0, col = q - orow * kW, row = r0 + orow;
            if (q < kTileP && row < kH) s_act[ring_slot(base, row - kStepRows) * kRowF + col * kC + ch] = fmaxf(acc[mt][r] + bp, 0.0f);
          }
        }
      }
      __syncthreads();
      // (the next iteration's pointwise writes the two spare slots only, so this read of all 25 rows needs no barrier after it)
      if (it > 0 && it % kSteps == 0 && a.tap_stage == it / kSteps)
        store_stage(s_act, (kRing - kStepRows * (it / kSteps)) % kRing, a.tap + (size_t)clip * (kH * kRowF), tid);
    }
    const int base = (kRing - kStepRows * kBlocks) % kRing;

    // ---- mean over rows 0..23, dense, softmax --------------------------------------------------------------------------------------
    // (float64 for the 480-term sums and the 64-term dot products: they are a few thousand operations per clip, and the centring dense
    //  bias makes the logits small differences of larger terms)
    {
      double sum = 0.0;
#pragma unroll 4
      for (int q = wave; q < kPoolRows * kW; q += kThreads / 64) {
        const int row = q / kW, col = q - row * kW;
        sum += (double)s_act[ring_slot(base, row) * kRowF + col * kC + lane];
      }
      s_part[wave * kC + lane] = sum;
    }
    __syncthreads();
    if (tid < kC) {
      double sum = 0.0;
#pragma unroll 1
      for (int w = 0; w < kThreads / 64; ++w) sum += s_part[w * kC + tid];
      const float m = (float)(sum / (double)(kPoolRows * kW));
      s_pool[tid] = m;
      if (a.tap_stage == 5) a.tap[(size_t)clip * kC + tid] = m;
    }
    __syncthreads();
    {                                                            // eight threads per label, eight terms each, folded in a fixed order
      const int j = tid >> 3, part = tid & 7;
      double z = 0.0;
      if (j < L) {
#pragma unroll
        for (int k = 0; k < 8; ++k) z += (double)s_pool[8 * part + k] * (double)a.w[kFDenseW + (8 * part + k) * L + j];
      }
      s_dot[tid] = z;
    }
    __syncthreads();
    if (tid < L) {
      double z = (double)a.w[kFDenseW + kC * L + tid];
#pragma unroll
      for (int part = 0; part < 8; ++part) z += s_dot[8 * tid + part];
      s_logit[tid] = (float)z;
      if (a.logits) a.logits[(size_t)clip * L + tid] = (float)z;
    }
    __syncthreads();
    if (tid < L && a.probs) {
      float m = s_logit[0];
#pragma unroll 1
      for (int j = 1; j < L; ++j) m = fmaxf(m, s_logit[j]);
      float s = 0.0f;
#pragma unroll 1
      for (int j = 0; j < L; ++j) s += expf(s_logit[j] - m);
      a.probs[(size_t)clip * L + tid] = expf(s_logit[tid] - m) / s;
    }
    __syncthreads();                                             // the next clip's spectrogram goes over the pool's scratch
  }
}

struct Tensor {
  std::string name;
  std::vector<int> shape;
  size_t offset, count;
};

std::vector<Tensor> enumerate_tensors(int L) {
  std::vector<Tensor> v;
  size_t at = 0;
  auto add = [&](const std::string& name, std::vector<int> shape) {
    size_t n = 1;
    for (int d : shape) n *= (size_t)d;
    v.push_back({name, shape, at, n});
    at += n;
  };
  auto suffix = [](const char* kind, int i) { return i ? std::string(kind) + "_" + std::to_string(i) : std::string(kind); };
  int bn = 0;
  auto add_bn = [&]() {
    const std::string p = suffix("batch_normalization", bn++);
    for (const char* leaf : {"gamma", "beta", "moving_mean", "moving_variance"}) add(p + "/" + leaf, {kC});
  };
  add("conv2d/kernel", {kStemKH, kStemKW, 1, kC});
  add("conv2d/bias", {kC});
  add_bn();
  for (int b = 0; b < kBlocks; ++b) {
    add(suffix("depthwise_conv2d", b) + "/depthwise_kernel", {3, 3, kC, 1});
    add(suffix("depthwise_conv2d", b) + "/bias", {kC});
    add_bn();
    add(suffix("conv2d", b + 1) + "/kernel", {1, 1, kC, kC});
    add(suffix("conv2d", b + 1) + "/bias", {kC});
    add_bn();
  }
  add("dense/kernel", {kC, L});
  add("dense/bias", {L});
  return v;
}

// w [taps][64] (output channel last), bias [64], then gamma, beta, moving_mean, moving_variance -> folded w, b.  float64, rounded once.
bool fold_conv_bn(const float* w, int taps, const float* bias, const float* bn, float* fw, float* fb) {
  for (int co = 0; co < kC; ++co) {
    const double var = (double)bn[3 * kC + co] + (double)kBnEps;
    if (!(var > 0.0)) return false;
    const double scale = (double)bn[co] / std::sqrt(var);
    for (int t = 0; t < taps; ++t) fw[t * kC + co] = (float)((double)w[t * kC + co] * scale);
    fb[co] = (float)(((double)bias[co] - (double)bn[2 * kC + co]) * scale + (double)bn[kC + co]);
  }
  return true;
}

bool labels_ok(int L) { return L >= kMinLabels && L <= kMaxLabels; }

}  // namespace

struct mkws_dscnn {
  float* d_w = nullptr;
  int L = 0, max_batch = 0, grid = 0, device = 0;
};

extern "C" {

size_t mkws_dscnn_param_count(int label_count) {
  return labels_ok(label_count) ? (size_t)kRawTrunk + (size_t)(kC + 1) * label_count : 0;
}

int mkws_dscnn_weight_manifest(int label_count, char* dst, size_t cap) {
  if (!labels_ok(label_count)) return fail(MKWS_ERR_INVALID_ARG, "label_count %d outside [%d, %d]", label_count, kMinLabels, kMaxLabels);
  const auto v = enumerate_tensors(label_count);
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

int mkws_dscnn_create(const float* h, size_t n_floats, int label_count, int max_batch, mkws_dscnn** out) {
  if (!h || !out) return fail(MKWS_ERR_INVALID_ARG, "params/out is NULL");
  *out = nullptr;
  if (max_batch <= 0) return fail(MKWS_ERR_INVALID_ARG, "max_batch must be positive");
  if (!labels_ok(label_count)) return fail(MKWS_ERR_BAD_WEIGHTS, "label_count %d outside [%d, %d]", label_count, kMinLabels, kMaxLabels);
  if (n_floats != mkws_dscnn_param_count(label_count))
    return fail(MKWS_ERR_BAD_WEIGHTS, "parameter blob has %zu floats, a DS-CNN of %d labels needs %zu", n_floats, label_count, mkws_dscnn_param_count(label_count));
  for (size_t i = 0; i < n_floats; ++i)
    if (!std::isfinite(h[i])) return fail(MKWS_ERR_BAD_WEIGHTS, "parameter blob has a non-finite value at %zu", i);
  const int L = label_count;
  std::vector<float> f((size_t)kFDenseW + (size_t)(kC + 1) * L);
  {
    const float* p = h;
    bool ok = fold_conv_bn(p, kStemKH * kStemKW, p + kStemKH * kStemKW * kC, p + kStemKH * kStemKW * kC + kC, &f[kFStemW], &f[kFStemB]);
    p += kRawStem;
    for (int b = 0; b < kBlocks; ++b) {
      float* fb = &f[kFBlock0 + b * kFBlockSize];
      ok = ok && fold_conv_bn(p, 9, p + 9 * kC, p + 10 * kC, fb + kFDwW, fb + kFDwB);
      p += 14 * kC;
      ok = ok && fold_conv_bn(p, kC, p + kC * kC, p + kC * kC + kC, fb + kFPwW, fb + kFPwB);
      p += kC * kC + 5 * kC;
    }
    if (!ok) return fail(MKWS_ERR_BAD_WEIGHTS, "a BatchNorm moving variance plus epsilon is not positive");
    memcpy(&f[kFDenseW], p, sizeof(float) * (size_t)(kC + 1) * L);
  }
  int rc = mkws::require_device();
  if (rc != MKWS_OK) return rc;

  mkws_dscnn* m = new (std::nothrow) mkws_dscnn();
  if (!m) return fail(MKWS_ERR_ALLOC, "out of host memory");
  m->L = L;
  m->max_batch = max_batch;
  hipDeviceProp_t prop;
  if (hipGetDevice(&m->device) != hipSuccess || hipGetDeviceProperties(&prop, m->device) != hipSuccess) { delete m; return fail(MKWS_ERR_HIP, "hipGetDeviceProperties failed"); }
  m->grid = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;      // the LDS footprint admits one workgroup per CU
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(dscnn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes) != hipSuccess) {
    delete m;
    return fail(MKWS_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed", kLdsBytes);
  }
  if (hipMalloc(reinterpret_cast<void**>(&m->d_w), f.size() * sizeof(float)) != hipSuccess) { delete m; return fail(MKWS_ERR_ALLOC, "hipMalloc(%zu) for weights failed", f.size() * sizeof(float)); }
  if (hipMemcpy(m->d_w, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { mkws_dscnn_destroy(m); return fail(MKWS_ERR_HIP, "weight upload failed"); }
  *out = m;
  return MKWS_OK;
}

void mkws_dscnn_destroy(mkws_dscnn* m) {
  if (!m) return;
  if (m->d_w) (void)hipFree(m->d_w);
  delete m;
}

int mkws_dscnn_grid(const mkws_dscnn* m) {
  if (!m) return fail(MKWS_ERR_INVALID_ARG, "dscnn handle is NULL");
  return m->grid;
}

static int launch(mkws_dscnn* m, const float* d_spec, int B, float* d_probs, float* d_logits, int stage, float* d_tap, void* stream) {
  if (!m) return fail(MKWS_ERR_INVALID_ARG, "dscnn handle is NULL");
  if (B < 0 || B > m->max_batch) return fail(MKWS_ERR_INVALID_ARG, "batch %d outside [0, max_batch=%d]", B, m->max_batch);
  if (B == 0) return MKWS_OK;
  DscnnArgs a;
  a.w = m->d_w; a.spec = d_spec; a.probs = d_probs; a.logits = d_logits; a.tap = d_tap;
  a.B = B; a.L = m->L; a.tap_stage = stage;
  const int grid = B < m->grid ? B : m->grid;
  hipLaunchKernelGGL(dscnn_kernel, dim3(grid), dim3(kThreads), kLdsBytes, static_cast<hipStream_t>(stream), a);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

int mkws_dscnn_forward(mkws_dscnn* m, const float* d_spec, int B, float* d_probs, float* d_logits, void* stream) {
  if (B > 0 && (!d_spec || !d_probs)) return fail(MKWS_ERR_INVALID_ARG, "d_spec/d_probs is NULL");
  return launch(m, d_spec, B, d_probs, d_logits, -1, nullptr, stream);
}

int mkws_dscnn_tap(mkws_dscnn* m, const float* d_spec, int B, int stage, float* d_out, void* stream) {
  if (stage < 0 || stage > 5) return fail(MKWS_ERR_INVALID_ARG, "stage %d outside [0, 5]", stage);
  if (B > 0 && (!d_spec || !d_out)) return fail(MKWS_ERR_INVALID_ARG, "d_spec/d_out is NULL");
  return launch(m, d_spec, B, nullptr, nullptr, stage, d_out, stream);
}

}  // extern "C"
