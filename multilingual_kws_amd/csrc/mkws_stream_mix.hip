// Test streams assembled on the device (include/mkws.h, "Test streams assembled on the device"): one launch lays the items of R streams
// out on their time lines -- a window of a float32 recording, a gain, two linear fades each -- sums them where they overlap, adds a
// looped background bed at a gain per stream and clips.  mkws_stream_power / mkws_stream_bed_gain find that gain for a wanted
// signal-to-noise ratio without leaving the device.
//
// A workgroup of 256 lanes owns kTile = 1024 consecutive positions of one stream.  It finds the items that can reach its tile by a
// binary search in the stream's ascending out_start (the first with out_start > tile begin - max_frames) and a scan forward to the
// first with out_start >= tile end; every value in that search is the same in all lanes.  The common tile -- one item that covers it
// whole, no fade and no edge of the recording inside -- runs a body without per-position tests: a lane takes four neighbouring
// positions, stored as one 16-byte word where the output address allows it (loaded as one where the source address does too), and the
// at most three positions on either side of the aligned words go out as dwords.  Every other tile takes the general body: the items
// outermost, a lane's four positions (tid, tid + 256, ...) in registers.  Both write every position of the tile once and nothing else.
// The bed index costs one 64-bit modulo per tile and an add with one wrap per position (a bed shorter than a tile: a 32-bit modulo).
// Every workgroup checks the stream and the items it uses itself, in 64-bit, before it reads or writes for them, so nothing depends on
// the order of workgroups; the leading workgroups also count the invalid items and streams, one per lane.
#include <cstdint>

#include "mkws_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;                  // positions of one workgroup
constexpr int kPer = kTile / kThreads;       // positions of one lane
constexpr int64_t kStartLimit = (int64_t)1 << 61;

__device__ __forceinline__ bool stream_is_valid(const mkws_stream_desc& d, int64_t src_floats, int n_items, int64_t max_out, int64_t out_floats) {
  if (d.n_out < 0 || d.n_out > max_out) return false;
  if (d.out_offset < 0 || d.out_offset > out_floats || d.n_out > out_floats - d.out_offset) return false;
  if (d.first_item < 0 || d.n_items < 0 || (int64_t)d.first_item + (int64_t)d.n_items > (int64_t)n_items) return false;
  if (d.bed_len < 0) return false;
  if (d.bed_len > 0) {
    if (d.bed_offset < 0 || d.bed_offset > src_floats || d.bed_len > src_floats - d.bed_offset) return false;
    if (d.bed_start < 0 || d.bed_start >= d.bed_len) return false;
  }
  return true;
}

// Item k against the three fields of ITS stream's descriptor that concern it (the caller has checked that it.stream is in range).
__device__ __forceinline__ bool item_is_valid(const mkws_stream_item& it, int64_t k, int64_t first_item, int64_t n_items, int64_t max_frames,
                                              int64_t src_floats) {
  if (k < first_item || k - first_item >= n_items) return false;
  if (it.n_frames < 0 || it.n_frames > max_frames || it.fade_in < 0 || it.fade_out < 0 || it.src_len < 0) return false;
  if (it.start < -kStartLimit || it.start > kStartLimit || it.out_start < -kStartLimit || it.out_start > kStartLimit) return false;
  if (it.src_offset < 0 || it.src_offset > src_floats || it.src_len > src_floats - it.src_offset) return false;
  return true;
}

// The leading workgroups count: lane g takes item g, or stream g - n_items.  (atomicAdd of 1 from the lanes of a wave becomes one add.)
__device__ __forceinline__ void count_invalid(const mkws_stream_item* __restrict__ items, int n_items, const mkws_stream_desc* __restrict__ streams,
                                              int n_streams, int64_t src_floats, int64_t max_out, int64_t out_floats, int32_t* invalid) {
  const int64_t total = (int64_t)n_items + n_streams;
  const int64_t want = (total + kThreads - 1) / kThreads;
  const int64_t counters = want < (int64_t)gridDim.x ? want : (int64_t)gridDim.x;
  if ((int64_t)blockIdx.x >= counters) return;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < total; g += counters * kThreads) {
    bool ok;
    if (g < n_items) {
      const mkws_stream_item it = items[g];
      ok = it.stream >= 0 && it.stream < n_streams;
      if (ok) {
        const mkws_stream_desc d = streams[it.stream];
        ok = item_is_valid(it, g, d.first_item, d.n_items, d.max_frames, src_floats);
      }
    } else {
      ok = stream_is_valid(streams[g - n_items], src_floats, n_items, max_out, out_floats);
    }
    if (!ok) atomicAdd(invalid, 1);
  }
}

// v of frame i of a valid item, 0 <= i < n_frames: mkws_pcm_encode's rule.  |start| <= 2^61 and i < 2^62, so nothing overflows.
__device__ __forceinline__ float item_value(const mkws_stream_item& it, int64_t i, const float* __restrict__ src) {
  const int64_t p = it.start + i;
  const float x = (p >= 0 && p < it.src_len) ? src[it.src_offset + p] : 0.0f;
  const float f_in = i < it.fade_in ? __fdiv_rn((float)i, (float)it.fade_in) : 1.0f;
  const float f_out = i >= it.n_frames - it.fade_out ? __fdiv_rn((float)(it.n_frames - 1 - i), (float)it.fade_out) : 1.0f;
  return __fmul_rn(__fmul_rn(x, it.gain), __fmul_rn(f_in, f_out));
}

// The items of stream r (descriptor d, valid) that can reach positions [t0, t1): [ka, kb) of the table.  The same in every lane.
__device__ __forceinline__ void find_items(const mkws_stream_item* __restrict__ items, const mkws_stream_desc& d, int64_t t0, int64_t t1, int& ka,
                                           int& kb) {
  ka = kb = d.first_item;
  if (d.max_frames <= 0) return;                           // every item is empty or invalid
  const int64_t reach = t0 - d.max_frames;                 // an item that covers some t >= t0 has out_start > t0 - n_frames >= reach
  int lo = d.first_item, hi = d.first_item + d.n_items;
  const int end = hi;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (items[mid].out_start > reach) hi = mid; else lo = mid + 1;
  }
  ka = kb = lo;
  while (kb < end && items[kb].out_start < t1) ++kb;
}

// The foreground of the general body, shared by the mix and the power kernel: s[j] at the lane's position t0 + tid + j * 256 (positions
// at or past t1 are skipped), items [ka, kb) in ascending index.  Bit j of `covered` says that an item has set s[j].
__device__ __forceinline__ void foreground(const float* __restrict__ src, int64_t src_floats, const mkws_stream_item* __restrict__ items,
                                           const mkws_stream_desc& d, int r, int ka, int kb, int64_t t0, int64_t t1, float (&s)[kPer]) {
  unsigned covered = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) s[j] = 0.0f;
  for (int k = ka; k < kb; ++k) {
    const mkws_stream_item it = items[k];
    if (it.stream != r || !item_is_valid(it, k, d.first_item, d.n_items, d.max_frames, src_floats)) continue;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int64_t t = t0 + threadIdx.x + j * kThreads;
      const int64_t i = t - it.out_start;
      if (t < t1 && i >= 0 && i < it.n_frames) {
        const float v = item_value(it, i, src);
        s[j] = (covered >> j & 1u) ? __fadd_rn(s[j], v) : v;
        covered |= 1u << j;
      }
    }
  }
}

// The bed sample of the tile's position f (0 <= f < kTile); m0 = (bed_start + t0) mod bed_len.
__device__ __forceinline__ float bed_at(const float* __restrict__ bed, int64_t bed_len, int64_t m0, int f) {
  int64_t j;
  if (bed_len >= kTile) {
    j = m0 + f;
    if (j >= bed_len) j -= bed_len;
  } else {
    j = (int64_t)(((uint32_t)m0 + (uint32_t)f) % (uint32_t)bed_len);
  }
  return bed[j];
}

template <bool kBed, bool kClip>
__device__ __forceinline__ float finish(float s, float b, float g) {
  float y = kBed ? __fadd_rn(s, __fmul_rn(b, g)) : s;
  if (kClip) y = y > 1.0f ? 1.0f : (y < -1.0f ? -1.0f : y);     // comparisons: a NaN stays
  return y;
}

template <bool kBed, bool kClip>
__device__ __forceinline__ void mix_tile(const float* __restrict__ src, int64_t src_floats, const mkws_stream_item* __restrict__ items,
                                         const mkws_stream_desc& d, int r, float g, int64_t t0, int nf, float* __restrict__ out) {
  const int64_t t1 = t0 + nf;
  int ka, kb;
  find_items(items, d, t0, t1, ka, kb);
  const float* bed = src + (kBed ? d.bed_offset : 0);
  const int64_t m0 = kBed ? (d.bed_start + t0) % d.bed_len : 0;
  float* dst = out + (d.out_offset + t0);                    // [dst, dst + nf) is inside the stream's range

#ifndef MKWS_STREAM_GENERAL_ONLY      // a measuring build sends every tile through the general body
  if (kb - ka == 1) {
    const mkws_stream_item it = items[ka];
    const int64_t i0 = t0 - it.out_start;
    // one valid item over the whole tile, no fade and no edge of its recording inside: the body without per-position tests
    if (it.stream == r && item_is_valid(it, ka, d.first_item, d.n_items, d.max_frames, src_floats) && i0 >= 0 && i0 + nf <= it.n_frames &&
        i0 >= it.fade_in && i0 + nf <= it.n_frames - it.fade_out && it.start + i0 >= 0 && it.start + i0 + nf <= it.src_len) {
      const float* sp = src + (it.src_offset + it.start + i0);                    // [sp, sp + nf) is inside the recording
      const int to_word = (int)((4u - (unsigned)(((uintptr_t)dst >> 2) & 3u)) & 3u);
      const int head = to_word < nf ? to_word : nf;
      const int quads = (nf - head) / 4, tail = nf - head - 4 * quads;
      const int tid = threadIdx.x;
      if (tid < quads) {
        const int f = head + 4 * tid;
        float x[4];
        if ((((uintptr_t)(sp + head)) & 15u) == 0) {
          const float4 q = *(const float4*)(sp + f);
          x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = sp[f + e];
        }
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          y[e] = finish<kBed, kClip>(__fmul_rn(__fmul_rn(x[e], it.gain), 1.0f), kBed ? bed_at(bed, d.bed_len, m0, f + e) : 0.0f, g);
        *(float4*)(dst + f) = make_float4(y[0], y[1], y[2], y[3]);               // a multiple of 16 as an address
      }
      // the ragged ends, at most three positions each: lanes 64.. take the head, lanes 128.. the tail (waves other than the first)
      int f = -1;
      if (tid >= 64 && tid - 64 < head) f = tid - 64;
      if (tid >= 128 && tid - 128 < tail) f = head + 4 * quads + (tid - 128);
      if (f >= 0) dst[f] = finish<kBed, kClip>(__fmul_rn(__fmul_rn(sp[f], it.gain), 1.0f), kBed ? bed_at(bed, d.bed_len, m0, f) : 0.0f, g);
      return;
    }
  }
#endif

  float s[kPer];
  foreground(src, src_floats, items, d, r, ka, kb, t0, t1, s);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int f = threadIdx.x + j * kThreads;
    if (f < nf) dst[f] = finish<kBed, kClip>(s[j], kBed ? bed_at(bed, d.bed_len, m0, f) : 0.0f, g);
  }
}

__global__ __launch_bounds__(kThreads) void stream_mix_kernel(const float* __restrict__ src, int64_t src_floats,
                                                              const mkws_stream_item* __restrict__ items, int n_items,
                                                              const mkws_stream_desc* __restrict__ streams, int n_streams,
                                                              const float* __restrict__ bed_gain, int flags, uint32_t tiles, int64_t max_out,
                                                              float* __restrict__ out, int64_t out_floats, int32_t* invalid) {
  count_invalid(items, n_items, streams, n_streams, src_floats, max_out, out_floats, invalid);
  const int r = (int)(blockIdx.x / tiles);
  const uint32_t tile = blockIdx.x % tiles;
  const mkws_stream_desc d = streams[r];
  if (!stream_is_valid(d, src_floats, n_items, max_out, out_floats)) return;      // the same answer in every lane and tile
  const int64_t t0 = (int64_t)tile * kTile;
  if (t0 >= d.n_out) return;
  const int nf = (int)(d.n_out - t0 < kTile ? d.n_out - t0 : kTile);
  const bool with_bed = bed_gain != nullptr && d.bed_len > 0, clip = (flags & MKWS_STREAM_CLIP) != 0;
  const float g = with_bed ? bed_gain[r] : 0.0f;
  if (with_bed) {
    if (clip) mix_tile<true, true>(src, src_floats, items, d, r, g, t0, nf, out);
    else mix_tile<true, false>(src, src_floats, items, d, r, g, t0, nf, out);
  } else {
    if (clip) mix_tile<false, true>(src, src_floats, items, d, r, g, t0, nf, out);
    else mix_tile<false, false>(src, src_floats, items, d, r, g, t0, nf, out);
  }
}

// The sums of the 256 lanes' values, in an order fixed by the lane numbers alone: a butterfly inside each wave, then the four waves'
// sums in wave order.  Valid in lane 0.
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int wave = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) lds[wave] = v;
  __syncthreads();
  const double total = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(kThreads) void stream_power_kernel(const float* __restrict__ src, int64_t src_floats,
                                                                const mkws_stream_item* __restrict__ items, int n_items,
                                                                const mkws_stream_desc* __restrict__ streams, int n_streams, uint32_t tiles,
                                                                int64_t max_out, double* __restrict__ partials, int32_t* invalid) {
  __shared__ double lds[kThreads / 64];
  const int64_t no_out = INT64_MAX;                          // nothing is written at out_offset: only its sign is checked
  count_invalid(items, n_items, streams, n_streams, src_floats, max_out, no_out, invalid);
  const int r = (int)(blockIdx.x / tiles);
  const uint32_t tile = blockIdx.x % tiles;
  const mkws_stream_desc d = streams[r];
  const int64_t t0 = (int64_t)tile * kTile;
  double p_fg = 0.0, p_bed = 0.0;
  if (stream_is_valid(d, src_floats, n_items, max_out, no_out) && t0 < d.n_out) {  // the same answer in every lane
    const int nf = (int)(d.n_out - t0 < kTile ? d.n_out - t0 : kTile);
    int ka, kb;
    find_items(items, d, t0, t0 + nf, ka, kb);
    float s[kPer];
    foreground(src, src_floats, items, d, r, ka, kb, t0, t0 + nf, s);
    const int64_t m0 = d.bed_len > 0 ? (d.bed_start + t0) % d.bed_len : 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int f = threadIdx.x + j * kThreads;
      if (f < nf) {
        p_fg += (double)s[j] * (double)s[j];
        if (d.bed_len > 0) {
          const double b = (double)bed_at(src + d.bed_offset, d.bed_len, m0, f);
          p_bed += b * b;
        }
      }
    }
  }
  p_fg = block_sum(p_fg, lds);
  p_bed = block_sum(p_bed, lds);
  if (threadIdx.x == 0) {
    partials[2 * (size_t)blockIdx.x] = p_fg;
    partials[2 * (size_t)blockIdx.x + 1] = p_bed;
  }
}

__global__ __launch_bounds__(64) void stream_bed_gain_kernel(const double* __restrict__ partials, const mkws_stream_desc* __restrict__ streams,
                                                             uint32_t tiles, const double* __restrict__ snr_scale, float* __restrict__ bed_gain) {
  if (threadIdx.x != 0) return;
  const uint32_t r = blockIdx.x;
  const double* p = partials + 2 * (size_t)r * tiles;
  double p_fg = 0.0, p_bed = 0.0;
  for (uint32_t t = 0; t < tiles; ++t) {                     // ascending tile order
    p_fg += p[2 * (size_t)t];
    p_bed += p[2 * (size_t)t + 1];
  }
  float g = 0.0f;
  if (streams[r].bed_len > 0 && p_fg > 0.0 && p_bed > 0.0) g = (float)(sqrt(p_fg / p_bed) * snr_scale[r]);
  bed_gain[r] = g;
}

// The arguments the three entry points share -> MKWS_OK to go on, 1 for "nothing to do", or the error.
int check_grid(const char* what, int64_t src_floats, int n_items, int n_streams, int64_t max_out, int64_t* tiles) {
  if (src_floats < 0 || n_items < 0 || n_streams < 0 || max_out < 0)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "%s: src_floats = %lld, n_items = %d, n_streams = %d, max_out = %lld", what, (long long)src_floats,
                      n_items, n_streams, (long long)max_out);
  if (n_streams == 0 || max_out == 0) return 1;
  *tiles = (max_out - 1) / kTile + 1;
  if (*tiles > 0x7fffffffLL || *tiles * n_streams > 0x7fffffffLL)
    return mkws::fail(MKWS_ERR_UNSUPPORTED, "%s: %lld tiles x %d streams exceed one launch", what, (long long)*tiles, n_streams);
  return MKWS_OK;
}

}  // namespace

extern "C" {

int mkws_stream_mix(const float* d_src, int64_t src_floats, const mkws_stream_item* d_items, int n_items, const mkws_stream_desc* d_streams,
                    int n_streams, const float* d_bed_gain, int flags, int64_t max_out, float* d_out, int64_t out_floats, int32_t* d_invalid,
                    void* stream) {
  if (out_floats < 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "stream_mix: out_floats = %lld", (long long)out_floats);
  int64_t tiles = 0;
  const int rc = check_grid("stream_mix", src_floats, n_items, n_streams, max_out, &tiles);
  if (rc != MKWS_OK) return rc < 0 ? rc : MKWS_OK;
  if (!d_streams || !d_invalid || (!d_items && n_items > 0) || (!d_src && src_floats > 0) || (!d_out && out_floats > 0))
    return mkws::fail(MKWS_ERR_INVALID_ARG, "stream_mix: NULL buffer");
  if ((((uintptr_t)d_items | (uintptr_t)d_streams) & 7) != 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "stream_mix: a table is not 8-byte aligned");
  if ((((uintptr_t)d_src | (uintptr_t)d_out | (uintptr_t)d_bed_gain) & 3) != 0)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "stream_mix: a float buffer is not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  MKWS_HIP(hipMemsetAsync(d_invalid, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(stream_mix_kernel, dim3((uint32_t)(tiles * n_streams)), dim3(kThreads), 0, st, d_src, src_floats, d_items, n_items, d_streams,
                     n_streams, d_bed_gain, flags, (uint32_t)tiles, max_out, d_out, out_floats, d_invalid);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

int mkws_stream_power(const float* d_src, int64_t src_floats, const mkws_stream_item* d_items, int n_items, const mkws_stream_desc* d_streams,
                      int n_streams, int64_t max_out, double* d_partials, int32_t* d_invalid, void* stream) {
  int64_t tiles = 0;
  const int rc = check_grid("stream_power", src_floats, n_items, n_streams, max_out, &tiles);
  if (rc != MKWS_OK) return rc < 0 ? rc : MKWS_OK;
  if (!d_streams || !d_invalid || !d_partials || (!d_items && n_items > 0) || (!d_src && src_floats > 0))
    return mkws::fail(MKWS_ERR_INVALID_ARG, "stream_power: NULL buffer");
  if ((((uintptr_t)d_items | (uintptr_t)d_streams | (uintptr_t)d_partials) & 7) != 0)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "stream_power: a table or the partials are not 8-byte aligned");
  if (((uintptr_t)d_src & 3) != 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "stream_power: the source is not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  MKWS_HIP(hipMemsetAsync(d_invalid, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(stream_power_kernel, dim3((uint32_t)(tiles * n_streams)), dim3(kThreads), 0, st, d_src, src_floats, d_items, n_items,
                     d_streams, n_streams, (uint32_t)tiles, max_out, d_partials, d_invalid);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

int mkws_stream_bed_gain(const double* d_partials, const mkws_stream_desc* d_streams, int n_streams, int64_t max_out, const double* d_snr_scale,
                         float* d_bed_gain, void* stream) {
  int64_t tiles = 0;
  const int rc = check_grid("stream_bed_gain", 0, 0, n_streams, max_out, &tiles);
  if (rc != MKWS_OK) return rc < 0 ? rc : MKWS_OK;
  if (!d_partials || !d_streams || !d_snr_scale || !d_bed_gain) return mkws::fail(MKWS_ERR_INVALID_ARG, "stream_bed_gain: NULL buffer");
  if ((((uintptr_t)d_partials | (uintptr_t)d_streams | (uintptr_t)d_snr_scale) & 7) != 0 || ((uintptr_t)d_bed_gain & 3) != 0)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "stream_bed_gain: a buffer is not aligned to its element");
  hipLaunchKernelGGL(stream_bed_gain_kernel, dim3((uint32_t)n_streams), dim3(64), 0, (hipStream_t)stream, d_partials, d_streams, (uint32_t)tiles,
                     d_snr_scale, d_bed_gain);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

}  // extern "C"
