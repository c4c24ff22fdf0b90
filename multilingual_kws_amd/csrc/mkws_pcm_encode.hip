// Device audio encoded into WAV sample data (include/mkws.h, "Device audio encoded into WAV sample data"): one launch turns a table
// of work items -- a window of a float32 recording, a gain, two linear fades, a format -- into the bytes of mono sample data, each
// item at any byte of one byte buffer.  The inverse of mkws_pcm.hip.
//
// A workgroup of 256 lanes owns kTile = 1024 consecutive frames of one item, at most 8 KiB of output.  Neighbouring lanes take
// neighbouring frames (coalesced float loads), encode them and put the sample into an LDS image of the tile that is shifted by the
// low four bits of the tile's first output ADDRESS: byte j of the tile sits at lds[shift + j], so a 16-byte word of the image is a
// 16-byte aligned word of global memory.  A sample is put into LDS with one store where its LDS address is a multiple of its size
// and byte by byte otherwise (s24 always).  After the barrier the image leaves in 16-byte stores; the first and the last word of the
// image, where they are not wholly the tile's, are written byte by byte, so that no byte outside [byte_offset, byte_offset +
// n_frames * sample bytes) is touched -- two items, or two tiles of one item, may abut inside one 16-byte word.  Every item is checked
// against the buffers before anything is read or written for it; all of that arithmetic is 64-bit.
#include <cstdint>

#include "mkws_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;                  // frames of one workgroup
constexpr int kLdsBytes = kTile * 8 + 16;    // the widest sample, + the shift of the first word
constexpr int64_t kStartLimit = (int64_t)1 << 61;

__device__ __forceinline__ int sample_bytes(int format) {
  switch (format) {
    case MKWS_PCM_U8:
    case MKWS_PCM_MULAW:
    case MKWS_PCM_ALAW: return 1;
    case MKWS_PCM_S16: return 2;
    case MKWS_PCM_S24: return 3;
    case MKWS_PCM_S32:
    case MKWS_PCM_F32: return 4;
    case MKWS_PCM_F64: return 8;
    default: return 0;
  }
}

// rint(v * scale) clamped to [lo, hi], both exact in float32; NaN gives 0.  (fmaxf / fminf would send NaN to a rail.)
__device__ __forceinline__ int32_t quantise(float v, float scale, float lo, float hi) {
  const float r = rintf(__fmul_rn(v, scale));
  if (r != r) return 0;
  if (r <= lo) return (int32_t)lo;
  if (r >= hi) return (int32_t)hi;
  return (int32_t)r;
}

// G.711 compressors in their usual closed form (the header states them); q is a 16-bit linear sample.
__device__ __forceinline__ uint32_t mulaw_code(int q) {
  int m = q >> 2, mask = 0xFF;
  if (m < 0) { m = -m; mask = 0x7F; }
  if (m > 8159) m = 8159;
  m += 33;
  int seg = 0;
  while (seg < 8 && m > (0x40 << seg) - 1) ++seg;       // segment ends 0x3F, 0x7F, ..., 0x1FFF
  const int code = seg >= 8 ? 0x7F : ((seg << 4) | ((m >> (seg + 1)) & 15));
  return (uint32_t)(code ^ mask);
}

__device__ __forceinline__ uint32_t alaw_code(int q) {
  int m = q >> 3, mask = 0xD5;
  if (m < 0) { m = -m - 1; mask = 0x55; }
  int seg = 0;
  while (seg < 8 && m > (0x20 << seg) - 1) ++seg;       // segment ends 0x1F, 0x3F, ..., 0xFFF
  const int code = seg >= 8 ? 0x7F : ((seg << 4) | ((seg < 2 ? m >> 1 : m >> seg) & 15));
  return (uint32_t)(code ^ mask);
}

// The little-endian bytes of v in `format`, in the low sample_bytes(format) bytes of the result.
__device__ __forceinline__ uint64_t sample_code(int format, float v) {
  switch (format) {
    case MKWS_PCM_U8: return (uint64_t)(uint32_t)(quantise(v, 128.0f, -128.0f, 127.0f) + 128);
    case MKWS_PCM_S16: return (uint64_t)((uint32_t)quantise(v, 32768.0f, -32768.0f, 32767.0f) & 0xFFFFu);
    case MKWS_PCM_S24: return (uint64_t)((uint32_t)quantise(v, 8388608.0f, -8388608.0f, 8388607.0f) & 0xFFFFFFu);
    case MKWS_PCM_S32: {
      const float t = __fmul_rn(v, 2147483648.0f);
      if (t != t) return 0;
      if (t >= 2147483648.0f) return 0x7FFFFFFFull;
      if (t <= -2147483648.0f) return 0x80000000ull;
      return (uint64_t)(uint32_t)(int32_t)rintf(t);
    }
    case MKWS_PCM_F32: return (uint64_t)__float_as_uint(v);
    case MKWS_PCM_F64: return (uint64_t)__double_as_longlong((double)v);
    case MKWS_PCM_MULAW: return mulaw_code(quantise(v, 32768.0f, -32768.0f, 32767.0f));
    default: return alaw_code(quantise(v, 32768.0f, -32768.0f, 32767.0f));      // MKWS_PCM_ALAW
  }
}

// The low sb bytes of raw to the LDS address p: one store where the address allows it, else bytes.
__device__ __forceinline__ void store_raw(unsigned char* p, int sb, uint64_t raw) {
  const uintptr_t a = (uintptr_t)p;
  if (sb == 2 && (a & 1) == 0) { *(uint16_t*)p = (uint16_t)raw; return; }
  if (sb == 4 && (a & 3) == 0) { *(uint32_t*)p = (uint32_t)raw; return; }
  if (sb == 8 && (a & 7) == 0) { *(uint64_t*)p = raw; return; }
  for (int k = 0; k < sb; ++k) p[k] = (unsigned char)(raw >> (8 * k));
}

__device__ __forceinline__ bool item_is_valid(const mkws_pcm_encode_item& it, int64_t src_floats, int64_t max_frames, int64_t out_bytes) {
  if (it.format < 0 || it.format >= MKWS_PCM_NUM_FORMATS) return false;
  if (it.n_frames < 0 || it.n_frames > max_frames || it.fade_in < 0 || it.fade_out < 0 || it.src_len < 0) return false;
  if (it.start < -kStartLimit || it.start > kStartLimit) return false;
  if (it.src_offset < 0 || it.src_offset > src_floats || it.src_len > src_floats - it.src_offset) return false;
  if (it.byte_offset < 0 || it.byte_offset > out_bytes) return false;
  if (it.n_frames > (out_bytes - it.byte_offset) / sample_bytes(it.format)) return false;
  return true;
}

__global__ __launch_bounds__(kThreads) void pcm_encode_kernel(const float* __restrict__ src, int64_t src_floats,
                                                              const mkws_pcm_encode_item* __restrict__ items, uint32_t tiles, int64_t max_frames,
                                                              unsigned char* __restrict__ out, int64_t out_bytes, int32_t* invalid) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
  const uint32_t k = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const mkws_pcm_encode_item it = items[k];
  if (!item_is_valid(it, src_floats, max_frames, out_bytes)) {     // the same answer in every lane and every tile of the item
    if (tile == 0 && threadIdx.x == 0) atomicAdd(invalid, 1);
    return;
  }
  const int64_t n0 = (int64_t)tile * kTile;
  if (n0 >= it.n_frames) return;
  const int nf = (int)(it.n_frames - n0 < kTile ? it.n_frames - n0 : kTile);      // frames [n0, n0 + nf) are this workgroup's
  const int sb = sample_bytes(it.format);
  // frames [lo, hi) of the item lie inside the recording: |start| <= 2^61 and src_len < 2^62 (a real buffer), so nothing overflows
  const int64_t lo = it.start < 0 ? -it.start : 0, hi = it.src_len - it.start;
  // bytes [b0, b0 + nb) of the buffer, inside [0, out_bytes) by the item's check
  const int64_t b0 = it.byte_offset + n0 * sb;
  const int nb = nf * sb;
  const int shift = (int)(((uintptr_t)out + (uint64_t)b0) & 15);
  const float inv_in = (float)it.fade_in, inv_out = (float)it.fade_out;
  const int64_t out_from = it.n_frames - it.fade_out;

  for (int f = threadIdx.x; f < nf; f += kThreads) {
    const int64_t i = n0 + f;
    const float x = (i >= lo && i < hi) ? src[it.src_offset + (it.start + i)] : 0.0f;
    const float f_in = i < it.fade_in ? __fdiv_rn((float)i, inv_in) : 1.0f;
    const float f_out = i >= out_from ? __fdiv_rn((float)(it.n_frames - 1 - i), inv_out) : 1.0f;
    const float v = __fmul_rn(__fmul_rn(x, it.gain), __fmul_rn(f_in, f_out));
    store_raw(lds + shift + f * sb, sb, sample_code(it.format, v));
  }
  __syncthreads();
  const int end = shift + nb, words = (end + 15) / 16;                             // <= kLdsBytes / 16
  for (int w = threadIdx.x; w < words; w += kThreads) {
    const int l0 = w * 16;
    if (l0 >= shift && l0 + 16 <= end) {
      *(uint4*)(out + (b0 + (l0 - shift))) = *(const uint4*)(lds + l0);            // a multiple of 16 as an address
    } else {                                                                       // the ragged head or tail: the tile's own bytes only
      for (int l = l0 > shift ? l0 : shift; l < l0 + 16 && l < end; ++l) out[b0 + (l - shift)] = lds[l];
    }
  }
}

}  // namespace

extern "C" {

int mkws_pcm_encode(const float* d_src, int64_t src_floats, const mkws_pcm_encode_item* d_items, int n_items, int64_t max_frames,
                    uint8_t* d_out, int64_t out_bytes, int32_t* d_invalid, void* stream) {
  if (src_floats < 0 || n_items < 0 || max_frames < 0 || out_bytes < 0)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "pcm_encode: src_floats = %lld, n_items = %d, max_frames = %lld, out_bytes = %lld", (long long)src_floats,
                      n_items, (long long)max_frames, (long long)out_bytes);
  if (n_items == 0 || max_frames == 0) return MKWS_OK;
  if (!d_items || !d_invalid || (!d_src && src_floats > 0) || (!d_out && out_bytes > 0))
    return mkws::fail(MKWS_ERR_INVALID_ARG, "pcm_encode: NULL buffer");
  if (((uintptr_t)d_items & 7) != 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "pcm_encode: the item table is not 8-byte aligned");
  if (((uintptr_t)d_src & 3) != 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "pcm_encode: the source is not 4-byte aligned");
  const int64_t tiles = (max_frames - 1) / kTile + 1;
  if (tiles > 0x7fffffffLL || tiles * n_items > 0x7fffffffLL)
    return mkws::fail(MKWS_ERR_UNSUPPORTED, "pcm_encode: %lld tiles x %d items exceed one launch", (long long)tiles, n_items);
  hipStream_t st = (hipStream_t)stream;
  MKWS_HIP(hipMemsetAsync(d_invalid, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(pcm_encode_kernel, dim3((uint32_t)(tiles * n_items)), dim3(kThreads), 0, st, d_src, src_floats, d_items, (uint32_t)tiles,
                     max_frames, (unsigned char*)d_out, out_bytes, d_invalid);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

}  // extern "C"
