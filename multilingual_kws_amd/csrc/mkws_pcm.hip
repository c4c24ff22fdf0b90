// WAV sample data decoded on the device (include/mkws.h, "WAV sample data decoded on the device"): one launch turns a table of work
// items -- byte ranges of any format and channel layout inside one byte buffer -- into float32 rows.
//
// A workgroup of 256 lanes owns kTile = 1024 consecutive outputs of one item.  It walks the frames of its tile in chunks whose byte
// span fits kStageBytes of LDS: the span is staged with 16-byte loads aligned on the ADDRESS (byte_offset has byte granularity, and s24
// frames are 3, 6, 9 ... bytes), the first and the last 16-byte word of a span are clamped to the byte buffer and assembled from byte
// loads, and the samples are then assembled from LDS -- by one aligned LDS read where the sample's LDS address is a multiple of its
// size, byte by byte otherwise.  Neighbouring lanes take neighbouring frames, so the stores are coalesced.  A frame wider than
// kStageBytes (more than 2048 channels of f64) is read from global memory byte by byte instead: same arithmetic, no staging.  Every
// item is checked against the buffers before anything is read or written for it; all of that arithmetic is 64-bit.
#include <cstdint>

#include "mkws_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;                 // outputs of one workgroup
constexpr int kStageBytes = 16 * 1024;      // bytes of frames staged at a time
constexpr int kLdsBytes = kStageBytes + 32; // + the alignment slack of the first and of the last 16-byte word

__host__ __device__ __forceinline__ int sample_bytes(int format) {
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

// The value of the sample whose little-endian bytes are the low sample_bytes(format) bytes of `raw`.
__device__ __forceinline__ float sample_value(int format, uint64_t raw) {
  switch (format) {
    case MKWS_PCM_U8: return (float)((int)(raw & 0xFF) - 128) / 128.0f;
    case MKWS_PCM_S16: return (float)(int16_t)(raw & 0xFFFF) / 32768.0f;
    case MKWS_PCM_S24: return (float)((int32_t)((uint32_t)raw << 8) >> 8) / 8388608.0f;
    case MKWS_PCM_S32: return __fmul_rn((float)(int32_t)(uint32_t)raw, 4.656612873077392578125e-10f);      // 2^-31
    case MKWS_PCM_F32: return __uint_as_float((uint32_t)raw);
    case MKWS_PCM_F64: return (float)__longlong_as_double((long long)raw);
    case MKWS_PCM_MULAW: {
      int u = ~(int)raw & 0xFF;
      int t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7);
      int s = (u & 0x80) ? 0x84 - t : t - 0x84;
      return (float)s / 32768.0f;
    }
    default: {                               // MKWS_PCM_ALAW
      int a = ((int)raw & 0xFF) ^ 0x55;
      int t = (a & 0x0F) << 4, seg = (a & 0x70) >> 4;
      if (seg == 0) t += 8;
      else if (seg == 1) t += 0x108;
      else t = (t + 0x108) << (seg - 1);
      int s = (a & 0x80) ? t : -t;
      return (float)s / 32768.0f;
    }
  }
}

// sb bytes at p (LDS or global), little-endian.  LDS: one read where the address allows it, else bytes; global: bytes.
template <bool LDS>
__device__ __forceinline__ uint64_t load_raw(const unsigned char* p, int sb) {
  if (LDS) {
    const uintptr_t a = (uintptr_t)p;
    if (sb == 2 && (a & 1) == 0) return *(const uint16_t*)p;
    if (sb == 4 && (a & 3) == 0) return *(const uint32_t*)p;
    if (sb == 8 && (a & 7) == 0) return *(const uint64_t*)p;
  }
  uint64_t raw = 0;
  for (int k = 0; k < sb; ++k) raw |= (uint64_t)p[k] << (8 * k);
  return raw;
}

// The float of one frame whose first byte is at p.
template <bool LDS>
__device__ __forceinline__ float frame_value(const unsigned char* p, int format, int sb, int channels, int channel) {
  if (channel >= 0) return sample_value(format, load_raw<LDS>(p + (int64_t)channel * sb, sb));
  float acc = 0.0f;
  for (int c = 0; c < channels; ++c) acc = __fadd_rn(acc, sample_value(format, load_raw<LDS>(p + (int64_t)c * sb, sb)));
  return __fdiv_rn(acc, (float)channels);
}

__device__ __forceinline__ bool item_is_valid(const mkws_pcm_item& it, int64_t n_bytes, int64_t max_out_len, int64_t out_floats) {
  if (it.format < 0 || it.format >= MKWS_PCM_NUM_FORMATS) return false;
  if (it.channels < 1 || it.channel < -1 || it.channel >= it.channels) return false;
  if (it.n_frames < 0 || it.out_len < 0 || it.out_len > max_out_len) return false;
  if (it.byte_offset < 0 || it.byte_offset > n_bytes) return false;
  const int64_t fb = (int64_t)sample_bytes(it.format) * (int64_t)it.channels;     // <= 8 * (2^31 - 1)
  if (it.n_frames > (n_bytes - it.byte_offset) / fb) return false;
  if (it.out_offset < 0 || it.out_offset > out_floats || it.out_len > out_floats - it.out_offset) return false;
  return true;
}

__global__ __launch_bounds__(kThreads) void pcm_decode_kernel(const unsigned char* __restrict__ bytes, int64_t n_bytes,
                                                              const mkws_pcm_item* __restrict__ items, uint32_t tiles, int64_t max_out_len,
                                                              float* __restrict__ out, int64_t out_floats, int32_t* invalid) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLdsBytes];
  const uint32_t k = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const mkws_pcm_item it = items[k];
  if (!item_is_valid(it, n_bytes, max_out_len, out_floats)) {      // the same answer in every lane and every tile of the item
    if (tile == 0 && threadIdx.x == 0) atomicAdd(invalid, 1);
    return;
  }
  const int64_t n0 = (int64_t)tile * kTile;
  if (n0 >= it.out_len) return;
  const int64_t n1 = n0 + kTile < it.out_len ? n0 + kTile : it.out_len;          // outputs [n0, n1) are this workgroup's
  const int64_t f1 = n1 < it.n_frames ? n1 : it.n_frames;                        // frames [n0, f1) exist (none if f1 <= n0)
  float* orow = out + it.out_offset;
  const int sb = sample_bytes(it.format);
  const int64_t fb = (int64_t)sb * it.channels;

  if (fb > kStageBytes) {
    for (int64_t f = n0 + threadIdx.x; f < f1; f += kThreads)
      orow[f] = frame_value<false>(bytes + it.byte_offset + f * fb, it.format, sb, it.channels, it.channel);
  } else {
    const int chunk = (int)(kStageBytes / fb);                                    // frames per staged chunk, at least 1
    for (int64_t c0 = n0; c0 < f1; c0 += chunk) {
      const int cf = (int)(f1 - c0 < chunk ? f1 - c0 : chunk);
      // bytes [b0, b1) of the buffer, inside [0, n_bytes) by the item's check; staged from the 16-byte word that holds b0
      const int64_t b0 = it.byte_offset + c0 * fb, b1 = b0 + (int64_t)cf * fb;
      const int shift = (int)(((uintptr_t)bytes + (uint64_t)b0) & 15);
      const int64_t w0 = b0 - shift;                                              // may be below 0: clamped below
      const int words = (int)((b1 - w0 + 15) / 16);                               // <= kStageBytes / 16 + 2
      __syncthreads();                                                            // the previous chunk has been read
      for (int w = threadIdx.x; w < words; w += kThreads) {
        const int64_t at = w0 + (int64_t)w * 16;
        uint4 v;
        if (at >= 0 && at + 16 <= n_bytes) {
          v = *(const uint4*)(bytes + at);
        } else {
          uint32_t part[4] = {0u, 0u, 0u, 0u};
          for (int j = 0; j < 16; ++j) {
            const int64_t g = at + j;
            if (g >= 0 && g < n_bytes) part[j >> 2] |= (uint32_t)bytes[g] << (8 * (j & 3));
          }
          v = make_uint4(part[0], part[1], part[2], part[3]);
        }
        *(uint4*)(lds + w * 16) = v;
      }
      __syncthreads();
      for (int f = threadIdx.x; f < cf; f += kThreads)
        orow[c0 + f] = frame_value<true>(lds + shift + (int64_t)f * fb, it.format, sb, it.channels, it.channel);
    }
  }
  const int64_t z0 = n0 > it.n_frames ? n0 : it.n_frames;
  for (int64_t i = z0 + threadIdx.x; i < n1; i += kThreads) orow[i] = 0.0f;
}

}  // namespace

extern "C" {

int mkws_pcm_frame_bytes(int format, int channels) {
  const int sb = sample_bytes(format);
  if (sb == 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "pcm_frame_bytes: format %d (0 .. %d)", format, MKWS_PCM_NUM_FORMATS - 1);
  if (channels < 1) return mkws::fail(MKWS_ERR_INVALID_ARG, "pcm_frame_bytes: channels = %d (at least 1)", channels);
  if ((int64_t)sb * channels > 0x7fffffffLL) return mkws::fail(MKWS_ERR_INVALID_ARG, "pcm_frame_bytes: %d channels of %d bytes overflow", channels, sb);
  return sb * channels;
}

int mkws_pcm_decode(const uint8_t* d_bytes, int64_t n_bytes, const mkws_pcm_item* d_items, int n_items, int64_t max_out_len, float* d_out,
                    int64_t out_floats, int32_t* d_invalid, void* stream) {
  if (n_bytes < 0 || n_items < 0 || max_out_len < 0 || out_floats < 0)
    return mkws::fail(MKWS_ERR_INVALID_ARG, "pcm_decode: n_bytes = %lld, n_items = %d, max_out_len = %lld, out_floats = %lld", (long long)n_bytes,
                      n_items, (long long)max_out_len, (long long)out_floats);
  if (n_items == 0 || max_out_len == 0) return MKWS_OK;
  if (!d_items || !d_invalid || (!d_bytes && n_bytes > 0) || (!d_out && out_floats > 0))
    return mkws::fail(MKWS_ERR_INVALID_ARG, "pcm_decode: NULL buffer");
  if (((uintptr_t)d_items & 7) != 0) return mkws::fail(MKWS_ERR_INVALID_ARG, "pcm_decode: the item table is not 8-byte aligned");
  const int64_t tiles = (max_out_len + kTile - 1) / kTile;
  if (tiles > 0x7fffffffLL || tiles * n_items > 0x7fffffffLL)
    return mkws::fail(MKWS_ERR_UNSUPPORTED, "pcm_decode: %lld tiles x %d items exceed one launch", (long long)tiles, n_items);
  hipStream_t st = (hipStream_t)stream;
  MKWS_HIP(hipMemsetAsync(d_invalid, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(pcm_decode_kernel, dim3((uint32_t)(tiles * n_items)), dim3(kThreads), 0, st, (const unsigned char*)d_bytes, n_bytes, d_items,
                     (uint32_t)tiles, max_out_len, d_out, out_floats, d_invalid);
  MKWS_HIP(hipGetLastError());
  return MKWS_OK;
}

}  // extern "C"
