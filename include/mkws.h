/*
 * mkws.h -- C-ABI of libmkws_hip.so: the MI355X (gfx950) hot path of multilingual_kws
 * (micro-frontend features -> EfficientNet-B0 embedding -> few-shot head).
 *
 * The reference (harvard-edge/multilingual_kws) is pure Python on TensorFlow and has no FFI; its
 * boundary for this path is a Python function surface.  Each entry point below names the reference
 * call it replaces (file:line relative to the reference repo).  INTEGRATION.md shows the ctypes
 * binding a reference maintainer would add.
 *
 * Conventions
 *  - plain C: pointers + sizes, no C++/torch types.  Returns MKWS_OK (0) or a negative mkws_status;
 *    never throws.  mkws_last_error() returns a thread-local message for the last failure.
 *  - every `d_*` pointer is caller-owned DEVICE memory (e.g. torch tensor.data_ptr()), contiguous,
 *    row-major.  `h_*` pointers are host memory.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  All *_forward / *_step
 *    calls are asynchronous on that stream, allocate nothing and never synchronise the device, so
 *    they are hipGraph-capturable.  Handles own only tables, weights and a workspace sized at create.
 *  - a handle belongs to the device that was current at create; not thread-safe; distinct handles are.
 *  - there is no CPU fallback: with no usable GPU, create fails with MKWS_ERR_NO_DEVICE.
 */
#ifndef MKWS_H_
#define MKWS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKWS_ABI_VERSION 5

typedef enum mkws_status {
  MKWS_OK = 0,
  MKWS_ERR_INVALID_ARG = -1,   /* NULL pointer, negative size, batch > max_batch, ... */
  MKWS_ERR_UNSUPPORTED = -2,   /* configuration outside what the kernels implement */
  MKWS_ERR_NO_DEVICE = -3,     /* no HIP device / not gfx950 */
  MKWS_ERR_HIP = -4,           /* a HIP runtime call failed; see mkws_last_error() */
  MKWS_ERR_ALLOC = -5,
  MKWS_ERR_BAD_WEIGHTS = -6,   /* weight blob does not match the architecture */
  MKWS_ERR_EXCHANGE = -7       /* an in-kernel exchange of the paired whole-block kernel failed in an EARLIER forward of this
                                  handle (its embeddings are NaN); the handle has switched plans: repeat the call */
} mkws_status;

int mkws_abi_version(void);
const char* mkws_last_error(void);
/* Name of the architecture the device code was compiled for ("gfx950"). */
const char* mkws_build_arch(void);

/* ------------------------------------------------------------------------------------------------
 * Micro-frontend.  Replaces the AudioMicrofrontend op call in
 *   multilingual_kws/embedding/input_data.py:19-35  (to_micro_spectrogram)
 * including the `audio * 32768 -> int16` cast (:23) and the `* 10/256` scaling (:34), batched.
 * Field defaults = input_data.py:25-33 plus the TF Python wrapper's own defaults.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mkws_frontend_cfg {
  int32_t sample_rate;          /* 16000 */
  int32_t window_size_ms;       /* 30  (model_settings["window_size_samples"]*1000/sample_rate) */
  int32_t window_step_ms;       /* 20 */
  int32_t num_channels;         /* 40  (model_settings["fingerprint_width"]) */
  float upper_band_limit;       /* 7500 */
  float lower_band_limit;       /* 125 */
  int32_t smoothing_bits;       /* 10 */
  float even_smoothing;         /* 0.025 */
  float odd_smoothing;          /* 0.06 */
  float min_signal_remaining;   /* 0.05 */
  int32_t enable_pcan;          /* 1 */
  float pcan_strength;          /* 0.95 */
  float pcan_offset;            /* 80 */
  int32_t gain_bits;            /* 21 */
  int32_t enable_log;           /* 1 */
  int32_t scale_shift;          /* 6 */
} mkws_frontend_cfg;

typedef struct mkws_frontend mkws_frontend;

/* Fills *cfg with the defaults above. */
void mkws_frontend_default_cfg(mkws_frontend_cfg* cfg);

/* Host-only (no GPU needed): builds the integer tables for `cfg` exactly as the upstream C library
 * does and copies table `which` into dst (at most cap_bytes).  Returns the table's size in bytes,
 * or a negative mkws_status.  `which`: */
enum {
  MKWS_FT_WINDOW_COEF = 0,     /* int16[window_size] */
  MKWS_FT_TWIDDLES = 1,        /* int16[2*ncfft]  (r,i) pairs of the ncfft-point complex FFT */
  MKWS_FT_SUPER_TWIDDLES = 2,  /* int16[2*(ncfft/2)] */
  MKWS_FT_FB_WEIGHTS = 3,      /* int16[num_weights] */
  MKWS_FT_FB_UNWEIGHTS = 4,    /* int16[num_weights] */
  MKWS_FT_FB_FREQ_STARTS = 5,  /* int16[num_channels+1] */
  MKWS_FT_FB_WEIGHT_STARTS = 6,/* int16[num_channels+1] */
  MKWS_FT_FB_WIDTHS = 7,       /* int16[num_channels+1] */
  MKWS_FT_PCAN_LUT = 8,        /* int16[125] */
  MKWS_FT_LOG_LUT = 9,         /* uint16[130] */
  MKWS_FT_SCALARS = 10         /* int32[8]: window_size, window_step, fft_size, start_index, end_index,
                                  num_weights, snr_shift, correction_bits */
};
int mkws_frontend_host_table(const mkws_frontend_cfg* cfg, int which, void* dst, size_t cap_bytes);

/* Number of frames the op emits for n_samples of audio (0 if shorter than one window). */
int mkws_frontend_num_frames(const mkws_frontend_cfg* cfg, int n_samples);

/* Builds the tables on the host, uploads them once.  max_samples bounds n_samples of later calls. */
int mkws_frontend_create(const mkws_frontend_cfg* cfg, int max_samples, mkws_frontend** out);
void mkws_frontend_destroy(mkws_frontend* fe);

/* d_audio float32 [B, n_samples] in [-1,1]  ->  d_spec float32 [B, frames, channels]
 * (= raw uint16 * 10/256, what to_micro_spectrogram returns).  d_raw (optional, may be NULL) receives
 * the op's raw uint16 [B, frames, channels] for bit-exact checks. */
int mkws_frontend_forward_f32(mkws_frontend* fe, const float* d_audio, int B, int n_samples,
                              float* d_spec, uint16_t* d_raw, void* stream);
/* Same with int16 PCM input (what decode_wav holds before the /32768, input_data.py:41-45). */
int mkws_frontend_forward_i16(mkws_frontend* fe, const int16_t* d_audio, int B, int n_samples,
                              float* d_spec, uint16_t* d_raw, void* stream);

/* Streaming form of batch_streaming_analysis.py:99-117: one long recording d_audio [n_samples]
 * (float32), windows of `window_samples` every `hop_samples`; window w covers samples
 * [w*hop, w*hop + window_samples).  Emits d_spec [num_windows, frames, channels] with
 * num_windows = 1 + (n_samples - window_samples) / hop_samples... (0 if too short).  Requires
 * hop_samples to be a multiple of the frame step so per-frame FFT/filterbank work is shared
 * across overlapping windows; the noise-reduction/PCAN recurrence restarts per window exactly as
 * the reference's per-window op call does.  Returns num_windows or a negative mkws_status. */
int mkws_frontend_stream_f32(mkws_frontend* fe, const float* d_audio, int n_samples,
                             int window_samples, int hop_samples, float* d_spec, uint16_t* d_raw,
                             int max_windows, void* stream);

/* Live form of mkws_frontend_stream_f32: the same stream fed push by push.  A push is hops_per_push * hop_samples NEW samples (d_audio,
 * float32); what the stream has to remember between pushes -- its position, the audio of the frame that is not complete yet and a ring
 * of per-frame filterbank outputs -- lives in d_state, a caller-owned device block of mkws_frontend_live_state_bytes() bytes, 8-byte
 * aligned.  A zero-filled block is a fresh stream (reset = memset, snapshot / restore = copies; the handle holds nothing of the stream,
 * so one handle serves any number of them).  Its first int64 is the number of samples pushed so far.
 * After pushes totalling n samples the windows w < W(n) exist, W(n) = 0 for n < window_samples, else 1 + (n - window_samples) /
 * hop_samples (the num_windows of mkws_frontend_stream_f32).  A push emits the windows it completed, in order, into rows 0 .. count-1
 * of d_spec [hops_per_push, frames, channels] and d_raw (either may be NULL, not both): count = W(n + push) - W(n), i.e. 0 while the
 * first window fills, then hops_per_push.  Rows from count on are left untouched.  Row of window w = row w of
 * mkws_frontend_stream_f32 over the whole recording, bit for bit.
 * d_meta int64 [2 + hops_per_push] = {count, index of the first new window, time_ms of each new window}; the time of window w is
 * (w * hop_samples * 1000) / sample_rate in integers, the start of the window; entries from 2 + count on are left untouched.
 * MKWS_ERR_INVALID_ARG for NULL pointers, non-positive sizes and a window shorter than one frame; MKWS_ERR_UNSUPPORTED for a hop that is
 * not a multiple of the frame step.  mkws_frontend_live_state_bytes returns 0 for what the push would refuse.  Two launches,
 * asynchronous on `stream`, allocates nothing, never synchronises: capturable like every other call (a replayed graph advances the
 * stream by itself: the position is device state). */
size_t mkws_frontend_live_state_bytes(const mkws_frontend* fe, int window_samples, int hop_samples, int hops_per_push);
int mkws_frontend_live_push_f32(mkws_frontend* fe, void* d_state, const float* d_audio, int window_samples, int hop_samples,
                                int hops_per_push, float* d_spec, uint16_t* d_raw, int64_t* d_meta, void* stream);

/* n_streams live streams advanced by one push each, in the same two launches.  Stream s's state block is d_states + s *
 * state_stride_bytes (a multiple of 8, at least mkws_frontend_live_state_bytes(); MKWS_ERR_INVALID_ARG otherwise) and is exactly the
 * block the one-stream call takes: a slice may be copied out, pushed with mkws_frontend_live_push_f32 and copied back.  The call is
 * that call applied to every ACTIVE stream's slice, byte for byte: d_active int32 [n_streams] (NULL = all active); d_audio
 * [n_streams, hops_per_push * hop_samples]; stream s owns rows s * hops_per_push .. + count_s - 1 of d_spec / d_raw
 * [n_streams * hops_per_push, frames, channels] (the rows of one embedding batch) and row s of d_meta [n_streams, 2 + hops_per_push].
 * A stream with d_active[s] == 0 is not advanced: its state slice and its spec / raw rows are untouched (its audio row is not read) and
 * its meta row gets count = 0 and the index of the window it is at.  The streams are independent: each is wherever its own pushes
 * have brought it.  Refusals as the one-stream call, and n_streams < 0; n_streams == 0 returns MKWS_OK with nothing launched.  Two
 * launches for any n_streams, asynchronous on `stream`, allocates nothing, never synchronises: capturable. */
int mkws_frontend_live_push_many_f32(mkws_frontend* fe, void* d_states, size_t state_stride_bytes, int n_streams, const int32_t* d_active,
                                     const float* d_audio, int window_samples, int hop_samples, int hops_per_push, float* d_spec,
                                     uint16_t* d_raw, int64_t* d_meta, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The mfcc and average feature modes.  Replaces the non-micro branch of the reference's pipeline,
 *   tf_v1_speechcommands/input_data_fix_bg.py:444-475
 * audio_ops.audio_spectrogram(window_size, stride, magnitude_squared=True), then audio_ops.mfcc(spectrogram, sample_rate,
 * dct_coefficient_count) or tf.nn.pool(AVG, SAME) over average_window_width bins.  The arithmetic, from TensorFlow's spectrogram.cc,
 * mfcc_mel_filterbank.cc, mfcc_dct.cc and mfcc.cc; tables are built on the host in double and rounded once to float, the device works in
 * fp32 with unfused multiplies and adds:
 *   window    periodic Hann, w[i] = 0.5 - 0.5 cos(2 pi i / window); the frame is zero padded to fft_size = next_power_of_two(window);
 *             bins = fft_size / 2 + 1; power[k] = re^2 + im^2.  Frame f covers samples [f * stride, f * stride + window); trailing
 *             samples that do not fill a window are ignored.  int16 input is x / 32768 exactly.
 *   mel       mel(f) = 1127 ln(1 + f / 700); centre[i] = mel(lower) + (i + 1) * (mel(upper) - mel(lower)) / (channels + 1), i <= channels;
 *             hz_per_bin = 0.5 * sample_rate / (bins - 1); start = int(1.5 + lower / hz_per_bin), end = int(upper / hz_per_bin); bins
 *             outside [start, end] contribute nothing.  Bin i inside: band b = index of the last centre below mel(i * hz_per_bin) or -1;
 *             weight = (centre[b+1] - mel) / (centre[b+1] - centre[b]), for b == -1 (centre[0] - mel) / (centre[0] - mel(lower)); it adds
 *             sqrt(power[i]) * weight to channel b if b >= 0 and sqrt(power[i]) * (1 - weight) to channel b + 1 if b + 1 < channels.
 *             Every channel is summed in ascending bin order.
 *   log, DCT  lg[j] = ln(max(mel_out[j], 1e-12)); feat[k] = sum_j sqrt(2 / channels) * cos(k * pi / channels * (j + 0.5)) * lg[j],
 *             k < num_features, summed in ascending j.
 *   average   output o = the mean of power[o * w .. min((o + 1) * w, bins)), w = average_window_width: SAME pooling pads on the right only
 *             and divides by the number of real bins.
 * ---------------------------------------------------------------------------------------------- */
#define MKWS_SPECTRAL_MFCC 0
#define MKWS_SPECTRAL_AVERAGE 1
typedef struct mkws_spectral_cfg {
  int32_t sample_rate;            /* 16000 */
  int32_t window_size_samples;    /* 480  (model_settings["window_size_samples"]) */
  int32_t window_stride_samples;  /* 320  (model_settings["window_stride_samples"]) */
  int32_t mode;                   /* MKWS_SPECTRAL_MFCC */
  int32_t num_features;           /* 40   mfcc: dct_coefficient_count (model_settings["fingerprint_width"]);
                                          average: ceil(bins / average_window_width), checked */
  int32_t filterbank_channels;    /* 40   (audio_ops.mfcc default); mfcc mode only */
  float lower_frequency_limit;    /* 20 */
  float upper_frequency_limit;    /* 4000 */
  int32_t average_window_width;   /* 1    average mode only (model_settings["average_window_width"]) */
} mkws_spectral_cfg;

typedef struct mkws_spectral mkws_spectral;

/* Fills *cfg with the defaults above. */
void mkws_spectral_default_cfg(mkws_spectral_cfg* cfg);

/* Host only.  Supported: fft_size in {256, 512, 1024} (windows of 129 .. 1024 samples; MKWS_ERR_UNSUPPORTED otherwise), a stride of at
 * least one sample; mfcc mode: 1 <= num_features <= filterbank_channels <= 64 (more than 64 channels: MKWS_ERR_UNSUPPORTED), 0 <= lower <
 * upper <= sample_rate / 2; average mode: average_window_width >= 1 and num_features == ceil(bins / average_window_width).  Everything
 * else is MKWS_ERR_INVALID_ARG; the message names the field.  Any of the three outputs may be NULL; width = num_features. */
int mkws_spectral_geometry(const mkws_spectral_cfg* cfg, int* fft_size, int* bins, int* width);

/* Host only: n_samples < window ? 0 : 1 + (n_samples - window) / stride. */
int mkws_spectral_num_frames(const mkws_spectral_cfg* cfg, int n_samples);

/* Host only: copies table `which` into dst (at most cap_bytes) and returns its size in bytes, or a negative mkws_status.  The mel
 * weights, the band mapper and the DCT exist in mfcc mode only (MKWS_ERR_INVALID_ARG in average mode). */
enum {
  MKWS_ST_WINDOW = 0,       /* float32[window] */
  MKWS_ST_MEL_WEIGHTS = 1,  /* float32[bins], 0 outside [start, end] */
  MKWS_ST_BAND_MAPPER = 2,  /* int32[bins], -2 outside [start, end] */
  MKWS_ST_DCT = 3,          /* float32[num_features * channels] */
  MKWS_ST_SCALARS = 4       /* int32[8]: window, stride, fft_size, bins, width, channels (0 in average mode), start, end */
};
int mkws_spectral_host_table(const mkws_spectral_cfg* cfg, int which, void* dst, size_t cap_bytes);

/* Builds the tables, uploads them once and allocates the streaming form's workspace (the frames of max_samples).  The refusals of
 * mkws_spectral_geometry come first, then MKWS_ERR_NO_DEVICE without a gfx950 device. */
int mkws_spectral_create(const mkws_spectral_cfg* cfg, int max_samples, mkws_spectral** out);
void mkws_spectral_destroy(mkws_spectral* h);

/* d_audio [B, n_samples], float32 or int16 PCM -> d_feat float32 [B, frames, width].  Two optional taps, either may be NULL and then
 * costs nothing: d_power float32 [B, frames, bins], the squared-magnitude spectrogram (what audio_spectrogram returns), and, in mfcc mode
 * only (MKWS_ERR_INVALID_ARG in average mode), d_mel float32 [B, frames, channels], the filterbank outputs before the log.  d_feat has
 * the same bits with and without taps, a clip's rows do not depend on the batch it is in, and rows of any alignment are taken.
 * MKWS_ERR_INVALID_ARG for NULL required pointers, negative sizes and n_samples > max_samples; B == 0 or zero frames returns MKWS_OK
 * with nothing launched.  One launch, asynchronous on `stream`, allocates nothing, never synchronises: capturable. */
int mkws_spectral_forward_f32(mkws_spectral* h, const float* d_audio, int B, int n_samples, float* d_feat, float* d_power, float* d_mel,
                              void* stream);
int mkws_spectral_forward_i16(mkws_spectral* h, const int16_t* d_audio, int B, int n_samples, float* d_feat, float* d_power, float* d_mel,
                              void* stream);

/* Streaming form: one recording d_audio [n_samples], windows of window_samples every hop_samples.  Frames carry no recurrence in these
 * modes, so window w is exactly frames [w * hop_samples / stride, + frames_per_window) of the recording: every frame is computed once
 * and d_feat [num_windows, frames_per_window, width] is materialised from them, row w bit-equal to the forward call on the cut window.
 * hop_samples must be a positive multiple of the stride (MKWS_ERR_UNSUPPORTED otherwise).  Returns num_windows = n_samples <
 * window_samples ? 0 : 1 + (n_samples - window_samples) / hop_samples (nothing launched when 0, or when the window holds no frame) or a
 * negative mkws_status; MKWS_ERR_INVALID_ARG for num_windows > max_windows, n_samples > max_samples, NULL pointers and non-positive
 * sizes.  Two launches, asynchronous on `stream`, allocates nothing, never synchronises: capturable. */
int mkws_spectral_stream_f32(mkws_spectral* h, const float* d_audio, int n_samples, int window_samples, int hop_samples, float* d_feat,
                             int max_windows, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sample-rate conversion in front of the frontend: a rational-ratio polyphase FIR resampler.  The reference converts its 48 kHz
 * sources outside Python (`sox ... convert(samplerate=16000)`, luganda/luganda.py:145, notebooks/clean_msc_gsc.py:71); here it is a
 * device stage with a stated filter.  With g = gcd(rate_in, rate_out): L = rate_out / g, M = rate_in / g, big = max(L, M),
 * half = zero_crossings * big, fc = rolloff / big.  The prototype, in double for i = -half .. half, is
 *   h[i + half] = L * fc * sinc(fc * i) * kaiser(2 * half + 1, kaiser_beta)[i + half]      (sinc(x) = sin(pi x) / (pi x)),
 * T = ceil((2 * half + 1) / L) taps per phase, and the table is tab[j * L + p] = (float) h[p + j * L], zero where p + j * L > 2 * half.
 * Output sample n, with m = n * M + off, q = m div L, p = m mod L (64-bit):
 *   y[n] = sum_{j = 0 .. T-1} tab[j * L + p] * x[q - j],     x outside [0, n_in) = 0,
 * accumulated from +0.0f with one float32 multiply and one float32 add per tap, j ascending, never fused: a numpy loop over float32
 * reproduces every bit.  off = half is the time-aligned (centred) output, off = 0 the causal one = the centred one delayed by
 * half / (L * rate_in) seconds = zero_crossings / min(rate_in, rate_out) (2 ms at the defaults down to 16 kHz).  n_in samples give
 * ceil(n_in * L / M) output samples.  int16 input is (float) s / 32768.0f.
 * ---------------------------------------------------------------------------------------------- */
#define MKWS_RESAMPLE_MAX_TABLE_FLOATS (1 << 22)

typedef struct mkws_resample_cfg {
  int32_t rate_in;
  int32_t rate_out;        /* 16000 */
  int32_t zero_crossings;  /* 32 */
  float kaiser_beta;       /* 9.0 */
  float rolloff;           /* 0.95 */
} mkws_resample_cfg;

typedef struct mkws_resample mkws_resample;

/* The defaults above for the given pair of rates. */
void mkws_resample_default_cfg(mkws_resample_cfg* cfg, int rate_in, int rate_out);

/* Host only (no GPU needed).  geometry: out = {L, M, T, half}.  host_taps: the table tab[j * L + p] as specified above (the device
 * keeps its own arrangement of the same values); returns T * L, and writes nothing when dst is NULL or cap_floats is too small.
 * out_samples: ceil(n_in * L / M).  MKWS_ERR_INVALID_ARG for NULL pointers, rates < 1, zero_crossings < 1, a rolloff outside (0, 1], a
 * negative or non-finite kaiser_beta and n_in < 0; MKWS_ERR_UNSUPPORTED when T * L exceeds MKWS_RESAMPLE_MAX_TABLE_FLOATS.  Equal rates
 * are legal (L = M = 1: a low-pass at rolloff * Nyquist). */
int mkws_resample_geometry(const mkws_resample_cfg* cfg, int32_t out[4]);
int mkws_resample_host_taps(const mkws_resample_cfg* cfg, float* dst, size_t cap_floats);
int64_t mkws_resample_out_samples(const mkws_resample_cfg* cfg, int64_t n_in);

/* The device handle: the table, uploaded once.  Refusals as mkws_resample_geometry, and MKWS_ERR_UNSUPPORTED for a ratio M / L so large
 * that one workgroup's input span does not fit its LDS. */
int mkws_resample_create(const mkws_resample_cfg* cfg, mkws_resample** out);
void mkws_resample_destroy(mkws_resample* rs);

/* Stateless batch form: B rows of n_in samples (float32, or int16 with in_i16 != 0), row b at d_in + b * in_stride elements ->
 * row b of d_out at d_out + b * out_stride, mkws_resample_out_samples(n_in) samples each; centred != 0 selects off = half, else off = 0.
 * MKWS_ERR_INVALID_ARG for NULL pointers, negative sizes and strides shorter than the rows; B == 0 and n_in == 0 return MKWS_OK with
 * nothing launched.  One launch, asynchronous on `stream`, allocates nothing, never synchronises: capturable. */
int mkws_resample_forward(mkws_resample* rs, const void* d_in, int in_i16, int B, int64_t n_in, int64_t in_stride, int centred,
                          float* d_out, int64_t out_stride, void* stream);

/* Live form: the causal output fed push by push, written where mkws_frontend_live_push_many_f32 reads its d_audio.  A push takes
 * exactly mkws_resample_live_in_samples(out_samples) = out_samples * M / L NEW input samples per active stream (MKWS_ERR_UNSUPPORTED
 * if that is not a whole number) and writes exactly out_samples output samples into that stream's row of d_out
 * [n_streams, out_samples]; d_in is [n_streams, in_samples].  Because in_samples * L = out_samples * M every push starts on phase 0.
 * Stream s's state block is d_states + s * state_stride_bytes (a multiple of 8, at least mkws_resample_live_state_bytes();
 * MKWS_ERR_INVALID_ARG otherwise), caller-owned: the int64 count of input samples pushed, then the last T - 1 input samples as float32,
 * oldest first.  A zero-filled block is a fresh stream (reset = memset, snapshot / restore = copies, a slice of the many-stream tensor
 * is a one-stream block).  A stream with d_active[s] == 0 (int32 [n_streams]; NULL = all active) is not advanced: its state slice and
 * its output row are untouched and its input row is not read.
 * The pushes of a stream, concatenated, are the first pushes * out_samples samples of mkws_resample_forward(centred = 0) over that
 * stream's whole input, bit for bit -- whatever the chunking, whatever the other streams do, and whether the input arrived as int16 or
 * as the same values in float32.  n_streams == 0 and out_samples == 0 return MKWS_OK with nothing launched.  One launch for any
 * n_streams (one workgroup per stream: it reads the old history before it writes the new one), asynchronous on `stream`, allocates
 * nothing, never synchronises: capturable (a replayed graph advances the streams: the state is device memory). */
int mkws_resample_live_in_samples(const mkws_resample* rs, int out_samples);
size_t mkws_resample_live_state_bytes(const mkws_resample* rs);
int mkws_resample_live_push_many(mkws_resample* rs, void* d_states, size_t state_stride_bytes, int n_streams, const int32_t* d_active,
                                 const void* d_in, int in_i16, int out_samples, float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Loudness and true peak: level normalisation of device audio.  The reference leaves it to `ffmpeg -af loudnorm=I=-16:TP=-1.5:LRA=11`
 * (notebooks/dataperf_validation_filter.py:23-40), to pydub.effects.normalize (label_directory_dataperf.py:56-61) and to `sox ... stat`
 * (notebooks/dataperf_experiments.py:468-477).  What is built is the MEASUREMENT of ITU-R BS.1770-4 and the linear gain that loudnorm's
 * two-pass linear mode applies -- not loudnorm's single-pass dynamic compressor, which has no specification.
 * A row is mono audio at `rate` Hz, float32 or int16 ((float) s / 32768.0f), of len = d_lengths[b] clamped to [0, n] samples (n when
 * d_lengths is NULL); nothing beyond len is read.
 *   K-weighting   two biquads by the bilinear form of libebur128 (at 48 kHz: the table of BS.1770), each row from zero state, in double:
 *                 shelf f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; high-pass f0 = 38.13547087602444,
 *                 Q = 0.5003270373238773 (the formulas: DESIGN.md section 40; the numbers: mkws_loudness_coeffs).
 *   blocks        hop = rate / 10, block = 4 hop; block j = filtered samples [j hop, j hop + block), j = 0 .. floor((len - block) / hop);
 *                 z_j = its mean square, l_j = -0.691 + 10 log10(z_j).
 *   gates         absolute: l_j > -70; relative: also l_j > -0.691 + 10 log10(mean z over the absolute set) - 10;
 *                 L = -0.691 + 10 log10(mean z over the relative set), -inf when no block passes the absolute gate.
 *   true peak     max |y| over the 4 len samples of the row through mkws_resample's filter with L = 4, M = 1, centred, zeros outside the
 *                 row (the float32 taps and samples, every product and sum in double, j ascending), with this cfg's zero_crossings,
 *                 kaiser_beta and rolloff.  The sample peak max |x| and the mean square of the unweighted row ride on the same pass.
 *   gain          loudness mode: g_dB = target_lufs - L; if 20 log10(true_peak) + g_dB > true_peak_db then g_dB = true_peak_db -
 *                 20 log10(true_peak) (flag PEAK_LIMITED); gain = (float) 10^(g_dB / 20), in double.  L = -inf (silence, a row shorter
 *                 than a block): gain = 1, flag UNMEASURED.  Peak mode (pydub's rule): gain = (float)(10^(-headroom_db / 20) /
 *                 sample_peak); an all-zero row: gain = 1, flag UNMEASURED.  Both modes measure everything; the mode selects the rule.
 * ---------------------------------------------------------------------------------------------- */
#define MKWS_LOUDNESS_MAX_WORKSPACE_BYTES ((int64_t)1 << 32)
#define MKWS_LOUDNESS_MAX_ZERO_CROSSINGS 2048

enum { MKWS_LOUDNESS_MODE_LOUDNESS = 0, MKWS_LOUDNESS_MODE_PEAK = 1 };
enum { MKWS_LOUDNESS_FLAG_UNMEASURED = 1, MKWS_LOUDNESS_FLAG_PEAK_LIMITED = 2 };

typedef struct mkws_loudness_cfg {
  int32_t rate;            /* 16000 */
  int32_t mode;            /* MKWS_LOUDNESS_MODE_LOUDNESS */
  double target_lufs;      /* -16.0 */
  double true_peak_db;     /* -1.5 */
  double headroom_db;      /* 0.1 (peak mode; pydub's default) */
  int32_t zero_crossings;  /* 32 */
  float kaiser_beta;       /* 9.0 */
  float rolloff;           /* 0.95 */
} mkws_loudness_cfg;

typedef struct mkws_loudness mkws_loudness;

/* The defaults above at the given rate. */
void mkws_loudness_default_cfg(mkws_loudness_cfg* cfg, int rate);

/* Host only (no GPU needed).  coeffs: out = shelf {b0, b1, b2, a1, a2}, high-pass {b0, b1, b2, a1, a2}.  geometry: out = {hop, block,
 * chunk, tile}: the kernels cut a row into chunks of `chunk` samples (the largest divisor of the hop that is at most 32) and give a
 * workgroup `tile` = 256 chunks.  MKWS_ERR_INVALID_ARG for NULL pointers, rate < 1, an unknown mode, a non-finite target_lufs,
 * true_peak_db or headroom_db, zero_crossings < 1, a rolloff outside (0, 1] and a negative or non-finite kaiser_beta;
 * MKWS_ERR_UNSUPPORTED for a rate that is not a multiple of 10, a rate at or below twice the shelf frequency, and zero_crossings above
 * MKWS_LOUDNESS_MAX_ZERO_CROSSINGS. */
int mkws_loudness_coeffs(const mkws_loudness_cfg* cfg, double out[10]);
int mkws_loudness_geometry(const mkws_loudness_cfg* cfg, int32_t out[4]);

/* The device handle: the tables and a workspace for up to max_rows rows of up to max_samples samples.  Refusals, all before a device is
 * looked for: those above, MKWS_ERR_INVALID_ARG for max_rows < 1 or max_samples < 1, MKWS_ERR_UNSUPPORTED for a workspace above
 * MKWS_LOUDNESS_MAX_WORKSPACE_BYTES (about 1.3 bytes per sample of max_rows * max_samples at a chunk of 32). */
int mkws_loudness_create(const mkws_loudness_cfg* cfg, int max_rows, int64_t max_samples, mkws_loudness** out);
void mkws_loudness_destroy(mkws_loudness* h);

/* measure: B rows of n samples, row b at d_in + b * in_stride elements; d_lengths int64 [B] or NULL.  Writes, per row, d_stats
 * float64 [B, 4] = {L, true_peak, sample_peak, mean_square} (linear peaks; mean_square = 0 for len = 0), d_counts int32 [B, 4] =
 * {blocks, blocks past the absolute gate, blocks past both gates, flags} and d_gain float32 [B].  Five launches (one for n == 0).
 * apply: d_out row b at d_out + b * out_stride = (float) x * d_gain[b] (one rounding) for the first len samples and 0.0f up to n;
 * d_gain is read on the device.  d_out may be d_in itself (float32, equal strides); any other overlap is undefined.
 * MKWS_ERR_INVALID_ARG for NULL pointers, negative sizes, B > max_rows, n > max_samples and strides shorter than the rows; B == 0
 * returns MKWS_OK with nothing launched.  Every sum and maximum across lanes is taken in a fixed order without atomics: the same call
 * gives the same bits, and a row's results do not depend on the other rows.  Asynchronous on `stream`, allocates nothing, never
 * synchronises: capturable. */
int mkws_loudness_measure(mkws_loudness* h, const void* d_in, int in_i16, int B, int64_t n, int64_t in_stride, const int64_t* d_lengths,
                          double* d_stats, int32_t* d_counts, float* d_gain, void* stream);
int mkws_loudness_apply(mkws_loudness* h, const void* d_in, int in_i16, int B, int64_t n, int64_t in_stride, const int64_t* d_lengths,
                        const float* d_gain, float* d_out, int64_t out_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * WAV sample data decoded on the device: the bytes of a file's `data` chunk, in any common format and channel layout, become float32
 * audio in one launch for a whole batch of files.  The reference leaves formats and channels to `sox` / `soxi` (run.py:259-268,
 * luganda/luganda.py:145, word_extraction.py:223-231).  A FRAME is `channels` consecutive little-endian samples; a sample of b bytes
 * becomes a float32 by exactly this rule (s = the sign-extended little-endian integer, b0 = the single byte):
 *   MKWS_PCM_U8     1 byte    (float)((int)b0 - 128) / 128.0f
 *   MKWS_PCM_S16    2 bytes   (float)s / 32768.0f                    (what decode_wav and the resampler's int16 input do)
 *   MKWS_PCM_S24    3 bytes   (float)s / 8388608.0f                  (exact)
 *   MKWS_PCM_S32    4 bytes   (float)s, round to nearest even, times 2^-31   (so 2^31 - 1 gives 1.0f)
 *   MKWS_PCM_F32    4 bytes   the stored bits
 *   MKWS_PCM_F64    8 bytes   (float)d, round to nearest even (a result below the smallest normal float is not pinned)
 *   MKWS_PCM_MULAW  1 byte    u = ~b0 & 0xFF; t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7); s = (u & 0x80) ? 0x84 - t : t - 0x84;
 *                             (float)s / 32768.0f                    (G.711 mu-law: +-32124)
 *   MKWS_PCM_ALAW   1 byte    a = b0 ^ 0x55; t = (a & 0x0F) << 4; seg = (a & 0x70) >> 4; seg 0: t += 8; seg 1: t += 0x108;
 *                             else t = (t + 0x108) << (seg - 1); s = (a & 0x80) ? t : -t; (float)s / 32768.0f   (G.711 A-law: +-32256)
 * Channel c >= 0 of a frame is that sample's value.  Channel -1 (MKWS_PCM_MIX) starts from +0.0f, adds the channels' values in channel
 * order with one float32 add each and divides once by (float)channels: a sequential numpy float32 loop reproduces every bit.
 * ---------------------------------------------------------------------------------------------- */
enum {
  MKWS_PCM_U8 = 0,
  MKWS_PCM_S16 = 1,
  MKWS_PCM_S24 = 2,
  MKWS_PCM_S32 = 3,
  MKWS_PCM_F32 = 4,
  MKWS_PCM_F64 = 5,
  MKWS_PCM_MULAW = 6,
  MKWS_PCM_ALAW = 7,
  MKWS_PCM_NUM_FORMATS = 8
};
#define MKWS_PCM_MIX (-1)

/* One work item: n_frames frames that start at byte byte_offset of the byte buffer (any byte: no alignment is assumed) become out_len
 * floats at d_out + out_offset.  48 bytes; a table of them is 8-byte aligned. */
typedef struct mkws_pcm_item {
  int64_t byte_offset;
  int64_t n_frames;
  int64_t out_offset;   /* in floats */
  int64_t out_len;
  int32_t format;       /* MKWS_PCM_* */
  int32_t channels;
  int32_t channel;      /* 0 .. channels - 1, or MKWS_PCM_MIX */
  int32_t reserved;     /* 0 */
} mkws_pcm_item;

/* Host only (no GPU needed): bytes of one frame = bytes of a sample * channels.  MKWS_ERR_INVALID_ARG for an unknown format, channels < 1
 * and a product above INT32_MAX. */
int mkws_pcm_frame_bytes(int format, int channels);

/* d_bytes uint8 [n_bytes], d_items [n_items] (device memory, like the route tables), d_out float32 [out_floats], d_invalid int32 [1].
 * For item k and i in [0, out_len): d_out[out_offset + i] = the value of frame i if i < n_frames, else +0.0f -- the launch writes the
 * zero padding itself, and out_len < n_frames truncates.  The kernel checks every item before it reads or writes for it, in 64-bit:
 * format in [0, MKWS_PCM_NUM_FORMATS), channels >= 1, -1 <= channel < channels, n_frames >= 0, 0 <= out_len <= max_out_len,
 * 0 <= byte_offset <= n_bytes with all n_frames frames inside [byte_offset, n_bytes), and [out_offset, out_offset + out_len) inside
 * [0, out_floats).  An item that fails writes nothing and adds 1 to *d_invalid (set to 0 by every call that launches); the other items
 * are unaffected.  No byte outside [0, n_bytes) is read and no float outside an item's own range is written; the ranges of two items
 * should not overlap (the order of their stores is then undefined).  MKWS_ERR_INVALID_ARG for negative sizes and NULL buffers,
 * MKWS_ERR_UNSUPPORTED for a grid of n_items * ceil(max_out_len / 1024) workgroups beyond one launch; n_items == 0 or max_out_len == 0
 * returns MKWS_OK with nothing launched (and *d_invalid untouched).  One launch for any n_items, asynchronous on `stream`, allocates
 * nothing, never synchronises: capturable. */
int mkws_pcm_decode(const uint8_t* d_bytes, int64_t n_bytes, const mkws_pcm_item* d_items, int n_items, int64_t max_out_len, float* d_out,
                    int64_t out_floats, int32_t* d_invalid, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device audio encoded into WAV sample data: the inverse of the decode above.  Windows of float32 recordings in device memory become
 * the bytes of MONO sample data in any of the MKWS_PCM_* formats, cut, faded and scaled on the way, in one launch for a whole batch of
 * files.  The reference leaves all of it to `sox` (`trim`, `fade`, `pad`, `convert`: embedding/word_extraction.py:223-231,
 * luganda/luganda.ipynb cell 21, notebooks/sox_batch.py).
 *
 * One work item: its recording is d_src[src_offset .. src_offset + src_len) of a flat float32 buffer.  For i in [0, n_frames)
 *   x = d_src[src_offset + start + i]  if 0 <= start + i < src_len,  else +0.0f      (zero padding on either side needs no buffer)
 *   f = f_in * f_out,  f_in  = (float)i / (float)fade_in                    if i < fade_in,              else 1.0f
 *                      f_out = (float)(n_frames - 1 - i) / (float)fade_out  if i >= n_frames - fade_out, else 1.0f
 *   v = (x * gain) * f                                  (every product and quotient one float32 operation, round to nearest even)
 * and the sample of v goes to bytes [byte_offset + i * b, byte_offset + (i + 1) * b) of the byte buffer, little-endian, b = the
 * sample's size.  With gain == 1.0f and no fade a finite x passes through bit for bit.  rint rounds half-way cases to even:
 *   MKWS_PCM_U8     rint(v * 128.0f) + 128 clamped to [0, 255]
 *   MKWS_PCM_S16    q = rint(v * 32768.0f) clamped to [-32768, 32767]
 *   MKWS_PCM_S24    rint(v * 8388608.0f) clamped to [-8388608, 8388607]
 *   MKWS_PCM_S32    t = v * 2147483648.0f;  t >= 2^31: 2^31 - 1;  t <= -2^31: -2^31;  else rint(t)
 *   MKWS_PCM_F32    the bits of v
 *   MKWS_PCM_F64    (double)v
 *   MKWS_PCM_MULAW  m = q >> 2; mask = 0xFF; m < 0: m = -m, mask = 0x7F; m = min(m, 8159) + 33; seg = the first of the segment ends
 *                   0x3F, 0x7F, ..., 0x1FFF that m does not exceed; code = (seg << 4) | ((m >> (seg + 1)) & 15), or 0x7F when m exceeds
 *                   them all (the clipped magnitude 8192 does); the byte is code ^ mask
 *   MKWS_PCM_ALAW   m = q >> 3; mask = 0xD5; m < 0: m = -m - 1, mask = 0x55; seg = the first of the ends 0x1F, 0x3F, ..., 0xFFF that m
 *                   does not exceed; code = (seg << 4) | ((seg < 2 ? m >> 1 : m >> seg) & 15); the byte is code ^ mask
 * A NaN v gives the code of zero in the integer and G.711 formats (u8: 128, mu-law: 0xFF, A-law: 0xD5).  The G.711 rules are the usual
 * closed-form compressors (CPython's audioop.lin2ulaw / lin2alaw give the same byte for all 65 536 inputs), NOT the nearest decoded
 * value; they invert the decode rule above on every code but mu-law 0x7F (negative zero, re-encoded as 0xFF).
 * ---------------------------------------------------------------------------------------------- */

/* 64 bytes; a table of them is 8-byte aligned. */
typedef struct mkws_pcm_encode_item {
  int64_t src_offset;   /* in floats */
  int64_t src_len;
  int64_t start;        /* frame 0 of the item is sample `start` of its recording; may be negative or past the end */
  int64_t n_frames;
  int64_t byte_offset;  /* any byte: no alignment is assumed */
  int64_t fade_in;      /* frames, >= 0 */
  int64_t fade_out;
  float gain;
  int32_t format;       /* MKWS_PCM_* */
} mkws_pcm_encode_item;

/* d_src float32 [src_floats], d_items [n_items] (device memory), d_out uint8 [out_bytes], d_invalid int32 [1].  The kernel checks every
 * item before it reads or writes for it, in 64-bit: format in [0, MKWS_PCM_NUM_FORMATS), 0 <= n_frames <= max_frames, fade_in >= 0,
 * fade_out >= 0, src_len >= 0, -2^61 <= start <= 2^61, [src_offset, src_offset + src_len) inside [0, src_floats) and
 * [byte_offset, byte_offset + n_frames * b) inside [0, out_bytes).  An item that fails writes nothing and adds 1 to *d_invalid (set to
 * 0 by every call that launches); the other items are unaffected.  No float outside an item's [src_offset, src_offset + src_len) is
 * read and NO BYTE OUTSIDE AN ITEM'S OWN BYTE RANGE IS WRITTEN: items of 1-byte and 3-byte samples may start and end at any address and
 * may abut (the ranges of two items should not overlap: the order of their stores is then undefined).  MKWS_ERR_INVALID_ARG for
 * negative sizes and NULL buffers, MKWS_ERR_UNSUPPORTED for a grid of n_items * ceil(max_frames / 1024) workgroups beyond one launch;
 * n_items == 0 or max_frames == 0 returns MKWS_OK with nothing launched (and *d_invalid untouched).  One launch for any n_items,
 * asynchronous on `stream`, allocates nothing, never synchronises: capturable. */
int mkws_pcm_encode(const float* d_src, int64_t src_floats, const mkws_pcm_encode_item* d_items, int n_items, int64_t max_frames,
                    uint8_t* d_out, int64_t out_bytes, int32_t* d_invalid, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Test streams assembled on the device: pieces of float32 recordings in device memory are laid out on the time lines of R streams,
 * faded, scaled, summed where they overlap, put over a looped background bed and clipped, in one launch for all R streams.  The
 * reference strings its streaming tests together with one sox process per piece and one for the join
 * (embedding/generate_stream_sentences.py:144-245, luganda/luganda.py:164-217); it has no background and no overlap.
 *
 * A stream r is d_out[out_offset .. out_offset + n_out).  Its items are d_items[first_item .. first_item + n_items), in ascending
 * out_start.  The value at position t of stream r, for t in [0, n_out):
 *   item k COVERS t iff 0 <= i < n_frames with i = t - out_start; its value there is
 *     v_k = (x * gain) * (f_in * f_out)      x, f_in and f_out exactly as in mkws_pcm_encode above (x = +0.0f outside the recording;
 *                                            every product and quotient one float32 operation, round to nearest even)
 *   foreground s: the first covering item in table order sets s = v_k (no add to a zero: a lone item at gain 1.0f passes every bit
 *     through, -0.0f and a quiet NaN included); every further covering item does s = s + v_k, one float32 add each, in ascending item
 *     index; a position that no item covers has s = +0.0f
 *   bed (bed_len > 0 and d_bed_gain given): b = d_src[bed_offset + ((bed_start + t) mod bed_len)], y = s + b * d_bed_gain[r] (a
 *     multiply, then an add); without a bed y = s
 *   with MKWS_STREAM_CLIP in `flags`: y > 1.0f gives 1.0f, y < -1.0f gives -1.0f, anything else (a NaN too) stays
 * and d_out[out_offset + t] = y.  A sequential numpy float32 loop reproduces every bit (compose.mix_host).
 * ---------------------------------------------------------------------------------------------- */
#define MKWS_STREAM_CLIP 1

/* 64 bytes; a table of them is 8-byte aligned. */
typedef struct mkws_stream_item {
  int64_t src_offset;   /* the piece's recording: d_src[src_offset .. src_offset + src_len) of one flat float32 buffer */
  int64_t src_len;
  int64_t start;        /* frame 0 of the item is sample `start` of its recording; may leave it on either side (+0.0f there) */
  int64_t n_frames;
  int64_t out_start;    /* stream position of frame 0; may be negative or past the stream's end (the item is clipped to the stream) */
  int64_t fade_in;      /* frames, >= 0, linear: mkws_pcm_encode's f_in / f_out */
  int64_t fade_out;
  float gain;
  int32_t stream;       /* index of the stream descriptor it belongs to */
} mkws_stream_item;

/* 56 bytes; a table of them is 8-byte aligned. */
typedef struct mkws_stream_desc {
  int64_t out_offset;   /* in floats */
  int64_t n_out;
  int64_t bed_offset;   /* the background bed: d_src[bed_offset .. bed_offset + bed_len); bed_len == 0: no bed */
  int64_t bed_len;
  int64_t bed_start;    /* in [0, bed_len) when bed_len > 0 */
  int64_t max_frames;   /* >= n_frames of every item of the stream: bounds the search for the items that reach a tile */
  int32_t first_item;
  int32_t n_items;
} mkws_stream_desc;

/* d_src float32 [src_floats], d_items [n_items], d_streams [n_streams] (device memory), d_bed_gain float32 [n_streams] or NULL (every
 * stream then goes without its bed), d_out float32 [out_floats], d_invalid int32 [1]; max_out >= every n_out sizes the grid of
 * n_streams * ceil(max_out / 1024) workgroups.  The kernel checks, in 64-bit, before anything is read or written for the thing
 * checked.  An item: `stream` in [0, n_streams) and its own index inside that stream's [first_item, first_item + n_items);
 * 0 <= n_frames <= the stream's max_frames; fade_in, fade_out, src_len >= 0; |start| <= 2^61 and |out_start| <= 2^61;
 * [src_offset, src_offset + src_len) inside [0, src_floats).  A stream: 0 <= n_out <= max_out; [out_offset, out_offset + n_out) inside
 * [0, out_floats); first_item, n_items >= 0 with first_item + n_items <= the table's n_items; bed_len >= 0, and when bed_len > 0 the bed
 * inside [0, src_floats) and 0 <= bed_start < bed_len.  An invalid item contributes nothing; an invalid stream is not written at all;
 * *d_invalid (set to 0 by every call that launches) ends as the number of invalid items plus invalid streams.  No float outside a
 * valid item's recording or a valid stream's bed is read and NO FLOAT OUTSIDE A VALID STREAM'S OWN RANGE IS WRITTEN; every float of
 * that range is written once (streams may abut; their ranges should not overlap).  Ascending out_start inside a stream is a
 * PRECONDITION that the kernel does not check: the values of an unordered stream are unspecified, the guarantees on what is read and
 * written hold all the same.  MKWS_ERR_INVALID_ARG for negative sizes and NULL buffers, MKWS_ERR_UNSUPPORTED for a grid beyond one
 * launch; n_streams == 0 or max_out == 0 returns MKWS_OK with nothing launched (and *d_invalid untouched).  Asynchronous on `stream`,
 * allocates nothing, never synchronises: capturable. */
int mkws_stream_mix(const float* d_src, int64_t src_floats, const mkws_stream_item* d_items, int n_items, const mkws_stream_desc* d_streams,
                    int n_streams, const float* d_bed_gain, int flags, int64_t max_out, float* d_out, int64_t out_floats, int32_t* d_invalid,
                    void* stream);

/* The powers a signal-to-noise ratio needs, from the same tables with the same checks (out_offset only has to be >= 0: nothing is
 * written there).  d_partials float64 [n_streams * ceil(max_out / 1024) * 2]: slot (r * tiles + tile) holds the sum of (double)s *
 * (double)s and the sum of (double)b * (double)b -- the foreground as defined above and the RAW bed -- over the tile's positions
 * below n_out; a tile past n_out, an invalid stream and a stream without a bed (second sum) get +0.0.  One workgroup owns one slot:
 * no atomics, and the order of the adds inside a tile depends on nothing but the tile, so a replay gives the same bits. */
int mkws_stream_power(const float* d_src, int64_t src_floats, const mkws_stream_item* d_items, int n_items, const mkws_stream_desc* d_streams,
                      int n_streams, int64_t max_out, double* d_partials, int32_t* d_invalid, void* stream);

/* One workgroup per stream folds its slots in ascending tile order into P_fg and P_bed and writes
 * d_bed_gain[r] = (float)(sqrt(P_fg / P_bed) * d_snr_scale[r]), or 0.0f where either power is not above zero or bed_len <= 0: with
 * d_snr_scale[r] = 10^(-snr_db / 20) (computed by the host) the mixed stream has 10 log10(sum s^2 / sum (g b)^2) = snr_db over its n_out
 * positions.  Reads nothing but the partials, the descriptors' bed_len and the scales.  Same errors and no-ops as above. */
int mkws_stream_bed_gain(const double* d_partials, const mkws_stream_desc* d_streams, int n_streams, int64_t max_out, const double* d_snr_scale,
                         float* d_bed_gain, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Embedding model.  Replaces `embedding.predict(x)` on the Keras model
 *   EfficientNetB0(include_top=False, weights=None, input_shape=(49,40,1)) -> GAP ->
 *   Dense 2048 relu -> Dense 2048 relu -> Dense 1024 selu ("dense_2")
 * defined at multilingual_kws/train_multilingual_embedding.py:58-83 and cut at dense_2 by
 * multilingual_kws/embedding/transfer_learning.py:36-43 / distance_filtering.py:18-27.
 * Weights arrive as one host blob of float32 tensors in Keras order/layout (HWIO conv kernels,
 * [in,out] dense kernels, BN gamma/beta/mean/var); multilingual_kws_amd/weights.py writes it.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mkws_embed mkws_embed;

/* Number of float32 values the weight blob must hold (12 967 004 params + BN statistics). */
size_t mkws_embed_weight_count(void);
/* Host-only: writes a JSON manifest (tensor name, shape, offset into the blob) into dst; returns
 * bytes needed (call with cap 0 to size). */
int mkws_embed_weight_manifest(char* dst, size_t cap_bytes);

int mkws_embed_create(const float* h_weights, size_t n_floats, int max_batch, mkws_embed** out);
void mkws_embed_destroy(mkws_embed* em);
/* d_spec float32 [B,49,40,1] (NHWC, i.e. the frontend's output) -> d_emb float32 [B,1024]. */
int mkws_embed_forward(mkws_embed* em, const float* d_spec, int B, float* d_emb, void* stream);
/* Failure contract of the paired whole-block kernel ("fuse_pair", below) and of the cluster kernel ("fuse_cluster").  Its two workgroups find each other through the
 * GPU's dispatch order (workgroups are dealt round-robin over the 8 XCDs, so linear ids b and b^8 run on one XCD, adjacent in
 * its queue).  That order is observed, probed at create and re-checked by every pair at run time, but it is NOT a documented
 * guarantee (CU masking, CPX/DPX partitions, a second process holding CUs can break it).  When a pair finds itself on two XCDs,
 * or a half waits ~0.5 s for a partner that is not resident, the launch fills its outputs with NaN and records the failure; all
 * later paired launches of the handle poison without exchanging, and the last layer of every forward that ran after the failure
 * stores NaN for EVERY embedding (NaN inside the network would not survive the ReLUs of the dense layers).  The next mkws_embed_forward / _forward_tap / _profile on the
 * handle notices (a host-mapped word, no synchronisation), switches the handle to the one-workgroup-per-4-clips kernel for
 * good ("fuse_pair" = 0, mkws_embed_get_option("pair_degraded") counts it) and returns MKWS_ERR_EXCHANGE: the earlier result is
 * invalid, the repeated call is correct.  A captured hipGraph keeps replaying the paired launch: graph users poll
 * mkws_embed_get_option(em, "exchange_error") (nonzero = a launch that already executed recorded a failure; host-mapped word, no
 * synchronisation) before a replay, and on a hit make one eager mkws_embed_forward (which heals the handle and returns
 * MKWS_ERR_EXCHANGE), repeat it, and re-capture -- multilingual_kws_amd/embedding/batch_streaming_analysis.py does exactly that --
 * or capture with "fuse_pair" = 0.  The exchange kernels assume that no OTHER kernel competes for the XCD's CUs while they spin:
 * the paired kernel tolerates concurrent launches (at most one unmatched half per launch and XCD), the cluster kernel (10-14 members)
 * does not, so handles that run concurrently (serving lanes) must not use "fuse_cluster".
 *
 * Execution options (A/B switches for measurement; results are equal up to fp32 rounding):
 *   "fuse_front" (default 1): expand 1x1 conv + depthwise conv in one kernel (expanded tensor stays in LDS);
 *                 0 = separate GEMM and depthwise kernels.
 *   "fuse_block" (default 2): blocks with 4x3 and 2x2 images (4b..7a) run expand -> depthwise -> SE -> project as
 *                 ONE kernel, 4 clips per workgroup, activations resident in LDS; 1 = only the 2x2 blocks
 *                 (6b..7a); 0 = the multi-kernel path everywhere.
 *   "fuse_chain" (default 1; needs "fuse_block" = 2; 2 / 3 = only the first / second of the two chains): the stride-1 2x2-image blocks
 *                 (6b, 6c, 6d, 7a) run as ONE paired launch (exchange 2 carries all projection tiles and both halves finish them), and
 *                 consecutive 4x3-image blocks (4b, 4c, 5a, 5b, 5c, 6a) run as ONE launch: a workgroup
 *                 keeps its clips' activations in LDS from block to block (a block's projection writes the next block's MFMA operand
 *                 fragments), the residual rides in registers, the next block's weight ring is requested during the current block's
 *                 projection.  Bit-identical to one whole-block launch per block (0).  Not used by handles that plan the cluster kernel.
 *   "fuse_top" (default 1; needs "fuse_chain" 1 or 3 and "fuse_gap"): the top conv + BN + swish + global average pool run as the LAST PHASE of
 *                 the paired chain (both halves hold block 7a's output as fragments; they split the 80 output tiles, nothing is exchanged)
 *                 instead of a launch of their own.  Bit-identical pooled features.
 *   "fuse_pair" (default 1 when the probe at create passed; needs "fuse_block"): the stride-1 2x2-image blocks (6b, 6c, 6d, 7a) run on
 *                 the PAIRED whole-block kernel: two workgroups on two CUs of one XCD share 8 clips and split the expanded channels,
 *                 so each CU streams half of the block's weights; two small in-kernel exchanges through L2.  0 = one workgroup per 4 clips.
 *                 mkws_embed_create turns it on only after a probe launch has shown that workgroups b and b^8 share an XCD on this device.
 *                 Handles with max_batch <= 512 pair 4 clips (and give the 4x3-image whole-block kernels 2 clips per workgroup) so that
 *                 every CU still gets a workgroup.
 *   "fuse_cluster" (default 1 for handles with max_batch <= 32 when the probe at create passed; settable up to 64): the tiny-image
 *                 blocks (4b..7a) run on the CLUSTER kernel: P = 10 / 14 / 12 workgroups on CUs of one XCD share one 16-row tile (one
 *                 clip of a 4x3 image, four of a 2x2 image) and split the block's expanded channels, so that a single live window no
 *                 longer waits for one CU to pull a whole block's weights (batch-1 embedding 0.44 -> 0.30 ms); two in-kernel exchanges
 *                 with generation flags (graph-replayable).  Same failure contract as the paired kernel (above).
 *   "fuse_cluster_chain" (default 1 for one-clip handles, max_batch == 1, that run "fuse_cluster"; refused on larger handles): a live window's
 *                 blocks 4b..7a run as ONE launch of the cluster kernel's body: the 120 members of all ten blocks (block k on XCD k % 8) start
 *                 together and request every weight they will need, then wait for the previous block's `done` generations; a block hands its
 *                 output on with write-through stores + one generation word per member, the next reads it with L1-bypassing loads (placement-
 *                 free); every block owns an exchange slot.  Bit-identical to one cluster launch per block (0); batch-1 embedding 0.283 ->
 *                 0.255 ms.  Taps inside the range run launch by launch.  Same failure contract; several one-clip handles may run at once
 *                 (measured up to six on six streams), but on a chip crowded by OTHER kernels members can wait for CUs until the bounded
 *                 polls give up -- then the contract above applies.
 *   "fuse_back" (default 1): blocks 2a, 2b, 3b (and 3a / 4a on handles that do not run them on the whole-block kernel: one-clip handles,
 *                 "fuse_mid" = 0) run squeeze-excite + gated projection as
 *                 ONE kernel behind the fused expand+depthwise kernel (the clip's depthwise output is staged in LDS once);
 *                 0 = se_reduce + se_expand + projection GEMM launches.
 *   "fuse_mid" (default 1): blocks with big images run expand -> depthwise -> SE ->
 *                 project as ONE kernel per block (depthwise output of all channels resident in LDS): 1 = blocks 2b, 3a and 4a
 *                 (where it measured faster than the front / back kernel pair), 2 = all of 2a..4a, 3 = 3a and 4a only, 0 = never.
 *   "fuse_gemv" (default 1): handles planned for at most 4 rows (live serving: max_batch <= 4 for the dense layers, a one-clip handle for the
 *                 top conv + pool) run those layers as matrix-vector products, ONE launch per layer (a 16-wave workgroup per 16-column tile,
 *                 K split over its waves, partial columns folded in LDS in a fixed order); 0 = the MFMA GEMM + split-K fold launches.
 *   "fuse_se4" (default 1): the 4x3-image blocks (4b..6a, whole-block and chain kernels) run their squeeze-excite FCs on the 4x4x1 matrix
 *                 instruction -- a workgroup's 4 clips are exactly its N -- and the lanes that compute a gate multiply the clip's depthwise rows
 *                 by it on the spot (no gate buffer, no gate pass); 0 = the 16x16x4 weight streams (clips = 4 of 16 columns) + a gate pass.
 *                 Another summation order inside the two FCs: results agree at fp32 round-off (1e-6 of the block outputs), bit-identical per setting.
 *   "fuse_walk" (default 1): block 2a's expand + depthwise kernel runs ONE workgroup per clip that walks the clip's three 32-channel blocks
 *                 (the input is read from HBM once); 0 = one workgroup per (clip, channel block).  Bit-identical either way.
 *   "block_tiles" (set: 0 = the rule of the handle's max_batch, 1 / 2 / 3 = one / two / four clips per workgroup; get: the value in force):
 *                 row tiles per workgroup of the 4x3-image whole-block / chain kernels (blocks 4b..6a).  The rule picks the largest that
 *                 still gives every CU a workgroup: 3 from 1 024 clips, 2 for 512, 1 for 129..256-clip handles (round 6).  Another tile shape
 *                 = another summation order inside the SE sums: results agree at fp32 round-off, bit-identical per handle.
 *   "fuse_gap" (default 1): global average pool fused into the top conv epilogue (its [B*4,1280] output is never stored).
 *   "fuse_stem" (default 1): stem conv + the whole of block 1a in one kernel (persistent workgroups, one per CU, each walking
 *                 clips blockIdx, blockIdx + grid, ... with the next clip's spectrogram prefetched; both 25x20x32 activations stay
 *                 in LDS); 0 = separate kernels.
 *   "pair_fault" / "inject_exchange_error" (test hooks): force the exchange kernels' failure paths / leave the error words as a failed
 *                 exchange of an earlier launch would (tests/test_embedding_gpu.py, tests/test_streaming.py).
 *   "big_tiles" (A/B aid, default 0): 8-clip pairs and 4-clip 4x3 workgroups whatever max_batch is (what handles above 512 clips use).
 *   "plan_batch" (default max_batch; set: a clip count >= max_batch, 0 = back to max_batch): the workgroup shapes of the tiny-image kernels
 *                 (blocks 4b..7a: clips per workgroup / per pair) are those of a handle of this many clips.  For callers that run L handles
 *                 CONCURRENTLY on L streams (serving lanes): pass the clips they hold together and each of those launches takes 1 / L of the chip
 *                 instead of one clip per CU -- four 256-clip handles on four hardware queues then serve 1.03 M clips/s where one handle serves
 *                 0.56 M (profiles/r06_notes.md section 8).  A lone call on such a handle is SLOWER (0.46 -> 0.64 ms at 256 clips): leave the
 *                 option alone on handles that run by themselves.  The caller keeps lanes x 2 x ceil(max_batch / 8) within the CU count: the paired
 *                 kernels hold their CU while they wait for their partner (failure contract below).  Results: as "block_tiles". */
int mkws_embed_set_option(mkws_embed* em, const char* name, int value);
/* Current value of an option above, of "exchange_error" (see the failure contract), or of "pair_degraded" (times the handle left the paired kernel after a failed exchange) /
 * "max_batch"; negative mkws_status for an unknown name.  ("pair_fault" is a write-only test hook that forces those failures.)
 * Guard-band mode (test aid; MKWS_EMBED_GUARD=<floats> in the environment when the handle is created): the workspace starts as a NaN canary
 * pattern and every sub-buffer carved from it is followed -- the first one also preceded -- by that many floats no kernel may touch.
 * "guard_floats" / "guard_bands" = size and number of the bands (0 = mode off); "guard_violations" = SYNCHRONISES the device and counts the
 * guard words that no longer hold the canary (an out-of-range store of any kernel of the handle). */
int mkws_embed_get_option(const mkws_embed* em, const char* name);

/* Measurement aid (NOT capturable: it records a hipEvent pair around every kernel launch and
 * synchronises the stream after each of the `reps` passes).  Writes one line per launch,
 * "<stage>\t<kernel name as rocprofv3 shows it>\t<average ms>\n", into dst; returns the bytes needed. */
int mkws_embed_profile(mkws_embed* em, const float* d_spec, int B, int reps, float* d_emb, char* dst,
                       size_t cap_bytes, void* stream);

/* Debug/parity tap: runs the forward pass up to and including `stage` ("stem", "block2a_expand",
 * "block2a_dw", "block2a_gate", "block2a", ..., "top", "gap", "dense", "dense_1", "dense_2") and copies
 * that stage's output (float32, NHWC) into d_dst; returns its element count or a negative status. */
int mkws_embed_forward_tap(mkws_embed* em, const float* d_spec, int B, const char* stage, float* d_dst,
                           size_t cap_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Few-shot head.  Replaces Dense(18,tanh) -> Dense(3,softmax) + SparseCategoricalCrossentropy +
 * Adam of multilingual_kws/embedding/transfer_learning.py:47-59 and the per-step work of
 * xfer.fit (:86-93) on the frozen embedding.
 * Parameter vector layout (float32, P = in*hid + hid + hid*cls + cls = 18 507 for 1024/18/3):
 *   W1[in,hid] | b1[hid] | W2[hid,cls] | b2[cls]     (Keras [in,out] kernels)
 * ---------------------------------------------------------------------------------------------- */
typedef struct mkws_head mkws_head;

int mkws_head_create(int in_dim, int hidden, int classes, int max_batch, mkws_head** out);
void mkws_head_destroy(mkws_head* hd);
int mkws_head_param_count(const mkws_head* hd);
/* Device pointers into the handle's own state (valid until destroy): params, grads, Adam m, Adam v.
 * Exposed so the data-parallel host code can all-reduce the flat gradient with RCCL in place.
 * The gradient buffer holds mkws_head_grad_count() = P + 2 floats: the P gradients followed by the two
 * statistics of the last mkws_head_loss_grad call {sum of per-row loss, number of correct argmax rows}, so
 * that one data-parallel step is ONE all-reduce(sum) over that range. */
float* mkws_head_params(mkws_head* hd);
float* mkws_head_grads(mkws_head* hd);
int mkws_head_grad_count(const mkws_head* hd);
/* The handle's whole optimizer state is ONE contiguous range starting at mkws_head_params(): params | grads (+ 2 statistics) | Adam m |
 * Adam v, each padded to the same length; this is the length of the range in floats (snapshot / restore around a warm-up step). */
int mkws_head_state_floats(const mkws_head* hd);
/* Uploads h_params (host) and zeroes the gradient and Adam state, ordered on `stream`; returns after the
 * stream has drained (h_params may be pageable). */
int mkws_head_set_params(mkws_head* hd, const float* h_params, int n, void* stream);
int mkws_head_get_params(mkws_head* hd, float* h_params, int n, void* stream);
/* d_emb [B,in] -> d_probs [B,classes] (softmax probabilities, what model.predict returns). */
int mkws_head_forward(mkws_head* hd, const float* d_emb, int B, float* d_probs, void* stream);
/* Multi-keyword serving (batch_streaming_analysis.py runs one full model per keyword; here N keywords share one
 * embedding pass): n_heads heads of equal dimensions over the same d_emb [B,in] in ONE launch (per 64 heads)
 * -> d_probs [n_heads, B, classes].  `heads` is a host array of handles. */
int mkws_heads_forward(mkws_head* const* heads, int n_heads, const float* d_emb, int B, float* d_probs, void* stream);
/* Forward + mean sparse-CE loss + backward into the handle's grad buffer (gradient of the MEAN loss
 * over these B rows).  d_labels int32 [B].  d_stats float32[2] (optional, may be NULL) receives {sum of
 * per-row loss, number of correct argmax predictions} for these B rows; the same two values are always
 * written behind the gradient (mkws_head_grads()[P], [P+1]). */
int mkws_head_loss_grad(mkws_head* hd, const float* d_emb, const int32_t* d_labels, int B,
                        float* d_stats, void* stream);
/* After mkws_head_loss_grad on the same B rows: d(mean loss)/d(embedding rows) -> d_dx [B, in]  (what
 * backprop_into_embedding=True propagates into the embedding network, transfer_learning.py:94-112). */
int mkws_head_input_grad(mkws_head* hd, float* d_dx, int B, void* stream);
/* Keras Adam update from the grad buffer (grad is multiplied by grad_scale first, e.g. 1/world_size
 * after a sum all-reduce): lr_t = lr*sqrt(1-b2^t)/(1-b1^t); theta -= lr_t*m/(sqrt(v)+eps). */
int mkws_head_adam_step(mkws_head* hd, float lr, float beta1, float beta2, float eps, int step_t,
                        float grad_scale, void* stream);
/* The same update with the step index t read from device memory (*d_step >= 1, see mkws_op_step_inc): a captured hipGraph
 * replays ONE launch for every step, so t cannot be a launch argument there. */
int mkws_head_adam_step_dev(mkws_head* hd, float lr, float beta1, float beta2, float eps, const int* d_step,
                            float grad_scale, void* stream);

/* Side-by-side training of several keyword heads: a head group is a thin object over existing mkws_head handles of equal
 * dimensions (at least one, none NULL, none twice).  One call steps EVERY member -- one launch per stage (rows, dW1 partials,
 * finish, Adam) per 64 heads, the head being a grid dimension -- where the single-head entry points pay four small dependent
 * launches per head.  Each head's arithmetic is that of mkws_head_loss_grad / mkws_head_adam_step, bit for bit; the members stay
 * ordinary heads (serving, get_params, state).  The group keeps device pointers into its members: destroy the group before any
 * of them.  mkws_head_group_create allocates and uploads the group's pointer table (synchronous); the two step calls only launch
 * kernels on `stream` (asynchronous, capturable). */
typedef struct mkws_head_group mkws_head_group;
int mkws_head_group_create(mkws_head* const* heads, int n_heads, mkws_head_group** out);
void mkws_head_group_destroy(mkws_head_group* g);      /* does not destroy the heads; NULL is a no-op */
int mkws_head_group_size(const mkws_head_group* g);
/* Serving with the group as a head table: every row of a batch under the head of the SEGMENT it lies in (K keyword recordings
 * concatenated, each with its own fine-tuned head), in one launch.  Reads the members' parameters only; the training buffers are not
 * touched.  d_emb float32 [B, in] is one batch of the concatenation, its first row being global row row_base (>= 0).  Segment s holds
 * global rows d_seg_offsets[s] .. d_seg_offsets[s + 1] (int32 [n_seg + 1], non-decreasing: the caller checks; a range may be empty; an
 * unsorted list gives wrong answers, never an access outside the buffers named here: the search over it is bounded by [0, n_seg]) and is
 * served by member d_seg_head[s] (int32 [n_seg]; one head may serve several segments).  d_probs float32 [B, classes] in row order.
 * A row's output is, bit for bit, what mkws_head_forward of its head writes for that row: the kernel is that call's -- the K walk in
 * ascending chunks of 16, the four-wave K split joined in wave order, the epilogue -- and only the mapping of a 16-row tile to heads is
 * new: a tile that straddles segments (runs of one-row and empty segments included) is finished once per segment it intersects, with the
 * stores masked to that segment's rows.
 * A row that lies in no segment, or in a segment whose head index is outside [0, mkws_head_group_size), gets NaN in every class (the
 * detector treats a NaN score as no event) and is counted in *d_invalid (int32 [1], set by every call that launches); such a head index
 * is never dereferenced.  Rows outside [0, B) are not written.
 * MKWS_ERR_UNSUPPORTED unless in % 16 == 0 and hidden <= 32 (the matrix-core path only); MKWS_ERR_INVALID_ARG for NULL pointers and
 * negative B, n_seg or row_base; B == 0 or n_seg == 0 returns MKWS_OK with nothing launched and nothing written.  Asynchronous on
 * `stream`, allocates nothing, never synchronises: capturable like every other call. */
int mkws_head_group_forward_segments(mkws_head_group* g, const float* d_emb, int B, int64_t row_base, const int32_t* d_seg_offsets,
                                     const int32_t* d_seg_head, int n_seg, float* d_probs, int32_t* d_invalid, void* stream);
/* Serving with the group as a head table and a ROUTE table in device memory: route r = (d_route_slot[r], d_route_head[r]) says "this slot
 * listens for this keyword".  d_emb float32 [B, in] holds rows_per_slot rows per slot, slot s in rows s * rows_per_slot .. (the batch
 * mkws_frontend_live_push_many_f32 filled, embedded); route r's rows_per_slot output rows, rows r * rows_per_slot .. of d_probs float32
 * [n_routes, rows_per_slot, classes], are the outputs of member d_route_head[r] on its slot's rows -- work per route, not per
 * (slot, head), and what mkws_detect_live_step_routes reads.  Both tables are int32 [n_routes] and are read by the kernel, so they may be
 * rewritten between calls (or between replays of a captured call) without touching the launch.
 * An output row is, bit for bit, what mkws_head_forward of that head writes for that embedding row: the kernel is that call's -- the K
 * walk in ascending chunks of 16, the four-wave K split joined in wave order, the epilogue -- and only the mapping of a workgroup to
 * (route, 16-row tile of the slot's rows) and an output row base different from the input row base are new.
 * slot < 0 is a disabled route: nothing of it is read (not its head index either) or written.  A route whose slot is >= n_slots, whose
 * head index is outside [0, mkws_head_group_size) or whose rows would pass B is invalid: it gets NaN in all its rows (the detector
 * treats a NaN score as no event) and is counted once in *d_invalid (int32 [1], set by every call that launches, by a plain store of the
 * kernel's: the call adds no memset and no atomic to a captured chain); the bad index is never dereferenced.
 * MKWS_ERR_UNSUPPORTED unless in % 16 == 0 and hidden <= 32 (the matrix-core path only); MKWS_ERR_INVALID_ARG for NULL pointers and
 * negative sizes; n_routes == 0 or rows_per_slot == 0 returns MKWS_OK with nothing launched and nothing written.  One launch, one
 * workgroup per (route, tile), asynchronous on `stream`, allocates nothing, never synchronises: capturable. */
int mkws_head_group_forward_routes(mkws_head_group* g, const float* d_emb, int B, int rows_per_slot, int n_slots, const int32_t* d_route_slot,
                                   const int32_t* d_route_head, int n_routes, float* d_probs, int32_t* d_invalid, void* stream);
/* mkws_head_loss_grad of head h on the B rows at d_emb + h * emb_stride (stride in floats) with the labels at
 * d_labels + h * label_stride (in int32s), for every h; B at most the smallest max_batch of the group.
 * d_stats (optional, may be NULL): float32 [n_heads][2] = {sum of per-row loss, number of correct rows} of each head; the same
 * two values are written behind each head's gradient as in the single-head call. */
int mkws_head_group_loss_grad(mkws_head_group* g, const float* d_emb, int64_t emb_stride, const int32_t* d_labels,
                              int64_t label_stride, int B, float* d_stats, void* stream);
/* mkws_head_adam_step of every member with the same step index (lr_t is evaluated once, on the host, in double). */
int mkws_head_group_adam_step(mkws_head_group* g, float lr, float beta1, float beta2, float eps, int step_t,
                              float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming detector.  Replaces SingleTargetRecognizeCommands.process_latest_result
 * (multilingual_kws/embedding/single_target_recognize_commands.py:94-207) and the per-window, per-keyword, per-threshold Python loop
 * that drives it (batch_streaming_analysis.py:124-177): every window of a stream, n_heads keyword heads x n_thr detection thresholds,
 * in ONE launch.  multilingual_kws_amd/embedding/single_target_recognize_commands.py is the host restatement and the specification.
 * For window w at time t[w] (milliseconds): head = the smallest j <= w with t[j] >= t[w] - average_window_duration_ms;
 * how_many = w - head + 1.  A window with how_many < minimum_count or t[w] - t[head] < average_window_duration_ms / 4 is not evaluated
 * (score 0.0, the label of the previous event, no event).  Otherwise score = sum over j = head..w, in that order, of
 * (double)p[j][target_id] / (double)how_many, in float64 with one IEEE division and one IEEE addition per term (bit-equal to the host
 * class); a score above the threshold fires when the last event's label is silence, a score below it releases, either only when more
 * than suppression_ms have passed since the last event that left the label at the keyword.  A NaN score is no event.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mkws_detect_event {
  int32_t window;   /* index of the window the event happened in */
  int32_t fired;    /* 1: the keyword fired; 0: release (is_new_command with the silence label) */
  double score;
} mkws_detect_event;

/* d_probs [n_heads, n_windows, classes] float32 (what mkws_heads_forward writes) or float64 (probs_f64 != 0);
 * d_times_ms int64 [n_windows], non-decreasing and within +-2^61 (the caller checks; unsorted times give wrong answers, never a
 * wild access);
 * d_thresholds double [n_thr].
 * d_events [n_heads, n_thr, event_cap], d_counts int32 [n_heads, n_thr] = events that OCCURRED (a count above event_cap tells the
 * caller that the list is cut; nothing is stored past the cap).  fired_only = 0: every is_new_command step is an event.  The host
 * class also reports a release on EVERY evaluated sub-threshold window while the label already is silence, so a quiet stream has
 * about one event per window and lane.  fired_only != 0: only fired events are stored and counted -- what the callers of detect()
 * keep -- and successive fires of a lane are more than suppression_ms apart, which bounds the list.
 * Optional dense trace for parity checks (either may be NULL): d_scores double [n_heads, n_windows] (0.0 where not evaluated),
 * d_flags uint8 [n_heads, n_thr, n_windows]: bit 0 found_command is the keyword, bit 1 is_new_command.
 * MKWS_ERR_INVALID_ARG for NULL required pointers, negative sizes, target_id outside [0, classes), average_window_duration_ms < 0
 * (the host class would pop its own newest entry) and n_thr < 1; n_windows == 0 or n_heads == 0 returns MKWS_OK with nothing
 * launched and nothing written.  Asynchronous on `stream`, allocates nothing, never synchronises: capturable like every other call. */
int mkws_detect_stream(const void* d_probs, int probs_f64, int n_heads, int n_windows, int classes, int target_id,
                       const int64_t* d_times_ms, const double* d_thresholds, int n_thr, double average_window_duration_ms,
                       double suppression_ms, int minimum_count, int fired_only, mkws_detect_event* d_events, int event_cap,
                       int32_t* d_counts, double* d_scores, uint8_t* d_flags, void* stream);

/* Live form of mkws_detect_stream: the detector stepped over the few windows a push completed, its state kept between calls in
 * d_state, a caller-owned device block of mkws_detect_live_state_bytes() bytes, 8-byte aligned.  A zero-filled block is a fresh stream
 * (reset = memset, snapshot / restore = copies).  It holds, per head, the last `history` (time, target probability) pairs and the
 * {label of the last event, time after which it may change} of each threshold's lane.
 * d_probs float32 [n_heads, max_new, classes]; d_meta int64 [2 + max_new] as mkws_frontend_live_push_f32 writes it: {count, (index of
 * the first new window: not read), time_ms of each new window}; rows and times from count on are not read; count is clamped into
 * [0, max_new].  Times must not decrease, from call to call either (the caller checks).
 * The specification is mkws_detect_stream's: calls whose windows add up to a stream leave, concatenated, that call's events, counts
 * and scores on the whole stream, byte for byte -- provided `history` is at least the largest number of windows an average spans
 * (the windows within average_window_duration_ms of each other; multilingual_kws_amd/detector.py, live_history).  Above
 * MKWS_DETECT_LIVE_MAX_HISTORY the call returns MKWS_ERR_UNSUPPORTED.
 * d_events [n_heads, n_thr, max_new]: event.window is the index inside this push (0 .. count-1; the caller adds d_meta[1]); a lane has
 * at most one event per window, so the lists are never cut.  d_counts int32 [n_heads, n_thr]: events of THIS push.  d_scores (optional)
 * double [n_heads, max_new].  count == 0: the state is left as it is and zero counts are written.
 * MKWS_ERR_INVALID_ARG as mkws_detect_stream, and for history < 1; MKWS_ERR_UNSUPPORTED for n_thr above 1024 and max_new above
 * MKWS_DETECT_LIVE_MAX_NEW; n_heads == 0 or max_new == 0 returns MKWS_OK with nothing launched.  mkws_detect_live_state_bytes returns 0
 * for sizes the step would refuse.  One launch, asynchronous on `stream`, allocates nothing, never synchronises: capturable. */
#define MKWS_DETECT_LIVE_MAX_HISTORY 256
#define MKWS_DETECT_LIVE_MAX_NEW 1024
size_t mkws_detect_live_state_bytes(int n_heads, int n_thr, int history);
int mkws_detect_live_step(void* d_state, const float* d_probs, const int64_t* d_meta, int max_new, int n_heads, int classes, int target_id,
                          const double* d_thresholds, int n_thr, double average_window_duration_ms, double suppression_ms,
                          int minimum_count, int fired_only, int history, mkws_detect_event* d_events, int32_t* d_counts,
                          double* d_scores, void* stream);

/* n_streams live detectors stepped in one launch.  Stream s's state block is d_states + s * state_stride_bytes (a multiple of 8, at
 * least mkws_detect_live_state_bytes(); MKWS_ERR_INVALID_ARG otherwise), exactly the block of the one-stream call, and the call is
 * that call applied to every stream's slice, byte for byte, on: rows s * max_new .. of every head's plane of d_probs
 * [n_heads, n_streams * max_new, classes] (what mkws_heads_forward writes for the batch mkws_frontend_live_push_many_f32 filled), row s
 * of d_meta [n_streams, 2 + max_new], d_events [n_streams, n_heads, n_thr, max_new], d_counts [n_streams, n_heads, n_thr] and the
 * optional d_scores [n_streams, n_heads, max_new].  There is no activity mask: a meta row with count == 0 leaves that stream's state as
 * it is and writes zero counts.  Refusals and limits as the one-stream call, and n_streams < 0; n_streams == 0 returns MKWS_OK with
 * nothing launched.  One launch for any n_streams, asynchronous on `stream`, allocates nothing, never synchronises: capturable. */
int mkws_detect_live_step_many(void* d_states, size_t state_stride_bytes, int n_streams, const float* d_probs, const int64_t* d_meta,
                               int max_new, int n_heads, int classes, int target_id, const double* d_thresholds, int n_thr,
                               double average_window_duration_ms, double suppression_ms, int minimum_count, int fired_only, int history,
                               mkws_detect_event* d_events, int32_t* d_counts, double* d_scores, void* stream);

/* mkws_detect_live_step_many with "stream" replaced by "route", one head per route: n_routes live detectors, each listening to one slot
 * with thresholds of its own, stepped in one launch.  Route r's state block is d_states + r * state_stride_bytes, exactly the block
 * mkws_detect_live_step takes for n_heads = 1; its probability rows are r * max_new .. of d_probs [n_routes * max_new, classes] (what
 * mkws_head_group_forward_routes writes); its meta row is row d_route_slot[r] of d_meta [n_slots, 2 + max_new] -- the SLOT's row, as
 * mkws_frontend_live_push_many_f32 writes it, shared by the routes of that slot; its thresholds are row r of d_thresholds double
 * [n_routes, n_thr].  d_events [n_routes, n_thr, max_new], d_counts int32 [n_routes, n_thr], optional d_scores [n_routes, max_new].
 * Specification, byte for byte: route r is mkws_detect_live_step(n_heads = 1) on its own block, its own probability rows, its slot's
 * meta row and its own threshold row.  A route whose slot is outside [0, n_slots) (d_route_slot int32 [n_routes]; -1 = disabled) leaves
 * its state untouched, gets zero counts and never has a meta row read; a meta row with count == 0 behaves as in the one-stream call.
 * The tables are read by the kernel, so they may be rewritten between calls (or replays of a captured call).
 * Refusals and limits as mkws_detect_live_step_many, and a NULL d_route_slot or n_slots < 0; n_routes == 0 returns MKWS_OK with nothing
 * launched.  One launch for any n_routes, asynchronous on `stream`, allocates nothing, never synchronises: capturable. */
int mkws_detect_live_step_routes(void* d_states, size_t state_stride_bytes, int n_routes, const int32_t* d_route_slot, int n_slots,
                                 const float* d_probs, const int64_t* d_meta, int max_new, int classes, int target_id,
                                 const double* d_thresholds, int n_thr, double average_window_duration_ms, double suppression_ms,
                                 int minimum_count, int fired_only, int history, mkws_detect_event* d_events, int32_t* d_counts,
                                 double* d_scores, void* stream);

/* Scoring against ground truth: tpr_fpr's counts (multilingual_kws/embedding/tpr_fpr.py:72-107) for every (head, threshold) lane in
 * one launch, on what mkws_detect_stream(..., fired_only = 1, ...) left on the same stream: d_events [n_heads, n_thr, event_cap] and
 * d_counts, with the d_times_ms [n_windows] of that call (an event's time is d_times_ms[window]).  Head n's ground-truth times are
 * d_gt_ms[d_gt_offsets[n] .. d_gt_offsets[n + 1]) (d_gt_offsets int32 [n_heads + 1], non-decreasing), in the caller's order; the
 * range may be empty.  d_gt_ms must be a valid pointer even when every range is empty; its values finite.
 * d_tally int32 [n_heads, n_thr, 4], 16-byte aligned, per lane {found, true_positives_raw, false_negatives, cut}:
 *   found               = the lane's count;
 *   true_positives_raw  = detections t for which the scan over the head's ground truth IN LIST ORDER meets an entry >= t - tol before
 *                         it meets one > t + tol (the scan stops there: on an unsorted list an in-window entry behind an out-of-window
 *                         one is not seen).  NOT capped to the number of ground-truth entries: that, and every rate derived from it,
 *                         is host arithmetic on these integers;
 *   false_negatives     = ground-truth entries g with no detection of the lane in [g - tol, g + tol];
 *   cut                 = 1 when count > event_cap: the list is incomplete, true_positives_raw and false_negatives are unspecified.
 * t +- tol and g +- tol are formed in float64 with one IEEE operation each and compared with the other side converted to double
 * (exact while |t| < 2^53, which the caller checks); an entry on the edge of the window matches.  n_windows == 0 (the detector then
 * launched nothing and wrote no counts): every lane is {0, 0, entries of its head, 0} and d_counts is not read.
 * MKWS_ERR_INVALID_ARG for NULL required pointers (d_events may be NULL when event_cap is 0), negative sizes, n_thr < 1 and a
 * time_tolerance_ms that is NaN or negative; n_heads == 0 returns MKWS_OK with nothing launched.  Asynchronous on `stream`,
 * allocates nothing, never synchronises: capturable like every other call. */
int mkws_detect_score(const mkws_detect_event* d_events, const int32_t* d_counts, int n_heads, int n_thr, int event_cap,
                      const int64_t* d_times_ms, int n_windows, const double* d_gt_ms, const int32_t* d_gt_offsets,
                      double time_tolerance_ms, int32_t* d_tally, void* stream);

/* mkws_detect_stream with "head" replaced by "segment": n_seg recordings concatenated, each with its own windows, times and
 * probabilities (K keyword recordings, one fine-tuned head each), in ONE launch.  d_probs [n_rows, classes] float32 or float64
 * (probs_f64 != 0): what mkws_head_group_forward_segments writes; d_times_ms int64 [n_rows], non-decreasing WITHIN each segment.
 * Segment s holds rows d_seg_offsets[s] .. d_seg_offsets[s + 1] (int32 [n_seg + 1], non-decreasing with values in [0, n_rows]: the caller
 * checks; the kernel clamps what it reads into [0, n_rows], so a bad list gives wrong answers, never a wild access).
 * d_events [n_seg, n_thr, event_cap], d_counts int32 [n_seg, n_thr]; event.window is the index INSIDE the segment, so that segment s of
 * this call equals mkws_detect_stream(n_heads = 1) on that slice alone, byte for byte: the lookback of a window's average is searched
 * over [segment start, w] and never leaves the segment.  Counts are written for EVERY segment: an empty one gets 0 (the unsegmented
 * call launches nothing for zero windows).
 * Optional trace (either may be NULL): d_scores double [n_rows]; d_flags uint8 [n_thr * n_rows]: the per-segment [n_thr, len_s] blocks
 * back to back, i.e. segment s, threshold k, window w at n_thr * d_seg_offsets[s] + k * len_s + w.
 * The argument checks are those of mkws_detect_stream (d_probs and d_times_ms may be NULL when n_rows is 0); n_seg == 0 returns MKWS_OK with nothing launched and nothing written.
 * Asynchronous on `stream`, allocates nothing, never synchronises: capturable like every other call. */
int mkws_detect_segments(const void* d_probs, int probs_f64, const int32_t* d_seg_offsets, int n_seg, int n_rows, int classes, int target_id,
                         const int64_t* d_times_ms, const double* d_thresholds, int n_thr, double average_window_duration_ms,
                         double suppression_ms, int minimum_count, int fired_only, mkws_detect_event* d_events, int event_cap,
                         int32_t* d_counts, double* d_scores, uint8_t* d_flags, void* stream);

/* mkws_detect_score on what mkws_detect_segments(..., fired_only = 1, ...) left on the same stream, with that call's d_seg_offsets,
 * n_rows and d_times_ms: the time of an event of segment s is d_times_ms[d_seg_offsets[s] + window], window clamped into the segment.
 * Segment s is matched against d_gt_ms[d_gt_offsets[s] .. d_gt_offsets[s + 1]) (int32 [n_seg + 1]).  d_tally int32 [n_seg, n_thr, 4],
 * 16-byte aligned, the four fields of mkws_detect_score; an empty segment gives {0, 0, entries of its ground truth, 0}.
 * MKWS_ERR_INVALID_ARG as mkws_detect_score; n_seg == 0 returns MKWS_OK with nothing launched.  Asynchronous on `stream`, allocates
 * nothing, never synchronises: capturable like every other call. */
int mkws_detect_score_segments(const mkws_detect_event* d_events, const int32_t* d_counts, const int32_t* d_seg_offsets, int n_seg, int n_rows,
                               int n_thr, int event_cap, const int64_t* d_times_ms, const double* d_gt_ms, const int32_t* d_gt_offsets,
                               double time_tolerance_ms, int32_t* d_tally, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Classification ROC counts: roc_single_target / roc_sc / calc_roc
 * (multilingual_kws/embedding/transfer_learning_analysis.py:181-222, :345-404) for n_heads keyword heads and n_thr thresholds in one
 * launch.  d_probs [n_heads, n_rows, classes] float32 (what mkws_heads_forward writes).  Head h's positive clips are the rows
 * d_pos_rows[d_pos_offsets[h] .. d_pos_offsets[h + 1]) of ITS OWN probability plane, its negatives d_neg_rows[d_neg_offsets[h] ..
 * d_neg_offsets[h + 1]) (offsets int32 [n_heads + 1], non-decreasing and inside their list: the caller checks).  A row may appear
 * several times and then counts several times (the reference counts list entries); either range may be empty.  An entry outside
 * [0, n_rows) is never dereferenced: it is skipped and counted in d_invalid[h] (int32 [n_heads], entries of both lists).
 * d_thresholds double [n_thr], ascending (non-decreasing, equal neighbours allowed) and NaN-free: the caller checks; an unsorted list
 * gives wrong counts, never a wild access.
 * d_counts int32 [n_heads, n_thr, 2]: {positive entries with score > thr[j], negative entries with score > thr[j]}, exact, the same
 * on every run.  The comparison is (double)score > thr[j] -- the float32 probability widened, strictly greater, which is what NumPy
 * computes for a float32 array against an np.float64 threshold; it is NOT the float32 comparison.  A NaN score is above no threshold.
 *   mode 0 (roc_single_target): score = p[row][pos_class] on both sides; neg_class is ignored.
 *   mode 1 (roc_sc / calc_roc on evaluate_files_multiclass dicts): a = first index of the row's maximum (np.argmax); a positive entry
 *     takes part only when a == pos_class, a negative one only when a != neg_class; score = p[row][a].  A row holding a NaN is never
 *     counted.
 * MKWS_ERR_INVALID_ARG for NULL required pointers (d_probs may be NULL when n_rows is 0), negative sizes, n_thr < 1, classes < 1, a mode
 * other than 0 / 1, pos_class (mode 1: and neg_class) outside [0, classes); MKWS_ERR_UNSUPPORTED for n_thr above
 * MKWS_ROC_MAX_THRESHOLDS (the thresholds and one bin each live in LDS): run a longer list in pieces.  n_heads == 0 returns MKWS_OK
 * with nothing launched (the buffers may then be NULL); n_rows == 0 with empty lists writes zero counts.  Asynchronous on `stream`, allocates nothing, never
 * synchronises: capturable like every other call.
 * ---------------------------------------------------------------------------------------------- */
#define MKWS_ROC_MAX_THRESHOLDS 4096
int mkws_roc_count(const float* d_probs, int n_heads, int n_rows, int classes, const int32_t* d_pos_rows, const int32_t* d_pos_offsets,
                   const int32_t* d_neg_rows, const int32_t* d_neg_offsets, const double* d_thresholds, int n_thr, int mode,
                   int pos_class, int neg_class, int32_t* d_counts, int32_t* d_invalid, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Classification point scores: what Keras' model.evaluate(ds) (sparse categorical cross-entropy + accuracy) and
 * tf.math.confusion_matrix report, for n_models classifiers over n_rows shared rows, ADDED to accumulators that the caller zeroed once:
 * a dataset is scored by one call per batch and read with one synchronisation at the end.  multilingual_kws_amd/scoring.py (score_host)
 * is the specification.
 * d_scores float32 [n_models, n_rows, classes]; d_labels int32, [n_rows] shared by the models (labels_per_model = 0) or
 * [n_models, n_rows] (labels_per_model = 1); d_groups int32 [n_rows] shared by the models, or NULL: no groups (n_groups and
 * d_group_tally are then ignored).
 *   prediction: the first index of the row's maximum over the float32 scores (np.argmax); a NaN wins, among several NaNs the first.  An
 *     exact function of the row's bits.
 *   row loss, float64 from the float32 scores:
 *     mode 0 (probabilities, Keras' backend formula): -log(min(max(p[y], lo), hi)), lo = (double)(float)1e-7 and
 *       hi = (double)(1.0f - (float)1e-7) = 1 - 2^-23 -- Keras' float32 epsilon and its float32 1 - epsilon, widened; the clip is made on
 *       the float32 value, the log is taken in double.  A NaN p[y] gives NaN.
 *     mode 1 (logits): (log(sum_c exp(z[c] - max z)) + max z) - z[y].  A NaN anywhere in the row gives NaN; so does a maximum of +inf
 *       (inf - inf), as in the float64 specification.
 *     The loss of row (m, r) is a function of that row alone: the same bits in every batch that holds it.
 *   labels: -1 means "ignore this row" (batch padding): counted in `ignored`, tallied nowhere else.  Any other label outside
 *     [0, classes) is never used as an index: counted in `invalid`, tallied nowhere else; with d_groups, a group outside [0, n_groups)
 *     makes the row invalid in the same way (label -1 is looked at first).
 * Outputs, all of them += except the last two:
 *   d_loss double [n_models]: every row's loss goes to the workspace first (0 for ignored and invalid rows); a second kernel adds a
 *     model's n_rows values in an order that depends on n_rows alone and adds that sum to d_loss[m].  No floating-point atomics: two
 *     runs give the same bits.  A NaN row loss reaches d_loss.
 *   d_tally int64 [n_models, 4] = {rows tallied, correct (prediction == label), ignored, invalid};
 *   d_confusion int64 [n_models, classes, classes] or NULL, row = true class, column = prediction;
 *   d_group_tally int64 [n_models, n_groups, 2] = {rows, correct} or NULL.
 *     The integers are exact and do not depend on how the rows were cut into calls.  classes <= 32: a workgroup keeps its matrix in LDS
 *     and flushes its non-zero cells with 64-bit atomics; above, every row adds its cell with a 64-bit atomic in global memory.
 *   d_row_loss double [n_models, n_rows] or NULL: written (not added), NaN for ignored and invalid rows;
 *   d_pred int32 [n_models, n_rows] or NULL: written for every row.
 * d_work: mkws_score_work_bytes(n_models, n_rows) bytes (8 per row and model), 8-byte aligned, caller-owned, contents unspecified.
 * MKWS_ERR_INVALID_ARG for NULL required pointers (d_scores, d_labels, d_loss, d_tally, d_work), negative sizes, classes < 2, a mode
 * or labels_per_model other than 0 / 1, n_groups < 0 and d_groups given with n_groups == 0; MKWS_ERR_UNSUPPORTED for classes above
 * MKWS_SCORE_MAX_CLASSES and for more than 2^31 - 1 workgroups (n_models * ceil(n_rows / 256), classes > 32: n_rows / 32).
 * n_models == 0 or n_rows == 0 returns MKWS_OK with nothing launched and the accumulators untouched (the buffers may then be NULL).
 * Asynchronous on `stream`, allocates nothing, never synchronises: capturable like every other call.
 * ---------------------------------------------------------------------------------------------- */
#define MKWS_SCORE_MAX_CLASSES 4096
/* Host only: bytes of d_work for one call (0 for non-positive sizes). */
size_t mkws_score_work_bytes(int n_models, int n_rows);
int mkws_score_accumulate(const float* d_scores, int n_models, int n_rows, int classes, int mode, const int32_t* d_labels,
                          int labels_per_model, const int32_t* d_groups, int n_groups, double* d_loss, int64_t* d_tally,
                          int64_t* d_confusion, int64_t* d_group_tally, double* d_row_loss, int32_t* d_pred, void* d_work,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * k-means of the MSWC outlier filter: what distance_filtering.cluster_and_sort
 * (multilingual_kws/embedding/distance_filtering.py:30-83) does per keyword with sklearn.cluster.KMeans(n_clusters, random_state).fit
 * and np.linalg.norm, for n_groups keywords in one launch.  multilingual_kws_amd/kmeans.py (kmeans_host) is the specification:
 * mean-centring, greedy k-means++ with n_trials local trials, Lloyd with sklearn's two stopping rules (labels unchanged; squared centre
 * shift <= tol * mean column variance), the final assignment; float64 arithmetic on the widened float32 points throughout.  The random
 * draws are data-independent uniforms and are made by the host (kmeans.kmeans_draws).  An empty cluster in a Lloyd step is NOT restated
 * (sklearn relocates a centre there): it is reported, and the caller runs sklearn for that group.
 * ---------------------------------------------------------------------------------------------- */
#define MKWS_KMEANS_MAX_POINTS 1024        /* points of one group */
#define MKWS_KMEANS_MAX_CLUSTERS 16
#define MKWS_KMEANS_MAX_CENTER_VALUES 16384 /* n_clusters * dim: the float64 centres of a group live in LDS (128 KB) ... */
#define MKWS_KMEANS_MAX_LDS_VALUES 17408    /* ... beside the float64 column means: (n_clusters + 1) * dim */
#define MKWS_KMEANS_MAX_TRIALS 64          /* n_trials (sklearn's is 2 + int(log(n_clusters)) <= 4 at the cluster cap) */

/* d_x float32 [rows, dim]; group g = rows d_offsets[g] .. d_offsets[g+1]  (int32 [n_groups+1], non-decreasing and inside d_x: the
 * caller checks).
 * d_draws double [n_groups, 1 + (n_clusters-1) * n_trials]: u0, then U[1], U[2], ... (n_trials each; made by the host).
 * d_centers float32 [n_groups, n_clusters, dim] (the float64 result rounded once); d_centers_f64 (optional, may be NULL) the unrounded
 * values; d_labels int32 [rows]; d_init int32 [n_groups, n_clusters] (optional, may be NULL) = the rows (within the group) k-means++
 * picked; d_info int32 [n_groups, 4] = {status, n_iter, stop reason, smallest cluster size}; stop reason 0 = the labels did not change,
 * 1 = the centre shift fell to the tolerance, 2 = max_iter reached.
 *   status 0 ok;
 *   status 1 = a Lloyd step met an empty cluster: d_info = {1, the iteration, 0, 0}; the other outputs of the group are unspecified
 *              (finite or not; never a wild access);
 *   status 2 = the group has fewer points than n_clusters or more than MKWS_KMEANS_MAX_POINTS: d_info = {2, 0, 0, 0}, nothing else is
 *              written for it.  Neighbouring groups of the same call are not affected by either.
 * One workgroup per group; no floating-point atomics, no workspace: two calls on the same input write the same bytes.
 * MKWS_ERR_INVALID_ARG for NULL required pointers, negative sizes, dim < 1, n_clusters < 1, n_trials < 1, max_iter < 1 and a NaN or
 * negative tol; MKWS_ERR_UNSUPPORTED above MKWS_KMEANS_MAX_CLUSTERS, MKWS_KMEANS_MAX_CENTER_VALUES, MKWS_KMEANS_MAX_LDS_VALUES or
 * MKWS_KMEANS_MAX_TRIALS.  n_groups == 0 returns MKWS_OK with nothing launched.  Asynchronous on `stream`, allocates nothing, never
 * synchronises: capturable like every other call. */
int mkws_kmeans_fit(const float* d_x, int dim, const int32_t* d_offsets, int n_groups, int n_clusters, const double* d_draws,
                    int n_trials, int max_iter, double tol, float* d_centers, double* d_centers_f64, int32_t* d_labels,
                    int32_t* d_init, int32_t* d_info, void* stream);

/* Distance of every row to the nearest centre of ITS group: d_x float32 [n_rows, dim], d_group int32 [n_rows] (rows in any order; a
 * batch may straddle groups), d_centers float32 [n_groups, n_clusters, dim] (what mkws_kmeans_fit wrote).
 * d_dist float32 [n_rows] = (float) sqrt( sum_d ((double)c[d] - (double)x[d])^2 ), the minimum over the group's centres taken on the
 * float64 values; d_which int32 [n_rows] = the first index of that minimum.  A row whose group is outside [0, n_groups) is never
 * dereferenced against a centre: it gets NaN / -1 and is counted in *d_invalid (int32 [1], set by every call that launches).
 * MKWS_ERR_INVALID_ARG for NULL required pointers (d_centers may be NULL when n_groups is 0), negative sizes, dim < 1 and
 * n_clusters < 1; MKWS_ERR_UNSUPPORTED above MKWS_KMEANS_MAX_CLUSTERS.  n_rows == 0 returns MKWS_OK with nothing launched and nothing
 * written.  Asynchronous on `stream`, allocates nothing, never synchronises: capturable like every other call. */
int mkws_kmeans_nearest(const float* d_x, int dim, int n_rows, const int32_t* d_group, const float* d_centers, int n_groups,
                        int n_clusters, float* d_dist, int32_t* d_which, int32_t* d_invalid, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K logistic regressions on embedding vectors: what the DataPerf selection harness of the reference
 * (notebooks/dataperf_test_harness.py:242-256,318-408, notebooks/dataperf_experiments.py:121-192) does per split with
 * sklearn.linear_model.LogisticRegression, for n_problems problems in one launch.  multilingual_kws_amd/logreg.py (objective,
 * logreg_host) is the specification: problem p minimises
 *     f(W, b) = C[p] * sum_i [ logsumexp_k(z_ik) - z_{i,y_i} ] + (kappa / 2) * sum W^2,   z_i = W x~_i + b,
 * W [n_classes, dim], b [n_classes] unpenalised, kappa = 2 for two classes (sklearn's binary objective in two-row form) and 1 above.
 * standardize = 1: x~ = (x - mu) / sigma over the problem's own rows (ddof 0, sigma = 0 -> 1); solved and penalised in that space,
 * returned in raw space (W = W~ / sigma, b = b~ - W~ . mu / sigma).  The intercepts come back with sum_k b~_k = 0.
 * ---------------------------------------------------------------------------------------------- */
#define MKWS_LOGREG_MAX_ROWS 1024          /* rows of one problem */
#define MKWS_LOGREG_MAX_CLASSES 8
#define MKWS_LOGREG_MAX_DIM 1024

/* Floats of workspace mkws_logreg_fit needs (the coefficients, the direction and the previous gradient of every problem). */
size_t mkws_logreg_work_floats(int dim, int n_problems, int n_classes);

/* d_x float32 [n_rows, dim]: the bank.  Problem p trains on bank rows d_rows[d_offsets[p] .. d_offsets[p+1]) with labels
 * d_labels[...] in [0, n_classes), gathered through the list: no row is copied, rows may repeat inside a problem and across problems
 * (d_offsets int32 [n_problems+1], non-decreasing and inside the lists: the caller checks).  d_C double [n_problems].
 * d_coef float32 [n_problems, n_classes, dim], d_intercept float32 [n_problems, n_classes], d_stats double [n_problems, 2] =
 * {objective, |gradient|_inf} as the device last saw them (at the returned point, in the space the problem was solved in),
 * d_info int32 [n_problems, 4] = {status, n_iter, stop reason, rows}; stop reason 0 = |gradient|_inf <= gtol, 1 = max_iter steps were
 * taken (sklearn's ConvergenceWarning, not an error).
 *   status 0 fitted;
 *   status 2 = an empty problem, more than MKWS_LOGREG_MAX_ROWS rows, a label outside [0, n_classes) or a row index outside
 *              [0, n_rows): d_info = {2, 0, 0, rows}, nothing else is written for it and no bank row is read.  Neighbouring problems are
 *              not affected.
 * The solver is non-linear conjugate gradients with an exact line search on cached logits; every class row is fitted, also one with
 * no sample.  One workgroup per problem, no floating-point atomics: two calls on the same input write the same bytes.
 * d_work: mkws_logreg_work_floats(...) floats, contents unspecified before and after.
 * MKWS_ERR_INVALID_ARG for NULL pointers, negative sizes, dim < 1, n_classes < 2, max_iter < 1, a NaN or negative gtol, standardize
 * other than 0 / 1 and a workspace that is too small; MKWS_ERR_UNSUPPORTED above MKWS_LOGREG_MAX_CLASSES or MKWS_LOGREG_MAX_DIM.
 * n_problems == 0 returns MKWS_OK with nothing launched.  Asynchronous on `stream`, allocates nothing, never synchronises: capturable
 * like every other call. */
int mkws_logreg_fit(const float* d_x, int n_rows, int dim, const int32_t* d_rows, const int32_t* d_labels, const int32_t* d_offsets,
                    int n_problems, int n_classes, const double* d_C, int standardize, int max_iter, double gtol, float* d_coef,
                    float* d_intercept, int32_t* d_info, double* d_stats, float* d_work, size_t work_floats, void* stream);

/* Every problem scored on its OWN row list: entry e of d_rows / d_true (int32 [total]) belongs to the problem p with
 * d_offsets[p] <= e < d_offsets[p+1].  logit_k = sum_d coef[p,k,d] * x[row,d] + intercept[p,k] in float32 (fused multiply-adds, lanes
 * across dim, a butterfly sum); d_pred int32 [total] = the first argmax of the logits; d_probs (optional, may be NULL) float32
 * [total, n_classes] their softmax; d_logits (optional, may be NULL) float32 [total, n_classes]; d_correct int32 [n_problems] = entries
 * with d_pred == d_true, zeroed by the call itself (integer adds).  An entry outside every list, or whose row is outside [0, n_rows),
 * is never dereferenced: d_pred = -1, NaN probabilities and logits, not counted.
 * MKWS_ERR_INVALID_ARG for NULL required pointers, negative sizes, dim < 1, n_classes < 2; MKWS_ERR_UNSUPPORTED above the caps.
 * Asynchronous on `stream`, allocates nothing, never synchronises: capturable like every other call. */
int mkws_logreg_score(const float* d_x, int n_rows, int dim, const int32_t* d_rows, const int32_t* d_true, const int32_t* d_offsets,
                      int n_problems, int n_classes, const float* d_coef, const float* d_intercept, int total, int32_t* d_pred,
                      float* d_probs, float* d_logits, int32_t* d_correct, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K L1-regularised logistic regressions on embedding vectors: the reference's `logistic_regression_with_l1_regularization`
 * (notebooks/dataperf_test_harness.py:277-280), sklearn.linear_model.LogisticRegression(penalty="l1", solver="liblinear"), for
 * n_problems problems in one launch.  multilingual_kws_amd/lr_l1.py (objective, lr_l1_host) is the specification: liblinear's L1R_LR is
 * one independent binary problem per class k (one-vs-rest), the bias an extra feature of value 1 that is penalised like a weight,
 *     f_k(w, b) = |w|_1 + |b| + C[p] * sum_i log(1 + exp(-s_ik (w . x_i + b))),   s_ik = +1 if label i is k, else -1,
 * and the prediction is the first argmax over k of w_k . x + b_k, which mkws_logreg_score evaluates on d_coef / d_intercept as this
 * call leaves them.  "violation" is the largest magnitude of the minimum-norm subgradient over the dim weights and the bias: with g
 * the gradient of the smooth part, |g_j + sign(w_j)| where w_j != 0 and max(|g_j| - 1, 0) where w_j = 0.
 * The caps are MKWS_LOGREG_MAX_ROWS, MKWS_LOGREG_MAX_CLASSES and MKWS_LOGREG_MAX_DIM.
 * ---------------------------------------------------------------------------------------------- */

/* Floats of workspace mkws_lr_l1_fit needs: none (0) -- the iterates live in registers and LDS. */
size_t mkws_lr_l1_work_floats(int dim, int n_problems, int n_classes);

/* The bank, the lists, d_offsets and d_C are those of mkws_logreg_fit.  d_coef float32 [n_problems, n_classes, dim] (a weight the solver
 * holds at zero is exactly 0.0f), d_intercept float32 [n_problems, n_classes], d_info int32 [n_problems, n_classes, 4] = {status, n_iter,
 * stop reason, non-zero weights among the dim (the bias is not counted)} per class, d_stats double [n_problems, n_classes, 2] = {f_k,
 * violation} at the returned point, computed from logits formed afresh from the returned weights; stop reason 0 = violation <= vtol
 * (looked at every 8 iterations and after the last), 1 = max_iter iterations were made (sklearn's ConvergenceWarning, not an error).
 *   status 0 fitted;
 *   status 2 = an empty problem, more than MKWS_LOGREG_MAX_ROWS rows, a label outside [0, n_classes) or a row index outside
 *              [0, n_rows): all n_classes entries of d_info are {2, 0, 0, 0}, nothing else is written for the problem and no bank row is
 *              read.  Neighbouring problems are not affected.
 * Two classes: class 1 is solved and class 0 is written as its exact negation (zeros stay +0.0f), with the same info and stats.  Every
 * class problem is posed, also that of a class with no sample.
 * The solver is a proximal gradient iteration (FISTA with gradient restart, the step from a power iteration), one workgroup per
 * (problem, class), no floating-point atomics: two calls on the same input write the same bytes.
 * d_work / work_floats: mkws_lr_l1_work_floats(...) floats, that is none: d_work may be NULL and is never touched.
 * MKWS_ERR_INVALID_ARG for NULL pointers (other than d_work), negative sizes, dim < 1, n_classes < 2, max_iter < 1 and a NaN or negative
 * vtol; MKWS_ERR_UNSUPPORTED above MKWS_LOGREG_MAX_CLASSES or MKWS_LOGREG_MAX_DIM.  n_problems == 0 returns MKWS_OK with nothing
 * launched.  A refused call writes nothing.  Asynchronous on `stream`, allocates nothing, never synchronises: capturable like every
 * other call. */
int mkws_lr_l1_fit(const float* d_x, int n_rows, int dim, const int32_t* d_rows, const int32_t* d_labels, const int32_t* d_offsets,
                   int n_problems, int n_classes, const double* d_C, int max_iter, double vtol, float* d_coef, float* d_intercept,
                   int32_t* d_info, double* d_stats, float* d_work, size_t work_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K RBF support-vector classifiers on embedding vectors: what the DataPerf selection harness of the reference
 * (notebooks/dataperf_test_harness.py:224-239) does per split with sklearn.svm.SVC(), for n_problems problems side by side.
 * multilingual_kws_amd/svc.py (svc_host, decision_host, predict_host) is the specification: C-SVC, k(a, b) = exp(-gamma |a~ - b~|^2) with
 * a~ = (a - centre) * inv_scale, one machine per pair of present classes i < j (class i is +1), f_ij(x) = sum_t c_t k(x_t, x) - rho_ij,
 * one-vs-one votes with the lowest class on ties.  A fit is three calls on one stream: mkws_svc_prepare, mkws_svc_kernel with both lists
 * the training lists and d_out the workspace, mkws_svc_fit.  All four are asynchronous on `stream`, allocate nothing, never synchronise
 * and use no floating-point atomics: two runs on the same input write the same bytes.
 * The lists are as in mkws_logreg_fit: problem p owns entries d_offsets[p] .. d_offsets[p+1] of the flat d_rows / d_labels (d_offsets
 * int32 [n_problems+1], non-decreasing and inside the lists: the caller checks); rows may repeat inside and across problems.
 * MKWS_ERR_INVALID_ARG for NULL required pointers, negative sizes, dim < 1, n_classes < 2 and the values named below;
 * MKWS_ERR_UNSUPPORTED above the caps.  n_problems == 0 returns MKWS_OK with nothing launched.
 * ---------------------------------------------------------------------------------------------- */
#define MKWS_SVC_MAX_ROWS 1024             /* rows of one problem */
#define MKWS_SVC_MAX_CLASSES 8
#define MKWS_SVC_MAX_DIM 1024

/* Bytes of the Gram workspace of a fit: n_problems * max_rows^2 floats (problem p's n x n matrix starts at float p * max_rows^2). */
size_t mkws_svc_work_bytes(int n_problems, int max_rows);

/* Per problem: d_centre float32 [n_problems, dim] = the column mean of its own rows (always: the kernel is translation invariant and
 * distances are formed from centred rows), d_inv_scale float32 [n_problems, dim] = 1 / sigma with standardize = 1 (ddof 0, sigma = 0 ->
 * 1), ones with 0; d_gamma float32 [n_problems] = `gamma` where that is positive, otherwise sklearn's "scale" 1 / (dim * Var) over all
 * entries of the matrix the kernel sees (1 where Var = 0), every sum in float64; d_info int32 [n_problems, 4] = {status, present pairs,
 * 0, 0} and d_gap float32 [n_problems] = 0, which mkws_svc_fit completes.
 *   status 2 = no row, more than max_rows rows, a label outside [0, n_classes), a row outside [0, n_rows) or fewer than two classes
 *              with a row: d_info = {2, 0, 0, 0}, nothing else is written for the problem by any of the calls and no bank row of it
 *              is read.  Neighbouring problems are not affected.
 * max_rows in [1, MKWS_SVC_MAX_ROWS]: the caller's bound on the rows of one problem (it sizes the workspace and the grids).
 * standardize other than 0 / 1 and a gamma that is not finite are refused. */
int mkws_svc_prepare(const float* d_x, int n_rows, int dim, const int32_t* d_rows, const int32_t* d_labels, const int32_t* d_offsets,
                     int n_problems, int n_classes, int max_rows, int standardize, double gamma, float* d_centre, float* d_inv_scale,
                     float* d_gamma, int32_t* d_info, float* d_gap, void* stream);

/* The RBF cross-kernel of two gathered row lists per problem: for a in list A_p and b in list B_p
 *     d_out[p * out_stride + a * nb_p + b] = (float)exp(-gamma_p * max(0, s_a + s_b - 2 a~.b~)),
 * a~.b~ on the 16x16x4 fp32 matrix instruction (a float32 fused-multiply-add chain per 16 columns, the chains added in float64), the
 * operands gathered, centred and scaled in float32 as they are staged through LDS, s the float64 sums of squares of the same staged
 * values, the distance and the device library's exp in float64, rounded once.  NaN where a row is outside [0, n_rows) (never
 * dereferenced).  max_a / max_b: the caller's bounds on the list lengths (they size the grid; a problem whose lists are longer, or
 * whose na * nb exceeds out_stride, is skipped); out_stride >= max_a * max_b floats.  d_info (may be NULL): int32 [n_problems, 4]; a
 * problem whose first word is not 0 is skipped. */
int mkws_svc_kernel(const float* d_x, int n_rows, int dim, const int32_t* d_rows_a, const int32_t* d_offsets_a, int max_a,
                    const int32_t* d_rows_b, const int32_t* d_offsets_b, int max_b, int n_problems, const float* d_centre,
                    const float* d_inv_scale, const float* d_gamma, const int32_t* d_info, float* d_out, size_t out_stride, void* stream);

/* SMO on the Gram matrices d_gram (problem p: n_p x n_p floats at p * gram_stride, as mkws_svc_kernel wrote them), one workgroup per
 * (problem, pair of classes): libsvm's second-order working-set selection (the later index on ties), clipping and TAU guard, no
 * shrinking, until m(alpha) - M(alpha) < tol or max_iter iterations.  alpha and the gradient are float64, the kernel values float32.
 * d_C double [n_problems].  d_coef float32 [list entries, n_classes - 1]: entry t's alpha_t y_t in the machine against the m-th other
 * class in ascending order (libsvm's dual_coef_, aligned with the flat row list); d_rho float32 [n_problems, n_classes (n_classes-1)/2],
 * pairs in the order (0,1), (0,2), ...; a pair with an absent class gets zero coefficients and rho = 0.  d_info (from mkws_svc_prepare)
 * gains {., ., pairs cut at max_iter, the largest iteration count of a pair}, d_gap the largest final m - M of a pair.  A problem with
 * status 2 is skipped.  max_iter < 1, a NaN or negative tol and gram_stride < max_rows^2 are refused. */
int mkws_svc_fit(const int32_t* d_labels, const int32_t* d_offsets, int n_problems, int n_classes, int max_rows, const double* d_C,
                 double tol, int max_iter, const float* d_gram, size_t gram_stride, float* d_coef, float* d_rho, int32_t* d_info,
                 float* d_gap, void* stream);

/* Every problem scored on its OWN evaluation list (d_rows / d_true int32 [total], d_offsets int32 [n_problems+1]) under model p = its
 * training lists (d_train_*) and what the fit wrote.  The kernel values come from mkws_svc_kernel's device code (A = training rows,
 * B = evaluation rows); f_ij = (sum over class i's rows of coef * k + sum over class j's) - rho_ij in float32, the rows in list order;
 * f_ij > 0 votes i, otherwise j, over pairs of present classes; most votes wins, the lowest class on ties.  d_pred int32 [total];
 * d_correct int32 [n_problems] = entries with d_pred == d_true, zeroed by the call itself (integer adds); d_decision (optional, may be
 * NULL) float32 [total, n_classes (n_classes-1)/2], 0 for a pair with an absent class.  An entry outside every list, a row outside
 * [0, n_rows) and every entry of a problem whose d_info (optional) says status != 0 get d_pred = -1 and NaN decision values, are never
 * dereferenced and not counted.  max_train / max_eval: the caller's bounds on the list lengths (a longer list is not scored). */
int mkws_svc_score(const float* d_x, int n_rows, int dim, const int32_t* d_train_rows, const int32_t* d_train_labels,
                   const int32_t* d_train_offsets, int max_train, const float* d_coef, const float* d_rho, const float* d_gamma,
                   const float* d_centre, const float* d_inv_scale, const int32_t* d_info, int n_problems, int n_classes,
                   const int32_t* d_rows, const int32_t* d_true, const int32_t* d_offsets, int total, int max_eval, int32_t* d_pred,
                   int32_t* d_correct, float* d_decision, void* stream);

/* SVC(probability=True), given the folds (multilingual_kws_amd/svc.py: cv_folds, cv_decision_host, platt_host, couple_host).  The same
 * conventions as the four calls above. */
#define MKWS_SVC_MAX_FOLDS 16

/* The cross-validated decision values, on the Gram matrices of mkws_svc_kernel and with the SMO of mkws_svc_fit, one workgroup per
 * (problem, pair, fold): d_folds int32 [list entries] in [0, n_folds), n_folds in [2, MKWS_SVC_MAX_FOLDS].  d_cv_decision float32
 * [list entries, n_classes - 1], laid out as d_coef: entry t against its m-th other class holds f_ij(x_t) (positive means the lower
 * class i) of the pair's machine trained on the pair's entries of the other folds; where those hold no entry of either class 0, only
 * class i's +1, only class j's -1 (libsvm's svm_binary_svc_probability); 0 where the other class is absent from the problem.  d_info
 * (from mkws_svc_prepare) is read only.  d_cv_info int32 [n_problems, 4], zeroed by the call itself = {status, sub-fits solved,
 * sub-fits cut at max_iter, the largest iteration count of a sub-fit}; status 2 = the problem's d_info status is not 0, or one of its
 * fold values is outside [0, n_folds): nothing is written to d_cv_decision for it. */
int mkws_svc_fit_cv(const int32_t* d_labels, const int32_t* d_offsets, const int32_t* d_folds, int n_folds, int n_problems, int n_classes,
                    int max_rows, const double* d_C, double tol, int max_iter, const float* d_gram, size_t gram_stride,
                    const int32_t* d_info, float* d_cv_decision, int32_t* d_cv_info, void* stream);

/* Platt's sigmoids, one wave per (problem, pair): (A, B) minimising sum t z + log(1 + exp(-z)), z = A f + B, over the pair's entries of
 * d_cv_decision (class i is +1; targets (N+ + 1) / (N+ + 2) and 1 / (N- + 2)), by Newton steps from (0, log((N- + 1) / (N+ + 1))) with
 * a ridge of 1e-12, at most 100 iterations of at most 10 halvings, in float64, until |gradient|_inf < eps.  d_probA / d_probB double
 * [n_problems, n_classes (n_classes - 1) / 2], both 0 for a pair with an absent class; d_present (optional, may be NULL) int32
 * [n_problems]: bit k set where class k has an entry.  d_info / d_cv_info (optional, may be NULL): a problem whose first word in
 * either is not 0 is skipped and nothing is written for it; so is one of more than max_rows entries. */
int mkws_svc_platt(const int32_t* d_labels, const int32_t* d_offsets, int n_problems, int n_classes, int max_rows, const float* d_cv_decision,
                   const int32_t* d_info, const int32_t* d_cv_info, double eps, double* d_probA, double* d_probB, int32_t* d_present,
                   void* stream);

/* Pairwise coupling, a thread per evaluation entry (its problem by bisection of d_offsets): d_decision float32 [total, pairs] as
 * mkws_svc_score writes it; r_ij = 1 / (1 + exp(A_ij f_ij + B_ij)) clipped to [1e-7, 1 - 1e-7] over the classes of d_present[p];
 * p = argmin sum_i sum_{j != i} (r_ji p_i - r_ij p_j)^2 with sum p = 1 (Wu, Lin and Weng 2004, method 2), solved directly in float64.
 * d_probs float32 [total, n_classes], 0 for an absent class; d_pred = its first argmax; d_correct int32 [n_problems] = entries with
 * d_pred == d_true, zeroed by the call itself (integer adds).  An entry outside every list, one with a NaN decision value and one whose
 * problem has fewer than two present classes keep NaN probabilities and d_pred = -1. */
int mkws_svc_couple(const float* d_decision, const int32_t* d_true, const int32_t* d_offsets, int n_problems, int n_classes, int total,
                    const double* d_probA, const double* d_probB, const int32_t* d_present, float* d_probs, int32_t* d_pred,
                    int32_t* d_correct, void* stream);

/* The soft vote of two classifiers: d_pred int32 [total] = the first argmax over the classes of 0.5f * (a + b) in float32 for two
 * probability arrays float32 [total, n_classes]; d_correct as above; d_mean (optional, may be NULL) float32 [total, n_classes] = that
 * mean.  An entry outside every list or with a NaN in either row gets d_pred = -1 and is not counted. */
int mkws_soft_vote(const float* d_probs_a, const float* d_probs_b, const int32_t* d_true, const int32_t* d_offsets, int n_problems,
                   int n_classes, int total, int32_t* d_pred, int32_t* d_correct, float* d_mean, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training-batch assembly.  Replaces the per-clip tf.data map of AudioDataset.augment /
 * random_timeshift / random_background_sample / add_background
 * (multilingual_kws/embedding/input_data.py:141-157,227-304) and spec_augment (:306-369).
 * The random draws are made by the host (one item per clip); the sample-level work runs on device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mkws_augment_item {
  int32_t mode;     /* 0: out = shift(fg)            (random_timeshift, :245-268)
                       1: out = bg_slice * bg_vol    (silence branch, :284-287 / :227-243)
                       2: out = clip(shift(fg) + bg_slice * (rms(shift(fg))/rms(bg_slice) or 0) * bg_vol, -1, 1)
                          (add_background, :141-157): both RMS values are taken over exactly the n_samples of the
                          SHIFTED clip and of the slice; the ratio is 0 where rms(bg_slice) is 0 */
  int32_t bank;     /* foreground bank: 0 = d_bank0 (target clips), 1 = d_bank1 (unknown-word clips) */
  int32_t src;      /* row of the foreground clip in that bank */
  int32_t shift;    /* out[t] = fg[t - shift], zero-filled (positive = delay); |shift| >= n_samples yields zeros */
  int32_t bg_idx;   /* background track */
  int32_t bg_off;   /* first sample of the n_samples-long background slice */
  float bg_vol;
  int32_t reserved;
} mkws_augment_item;

/* d_bank0 [n0, n_samples], d_bank1 [n1, n_samples] (may be NULL when no item names bank 1), d_bg [tracks, bg_stride] float32;
 * d_items [B]; d_out [B, n_samples].  d_bg may be NULL (with any bg_stride) only if EVERY item is mode 0: a mode 1 or mode 2 item
 * reads its slice unconditionally.  The kernel checks nothing an item says: `src` must be a row of its bank, and
 * [bg_off, bg_off + n_samples) must lie inside track `bg_idx` -- the slice may end on the track's last sample, and neither the rows
 * nor bg_stride need any alignment beyond that of a float.  Nothing outside d_out [B, n_samples] is written.  B == 0 returns MKWS_OK
 * with nothing launched; MKWS_ERR_INVALID_ARG for B < 0, n_samples <= 0 and a NULL d_bank0, d_items or d_out.
 * (The cases: tests/util_assembly_cases.py.) */
int mkws_augment_batch(const float* d_bank0, const float* d_bank1, const float* d_bg, int64_t bg_stride,
                       const mkws_augment_item* d_items, int B, int n_samples, float* d_out, void* stream);
/* SpecAugment masking in place on d_spec [B, frames, channels]; d_masks int32 [B,8] =
 * {freq0 start, size, freq1 start, size, time0 start, size, time1 start, size}: element (frame f, channel c) is set to zero iff
 * some freq mask has start <= c < start + size or some time mask has start <= f < start + size.  The masks are intersected with the
 * image: a negative start and a mask that hangs over the last channel / frame are allowed, size <= 0 = no mask; every other element
 * keeps its bits.  MKWS_ERR_INVALID_ARG for B < 0, frames <= 0, channels <= 0 and (B > 0) NULL buffers. */
int mkws_specaug_apply(float* d_spec, const int32_t* d_masks, int B, int frames, int channels, void* stream);
/* The same with ANY number of masks per axis (the reference loops frequency_n / time_n times for whatever SpecAugParams says,
 * input_data.py:317-362): d_masks int32 [B, 2*(n_freq + n_time)] = n_freq x {channel start, size} then n_time x {frame start, size};
 * the same mask semantics, and (2, 2) is mkws_specaug_apply's table byte for byte.  Negative counts are MKWS_ERR_INVALID_ARG;
 * n_freq + n_time == 0 returns MKWS_OK with nothing launched (d_masks may then be NULL). */
int mkws_specaug_apply_n(float* d_spec, const int32_t* d_masks, int n_freq, int n_time, int B, int frames, int channels, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training operators for `backprop_into_embedding=True` (multilingual_kws/embedding/transfer_learning.py:94-112).
 * The reference un-freezes the whole nested EfficientNet, so Keras runs xfer.fit with training=True through
 * keras/applications/efficientnet.py: BatchNormalization on batch statistics (+ moving-average updates), per-block
 * drop-connect, gradients into every kernel / bias / gamma / beta, Adam.  Keras owns the graph there; here the tape
 * is host code (multilingual_kws_amd/embedding_trainer.py) and each numerical operator is one entry point below.
 * All tensors are device float32, NHWC viewed as row-major [M, C]; parameters keep their Keras layouts (1x1 conv
 * kernel = [K, N], depthwise [kh, kw, C], dense [in, out]).  `act`: 0 none, 1 swish, 2 relu, 3 selu, 4 sigmoid.
 * Cross-workgroup reductions are two-level and FIXED-ORDER (partial sums in a caller-provided scratch arena, folded in index
 * order by a second launch): no atomics, a step with the same inputs is bit-reproducible.
 * ---------------------------------------------------------------------------------------------- */
/* State of the training operators = a CONTEXT: the scratch arena (device memory, caller-owned) for those partial sums and the queue of
 * deferred second stages (mkws_op_fold_defer).  16 Mi floats cover every layer of the network at any batch (the largest user is the
 * split reduction of mkws_op_gemm, which splits only as far as the arena reaches); ops that need the arena fail with
 * MKWS_ERR_INVALID_ARG when it is missing or too small.  A context is used in stream order (ops on ONE stream share it safely; give
 * concurrent streams separate contexts).
 * The arena contract (tests/test_train_arena_gpu.py, tests/test_train_arena_cpu.py):
 *   - a refused call has launched nothing: an operator works out every arena need of the call before its first launch, so
 *     MKWS_ERR_INVALID_ARG leaves every output buffer as it was.  mkws_last_error() names the float count the call needs;
 *   - a call touches only the floats it asked for, starting past whatever queued folds (mkws_op_fold_defer) still hold;
 *   - results do not depend on what the arena held before: every slot a second stage reads was written by its first stage;
 *   - the arena size selects a route in two places, both functions of the shapes and the size only: the automatic split of mkws_op_gemm
 *     (ksplit = 0; never refused -- without an arena it does not split), and mkws_op_conv_bn_fwd, whose fused route (statistics in the GEMM
 *     epilogue) takes ceil(M / 64) * 2 * N floats and whose three-launch sequence takes min(ceil(M / 128), bn_chunk_cap) * 2 * N, never more:
 *     an arena that holds only the latter runs the sequence (equal up to fp32 summation order), one that holds neither is refused.
 *   mkws_train_ctx_create / _destroy   a context handle owning nothing but its bookkeeping (the arena stays the caller's)
 *   mkws_train_ctx_bind(ctx)           every mkws_op_* call of THIS host thread uses ctx until another bind; NULL = the thread's default
 *                                      context.  Distinct contexts are independent: two trainers on one thread each bind their own before
 *                                      their calls, a trainer handed to another thread binds there and finds its queue as it left it.
 *   mkws_op_set_scratch                the thread's DEFAULT context (rounds 2-3 interface): sets its arena and binds it. */
typedef struct mkws_train_ctx mkws_train_ctx;
int mkws_train_ctx_create(float* d_scratch, size_t floats, mkws_train_ctx** out);
void mkws_train_ctx_destroy(mkws_train_ctx* ctx);
int mkws_train_ctx_bind(mkws_train_ctx* ctx);
int mkws_op_set_scratch(float* d_scratch, size_t floats);
/* C[M,N] (+)= op(A)[M,K] . op(B)[K,N] on the fp32 MFMA; op(A)(m,k) = transA ? A[k*lda+m] : A[m*lda+k], likewise B.
 * ksplit > 1 splits K over workgroups (slice sums go to the scratch arena, a second launch folds them in order into C);
 * ksplit = 0 picks the split from the shapes and the arena size (small grids with a long K: ~512 workgroups). */
int mkws_op_gemm(const float* d_A, const float* d_B, float* d_C, int M, int N, int K, int lda, int ldb, int ldc, int transA, int transB,
                 int accumulate, int ksplit, void* stream);
/* Process-wide switches of the training operators (ABI 5; A/B aids, results equal up to fp32 summation order):
 *   "gemm_ring"    (default 1; initial value from MKWS_TRAIN_GEMM2): NN / NT GEMMs whose K, N and leading dimensions are multiples of 4 run on the
 *                  register-ring kernel (operands global / L2 -> registers through buffer loads, no LDS, no barriers: the scheme of the inference
 *                  GEMM); 0 = the LDS-staged kernel for everything.
 *   "gemm_ring_tn" (default 0; MKWS_TRAIN_GEMM_TN2): the same for weight gradients (transA = 1): 0 none, 1 small outputs over >= 4096 rows, 2 all.
 *                  Faster per launch and in a single-stream step, slower inside the trainer's two-stream step (profiles/r05_notes.md).
 * mkws_op_get_option returns the value, or a negative mkws_status for an unknown name.
 * mkws_op_get_option also answers the launch constants the operators route by -- read-only: mkws_op_set_option on one of these names
 * fails with MKWS_ERR_INVALID_ARG.  Tests take their shapes from them, so that a retune moves the tests along with the routes:
 *   "bn_small_rows"      (1024) mkws_op_bn_act_bwd(_ex): up to this many rows both backward steps are one launch, above it two
 *   "bn_chunk_cap"       (128)  row chunks of the BatchNorm statistics / backward-reduce launches: 128 rows each up to cap * 128 rows, even shares above
 *   "bn_apply_chunk_cap" (256)  the same for the normalise / backward-apply launches
 *   "bn_max_chunks"      (256)  mkws_op_dwconv_bn_fwd: up to this many chunks of 128 output rows the convolution leaves the chunk statistics itself
 *   "bn_max_gemm_tiles"  (160)  mkws_op_conv_bn_fwd: the same for the GEMM's 64-row tiles
 *   "grid_cap"           (8192) workgroups (256 elements each) of an elementwise launch; larger tensors are walked by grid-stride loops */
int mkws_op_set_option(const char* name, int value);
int mkws_op_get_option(const char* name);
/* Stream ordering for a trainer that spreads its launches over two streams (weight gradients next to the input-gradient chain): everything queued
 * on signalling_stream so far happens before whatever is queued on waiting_stream afterwards.  Events belong to the bound context.  Capturable. */
int mkws_op_stream_wait(void* waiting_stream, void* signalling_stream);
/* Deferred second stages.  With enable = 1 the fixed-order folds whose results only the optimizer (or a gradient all-reduce) reads -- the
 * split reduction of a weight-gradient GEMM (transA = 1), the bias gradient of mkws_op_bias_act_bwd, the weight gradients of
 * mkws_op_dwconv_bwd / mkws_op_stem_bwd_weight / mkws_op_se_wgrad (batches above 64 rows) -- are QUEUED (their partial sums stay in the scratch arena, handed out from a bump pointer)
 * and run as ONE launch at mkws_op_fold_flush, at enable = 0, or when the queue (24 entries) or the arena is full.  Same sums in the same
 * order: bit-identical results, ~90 launches fewer per training step.  Until the flush those outputs are not final.  Per host thread, like
 * the scratch arena; capturable. */
int mkws_op_fold_defer(int enable, void* stream);
int mkws_op_fold_flush(void* stream);
/* Dense / SE layer forward in one call: Z = X[M,K] . W[K,N] (kept: the backward pass differentiates the activation at Z + bias) and
 * A = act(Z + bias), the epilogue fused into the GEMM (or into its split-reduction fold). */
int mkws_op_dense_fwd(const float* d_X, const float* d_W, const float* d_bias, int act, float* d_Z, float* d_A, int M, int N, int K, void* stream);
/* Batch statistics of Z [M,C] per channel: mean, biased variance (per-chunk mean / M2, combined with Chan's update). */
int mkws_op_bn_stats(const float* d_Z, int M, int C, float* d_mean, float* d_var, void* stream);
/* Training-mode BatchNormalization forward in two launches: chunk statistics, then (fold of the chunks +) moving-average update
 * (moving = momentum * moving + (1 - momentum) * batch, variance Bessel-corrected) + A = act(gamma * xhat + beta).
 * d_mean / d_var receive the batch statistics the backward pass needs. */
int mkws_op_bn_train_fwd(const float* d_Z, int M, int C, const float* d_gamma, const float* d_beta, float eps, int act, float momentum,
                         float* d_moving_mean, float* d_moving_var, float* d_mean, float* d_var, float* d_A, void* stream);
/* The same with the residual branch of an MBConv block in the second launch (reference: the `layers.add([x, inputs])` behind Keras'
 * drop-connect Dropout(noise_shape=(None,1,1,1)), train_multilingual_embedding.py:58-83 via keras/applications/efficientnet.py):
 * A[r] = keep[r / group] * act(BN(Z)[r]) + d_res[r];  d_row_scale may be NULL (keep = 1), d_res NULL = plain mkws_op_bn_train_fwd. */
int mkws_op_bn_train_fwd_res(const float* d_Z, int M, int C, const float* d_gamma, const float* d_beta, float eps, int act, float momentum,
                             float* d_moving_mean, float* d_moving_var, float* d_mean, float* d_var, float* d_A, const float* d_res,
                             const float* d_row_scale, int group, void* stream);
/* A = act(gamma * (Z - mean) / sqrt(var + eps) + beta) */
int mkws_op_bn_act_fwd(const float* d_Z, const float* d_mean, const float* d_var, const float* d_gamma, const float* d_beta, float eps, int act,
                       float* d_A, int M, int C, void* stream);
/* Backward of the above through the batch statistics: d_dA [M,C] holds dLoss/dA on entry and dLoss/dZ on return;
 * d_dgamma / d_dbeta [C] are written; d_scratch: 2*C floats. */
int mkws_op_bn_act_bwd(const float* d_Z, const float* d_mean, const float* d_var, const float* d_gamma, const float* d_beta, float eps, int act,
                       float* d_dA, float* d_dgamma, float* d_dbeta, float* d_scratch, int M, int C, void* stream);
/* The same with the incoming gradient assembled on the fly (saves the launches that used to build it):
 *   dLoss/dA[r] = d_src[r] * d_row_scale[r / group] + d_bcast[r / group][:] * bscale      (each term optional; at least one of src / bcast)
 * e.g. the drop-connect scale of a residual block (src = gradient of the block output, kept intact for the shortcut), or the squeeze-excite
 * mean's gradient broadcast over the pixels (src = d_dA, bcast = dLoss/dmean, bscale = 1 / HW).  d_dA receives dLoss/dZ. */
int mkws_op_bn_act_bwd_ex(const float* d_Z, const float* d_mean, const float* d_var, const float* d_gamma, const float* d_beta, float eps, int act,
                          float* d_dA, const float* d_src, const float* d_row_scale, const float* d_bcast, float bscale, int group, float* d_dgamma,
                          float* d_dbeta, int M, int C, void* stream);
/* moving = momentum * moving + (1 - momentum) * batch; the variance enters Bessel-corrected (M/(M-1)) as in Keras' fused BN. */
int mkws_op_bn_update_moving(float* d_moving_mean, float* d_moving_var, const float* d_mean, const float* d_var, float momentum, int M, int C, void* stream);
/* 1x1 convolution Z [M,N] = X [M,K] W [K,N] followed by training-mode BatchNorm (+ activation, + residual branch) -- mkws_op_gemm +
 * mkws_op_bn_train_fwd_res as ONE operator, so that the GEMM's epilogue can leave the BatchNorm's chunk statistics (one chunk per 64-row tile)
 * when it is unsplit and has at most 160 row tiles: two launches instead of three and one pass less over Z.  Same arguments and results
 * (statistics up to summation order) as the two calls; Z keeps the raw convolution output for the backward pass. */
int mkws_op_conv_bn_fwd(const float* d_X, const float* d_W, float* d_Z, int M, int N, int K, const float* d_gamma, const float* d_beta, float eps, int act,
                        float momentum, float* d_moving_mean, float* d_moving_var, float* d_mean, float* d_var, float* d_A, const float* d_res,
                        const float* d_row_scale, int group, void* stream);
/* The same for the depthwise convolution (mkws_op_dwconv_fwd + mkws_op_bn_train_fwd): up to 256 chunks of 128 output rows the convolution launch
 * leaves the chunk statistics itself. */
int mkws_op_dwconv_bn_fwd(const float* d_X, const float* d_W, float* d_Z, int B, int H, int W, int C, int k, int stride, int pad_top, int pad_left, int Ho, int Wo,
                          const float* d_gamma, const float* d_beta, float eps, int act, float momentum, float* d_moving_mean, float* d_moving_var, float* d_mean,
                          float* d_var, float* d_A, void* stream);
/* Depthwise k x k conv (k = 3, 5; stride 1, 2) with explicit top / left padding (Keras "same" or correct_pad), raw output. */
int mkws_op_dwconv_fwd(const float* d_X, const float* d_W, float* d_Z, int B, int H, int W, int C, int k, int stride, int pad_top, int pad_left, int Ho,
                       int Wo, void* stream);
/* d_dX (may be NULL) <- input gradient, d_dW [k,k,C] (may be NULL; not both) <- weight gradient: two calls may split them over two streams. */
int mkws_op_dwconv_bwd(const float* d_X, const float* d_W, const float* d_dZ, float* d_dX, float* d_dW, int B, int H, int W, int C, int k, int stride,
                       int pad_top, int pad_left, int Ho, int Wo, void* stream);
/* Stem: Rescaling(1/255) + Normalization + ZeroPadding2D(((1,1),(0,1))) + Conv2D(32,3,s2,valid) on [B,49,40] -> raw [B,25,20,32]. */
int mkws_op_stem_fwd(const float* d_spec, const float* d_W, float norm_mean, float norm_std, float* d_Z, int B, void* stream);
int mkws_op_stem_bwd_weight(const float* d_spec, const float* d_dZ, float norm_mean, float norm_std, float* d_dW, int B, void* stream);
/* mean over HW: A [B,HW,C] -> [B,C] */
int mkws_op_pool_hw(const float* d_A, float* d_mean, int B, int HW, int C, void* stream);
/* out[b,hw,c] = A[b,hw,c] * g[b,c]   (SE excite) */
int mkws_op_scale_channels(const float* d_A, const float* d_g, float* d_out, int B, int HW, int C, void* stream);
/* backward of the excite multiply: dA = dOut * g,  dg[b,c] = sum_hw dOut * A */
int mkws_op_se_bwd(const float* d_A, const float* d_g, const float* d_dOut, float* d_dA, float* d_dg, int B, int HW, int C, void* stream);
/* The squeeze-excite branch of one MBConv block (Keras: GlobalAveragePooling2D -> Conv2D(se, swish) -> Conv2D(C, sigmoid) -> multiply) in two
 * launches, one workgroup per (clip, 128-channel slab):  mean [B,C] = pool(A [B,HW,C]);  Yr [B,se] = mean Wr + br;  R = swish(Yr);
 * G [B,C] = sigmoid(R We + be);  out = A * G.  Wr [C,se], We [se,C] are the Keras 1x1 kernels.  C % 4 == 0, C <= 1152, se <= 48.
 * d_work: B * ceil(C / 128) * se floats of scratch (the per-slab partial sums; folded in slab order).  Same results as pool_hw + dense_fwd x 2 +
 * scale_channels up to summation order. */
int mkws_op_se_fwd(const float* d_A, const float* d_Wr, const float* d_br, const float* d_We, const float* d_be, float* d_mean, float* d_Yr, float* d_R, float* d_G,
                   float* d_out, float* d_work, int B, int HW, int C, int se, void* stream);
/* Its backward in three launches: given dOut = dLoss/d(out):  dA = dOut * G (the multiply's direct path; the squeeze's path comes back as dmean [B,C]
 * = dLoss/d(mean), which mkws_op_bn_act_bwd_ex spreads over the pixels), and the gradients of the four parameter tensors (written, not accumulated;
 * batch sums in row order).  dYg [B,C] / dYr [B,se] are outputs too (the pre-activation gradients); d_work as above. */
int mkws_op_se_bwd_fused(const float* d_A, const float* d_G, const float* d_dOut, const float* d_mean, const float* d_Yr, const float* d_R, const float* d_Wr,
                         const float* d_We, float* d_dA, float* d_dmean, float* d_dYg, float* d_dYr, float* d_dWr, float* d_dbr, float* d_dWe, float* d_dbe,
                         float* d_work, int B, int HW, int C, int se, void* stream);
/* The parameter-gradient launch alone (mkws_op_se_bwd_fused with the four gradient pointers NULL skips it): nothing downstream waits for it, so a
 * trainer may run it on a second stream next to the input-gradient chain.  Batches above 64 rows are summed in chunks of 64 rows whose partial
 * sums (context scratch arena) are folded in chunk order -- deferrable like the other weight-gradient folds (mkws_op_fold_defer). */
int mkws_op_se_wgrad(const float* d_mean, const float* d_R, const float* d_dYg, const float* d_dYr, float* d_dWr, float* d_dbr, float* d_dWe, float* d_dbe, int B,
                     int C, int se, void* stream);
/* X[b,hw,c] += v[b,c] * scale   (backward of a mean over HW) */
int mkws_op_add_bcast(float* d_X, const float* d_v, float scale, int B, int HW, int C, void* stream);
/* A = act(Z + bias);  backward: d_dA <- dA * act'(Z + bias) in place, d_dbias [N] <- its column sums */
int mkws_op_bias_act_fwd(const float* d_Z, const float* d_bias, int act, float* d_A, int M, int N, void* stream);
int mkws_op_bias_act_bwd(const float* d_Z, const float* d_bias, int act, float* d_dA, float* d_dbias, int M, int N, void* stream);
/* out[b,:] = a[b,:] * row_scale[b] (+ c[b,:] if c != NULL): drop-connect (keep / (1 - rate)) + residual add, and its backward */
int mkws_op_row_scale_add(const float* d_a, const float* d_row_scale, const float* d_c, float* d_out, int B, int64_t per_row, void* stream);
int mkws_op_axpy(float* d_y, const float* d_x, float alpha, int64_t n, void* stream);
/* Keras Adam over a flat buffer (same arithmetic as mkws_head_adam_step). */
int mkws_op_adam(float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps, int step_t,
                 float grad_scale, void* stream);
/* Sparse categorical cross-entropy from logits over N classes (the classifier the reference trains the embedding with,
 * train_multilingual_embedding.py:84-93): d_logits [B,N] is overwritten with d(mean loss)/d(logits); d_rowstat [B,2] receives
 * {-log softmax(z)[y], argmax(z) == y} per row and d_stats [2] their sums (rows folded in index order). */
int mkws_op_softmax_ce(float* d_logits, const int32_t* d_labels, int B, int N, float* d_rowstat, float* d_stats, void* stream);
/* Graph-replayable form: the step index lives in device memory.  mkws_op_step_inc adds 1 to *d_step (once per optimizer step,
 * before the Adam launches that share the counter); mkws_op_adam_dev computes lr_t from *d_step on the device. */
int mkws_op_step_inc(int* d_step, void* stream);
int mkws_op_adam_dev(float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                     const int* d_step, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DS-CNN baseline, inference: the MLPerf-Tiny keyword spotter the reference measures the few-shot models against
 * (notebooks/dscnn_comparison.py:45-102 model_def).  Input [B,49,40] float32 micro-frontend features, no rescaling.
 *   stem    Conv2D(64, 10x4, stride 2, SAME: pad top 4 / bottom 5 / left 1 / right 1) + bias, BN (eps 1e-3), ReLU  -> [25,20,64]
 *   4 x     DepthwiseConv2D(3x3, SAME) + bias, BN, ReLU;  Conv2D(64, 1x1) + bias, BN, ReLU                          -> [25,20,64]
 *   pool    mean over rows 0..23 (AveragePooling2D (24,20), valid: row 24 is computed and NOT pooled)                -> [64]
 *   dense   Dense(label_count) + bias, softmax
 * The parameter blob is float32 in Keras variable order and layout, BatchNorm tensors included (mkws_dscnn_weight_manifest);
 * create folds every BatchNorm into the convolution before it (float64, rounded once to float32), the device holds folded weights only.
 * One launch per forward: a workgroup keeps a clip's activation in LDS through all nine layers.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mkws_dscnn mkws_dscnn;

/* 24128 + 65 * label_count; 0 for a label_count outside [2, 64]. */
size_t mkws_dscnn_param_count(int label_count);
/* JSON {"tensors": [{name, shape, offset, count}]} as mkws_embed_weight_manifest; returns the length needed (without the NUL), or
 * MKWS_ERR_INVALID_ARG for a label_count outside [2, 64].  Host only. */
int mkws_dscnn_weight_manifest(int label_count, char* buf, size_t buf_len);
/* MKWS_ERR_BAD_WEIGHTS for a label_count outside [2, 64], n_floats != mkws_dscnn_param_count(label_count), a non-finite value or a
 * moving variance below -eps -- all before a device is looked for; then MKWS_ERR_NO_DEVICE without a gfx950. */
int mkws_dscnn_create(const float* h_params, size_t n_floats, int label_count, int max_batch, mkws_dscnn** out);
void mkws_dscnn_destroy(mkws_dscnn* h);
/* Workgroups a forward launches at most; a workgroup takes clips blockIdx, blockIdx + grid, ... */
int mkws_dscnn_grid(const mkws_dscnn* h);
/* d_spec [B,49,40] -> d_probs [B,label_count] (softmax) and, unless NULL, d_logits [B,label_count].  Asynchronous on `stream`, one
 * launch, allocates nothing: capturable.  B == 0 succeeds with nothing launched; B > max_batch is MKWS_ERR_INVALID_ARG. */
int mkws_dscnn_forward(mkws_dscnn* h, const float* d_spec, int B, float* d_probs, float* d_logits, void* stream);
/* The same kernel with one store added: stage 0 = stem, 1..4 = the blocks, each d_out [B,25,20,64] after its last ReLU; stage 5 =
 * the pooled [B,64]. */
int mkws_dscnn_tap(mkws_dscnn* h, const float* d_spec, int B, int stage, float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DS-CNN baseline, training: what one optimizer step of the network above needs beyond the mkws_op_* operators (the reference's
 * train(), notebooks/dscnn_comparison.py:147-195; the tape is multilingual_kws_amd/dscnn_trainer.py).  Same conventions as those
 * operators: device float32, NHWC viewed as [M, C], Keras layouts, asynchronous on `stream`, no allocation and no synchronisation
 * (capturable), cross-workgroup sums two-level and in index order through the bound context's scratch arena (bit-reproducible).
 * ---------------------------------------------------------------------------------------------- */
/* Raw Conv2D(64, (10,4), strides 2, SAME: pad top 4 / bottom 5 / left 1 / right 1) without bias: d_spec [B,49,40], d_W [10,4,1,64]
 * -> d_Z [B,25,20,64], on the fp32 MFMA with the patches gathered on the fly.  BatchNorm + ReLU follow through mkws_op_bn_train_fwd. */
int mkws_op_dscnn_stem_fwd(const float* d_spec, const float* d_W, float* d_Z, int B, void* stream);
/* d_dW [40,64] = patches^T . d_dZ [B,25,20,64] (written, not accumulated).  Needs up to 256 * 2560 floats of the scratch arena; folded at once
 * (it does not join the mkws_op_fold_defer queue). */
int mkws_op_dscnn_stem_bwd_weight(const float* d_spec, const float* d_dZ, float* d_dW, int B, void* stream);
/* Dropout without a stored mask: element i is kept when the top 24 bits of splitmix64(base + (i + 1) * 0x9E3779B97F4A7C15) are at least
 * floor(rate * 2^24), base = splitmix64(splitmix64(splitmix64(seed) + *d_step) + site); kept values are multiplied by the float32
 * 1 / (1 - rate), the others are zero.  0 <= rate < 1; rate = 0 is the identity.  *d_step is the device counter mkws_op_step_inc
 * advances, so a captured step draws a fresh mask on every replay; the backward pass is the same launch on the gradient.  In place
 * (d_out == d_X) is allowed.  dscnn_trainer.dropout_mask_host reproduces the bits on the host. */
int mkws_op_dropout_fwd(const float* d_X, float* d_out, int64_t n, float rate, uint64_t seed, const int* d_step, int site, void* stream);
int mkws_op_dropout_bwd(const float* d_dOut, float* d_dX, int64_t n, float rate, uint64_t seed, const int* d_step, int site, void* stream);
/* Dropout (mask index = the element's index in d_A [B,25,20,64]) fused with the mean over rows 0..23 (480 cells) -> d_pooled [B,64];
 * the backward writes mask * (1 / (1 - rate) / 480) * d_dpooled into rows 0..23 of d_dA and exact zeros into row 24 (16-byte aligned). */
int mkws_op_dscnn_pool_fwd(const float* d_A, int B, float rate, uint64_t seed, const int* d_step, int site, float* d_pooled, void* stream);
int mkws_op_dscnn_pool_bwd(const float* d_dpooled, int B, float rate, uint64_t seed, const int* d_step, int site, float* d_dA, void* stream);

/* ------------------------------------------------------------------------------------------------
 * wav2vec 2.0 baseline, inference: the encoder the reference uses as a clip embedding (notebooks/dataperf_wav2vec2.py:43-58:
 * Wav2Vec2Processor + Wav2Vec2Model, last hidden state max-pooled over time).  Driven by a configuration; float32 throughout.
 *   0  processor   per clip x <- (x - mean) / sqrt(var + 1e-7), population variance (switchable)
 *   1  encoder     seven valid 1-D convolutions without bias, kernels (10,3,3,3,3,2,2), strides (5,2,2,2,2,2,2); layer 0 is followed by a
 *                  GroupNorm with one group per channel (statistics over the clip's T_0 positions, eps 1e-5, affine); every layer ends
 *                  in the exact GELU.  T_i = (T_{i-1} - k_i) / s_i + 1: 16000 samples -> 49 frames, 400 -> 1.
 *   2  projection  LayerNorm over conv_dim[6], Linear(conv_dim[6] -> H) with bias
 *   3  position    grouped convolution over time (H channels, G groups, kernel K, zero padding K / 2, exactly T outputs, bias; the
 *                  weight-normalised kernel g * v / ||v|| is folded at create in float64), GELU, added to its input, LayerNorm
 *   4  layers      post-LN transformer layers: h = LN(h + Wo attention(h) + bo), h = LN(h + W2 GELU(W1 h + b1) + b2), attention over
 *                  all T frames without a mask, q scaled by head_dim^-0.5
 *   5  outputs     the last hidden state [B,T,H] and its maximum over the T frames [B,H]
 * The parameter blob is float32 with the names, layouts and order of Hugging Face's Wav2Vec2Model state dict, masked_spec_embed left
 * out (mkws_w2v2_weight_manifest).  All clips of a call have the same length.  The contractions run on the fp32 MFMA GEMM of
 * mkws_op_gemm (a long reduction split into slices that a second launch folds in slice order, through the handle's own buffer: no scratch
 * arena is involved); activations are channels-last, so a strided convolution is one GEMM over
 * overlapping row views of its input.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mkws_w2v2_cfg {
  int32_t conv_dim[7];
  int32_t conv_kernel[7];              /* (10,3,3,3,3,2,2): anything else is refused */
  int32_t conv_stride[7];              /* (5,2,2,2,2,2,2): anything else is refused */
  int32_t hidden_size;
  int32_t num_hidden_layers;
  int32_t num_attention_heads;         /* must divide hidden_size */
  int32_t intermediate_size;
  int32_t num_conv_pos_embeddings;     /* K */
  int32_t num_conv_pos_embedding_groups; /* G, must divide hidden_size */
  float layer_norm_eps;
  int32_t group_norm;                  /* 1: feat_extract_norm == "group" (the only supported value) */
  int32_t conv_bias;                   /* must be 0 */
  int32_t stable_layer_norm;           /* must be 0 */
  int32_t exact_gelu;                  /* 1: both activations are the exact GELU (the only supported value) */
} mkws_w2v2_cfg;
typedef struct mkws_w2v2 mkws_w2v2;

/* facebook/wav2vec2-base: conv_dim 512 x 7, H 768, 12 layers, 12 heads, FFN 3072, K 128, G 16, eps 1e-5. */
void mkws_w2v2_default_cfg(mkws_w2v2_cfg* cfg);
/* Floats of the blob; 0 for a configuration the build refuses (mkws_last_error says why).  Host only. */
size_t mkws_w2v2_param_count(const mkws_w2v2_cfg* cfg);
/* JSON {"tensors": [{name, shape, offset, count}]} in state-dict order; returns the length needed (without the NUL), or a negative
 * mkws_status for a refused configuration.  Host only. */
int mkws_w2v2_weight_manifest(const mkws_w2v2_cfg* cfg, char* buf, size_t buf_len);
/* Frames of a clip of n_samples; 0 or negative for an input shorter than 400 samples (and for a refused configuration).  Host only. */
int mkws_w2v2_num_frames(const mkws_w2v2_cfg* cfg, int n_samples);
/* MKWS_ERR_UNSUPPORTED / MKWS_ERR_INVALID_ARG for a refused configuration, max_batch < 1, max_samples < 400 and sizes beyond what one
 * handle addresses; MKWS_ERR_BAD_WEIGHTS for n_floats != mkws_w2v2_param_count(cfg), a non-finite value and a kernel position of the
 * positional convolution whose ||v|| is zero -- all before a device is looked for; then MKWS_ERR_NO_DEVICE without a gfx950.  Folds the
 * weight norm, re-lays the weights out for the kernels and allocates all workspace. */
int mkws_w2v2_create(const mkws_w2v2_cfg* cfg, const float* h_params, size_t n_floats, int max_batch, int max_samples, mkws_w2v2** out);
void mkws_w2v2_destroy(mkws_w2v2* h);
/* d_audio [B, n_samples] -> d_hidden [B,T,H] and / or d_embed [B,H] (either may be NULL, not both).  Asynchronous on `stream`, no
 * allocation and no synchronisation: capturable.  The same call twice gives the same bits.  B == 0 succeeds with nothing launched;
 * B > max_batch, n_samples > max_samples and n_samples < 400 are MKWS_ERR_INVALID_ARG. */
int mkws_w2v2_forward(mkws_w2v2* h, const float* d_audio, int B, int n_samples, int normalize, float* d_hidden, float* d_embed, void* stream);
/* The same chain stopped after `stage`, whose result goes to d_out: 0 the (normalised) audio [B,n]; 1..7 the convolution layers after
 * their GELU, [B,T_i,C_i] channels last; 8 the projection [B,T,H]; 9 positional convolution + LayerNorm; 10 + l transformer layer l. */
int mkws_w2v2_tap(mkws_w2v2* h, const float* d_audio, int B, int n_samples, int normalize, int stage, float* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MKWS_H_ */
