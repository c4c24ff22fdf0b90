// See mkws_spectral_tables.h.  The arithmetic restates TensorFlow's spectrogram.cc (periodic Hann), mfcc_mel_filterbank.cc (band mapper
// and weights) and mfcc_dct.cc, as include/mkws.h spells it out; everything is computed in double and rounded once to float.
#include "mkws_spectral_tables.h"

#include <cmath>

#include "mkws_common.h"

namespace mkws {
namespace {

const double kPi = 3.14159265358979323846;

double mel_of(double hz) { return 1127.0 * std::log1p(hz / 700.0); }

}  // namespace

int check_spectral_cfg(const mkws_spectral_cfg& c, int* fft_size, int* bins, int* width) {
  if (c.sample_rate < 1) return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: sample_rate %d must be positive", c.sample_rate);
  if (c.window_size_samples < 1) return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: window_size_samples %d must be positive", c.window_size_samples);
  if (c.window_stride_samples < 1) return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: window_stride_samples %d must be positive", c.window_stride_samples);
  int n = 1;
  while (n < c.window_size_samples && n < 2048) n <<= 1;
  if (n != 256 && n != 512 && n != 1024)
    return fail(MKWS_ERR_UNSUPPORTED, "spectral cfg: window_size_samples %d needs a %d-point FFT; 256, 512 and 1024 (windows of 129 .. 1024 samples) are implemented",
                c.window_size_samples, n);
  const int nb = n / 2 + 1;
  int w = 0;
  if (c.mode == MKWS_SPECTRAL_MFCC) {
    if (c.filterbank_channels < 1) return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: filterbank_channels %d must be positive", c.filterbank_channels);
    if (c.filterbank_channels > 64) return fail(MKWS_ERR_UNSUPPORTED, "spectral cfg: filterbank_channels %d > 64", c.filterbank_channels);
    if (c.num_features < 1 || c.num_features > c.filterbank_channels)
      return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: num_features %d must be in [1, filterbank_channels = %d]", c.num_features, c.filterbank_channels);
    if (!(c.lower_frequency_limit >= 0.0f) || !std::isfinite(c.lower_frequency_limit))
      return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: lower_frequency_limit %g must be finite and not negative", (double)c.lower_frequency_limit);
    if (!(c.upper_frequency_limit > c.lower_frequency_limit))
      return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: upper_frequency_limit %g must be above lower_frequency_limit %g", (double)c.upper_frequency_limit,
                  (double)c.lower_frequency_limit);
    if (!((double)c.upper_frequency_limit <= 0.5 * c.sample_rate))
      return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: upper_frequency_limit %g is above half the sample_rate %d", (double)c.upper_frequency_limit, c.sample_rate);
    w = c.num_features;
  } else if (c.mode == MKWS_SPECTRAL_AVERAGE) {
    if (c.average_window_width < 1) return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: average_window_width %d must be positive", c.average_window_width);
    w = (nb + c.average_window_width - 1) / c.average_window_width;
    if (c.num_features != w)
      return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: num_features %d, but %d bins averaged over average_window_width %d give %d", c.num_features, nb,
                  c.average_window_width, w);
  } else {
    return fail(MKWS_ERR_INVALID_ARG, "spectral cfg: mode %d is neither MKWS_SPECTRAL_MFCC nor MKWS_SPECTRAL_AVERAGE", c.mode);
  }
  if (fft_size) *fft_size = n;
  if (bins) *bins = nb;
  if (width) *width = w;
  return MKWS_OK;
}

int build_spectral_tables(const mkws_spectral_cfg& c, SpectralTables* t) {
  int rc = check_spectral_cfg(c, &t->fft_size, &t->bins, &t->width);
  if (rc != MKWS_OK) return rc;
  t->window = c.window_size_samples;
  t->stride = c.window_stride_samples;
  t->channels = c.mode == MKWS_SPECTRAL_MFCC ? c.filterbank_channels : 0;
  const int N = t->fft_size, M = N / 2, bins = t->bins;

  t->window_coef.resize(t->window);
  for (int i = 0; i < t->window; ++i) t->window_coef[i] = static_cast<float>(0.5 - 0.5 * std::cos(2.0 * kPi * i / t->window));
  t->twiddles.resize(2 * (M / 2));
  for (int j = 0; j < M / 2; ++j) {
    t->twiddles[2 * j] = static_cast<float>(std::cos(2.0 * kPi * j / M));
    t->twiddles[2 * j + 1] = static_cast<float>(-std::sin(2.0 * kPi * j / M));
  }
  t->split_twiddles.resize(2 * (M + 1));
  for (int k = 0; k <= M; ++k) {
    t->split_twiddles[2 * k] = static_cast<float>(std::cos(2.0 * kPi * k / N));
    t->split_twiddles[2 * k + 1] = static_cast<float>(-std::sin(2.0 * kPi * k / N));
  }
  t->mel_weights.clear(); t->band_mapper.clear(); t->chan_lo.clear(); t->chan_hi.clear(); t->dct.clear();
  t->start_index = t->end_index = 0;
  if (c.mode != MKWS_SPECTRAL_MFCC) return MKWS_OK;

  const int C = t->channels;
  const double lower = c.lower_frequency_limit, upper = c.upper_frequency_limit;
  const double mel_low = mel_of(lower), mel_span = mel_of(upper) - mel_low;
  std::vector<double> centre(C + 1);
  for (int i = 0; i <= C; ++i) centre[i] = mel_low + (i + 1) * mel_span / (C + 1);
  const double hz_per_bin = 0.5 * c.sample_rate / (bins - 1);
  t->start_index = static_cast<int>(1.5 + lower / hz_per_bin);
  t->end_index = static_cast<int>(upper / hz_per_bin);
  if (t->end_index > bins - 1) t->end_index = bins - 1;     // (upper <= sample_rate / 2 was checked: a guard against the last rounding)
  t->mel_weights.assign(bins, 0.0f);
  t->band_mapper.assign(bins, -2);
  int channel = 0;
  for (int i = t->start_index; i <= t->end_index; ++i) {
    const double m = mel_of(i * hz_per_bin);
    while (channel < C && centre[channel] < m) ++channel;
    const int b = channel - 1;
    t->band_mapper[i] = b;
    const double w = b >= 0 ? (centre[b + 1] - m) / (centre[b + 1] - centre[b]) : (centre[0] - m) / (centre[0] - mel_low);
    t->mel_weights[i] = static_cast<float>(w);
  }
  // channel ch is fed by the bins of band ch - 1 (with 1 - weight) and then by those of band ch (with weight): bands rise with the bin, so
  // they are one run [lo, hi) and ascending bins within it is the order in which the upstream loop adds them
  t->chan_lo.assign(C, 0);
  t->chan_hi.assign(C, 0);
  for (int ch = 0; ch < C; ++ch) {
    int lo = -1, hi = -1;
    for (int i = t->start_index; i <= t->end_index; ++i) {
      const int b = t->band_mapper[i];
      if (b == ch || b == ch - 1) { if (lo < 0) lo = i; hi = i + 1; }
    }
    if (lo >= 0) { t->chan_lo[ch] = lo; t->chan_hi[ch] = hi; }
  }
  const int F = c.num_features;
  t->dct.resize((size_t)F * C);
  const double scale = std::sqrt(2.0 / C), arg = kPi / C;
  for (int k = 0; k < F; ++k)
    for (int j = 0; j < C; ++j) t->dct[(size_t)k * C + j] = static_cast<float>(scale * std::cos(k * arg * (j + 0.5)));
  return MKWS_OK;
}

}  // namespace mkws
