// Host-side tables of the mfcc / average feature modes (mkws_spectral_*, include/mkws.h): built in double, rounded once to float.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mkws.h"

namespace mkws {

struct SpectralTables {
  int window = 0, stride = 0, fft_size = 0, bins = 0, width = 0, channels = 0;
  int start_index = 0, end_index = 0;          // mfcc mode: the bins the filterbank reads, both inclusive
  std::vector<float> window_coef;              // [window]  periodic Hann
  std::vector<float> twiddles;                 // [fft_size / 4] (re, im) of exp(-2 pi i j / (fft_size / 2)): the packed complex FFT
  std::vector<float> split_twiddles;           // [fft_size / 2 + 1] (re, im) of exp(-2 pi i k / fft_size): the real-FFT post-pass
  std::vector<float> mel_weights;              // [bins]    mfcc mode; 0 outside [start_index, end_index]
  std::vector<int32_t> band_mapper;            // [bins]    mfcc mode; -2 outside, else -1 .. channels - 1
  std::vector<int32_t> chan_lo, chan_hi;       // [channels] bins [lo, hi) that feed a channel (derived from band_mapper)
  std::vector<float> dct;                      // [num_features, channels]
};

// Geometry and field checks only (no tables): MKWS_OK or the refusal, its message naming the field.
int check_spectral_cfg(const mkws_spectral_cfg& cfg, int* fft_size, int* bins, int* width);
int build_spectral_tables(const mkws_spectral_cfg& cfg, SpectralTables* out);

}  // namespace mkws
