// MelSpec / MFCC: librosa's mel filter bank, and the DCT behind it, applied to magnitude frames - either frames that exist
// (mmk_melbank_f32: a spectrogram, or a mel tensor for the DCT alone) or frames that never reach memory (mmk_stft_mel_f32: output mode 6
// of the STFT kernels of istft.hip / spectral2048.hip).  Both run mel_epilogue of melbank.h on a frame staged in LDS.
#include "entry_util.h"
#include "melbank.h"

namespace mmk {

constexpr int kMelWaves = 4;      // rows in flight per workgroup of melbank_kernel, one per wave

// in: (rows, n_bins) rows in_row_stride apart -> out: (rows, n_out) contiguous.  A wave stages a row with coalesced loads into its share of
// LDS (n_bins floats, then n_mels floats for the bands in front of a DCT) and runs the epilogue on it.
__global__ __launch_bounds__(64 * kMelWaves) void melbank_kernel(const MelBank B, const float* __restrict__ in, int64_t in_row_stride, int64_t rows,
                                                                int n_bins, float* __restrict__ out) {
  extern __shared__ float mel_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* mag = mel_lds + (size_t)wave * (n_bins + B.n_mels);
  const int n_out = B.n_out();
  for (int64_t r = (int64_t)blockIdx.x * kMelWaves + wave; r < rows; r += (int64_t)gridDim.x * kMelWaves) {
    const float* row = in + r * in_row_stride;
    for (int k = lane; k < n_bins; k += 64) mag[k] = row[k];
    __builtin_amdgcn_wave_barrier();
    mel_epilogue<false>(B, mag, mag + n_bins, out + r * n_out, lane, 64);
    __builtin_amdgcn_wave_barrier();                        // mag is rewritten by the next row
  }
}

// the checks both entries share; bank_n_bins: the bins the bank was built for, n_bins: the bins of the frames at hand
static int check_bank(const char* who, int n_bins, int bank_n_bins, int n_mels, const int32_t* band_host, const int32_t* band, const float* weights,
                      int n_weights, const float* dct, int n_mfcc) {
  if (n_mels < 1) return fail(MMK_ERR_INVALID, "%s: n_mels must be at least 1, got %d", who, n_mels);
  if (dct ? (n_mfcc < 1 || n_mfcc > n_mels) : n_mfcc != 0)
    return fail(MMK_ERR_INVALID, "%s: n_mfcc = %d with%s a DCT matrix over %d bands (1 .. n_mels with one, 0 without)", who, n_mfcc,
                dct ? "" : "out", n_mels);
  if (!band) {
    if (band_host || weights || n_weights) return fail(MMK_ERR_INVALID, "%s: a bank needs band_host, band and weights together", who);
    if (!dct) return fail(MMK_ERR_INVALID, "%s: neither a bank nor a DCT matrix", who);
    if (n_mels != n_bins) return fail(MMK_ERR_INVALID, "%s: the DCT alone takes rows of n_mels = %d values, got %d", who, n_mels, n_bins);
    return MMK_OK;
  }
  if (!band_host || n_weights < 0 || (!weights && n_weights > 0)) return fail(MMK_ERR_INVALID, "%s: a bank needs band_host, band and weights together", who);
  if (bank_n_bins != n_bins) return fail(MMK_ERR_INVALID, "%s: the bank was built for %d bins, the frames have %d", who, bank_n_bins, n_bins);
  for (int m = 0; m < n_mels; ++m) {
    const int lo = band_host[3 * m], len = band_host[3 * m + 1], off = band_host[3 * m + 2];
    if (len < 0 || lo < 0 || off < 0 || (int64_t)lo + len > n_bins || (int64_t)off + len > n_weights)
      return fail(MMK_ERR_INVALID, "%s: band %d (first bin %d, length %d, offset %d) runs past %d bins or %d weights", who, m, lo, len, off, n_bins,
                  n_weights);
  }
  return MMK_OK;
}

}  // namespace mmk

extern "C" int mmk_melbank_f32(const float* in, int64_t in_row_stride, int64_t rows, int32_t n_bins, int32_t bank_n_bins, int32_t n_mels,
                               const int32_t* band_host, const int32_t* band, const float* weights, int32_t n_weights, const float* dct,
                               int32_t n_mfcc, float* out, mmk_stream_t stream) {
  using namespace mmk;
  if (!in || !out || rows < 1 || n_bins < 1 || in_row_stride < n_bins)
    return fail(MMK_ERR_INVALID, "melbank: bad arguments (in %p, out %p, rows %lld, n_bins %d, row stride %lld)", (const void*)in, (const void*)out,
                (long long)rows, n_bins, (long long)in_row_stride);
  if (int rc = check_bank("melbank", n_bins, bank_n_bins, n_mels, band_host, band, weights, n_weights, dct, n_mfcc)) return rc;
  if ((int64_t)n_bins + n_mels > MMK_MELBANK_MAX_ROW)
    return fail(MMK_ERR_UNSUPPORTED, "melbank: n_bins + n_mels = %d + %d, the limit is %d", n_bins, n_mels, MMK_MELBANK_MAX_ROW);
  const MelBank B{band, weights, dct, n_mels, dct ? n_mfcc : 0};
  const size_t lds = sizeof(float) * kMelWaves * (size_t)(n_bins + n_mels);
  const int64_t wgs = (rows + kMelWaves - 1) / kMelWaves;
  return launch(melbank_kernel, dim3((unsigned)(wgs < 2048 ? wgs : 2048)), dim3(64 * kMelWaves), lds, (hipStream_t)stream, B, in, in_row_stride, rows,
                n_bins, out);
}

extern "C" int mmk_stft_mel_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n_samples, int32_t n_fft, int32_t hop, int32_t center,
                                int32_t reflect, int32_t bank_n_bins, int32_t n_mels, const int32_t* band_host, const int32_t* band,
                                const float* weights, int32_t n_weights, const float* dct, int32_t n_mfcc, float* out, mmk_stream_t stream) {
  using namespace mmk;
  if (!x || !out || batch <= 0) return fail(MMK_ERR_INVALID, "stft_mel: bad arguments");
  if (hop <= 0 || hop >= n_fft) return fail(MMK_ERR_INVALID, "stft_mel: hop must be in [1, n_fft), got %d", hop);
  if (n_fft < 64 || n_fft > 4096 || (n_fft & (n_fft - 1)))
    return fail(MMK_ERR_UNSUPPORTED, "stft_mel: n_fft must be a power of two in [64, 4096], got %d", n_fft);
  if (mmk_stft_n_frames(n_samples, n_fft, hop, center) <= 0)
    return fail(MMK_ERR_INVALID, "stft_mel: input of %lld samples is shorter than one frame", (long long)n_samples);
  if (reflect && center && n_samples <= n_fft / 2)
    return fail(MMK_ERR_INVALID, "stft_mel: reflect padding of %d needs more than %d samples, got %lld", n_fft / 2, n_fft / 2, (long long)n_samples);
  if (!band) return fail(MMK_ERR_INVALID, "stft_mel: needs a bank");
  if (int rc = check_bank("stft_mel", n_fft / 2 + 1, bank_n_bins, n_mels, band_host, band, weights, n_weights, dct, n_mfcc)) return rc;
  if (n_mels > n_fft / 2)      // the bands of a frame pair share the wave's (workgroup's) transform buffer with its magnitudes
    return fail(MMK_ERR_UNSUPPORTED, "stft_mel: n_mels = %d, the limit at n_fft = %d is %d", n_mels, n_fft, n_fft / 2);
  const MelBank B{band, weights, dct, n_mels, dct ? n_mfcc : 0};
  hipStream_t st = (hipStream_t)stream;
  if (n_fft == 1024) return launch_stft1024(x, x_row_stride, batch, n_samples, hop, center, reflect, 6, out, nullptr, 0.f, st, &B);
  if (n_fft == 2048) return launch_stft2048(x, x_row_stride, batch, n_samples, hop, center, reflect, 6, out, st, &B);
  return launch_stft_generic(x, x_row_stride, batch, n_samples, n_fft, hop, center, reflect, 6, out, nullptr, 0.f, st, &B);
}
