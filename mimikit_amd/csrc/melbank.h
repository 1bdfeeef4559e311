// The banded mel weighting and the DCT behind it: one epilogue for the bank kernel of melbank.hip and for output mode 6 of the three
// STFT kernels (istft.hip, spectral2048.hip).  librosa's mel filter bank has at most two non-zero weights per bin and every band's
// non-zeros are one run of bins, so a band is (first bin, length, offset into one weight array) and a frame costs about two FMAs per bin.
#pragma once
#include <hip/hip_runtime.h>

namespace mmk {

struct MelBank {
  const int* band;        // [n_mels][3]: first bin, length (may be 0), offset into w;  nullptr: the input IS the bands (DCT only)
  const float* w;         // the bands' weights, one run per band
  const float* dct;       // [n_mels][n_mfcc] (the matrix transposed: lanes that take neighbouring coefficients read neighbours), or nullptr
  int n_mels, n_mfcc;
  __host__ __device__ int n_out() const { return dct ? n_mfcc : n_mels; }
};

// weights (matrix elements) fetched together before their terms are added: a loop of one load and one fmaf per turn waits out the load's
// whole latency every turn, and the turns of a band depend on one another
constexpr int kMelBatch = 8;

// One frame.  mag: the frame's magnitudes in LDS, written by the callers' threads and made visible by them (a barrier) before the call.
// bands: n_mels floats of LDS, touched only when a DCT follows a bank.  out: n_out() floats of global memory.  Thread t of nt takes
// bands (then coefficients) t, t + nt, ..; every sum runs in ascending bin (band) order as one fmaf chain from 0, so whoever calls this
// with the same magnitudes gets the same bits.  WG: the nt threads are a workgroup (else one wave); all of them must make the call.
template <bool WG>
__device__ __forceinline__ void mel_epilogue(const MelBank& B, const float* mag, float* bands, float* __restrict__ out, int t, int nt) {
  const float* src = mag;
  if (B.band) {
    float* dst = B.dct ? bands : out;
    for (int m = t; m < B.n_mels; m += nt) {
      const int lo = B.band[3 * m], len = B.band[3 * m + 1];
      const float* w = B.w + B.band[3 * m + 2];
      float acc = 0.f;
      for (int j = 0; j < len; j += kMelBatch) {            // kMelBatch loads in flight, then their terms in order: one wait per batch
        float wv[kMelBatch], xv[kMelBatch];
#pragma unroll
        for (int u = 0; u < kMelBatch; ++u) {
          const int jj = j + u < len ? j + u : len - 1;     // (past the band: a load that is not used)
          wv[u] = w[jj];
          xv[u] = mag[lo + jj];
        }
#pragma unroll
        for (int u = 0; u < kMelBatch; ++u) acc = j + u < len ? fmaf(wv[u], xv[u], acc) : acc;
      }
      dst[m] = acc;
    }
    src = bands;
  }
  if (B.dct) {
    if (B.band) {
      if (WG) __syncthreads();
      else __builtin_amdgcn_wave_barrier();
    }
    for (int c = t; c < B.n_mfcc; c += nt) {
      float acc = 0.f;
      for (int m = 0; m < B.n_mels; m += kMelBatch) {
        float dv[kMelBatch], xv[kMelBatch];
#pragma unroll
        for (int u = 0; u < kMelBatch; ++u) {
          const int mm = m + u < B.n_mels ? m + u : B.n_mels - 1;
          dv[u] = B.dct[mm * B.n_mfcc + c];
          xv[u] = src[mm];
        }
#pragma unroll
        for (int u = 0; u < kMelBatch; ++u) acc = m + u < B.n_mels ? fmaf(dv[u], xv[u], acc) : acc;
      }
      out[c] = acc;
    }
  }
}

}  // namespace mmk
