"""Generates tests/golden/melspec.npz: the mel filter banks of tests/melspec_refs.py, scipy's own DCT matrices and librosa's published anchors.

Run in the build container only (needs scipy, not the reference tree), from the repository root:
    python tests/golden/make_golden_melspec.py

The reference's MelSpec / MFCC (mimikit/features/functionals.py:650-707) are one call each, librosa.feature.melspectrogram(S=...) and
librosa.feature.mfcc(S=...), and librosa is not installed here.  What is recorded:

* bank_<set>_<n_bins>: librosa.filters.mel(sr=22050, n_fft=2 (n_bins - 1), norm="slaney", dtype=float32) for the parameter sets of
  melspec_refs.BANK_SETS, dense (n_mels, n_bins) float32.  THE BANK IS A RESTATEMENT WRITTEN FROM LIBROSA'S PUBLISHED SOURCE
  (tests/melspec_refs.py) AND HAS NOT BEEN RUN AGAINST LIBROSA.
* dct_t<type>_<norm>_<n_mels>: scipy.fft.dct(np.eye(n_mels), axis=0, type=type, norm=norm), float64: THE THIRD-PARTY ROUTINE ITSELF.
* mel40 and its indices / values, scale_*: the numbers librosa's documentation prints for mel_frequencies(40), hz_to_mel and mel_to_hz.
"""
import os
import sys

import numpy as np
import scipy.fft

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import melspec_refs as R  # noqa: E402


def make():
    arrays = {}
    for name, (n_mels, fmin, fmax, htk) in R.BANK_SETS.items():
        for n_bins in R.BANK_BINS:
            arrays[f"bank_{name}_{n_bins}"] = np.array(R.mel_bank(n_bins, n_mels, fmin, fmax, htk))
    for t in R.DCT_TYPES:
        for norm in R.DCT_NORMS:
            for n_mels in R.DCT_MELS:
                arrays[f"dct_t{t}_{norm}_{n_mels}"] = scipy.fft.dct(np.eye(n_mels), axis=0, type=t, norm=norm)
    arrays["mel40_index"] = np.array(sorted(R.ANCHOR_MEL40), dtype=np.int64)
    arrays["mel40_value"] = np.array([R.ANCHOR_MEL40[i] for i in sorted(R.ANCHOR_MEL40)], dtype=np.float64)
    arrays["scale_in"] = np.array([a[1] for a in R.ANCHOR_SCALE], dtype=np.float64)
    arrays["scale_out"] = np.array([a[2] for a in R.ANCHOR_SCALE], dtype=np.float64)
    arrays["scale_to_mel"] = np.array([a[0] == "hz_to_mel" for a in R.ANCHOR_SCALE])
    np.savez_compressed(os.path.join(OUT, "melspec.npz"), **arrays)
    print({k: (v.shape, str(v.dtype)) for k, v in arrays.items()})


if __name__ == "__main__":
    make()
