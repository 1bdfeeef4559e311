"""Generates tests/golden/hpss.npz: scipy's own running medians, and librosa's hpss / softmask arithmetic RESTATED in float32 numpy.

Run in the build container only (needs scipy, not the reference tree):
    python tests/golden/make_golden_hpss.py

The reference's HarmonicSource / PercussiveSource (mimikit/features/functionals.py:736-791) are one call each,
librosa.decompose.hpss(S=inputs.T, kernel_size, power, margin)[0 or 1].T, and librosa is not installed here.  What is recorded:

* med_x and scipy.ndimage.median_filter(med_x, size, mode="reflect") for windows 1, 2, 3, 4, 17, 31, 32 and 63 along either axis: THE
  ONE THIRD-PARTY ROUTINE THAT DOES THE WORK, CALLED ITSELF.  med_x is stored as librosa sees it, (bins, frames).
* hpss_x (time-major, (frames, bins), as the functionals take it) and both outputs for power in {1, 2, 0.5, inf} and margin in
  {1, 1.5, (1, 3)} at kernel_size 31, and for kernel_size (9, 5): the medians are scipy's; THE STEPS AFTER THEM (margins, split_zeros,
  softmask, the products) ARE WRITTEN FROM LIBROSA'S PUBLISHED hpss AND softmask SOURCE, FROM MEMORY, AND HAVE NOT BEEN RUN AGAINST LIBROSA.
  They are evaluated in float32 numpy in librosa's order of operations.
"""
import os

import numpy as np
from scipy.ndimage import median_filter

OUT = os.path.dirname(os.path.abspath(__file__))
WINDOWS = (1, 2, 3, 4, 17, 31, 32, 63)
POWERS = (1.0, 2.0, 0.5, float("inf"))
MARGINS = (1.0, 1.5, (1.0, 3.0))


def name(v):
    return "_".join(f"{x:g}" for x in v) if isinstance(v, tuple) else f"{v:g}"


def softmask(X, X_ref, power, split_zeros):
    """librosa.util.softmask, restated"""
    if power <= 0:
        raise ValueError("power must be strictly positive")
    dtype = X.dtype
    Z = np.maximum(X, X_ref).astype(dtype)
    bad_idx = Z < np.finfo(dtype).tiny
    Z[bad_idx] = 1
    if np.isfinite(power):
        mask = (X / Z) ** power
        ref_mask = (X_ref / Z) ** power
        good_idx = ~bad_idx
        mask[good_idx] /= mask[good_idx] + ref_mask[good_idx]
        mask[bad_idx] = 0.5 if split_zeros else 0.0
    else:
        mask = X > X_ref
    return mask


def hpss(S, kernel_size=31, power=2.0, margin=1.0):
    """librosa.decompose.hpss for a real S of (bins, frames), mask=False, restated"""
    win_harm, win_perc = kernel_size if isinstance(kernel_size, tuple) else (kernel_size, kernel_size)
    margin_harm, margin_perc = margin if isinstance(margin, tuple) else (margin, margin)
    if margin_harm < 1 or margin_perc < 1:
        raise ValueError("Margins must be >= 1.0")
    harm = median_filter(S, size=(1, win_harm), mode="reflect")
    perc = median_filter(S, size=(win_perc, 1), mode="reflect")
    split_zeros = margin_harm == 1 and margin_perc == 1
    mask_harm = softmask(harm, perc * margin_harm, power=power, split_zeros=split_zeros)
    mask_perc = softmask(perc, harm * margin_perc, power=power, split_zeros=split_zeros)
    return S * mask_harm, S * mask_perc


def make():
    rng = np.random.default_rng(736)
    arrays = {}
    x = rng.uniform(0.0, 1.0, size=(33, 32)).astype(np.float32)
    x[4:9] = np.round(x[4:9] * 3) / 4                      # ties
    x[12:16, 5:20] = 0.0                                   # exact zeros
    x[20:24] *= np.float32(1e-39)                          # subnormals
    arrays["med_x"] = x
    for w in WINDOWS:
        arrays[f"med_time_{w}"] = median_filter(x, size=(1, w), mode="reflect")
        arrays[f"med_freq_{w}"] = median_filter(x, size=(w, 1), mode="reflect")

    s = rng.uniform(0.0, 1.0, size=(20, 24)).astype(np.float32)
    s[3:17, 2:21] = 0.0                                    # more than half of either axis: both medians of 31 vanish inside
    s[5, 4] = 0.75                                         # a live bin whose medians are both zero: split_zeros shows
    s[12:15] *= np.float32(1e-39)
    arrays["hpss_x"] = s
    for power in POWERS:
        for margin in MARGINS:
            h, p = hpss(s.T.copy(), 31, power, margin)
            arrays[f"harm_31_p{name(power)}_m{name(margin)}"] = np.ascontiguousarray(h.T)
            arrays[f"perc_31_p{name(power)}_m{name(margin)}"] = np.ascontiguousarray(p.T)
    h, p = hpss(s.T.copy(), (9, 5), 1.0, 1.0)
    arrays["harm_9_5_p1_m1"], arrays["perc_9_5_p1_m1"] = np.ascontiguousarray(h.T), np.ascontiguousarray(p.T)
    for k, v in arrays.items():
        assert v.dtype == np.float32, (k, v.dtype)
    np.savez_compressed(os.path.join(OUT, "hpss.npz"), **arrays)
    print({k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    make()
