"""Generates tests/golden/envelope.npz FROM THE REFERENCE'S OWN Interpolate, Derivative and the tail of its Envelop.

Run in the build container only (needs the reference tree):
    python tests/golden/make_golden_envelope.py
The reference is imported unmodified through oracle/ref_shim.py (numba's njit is the identity there: derivative_np runs as plain numpy);
what is committed are seeded float32 inputs and the reference's outputs only.

Envelop.np_func itself cannot run here: its MagSpec is librosa's STFT, which is not installed (the shim's stand-in returns nothing).  So
Envelop is pinned by parts.  Its transform - librosa.stft(center=True, window="hann", pad_mode="reflect") - is by librosa's and torch's
documentation the same transform as torch.stft with a periodic Hann window and pad_mode="reflect", which tests/test_gpu_spectral_f64.py
checks the kernels against; THAT EQUALITY HAS NOT BEEN CHECKED WITH LIBROSA.  The steps after it are recorded here from the reference's
own code over a float64 torch.stft magnitude of the length-fixed input (the reference's STFT._fix_length): S.sum(axis=1), the reference's
Interpolate(length=T) (scipy), e /= e.max(), astype(float32) - the lines of Envelop.np_func (:816-823).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.ref_shim import load_reference  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
F = load_reference().functionals
torch.set_grad_enabled(False)

LAGS = (1, 3, 9, 33)
DERIV_N = 200                    # samples of the derivative inputs (> 33)
INTERP_N = 37                    # knots of the interpolation inputs
INTERP_TARGETS = (("length", 100), ("length", 13), ("length", 37), ("factor", 3))       # up, down, same size, factor
ENVELOPS = ((256, 64), (1024, 256))       # (n_fft, hop) of the by-parts Envelop cases
ENV_T = 3001                     # their input length: _fix_length cuts it


def make():
    rng = np.random.default_rng(794)
    arrays = {}
    x = rng.uniform(-1.0, 1.0, size=(3, DERIV_N)).astype(np.float32)
    arrays["deriv_x"] = x
    for lag in LAGS:
        arrays[f"deriv_torch_1d_{lag}"] = F.derivative_torch(torch.from_numpy(x[0].copy()), lag).numpy()
        # (derivative_torch fails for a 2-D input: y[..., 0] of shape (B,) does not broadcast against (B, lag).  Its 2-D record is its 1-D
        # result row by row - the meaning of derivative_np_2d, recorded below from the reference itself)
        arrays[f"deriv_torch_2d_{lag}"] = np.stack([F.derivative_torch(torch.from_numpy(r.copy()), lag).numpy() for r in x])
        arrays[f"deriv_np_1d_{lag}"] = F.derivative_np(x[0].copy(), lag)
        arrays[f"deriv_np_2d_{lag}"] = F.derivative_np(x.copy(), lag)
    arrays["deriv_np_normalized_3"] = F.Derivative(max_lag=3, normalize=True).np_func(x.copy())

    k = rng.uniform(-1.0, 1.0, size=(3, INTERP_N)).astype(np.float32)
    arrays["interp_x"] = k
    for key, val in INTERP_TARGETS:
        for mode in ("linear", "previous"):
            arrays[f"interp_np_{mode}_{key}{val}"] = F.Interpolate(mode=mode, **{key: val}).np_func(k.copy())
        arrays[f"interp_torch_2d_{key}{val}"] = F.Interpolate(**{key: val}).torch_func(torch.from_numpy(k.copy())).numpy()
        arrays[f"interp_torch_1d_{key}{val}"] = F.Interpolate(**{key: val}).torch_func(torch.from_numpy(k[0].copy())).numpy()

    t = np.arange(ENV_T) / 22050.0
    sig = (np.sin(2 * np.pi * 440.0 * t) * np.exp(-3.0 * t * 22050.0 / ENV_T) + 0.1 * rng.standard_normal(ENV_T)).astype(np.float32)
    arrays["env_x"] = sig
    for n_fft, hop in ENVELOPS:
        fft = F.MagSpec(n_fft, hop, center=True, window="hann", pad_mode="reflect")
        fixed = fft.stft._fix_length(sig)
        S = torch.stft(torch.from_numpy(fixed.copy()).double(), n_fft, hop_length=hop, return_complex=True, center=True,
                       window=torch.hann_window(n_fft, dtype=torch.float64), pad_mode="reflect").abs().transpose(-1, -2).numpy()
        e = S.sum(axis=1)
        arrays[f"env_{n_fft}_fixed_length"] = np.int64(fixed.shape[0])
        arrays[f"env_{n_fft}_sum"] = e.copy()
        ei = F.Interpolate(length=sig.shape[0])(e)
        arrays[f"env_{n_fft}_interp"] = ei.copy()
        arrays[f"env_{n_fft}_sum_normalized"] = (e / e.max()).astype(np.float32)
        ei /= ei.max()
        arrays[f"env_{n_fft}_interp_normalized"] = ei.astype(np.float32)
    path = os.path.join(OUT, "envelope.npz")
    np.savez(path, **arrays)
    print(f"envelope.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    make()
