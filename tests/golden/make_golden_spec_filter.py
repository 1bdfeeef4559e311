"""Writes tests/golden/spec_filter.npz: recorded results of the reference's AutoConvolve and F0Filter formulas on the seeded fixtures of
tests/spec_filter_refs.py.  Run from the repository root: ``python -m tests.golden.make_golden_spec_filter``.  Needs numpy and scipy; it
imports nothing from the reference tree and not librosa, whose two calls are restated from memory of the published source:

  AutoConvolve  np.pad, slices, np.prod and np.log exactly as the reference's np_func writes them (spec_filter_refs.auto_convolve_numpy);
                librosa.feature.stack_memory(n_steps=k, delay=-1, constant_values=1) is the restated step.  Recorded: the float64 result
                rounded to float32, `ac_<fixture>_k<k>`.
  F0Filter      librosa.interp_harmonics(z, librosa.fft_frequencies(), harmonics) with the reference's positional arguments (librosa
                0.9's signature) is scipy.interpolate.interp1d(freqs, z, kind="linear", axis=0, copy=False, bounds_error=False,
                fill_value=0) evaluated at h * freqs, freqs = np.fft.rfftfreq(2 (F - 1), 1 / 22050); scipy is called itself.  Recorded:
                y = sl - sl2 in float64, `y_<fixture>_<n_overtone>_<n_undertone>`; the reference's last lines (soft, normalize, the
                product) are spec_filter_refs.f0_from_y.

A fixture is refused unless (1) the float64 restatement lies inside the bound of scipy's result - y within E_b, the four outputs within
their bounds; (2) |y_b| >= 4 E_b at every bin, for scipy's y and the restatement's, so that no decision y > 0 can flip; (3) it holds a
zero frame and a frame whose upper half is zero.  Every shape x parameter pair is held to this at the seeds 0 to 3; the pairs of
F0_RECORDED are written (all sixteen would not fit the size limit of a committed file)."""
import os

import numpy as np
import scipy
import scipy.interpolate

from tests import spec_filter_refs as R

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "spec_filter.npz")
SR = 22050


def scipy_y(s, n_overtone, n_undertone):
    """y of the reference's np_func: interp_harmonics restated around scipy's own interp1d"""
    z = s.T
    freqs = np.fft.rfftfreq(2 * (z.shape[0] - 1), 1.0 / SR)
    f_interp = scipy.interpolate.interp1d(freqs, z, kind="linear", axis=0, copy=False, bounds_error=False, fill_value=0)

    def harmonics(h_range):
        if not h_range:
            return np.zeros(z.shape, dtype=np.float64)
        return np.stack([f_interp(h * freqs) for h in h_range]).astype(np.float64).sum(axis=0)
    sl = harmonics(list(range(1, n_overtone)))
    sl2 = harmonics([1 / x for x in list(range(2, n_undertone))])
    return (sl - sl2).T


def check_f0(s, n_overtone, n_undertone, what):
    assert not s[2].any() and s[3, :s.shape[1] // 2].all() and not s[3, s.shape[1] // 2:].any(), f"{what}: the zero frame or the half-zero frame is missing"
    y_sp = scipy_y(s, n_overtone, n_undertone)
    y, e_b = R.f0_parts64(s, n_overtone, n_undertone)
    worst_y = R.assert_inside(y, y_sp, e_b, f"{what}: y")
    gap = min(R.min_gap(y, e_b), R.min_gap(y_sp, e_b))
    assert gap >= R.MIN_GAP, f"{what}: the smallest gap is {gap:.2f} E_b"
    worst_out = 0.0
    for soft, normalize in R.MODES:
        out, bound = R.f0_filter64(s, n_overtone, n_undertone, soft, normalize)
        worst_out = max(worst_out, R.assert_inside(out, R.f0_from_y(s, y_sp, soft, normalize), bound, f"{what} soft={soft} normalize={normalize}"))
    return y_sp, gap, worst_y, worst_out


def main():
    rec = dict(numpy_version=np.__version__, scipy_version=scipy.__version__)
    gaps, ys, outs = [], [], []
    for name, (seed0, n_frames, bins) in R.F0_SHAPES.items():
        for n_over, n_under in R.F0_PARAMS:
            for seed in range(4):
                s = R.frames(seed, n_frames, bins)
                y_sp, gap, worst_y, worst_out = check_f0(s, n_over, n_under, f"{name} seed {seed} ({n_over}, {n_under})")
                gaps.append(gap), ys.append(worst_y), outs.append(worst_out)
                if seed == seed0 and (n_over, n_under) in R.F0_RECORDED[name]:
                    rec[f"y_{name}_{n_over}_{n_under}"] = y_sp
        rec[f"{name}_checksum"] = np.float64(R.f0_fixture(name).astype(np.float64).sum())
    print(f"F0Filter: {len(gaps)} cases; smallest gap {min(gaps):.1f} E_b, scipy's y within {max(ys):.2f} E_b, outputs within {max(outs):.2f} of the bound")
    differ = 0
    for name in R.AC_SHAPES:
        s = R.ac_fixture(name)
        rec[f"{name}_checksum"] = np.float64(s.astype(np.float64).sum())
        for k in R.AC_WINDOWS[name]:
            got = R.auto_convolve_numpy(s, k)
            assert got.dtype == np.float64 and got.shape == s.shape
            gold = got.astype(np.float32)
            assert gold.any(), f"{name} k={k}: the zero frame lies in every window, the result shows nothing"
            differ += R.ulp_rule(R.auto_convolve64(s, k).astype(np.float32), gold, f"{name} k={k}: the exact-sum restatement against numpy's order")
            rec[f"ac_{name}_k{k}"] = gold
    print(f"AutoConvolve: {differ} float32 elements differ between numpy's sum order and the exact sum")
    np.savez_compressed(OUT, **rec)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(rec)} arrays")
    assert os.path.getsize(OUT) < 1024 * 1024


if __name__ == "__main__":
    main()
