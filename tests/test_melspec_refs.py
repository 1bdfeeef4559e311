"""MelSpec / MFCC without a GPU: the host bank and DCT matrices of mimikit_amd/features/mel.py against tests/golden/melspec.npz (the banks of
tests/melspec_refs.py, scipy's own DCT matrices, librosa's published anchors), the bank's structure, the bounds against near misses, the
dataclasses, the exports, and the argument checks of mmk_melbank_f32 / mmk_stft_mel_f32, which return before any launch."""
import dataclasses as dtc
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import build, native
from mimikit_amd.features import mel
from mimikit_amd.features.functionals import MFCC, Continuous, Identity, MagSpec, MelSpec
from mimikit_amd.features.item_spec import Frame
from tests import melspec_refs as R

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "melspec.npz"))
torch.set_grad_enabled(False)
SETS = [(name, n_bins) for name in R.BANK_SETS for n_bins in R.BANK_BINS]


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name,n_bins", SETS)
def test_host_bank_is_the_golden_bank_bit_for_bit(name, n_bins):
    n_mels, fmin, fmax, htk = R.BANK_SETS[name]
    bank = mel.mel_filter_bank(n_bins, n_mels, fmin, fmax, htk)
    g = G[f"bank_{name}_{n_bins}"]
    assert same_bits(bank.dense(), g) and same_bits(mel.dense_mel_filter_bank(n_bins, n_mels, fmin, fmax, htk), g)
    assert same_bits(np.array(R.mel_bank(n_bins, n_mels, fmin, fmax, htk)), g)
    # banded form: runs inside the bins, offsets that tile one weight array, no zero at a run's ends
    lo, length = R.band_runs(g)
    assert np.array_equal(bank.length, length) and np.array_equal(bank.lo[length > 0], lo[length > 0])
    assert np.array_equal(bank.offset, np.cumsum(length) - length) and len(bank.weights) == length.sum() == np.count_nonzero(g)
    assert np.all(bank.lo >= 0) and np.all(bank.lo + bank.length <= n_bins)
    t = bank.table()
    assert t.dtype == np.int32 and t.shape == (n_mels, 3) and t.flags.c_contiguous and np.array_equal(t[:, 1], length)


@pytest.mark.parametrize("name,n_bins", SETS)
def test_bank_structure(name, n_bins):
    n_mels, fmin, fmax, htk = R.BANK_SETS[name]
    g = G[f"bank_{name}_{n_bins}"]
    assert g.min() >= 0 and np.isfinite(g).all()
    assert np.count_nonzero(g, axis=0).max() <= 2                                      # at most two bands hold a bin
    R.band_runs(g)                                                                     # (asserts that each band is one run)
    freqs = np.arange(n_bins) * R.SR / (2 * (n_bins - 1))
    top = R.SR / 2 if fmax is None else fmax
    assert not g[:, freqs >= top].any() and not g[:, freqs <= fmin].any()             # no weight outside (fmin, fmax)


def test_the_issue_s_counts():
    """non-zeros and the longest band for the shapes users meet (counted on the restatement)"""
    for (n_bins, n_mels), (total, longest) in {(1025, 128): (2018, None), (513, 128): (1008, None), (257, 128): (504, None),
                                               (33, 8): (51, None), (1025, 20): (1878, 285)}.items():
        bank = mel.mel_filter_bank(n_bins, n_mels)
        assert len(bank.weights) == total and (longest is None or bank.length.max() == longest)
    assert (mel.mel_filter_bank(129, 128).length == 0).sum() == 20                    # empty bands exist, and are kept as length 0


def test_anchors():
    for f in (mel.mel_frequencies(40, 0.0, 11025.0), R.mel_frequencies(40, 0.0, 11025.0)):
        assert np.array_equal(np.round(f[G["mel40_index"]], 3), G["mel40_value"])
        assert f[0] == 0 and abs(f[-1] - 11025.0) < 1e-9 and np.all(np.diff(f) > 0)
    for x, want, to_mel in zip(G["scale_in"], G["scale_out"], G["scale_to_mel"]):
        for fn in ((mel.hz_to_mel, R.hz_to_mel) if to_mel else (mel.mel_to_hz, R.mel_to_hz)):
            assert abs(float(fn(float(x))) - want) < 1e-12
    # HTK: 2595 log10(1 + f / 700), and both scales invert
    assert abs(float(mel.hz_to_mel(700.0, htk=True)) - 2595 * np.log10(2.0)) < 1e-12
    for htk in (False, True):
        f = np.array([0.0, 60.0, 999.0, 1000.0, 4000.0, 11025.0])
        assert np.allclose(mel.mel_to_hz(mel.hz_to_mel(f, htk), htk), f, rtol=1e-13, atol=1e-10)


@pytest.mark.parametrize("dct_type", R.DCT_TYPES)
@pytest.mark.parametrize("norm", R.DCT_NORMS)
def test_dct_matrices_are_scipy_s(dct_type, norm):
    for n_mels in R.DCT_MELS:
        g = G[f"dct_t{dct_type}_{norm}_{n_mels}"]
        for n_mfcc in (1, 13, 20, n_mels):
            for make in (mel.dct_matrix_f64, R.dct64):
                d = make(n_mfcc, n_mels, dct_type, norm, 0)
                assert d.dtype == np.float64 and d.shape == (n_mfcc, n_mels) and np.abs(d - g[:n_mfcc]).max() <= 1e-12
            d32 = mel.dct_matrix(n_mfcc, n_mels, dct_type, norm, 0)
            assert d32.dtype == np.float32 and np.array_equal(d32, mel.dct_matrix_f64(n_mfcc, n_mels, dct_type, norm, 0).astype(np.float32))
        # librosa's lifter, row c (from 0) times 1 + (L / 2) sin(pi (c + 1) / L)
        for lifter in (22, 5.5):
            d = mel.dct_matrix_f64(20, n_mels, dct_type, norm, lifter)
            for c in range(20):
                want = g[c] * (1 + (lifter / 2) * np.sin(np.pi * (c + 1) / lifter))
                assert np.abs(d[c] - want).max() <= 1e-12 * max(1.0, lifter)
            assert np.abs(R.dct64(20, n_mels, dct_type, norm, lifter) - d).max() <= 1e-12 * lifter


def test_host_errors():
    for kw in (dict(lifter=-1), dict(dct_type=4), dict(dct_type=0), dict(norm="backward"), dict(n_mfcc=0), dict(n_mfcc=41)):
        with pytest.raises(ValueError):
            mel.dct_matrix(**{**dict(n_mfcc=20, n_mels=40), **kw})
    with pytest.raises(ValueError):
        mel.dct_matrix(1, 1, dct_type=1)
    with pytest.raises(ValueError):
        R.dct64(20, 40, lifter=-1)
    for args in ((1, 8), (33, 0), (33, 8, 5000.0, 4000.0), (33, 8, -1.0)):
        with pytest.raises(ValueError):
            mel.mel_filter_bank(*args)


def test_bounds_reject_near_misses():
    """the bank shifted by one bin, and the bank without the Slaney factor, leave the bank bound; a DCT of the neighbouring type or without
    the lifter leaves the DCT bound"""
    for name, n_bins in (("slaney128", 1025), ("band40", 513), ("htk8", 33), ("slaney128", 129)):
        n_mels, fmin, fmax, htk = R.BANK_SETS[name]
        dense = R.mel_bank(n_bins, n_mels, fmin, fmax, htk)
        s = R.spectrogram(2, n_bins)
        want = R.mel64(s, dense)
        bound = R.bank_bound(want, dense, c=R.C_REFLECT)
        R.assert_inside(want.astype(np.float32), want, bound, "the rounded reference")
        R.assert_near_miss_leaves(R.mel64(s, R.shifted(dense)), want, bound, f"{name} {n_bins}: shifted by one bin")
        R.assert_near_miss_leaves(R.mel64(s, R.mel_bank(n_bins, n_mels, fmin, fmax, htk, slaney=False)), want, bound, f"{name} {n_bins}: no Slaney factor")
        R.assert_near_miss_leaves(want * (1 + 2.0 ** -15), want, bound, f"{name} {n_bins}: half-precision weights")
    x = R.mel_frames(2, 40)
    d32 = R.dct64(13, 40, 2, "ortho", 22).astype(np.float32)
    want = R.dct_apply64(x, d32)
    bound = R.dct_bound(x, d32)
    R.assert_inside(want.astype(np.float32), want, bound, "the rounded reference")
    R.assert_near_miss_leaves(R.dct_apply64(x, R.dct64(13, 40, 2, "ortho", 0)), want, bound, "no lifter")
    R.assert_near_miss_leaves(R.dct_apply64(x, R.dct64(13, 40, 2, None, 22)), want, bound, "norm=None")
    R.assert_near_miss_leaves(R.dct_apply64(x, R.dct64(13, 40, 3, "ortho", 22)), want, bound, "type 3")


def test_configs_are_the_reference_s():
    f = MelSpec()
    assert [x.name for x in dtc.fields(f) if x.name != "type"] == ["n_mels", "fmin", "fmax", "htk"]
    assert (f.n_mels, f.fmin, f.fmax, f.htk) == (128, 0., None, False)
    assert f.unit is None and f.elem_type == Continuous(0., float("inf"), 128) and f.inv == Identity()
    assert MelSpec(40).elem_type.size == 40
    g = MFCC()
    assert [x.name for x in dtc.fields(g) if x.name != "type"] == ["n_mfcc", "dct_type", "norm", "lifter"]
    assert (g.n_mfcc, g.dct_type, g.norm, g.lifter) == (20, 2, "ortho", 0)
    assert g.unit is None and g.elem_type == Continuous(0., float("inf"), 20) and g.inv == Identity()
    for fn in (f, g):
        with pytest.raises(NotImplementedError):
            fn.np_func(np.zeros((4, 1025), dtype=np.float32))
        with pytest.raises(NotImplementedError):
            fn(np.zeros((4, 1025), dtype=np.float32))
    chain = mmk.Compose(MagSpec(1024, 256), MelSpec(40), MFCC(13))
    assert chain.unit == Frame(1024, 256, padding=True) and chain.elem_type == Continuous(0., float("inf"), 13)


def test_serialise_round_trip():
    for fn in (MelSpec(), MelSpec(40, 300., 8000., True), MFCC(), MFCC(13, 3, None, 22)):
        text = fn.serialize()
        assert f"type: {type(fn).__name__}" in text
        back = mmk.Config.deserialize(text)
        assert type(back) is type(fn) and back == fn
    chain = mmk.Compose(MagSpec(1024, 256, center=False), MelSpec(40), MFCC(13, lifter=22))
    assert mmk.Config.deserialize(chain.serialize()) == chain
    ex = mmk.Config.deserialize("type: Compose\nfunctionals:\n- type: MagSpec\n- type: MelSpec\n  n_mels: 64\n  htk: true\n- type: MFCC\n  n_mfcc: 12\n")
    assert ex.functionals[1] == MelSpec(64, htk=True) and ex.functionals[2] == MFCC(12)


def test_exports_and_abi():
    for cls in ("MelSpec", "MFCC"):
        assert cls in mmk.features.functionals.__all__ and getattr(mmk, cls) is getattr(mmk.features.functionals, cls)
        assert getattr(mmk.features, cls) is getattr(mmk, cls)
    with open(os.path.join(os.path.dirname(build.HERE), "include", "mmk.h")) as fh:
        header = fh.read()
    assert f"#define MMK_MELBANK_MAX_ROW {native.MELBANK_MAX_ROW}\n" in header
    assert "int mmk_melbank_f32(const float* in, int64_t in_row_stride, int64_t rows, int32_t n_bins, int32_t bank_n_bins, int32_t n_mels," in header
    assert "int mmk_stft_mel_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n_samples, int32_t n_fft, int32_t hop, int32_t center," in header
    assert "melbank.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "melbank.h"))
    i32, i64, vp = native.i32, native.i64, native.vp
    assert native._SIGNATURES["mmk_melbank_f32"] == (i32, [vp, i64, i64, i32, i32, i32, vp, vp, vp, i32, vp, i32, vp, vp])
    assert native._SIGNATURES["mmk_stft_mel_f32"] == (i32, [vp, i64, i32, i64, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, i32, vp, vp])
    lib = native.load_library()
    assert lib.mmk_abi_version() == native.ABI_VERSION == 6 and hasattr(lib, "mmk_melbank_f32") and hasattr(lib, "mmk_stft_mel_f32")


def test_refusals_without_a_gpu():
    s = torch.zeros(4, 1025)
    for call in (lambda: MelSpec()(s), lambda: MFCC()(torch.zeros(4, 128)), lambda: MelSpec().from_signal(torch.zeros(4096), MagSpec()),
                 lambda: MFCC().from_signal(torch.zeros(2, 4096), MagSpec(), MelSpec())):
        with pytest.raises(RuntimeError, match="HIP device|MI355X"):
            call()
    with pytest.raises(TypeError, match="float32"):
        MelSpec()(s.double())
    with pytest.raises(ValueError):
        MelSpec()(torch.zeros(1025))
    with pytest.raises(ValueError):
        MFCC()(torch.zeros(2, 3, 4, 128))
    with pytest.raises(ValueError):
        MelSpec().from_signal(torch.zeros(2, 3, 4096), MagSpec())
    with pytest.raises(ValueError):
        MFCC(lifter=-1)._dct(128, "cpu")
    with pytest.raises(ValueError):
        MFCC(n_mfcc=129)._dct(128, "cpu")


def test_argument_checks_of_the_library_return_before_a_launch():
    """(device pointers are never dereferenced by the checks, the host table is read: every call below returns before a launch)"""
    lib = native.load_library()
    bank = mel.mel_filter_bank(33, 8)
    table = bank.table()

    def melbank(in_=16, stride=33, rows=4, n_bins=33, bank_bins=33, n_mels=8, host=table, band=1024, w=2048, n_w=len(bank.weights), dct=None,
                n_mfcc=0, out=4096):
        return lib.mmk_melbank_f32(in_, stride, rows, n_bins, bank_bins, n_mels, None if host is None else host.ctypes.data, band, w, n_w, dct,
                                   n_mfcc, out, None)

    def stft_mel(n=4096, n_fft=64, hop=16, bank_bins=33, n_mels=8, host=table, band=1024, n_w=len(bank.weights), dct=None, n_mfcc=0, center=1,
                 reflect=0):
        return lib.mmk_stft_mel_f32(16, n, 1, n, n_fft, hop, center, reflect, bank_bins, n_mels, None if host is None else host.ctypes.data, band, 2048,
                                    n_w, dct, n_mfcc, 4096, None)

    for call in (melbank, stft_mel):
        assert call(n_mels=0) == -1 and b"n_mels" in lib.mmk_last_error()
        assert call(bank_bins=129) == -1 and b"built for" in lib.mmk_last_error()              # a bank for another n_bins
        assert call(dct=8192, n_mfcc=9) == -1 and call(dct=8192, n_mfcc=0) == -1 and call(n_mfcc=3) == -1
        assert call(host=None) == -1
        past = table.copy()
        past[7, 1] = 33 - past[7, 0] + 1                                                          # the last band runs one bin past n_bins
        assert call(host=past) == -1 and b"runs past" in lib.mmk_last_error()
        neg = table.copy()
        neg[2, 0] = -1
        assert call(host=neg) == -1
        assert call(n_w=len(bank.weights) - 1) == -1 and b"runs past" in lib.mmk_last_error()  # ... or past the weights
    assert melbank(in_=None) == -1 and melbank(out=None) == -1 and melbank(rows=0) == -1 and melbank(stride=32) == -1
    assert melbank(host=None, band=None, w=None, n_w=0) == -1                                      # neither a bank nor a DCT
    assert melbank(host=None, band=None, w=None, n_w=0, dct=8192, n_mfcc=4, n_mels=8) == -1        # the DCT alone takes n_bins == n_mels
    assert melbank(n_bins=4000, stride=4000, bank_bins=4000, n_mels=128, host=np.zeros((128, 3), np.int32)) == -3
    assert stft_mel(n=40, center=0) == -1 and stft_mel(n_fft=96) == -3 and stft_mel(hop=64) == -1 and stft_mel(band=None) == -1
    assert stft_mel(n=20, reflect=1) == -1
    assert stft_mel(n_mels=33, host=np.zeros((33, 3), np.int32)) == -3 and b"limit" in lib.mmk_last_error()
