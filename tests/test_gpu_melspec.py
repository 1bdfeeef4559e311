"""MelSpec / MFCC on the MI355X (csrc/melbank.hip, output mode 6 of the STFT kernels) against the float64 references and derived bounds of
tests/melspec_refs.py.  The fused path is compared with the float64 bank applied to the magnitudes the existing MagSpec returns, never with
the new kernels themselves; with pad_mode="constant" it must also equal MelSpec()(MagSpec()(x)) bit for bit.  Each test prints its worst
error / bound."""
import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.features import mel
from mimikit_amd.features.functionals import MFCC, MagSpec, MelSpec
from tests import melspec_refs as R
from tests.strided_inputs import FLOAT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROWS = (1, 2, 65)
BATCH = 3
# (set of melspec_refs.BANK_SETS, the bins it is run at)
BANK_CASES = [("slaney128", 33), ("slaney128", 129), ("slaney128", 513), ("slaney128", 1025), ("band40", 33), ("band40", 129), ("band40", 513),
              ("band40", 1025), ("htk8", 33), ("htk8", 129), ("htk8", 513), ("htk8", 1025)]


def bits(t):
    return t.contiguous().view(torch.int32)


def melspec_of(name):
    n_mels, fmin, fmax, htk = R.BANK_SETS[name]
    return MelSpec(n_mels, fmin, fmax, htk), R.mel_bank


def dense_of(name, n_bins, **kw):
    n_mels, fmin, fmax, htk = R.BANK_SETS[name]
    return R.mel_bank(n_bins, n_mels, fmin, fmax, htk, **kw)


@surround_rule(*FLOAT_SURROUNDS)
def bank_on_placed_rows(f, s_np, device):
    return f(Strided.of(s_np, 1, device).view).cpu().numpy()


@pytest.mark.parametrize("name,n_bins", BANK_CASES)
def test_bank_kernel_within_the_bound_of_float64(device, name, n_bins):
    f = melspec_of(name)[0]
    dense = dense_of(name, n_bins)
    _, length = R.band_runs(dense)
    if (name, n_bins) == ("slaney128", 129):
        assert (length == 0).sum() >= 1, "this case is here for its empty bands"
    worst = 0.0
    for rows in ROWS:
        for shape in ((rows, n_bins), (BATCH, rows, n_bins)):
            s = R.spectrogram(int(np.prod(shape[:-1])), n_bins).reshape(shape)
            got = f(torch.from_numpy(s.copy()).to(device))
            assert got.shape == shape[:-1] + (f.n_mels,) and got.dtype == torch.float32 and got.device.type == device.type
            got = got.cpu().numpy()
            want = R.mel64(s, dense)
            bound = R.bank_bound(want, dense)
            worst = max(worst, R.assert_inside(got, want, bound, f"MelSpec {name} on {shape}"))
            assert not got[..., length == 0].any(), "a band of length 0 gives exactly 0"
            if len(shape) == 2:                           # the same frames as rows of a wider buffer: in_row_stride, and what lies around them
                assert np.array_equal(bank_on_placed_rows(f, s, device).view(np.int32), got.view(np.int32)), f"MelSpec {name} on placed rows of {shape}"
            if rows == 65 and len(shape) == 2:            # the bound is no wider than the defects it has to catch
                R.assert_near_miss_leaves(R.mel64(s, R.shifted(dense)), want, bound, f"{name} {n_bins}: shifted by one bin")
                R.assert_near_miss_leaves(R.mel64(s, dense_of(name, n_bins, slaney=False)), want, bound, f"{name} {n_bins}: no Slaney factor")
    print(f"bank {name} at {n_bins} bins: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name,n_bins", [("slaney128", 1025), ("band40", 513), ("htk8", 33), ("slaney128", 129)])
def test_one_bin_gives_exactly_its_weights(device, name, n_bins):
    """a spectrogram with one non-zero bin per row: w * s, rounded once, in the at most two bands that hold the bin and 0 elsewhere - an
    off-by-one band start or weight offset shows in every row"""
    f = melspec_of(name)[0]
    dense = dense_of(name, n_bins)
    s = np.zeros((n_bins, n_bins), dtype=np.float32)
    values = (1.0 + np.arange(n_bins) / 7.0).astype(np.float32)
    s[np.arange(n_bins), np.arange(n_bins)] = values
    got = f(torch.from_numpy(s).to(device)).cpu().numpy()
    want = (dense * values[None, :]).T                      # float32 products: (bin, band)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert (np.count_nonzero(got, axis=1) <= 2).all()


@pytest.mark.parametrize("dct_type", R.DCT_TYPES)
@pytest.mark.parametrize("norm", R.DCT_NORMS)
def test_dct_within_the_bound_of_float64(device, dct_type, norm):
    worst = 0.0
    for shape in ((65, 128), (2, 40), (BATCH, 65, 128), (1, 128)):
        n_mels = shape[-1]
        x = R.mel_frames(int(np.prod(shape[:-1])), n_mels).reshape(shape)
        xd = torch.from_numpy(x.copy()).to(device)
        for n_mfcc in (1, 13, 20, n_mels):
            for lifter in (0, 22):
                got = MFCC(n_mfcc, dct_type, norm, lifter)(xd)
                assert got.shape == shape[:-1] + (n_mfcc,) and got.dtype == torch.float32
                d32 = R.dct64(n_mfcc, n_mels, dct_type, norm, lifter).astype(np.float32)
                want = R.dct_apply64(x, d32)
                bound = R.dct_bound(x, d32)
                worst = max(worst, R.assert_inside(got.cpu().numpy(), want, bound, f"MFCC({n_mfcc}, {dct_type}, {norm}, {lifter}) on {shape}"))
                if n_mfcc == 13 and shape == (65, 128):
                    other = R.dct64(n_mfcc, n_mels, dct_type, norm, 22 - lifter)
                    R.assert_near_miss_leaves(R.dct_apply64(x, other), want, bound, "the lifter swapped")
    print(f"DCT type {dct_type} norm {norm}: worst error / bound {worst:.3f}")


def test_bank_and_dct_in_one_launch(device):
    """native.melbank with both: the bands stay in LDS"""
    worst = 0.0
    for name, n_bins in (("slaney128", 1025), ("band40", 513), ("slaney128", 129)):
        f = melspec_of(name)[0]
        dense = dense_of(name, n_bins)
        s = R.spectrogram(65, n_bins)
        sd = torch.from_numpy(s.copy()).to(device)
        for g in (MFCC(), MFCC(13, 3, None, 22), MFCC(f.n_mels, 1, "ortho")):
            got = native.melbank(sd, f._bank(n_bins, device), g._dct(f.n_mels, device))
            d32 = R.dct64(g.n_mfcc, f.n_mels, g.dct_type, g.norm, g.lifter).astype(np.float32)
            mel_ref = R.mel64(s, dense)
            worst = max(worst, R.assert_inside(got.cpu().numpy(), R.dct_apply64(mel_ref, d32), R.mfcc_bound(mel_ref, dense, d32), f"{name} {g}"))
            assert torch.equal(bits(got), bits(g(f(sd)))), "the bands in LDS are the bands MelSpec writes"
    print(f"bank + DCT: worst error / bound {worst:.3f}")


# (n_fft, hop, center, pad_mode, batch, n_samples or None for a count of frames, n_mels, what it covers)
FUSED = [
    (1024, 256, True, "constant", 1, 10 * 256, 128, "11 frames, odd: has_b false; the sliding run of pairs"),
    (1024, 256, False, "constant", 2, 16000, 128, "the bench configuration in small"),
    (1024, 200, True, "reflect", 2, 6000, 128, "the non-sliding load; reflect"),
    (1024, 256, False, "reflect", 1, 9 * 256 + 1024, 40, "center False with the polar magnitudes"),
    (2048, 512, True, "constant", 1, 22050, 128, "the package default; one clip"),
    (2048, 512, True, "reflect", 3, 12000, 128, "default, reflect; rows of a wider tensor"),
    (2048, 512, False, "constant", 3, 12000, 128, "rows of a wider tensor; center False"),
    (256, 64, True, "constant", 2, 3000, 128, "generic kernel; empty bands at 128 mels"),
    (256, 64, False, "reflect", 2, 3001, 40, "generic kernel; odd frame count"),
    (64, 16, True, "constant", 3, 1000, 8, "generic kernel, one wave"),
    (64, 16, False, "reflect", 1, 64 + 16 * 6, 8, "generic kernel; 7 frames"),
]


@surround_rule(*FLOAT_SURROUNDS)
def on_placed_rows(x_np, magspec, melspec, device):
    """MagSpec and MelSpec.from_signal on rows of a wider buffer (5 samples in, 37 more than a row apart) -> magnitudes, mel bands"""
    rows = Strided.of(x_np, 5, device, row_stride=x_np.shape[1] + 37, tail=32)
    x = rows.view if x_np.shape[0] > 1 else rows.view[0]
    return magspec(x), melspec.from_signal(x, magspec)


@pytest.mark.parametrize("n_fft,hop,center,pad_mode,batch,n,n_mels,covers", FUSED, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}" for c in FUSED])
def test_fused_path_against_float64_on_magspec(device, n_fft, hop, center, pad_mode, batch, n, n_mels, covers):
    magspec = MagSpec(n_fft, hop, center=center, pad_mode=pad_mode, alignment=None)
    melspec = MelSpec(n_mels)
    n_bins = n_fft // 2 + 1
    dense = R.mel_bank(n_bins, n_mels)
    wide = torch.from_numpy(R.signal(batch, n + 37).copy()).to(device)
    x = wide[:, 5:5 + n] if batch > 1 else wide[0, 5:5 + n]          # x_row_stride != n_samples for a batch
    assert batch == 1 or (x.stride(0) != n and not x.is_contiguous())
    mag = magspec(x)
    mag_bits = bits(mag).clone()
    got = melspec.from_signal(x, magspec)
    rows_mag, rows_mel = on_placed_rows(R.signal(batch, n + 37)[:, 5:5 + n], magspec, melspec, device)     # the same rows, other neighbours
    assert torch.equal(bits(rows_mag), bits(mag)) and torch.equal(bits(rows_mel), bits(got)), "what lies around the rows shows in the result"
    n_frames = mag.shape[-2]
    assert got.shape == mag.shape[:-1] + (n_mels,) and got.dtype == torch.float32
    if "odd" in covers or "7 frames" in covers:
        assert n_frames % 2 == 1
    if "empty bands" in covers:
        assert (R.band_runs(dense)[1] == 0).any()
    c = 0 if pad_mode == "constant" else R.C_REFLECT
    mag_np = mag.cpu().numpy()
    mel_ref = R.mel64(mag_np, dense)
    bound = R.bank_bound(mel_ref, dense, c)
    worst = R.assert_inside(got.cpu().numpy(), mel_ref, bound, f"MelSpec.from_signal {n_fft}/{hop} {pad_mode}")
    R.assert_near_miss_leaves(R.mel64(mag_np, R.shifted(dense)), mel_ref, bound, "shifted by one bin")
    R.assert_near_miss_leaves(R.mel64(mag_np, R.mel_bank(n_bins, n_mels, slaney=False)), mel_ref, bound, "no Slaney factor")
    worst_c = 0.0
    for g in (MFCC(min(20, n_mels)), MFCC(min(13, n_mels), 3, None, 22)):
        coef = g.from_signal(x, magspec, melspec)
        assert coef.shape == mag.shape[:-1] + (g.n_mfcc,)
        d32 = R.dct64(g.n_mfcc, n_mels, g.dct_type, g.norm, g.lifter).astype(np.float32)
        worst_c = max(worst_c, R.assert_inside(coef.cpu().numpy(), R.dct_apply64(mel_ref, d32), R.mfcc_bound(mel_ref, dense, d32, c),
                                               f"MFCC.from_signal {n_fft}/{hop} {pad_mode} {g}"))
        if pad_mode == "constant":
            assert torch.equal(bits(coef), bits(g(melspec(mag))))
    if pad_mode == "constant":                                        # same magnitudes, weights and summation order
        assert torch.equal(bits(got), bits(melspec(mag))), "from_signal is MelSpec()(MagSpec()(x)) bit for bit"
    assert torch.equal(bits(magspec(x)), mag_bits), "MagSpec is what it was before the fused calls (the tables are shared)"
    print(f"fused {n_fft}/{hop} center={center} {pad_mode} ({covers}): {n_frames} frames, worst error / bound mel {worst:.3f}, mfcc {worst_c:.3f}")


def test_fix_length_and_refusals(device):
    """from_signal applies the length fix-up of MagSpec (alignment "end"), so it is MelSpec of MagSpec for any length; an input shorter
    than one frame raises; a bank wider than the fused path takes raises"""
    x = torch.from_numpy(R.signal(2, 5000).copy()).to(device)
    for magspec in (MagSpec(1024, 256), MagSpec(256, 64, center=False)):
        assert torch.equal(bits(MelSpec(40).from_signal(x, magspec)), bits(MelSpec(40)(magspec(x))))
        assert torch.equal(bits(MelSpec(40).from_signal(x[0], magspec)), bits(MelSpec(40)(magspec(x[0]))))
    with pytest.raises(RuntimeError, match="shorter than one frame"):
        MelSpec().from_signal(x[:, :700], MagSpec(1024, 256, center=False, alignment=None))
    with pytest.raises(RuntimeError, match="shorter than one frame"):
        MFCC().from_signal(x[:, :700], MagSpec(1024, 256, center=False, alignment=None), MelSpec())
    with pytest.raises(NotImplementedError, match="limit"):
        MelSpec(40).from_signal(x, MagSpec(64, 16))
    with pytest.raises(ValueError, match="built for"):
        native.melbank(torch.zeros(4, 513, device=device), mel.device_bank(1025, 128, 0., None, False, device))
    with pytest.raises(ValueError):
        MFCC(41)(torch.zeros(4, 40, device=device))
    with pytest.raises(RuntimeError, match="HIP device|MI355X"):
        MelSpec()(torch.zeros(4, 1025))


def test_compose_and_exports(device):
    assert mmk.MelSpec is MelSpec and mmk.MFCC is MFCC and mmk.features.MelSpec is MelSpec
    x = torch.from_numpy(R.signal(1, 8000)[0].copy()).to(device)
    chain = mmk.Compose(MagSpec(1024, 256), MelSpec(), MFCC())
    out = chain(x)
    assert out.device.type == device.type and torch.equal(bits(out), bits(MFCC().from_signal(x, MagSpec(1024, 256), MelSpec())))
