"""The float64 references of the spectral tests are plain: torch.fft.rfft / irfft framing (tests/f64_bounds.py) against a float64
DFT-matrix product and against float64 torch.stft / torch.istft.  Then torch's own fp32 transforms on the CPU go through the checks of every
GPU case (tests/spectral_cases.py): they must pass them with C_FFT at twice their worst error, the caps on trivial bounds must hold, and
every near miss must leave its bound - all of it before a GPU is involved.  No test here needs a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import f64_bounds as fb
from tests import spectral_cases as sc

torch.set_grad_enabled(False)
SIZES = (64, 128, 256, 512, 1024, 2048, 4096)


@pytest.mark.parametrize("n_fft", SIZES)
def test_references_vs_dft_matrix(n_fft):
    hop = n_fft // 4 + 1
    x = torch.randn(2, n_fft + 3 * hop, generator=sc.gen(n_fft), dtype=torch.float64)
    S, fw = fb.stft_ref(x, n_fft, hop, True, "reflect")
    n = torch.arange(n_fft, dtype=torch.float64)
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)
    dft = torch.exp(-2j * math.pi * torch.remainder(k[:, None] * n[None, :], n_fft) / n_fft)          # (bins, n_fft)
    want = fw.to(torch.complex128) @ dft.t()
    rel = float(((S - want).abs().amax(-1) / fw.norm(dim=-1)).max())
    assert rel <= 1e-12, rel
    # the inverse: y[n] = (1 / N) sum over the Hermitian spectrum; irfft ignores the imaginary parts of DC and Nyquist
    Z = torch.randn(2, 3, n_fft // 2 + 1, dtype=torch.complex128, generator=sc.gen(n_fft + 1))
    Zr = Z.clone()
    Zr[..., 0] = Zr[..., 0].real + 0j
    Zr[..., -1] = Zr[..., -1].real + 0j
    full = torch.cat([Zr, Zr[..., 1:-1].flip(-1).conj()], -1)                                          # (2, 3, n_fft)
    nn_ = torch.arange(n_fft, dtype=torch.float64)
    idft = torch.exp(2j * math.pi * torch.remainder(nn_[:, None] * nn_[None, :], n_fft) / n_fft) / n_fft
    y = (full @ idft.t()).real
    got = torch.fft.irfft(Z, n=n_fft, dim=-1)
    rel = float(((got - y).abs().amax(-1) / y.norm(dim=-1)).max())
    assert rel <= 1e-12, rel


@pytest.mark.parametrize("n_fft,hop", [(64, 16), (256, 37), (1024, 256), (1024, 1000), (2048, 512), (4096, 1000)])
def test_references_vs_float64_torch(n_fft, hop):
    x = torch.randn(3, 5 * n_fft + 11, generator=sc.gen(hop), dtype=torch.float64)
    w = fb.hann64(n_fft)
    for center, pad in ((True, "reflect"), (True, "constant"), (False, "constant")):
        S, _ = fb.stft_ref(x, n_fft, hop, center, pad)
        want = torch.stft(x, n_fft, hop, window=w, center=center, pad_mode=pad, return_complex=True).transpose(1, 2)
        assert S.shape == want.shape and float((S - want).abs().max()) <= 1e-11 * float(want.abs().max())
    Z = torch.randn(3, 12, n_fft // 2 + 1, dtype=torch.complex128, generator=sc.gen(hop + 1))
    out, _ = fb.istft_ref(Z, n_fft, hop)
    want = torch.istft(Z.transpose(1, 2), n_fft, hop, window=w)
    assert out.shape == want.shape and float(((out - want).abs() / (want.abs() + 1)).max()) <= 1e-9


def test_resample_reference_vs_conv1d():
    from mimikit_amd.features.functionals import resample_filter_bank
    orig, new, width, table = resample_filter_bank(22050, 16000)
    x = torch.randn(2, 3001, generator=sc.gen(1), dtype=torch.float64)
    out, _ = fb.resample_ref(x, table.double(), orig, new, width)
    y = F.conv1d(F.pad(x, (width, width + orig))[:, None], table.double()[:, None], stride=orig).transpose(1, 2).reshape(2, -1)
    n_out = math.ceil(new * 3001 / orig)
    assert out.shape == (2, n_out) and torch.allclose(out, y[:, :n_out], rtol=0, atol=1e-13)


# ---------------------------------------------------------------------------------------------------- torch fp32 through the GPU checks
def stft_fp32(c, x):
    w = torch.hann_window(c.n_fft)
    S = torch.stft(x, c.n_fft, c.hop, window=w, center=c.center, pad_mode="reflect" if c.reflect else "constant",
                   return_complex=True).transpose(1, 2)
    return {"car": lambda: torch.view_as_real(S), "pol": lambda: torch.stack([S.abs(), S.angle()], -1), "angle": S.angle, "mag": S.abs}[c.coord]()


def complex_fp32(c, spec):
    return spec[..., 0] * torch.exp(1j * spec[..., 1]) if c.polar else torch.view_as_complex(spec.contiguous())


def istft_fp32(n_fft, hop, Z32):
    return torch.istft(Z32.transpose(1, 2), n_fft, hop, window=torch.hann_window(n_fft))


def gla_fp32(c, mag, init):
    Z = mag * (torch.ones_like(mag) if init is None else init)
    y = istft_fp32(c.n_fft, c.hop, Z.to(torch.complex64))
    for _ in range(c.n_iter):
        S = torch.stft(y, c.n_fft, c.hop, window=torch.hann_window(c.n_fft), center=True, pad_mode="reflect", return_complex=True).transpose(1, 2)
        y = istft_fp32(c.n_fft, c.hop, mag * (S / (S.abs() + 1e-16)))
    return y


@pytest.mark.parametrize("c", sc.stft_cases(), ids=lambda c: c.id)
def test_stft_cases_hold_for_torch_fp32(c):
    x = sc.stft_input(c, sc.ref_clips(c))
    ratio = sc.stft_check(c, x, stft_fp32(c, x))
    print(f"RATIO stft {c.n_fft} {c.coord} {ratio * fb.C_FFT:.2f} {c.id}")
    if c.coord == "car":
        assert 2 * ratio <= 1.0, f"torch fp32 at {ratio * fb.C_FFT:.2f} units: C_FFT = {fb.C_FFT} is less than twice that"


@pytest.mark.parametrize("c", sc.istft_cases(), ids=lambda c: c.id)
def test_istft_cases_hold_for_torch_fp32(c):
    spec = sc.istft_input(c, sc.ref_clips(c))
    ratio = sc.istft_check(c, spec, istft_fp32(c.n_fft, c.hop, complex_fp32(c, spec)))
    print(f"RATIO istft {c.n_fft} {'pol' if c.polar else 'car'} {ratio:.3f} {c.id}")
    assert 2 * ratio <= 1.0, f"torch fp32 at {ratio:.3f} of the ISTFT bound: more than one half"
    if c.polar:                                             # E_POL_REF is twice the fp32 conversion's worst error
        Z = sc.istft_spectrum(c, spec)
        e = float(((complex_fp32(c, spec).to(torch.complex128) - Z).abs() / Z.abs().clamp_min(1e-300)).max())
        print(f"EPOL {e / fb.U:.3f} u")
        assert 2 * e <= fb.E_POL_REF


@pytest.mark.parametrize("c", sc.gla_cases(), ids=lambda c: c.id)
def test_gla_cases_hold_for_torch_fp32(c):
    mag, init = sc.gla_input(c, sc.ref_clips(c))
    ratio = sc.gla_check(c, mag, init, gla_fp32(c, mag, init))
    print(f"RATIO gla {c.n_fft} {ratio:.3f} {c.id}")
    assert 2 * ratio <= 1.0, f"torch fp32 at {ratio:.3f} of the Griffin-Lim bound: more than one half"


@pytest.mark.parametrize("c", sc.resample_cases(), ids=lambda c: c.id)
def test_resample_cases_hold_for_torch_fp32(c):
    from mimikit_amd.features.functionals import resample_filter_bank
    orig, new, width, table = resample_filter_bank(c.orig_sr, c.new_sr)
    x = torch.randn(c.batch, c.T, generator=sc.gen(4000 + c.seed))
    steps = (c.T + orig - 1) // orig
    fr = F.pad(x, (width, steps * orig + width + orig - c.T)).unfold(-1, 2 * width + orig, orig)[:, :steps]
    got = (fr @ table.t()).reshape(c.batch, -1)[:, :math.ceil(new * c.T / orig)]
    sc.resample_check(c, x, table, orig, new, width, got)
