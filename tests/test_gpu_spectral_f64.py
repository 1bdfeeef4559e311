"""STFT, ISTFT, Griffin-Lim and resample kernels, each entry point of include/mmk.h against its float64 reference on the CPU
(tests/f64_bounds.py) with a bound per element - never max|want|.  The cases, their inputs and their checks live in
tests/spectral_cases.py, where tests/test_spectral_refs.py puts torch's own fp32 transforms through them; here the C ABI is called
directly, so that the test owns every buffer:
  * outputs are NaN before the call, longer than the output by a tail of 64 floats (the STFT's inside a larger buffer), and exactly the
    specified elements may have been written;
  * inputs are NaN wherever a kernel must not read: between the rows of a row-strided x, behind the last sample, all of `work`;
  * every element is checked, and every near miss of the case (a reference with one defect) must leave the bound;
  * a case of more than 98 304 output hops (two rounds of segments per wave) computes the reference for three clips, and ISTFT and
    Griffin-Lim there repeat bit for bit, run against run and against the same clip in a batch of one.
Every id names the kernel the case is meant to reach."""
import pytest
import torch

from mimikit_amd import native
from mimikit_amd.features.functionals import resample_filter_bank
from tests import spectral_cases as sc
from tests.f64_bounds import check_written

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NAN = float("nan")
TAIL = 64
STFT_COORD = {"car": 0, "pol": 1, "angle": 2}


def nan_dev(n):
    return torch.full((n,), NAN, dtype=torch.float32, device="cuda")


def written_mask(size, lo, n):
    mask = torch.zeros(size, dtype=torch.bool)
    mask[lo:lo + n] = True
    return mask


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("c", sc.stft_cases(), ids=lambda c: c.id)
def test_stft(device, c):
    lib = native.lib()
    x = sc.stft_input(c, sc.all_clips(c))
    stride = c.n + c.pad
    xb = nan_dev(c.batch * stride + TAIL)                     # NaN between the rows and behind the last sample
    xb[:c.batch * stride].view(c.batch, stride)[:, :c.n] = x.cuda()
    frames = lib.mmk_stft_n_frames(c.n, c.n_fft, c.hop, int(c.center))
    shape = (c.batch, frames, c.n_fft // 2 + 1) + ((2,) if c.coord in ("car", "pol") else ())
    numel = int(torch.Size(shape).numel())
    lead = 66                                                 # the output inside a larger buffer (8-byte aligned: (re, im) pairs)
    buf = nan_dev(lead + numel + TAIL)
    out = buf[lead:]
    if c.coord == "mag":
        native.check(lib.mmk_stft_mag_f32(native.ptr(xb), stride, c.batch, c.n, c.n_fft, c.hop, int(c.center), native.ptr(out),
                                          native.stream_ptr()), "mmk_stft_mag_f32")
    else:
        native.check(lib.mmk_stft_f32(native.ptr(xb), stride, c.batch, c.n, c.n_fft, c.hop, int(c.center), int(c.reflect), STFT_COORD[c.coord],
                                      native.ptr(out), native.stream_ptr()), "mmk_stft_f32")
    check_written(buf, written_mask(buf.numel(), lead, numel), f"stft {c.id}")
    clips = sc.ref_clips(c)
    sc.stft_check(c, x[clips], out[:numel].view(shape)[clips].cpu())


def run_istft(c, spec, offset, woff=0):
    lib = native.lib()
    batch, frames = spec.shape[0], spec.shape[1]
    n_out = lib.mmk_istft_n_samples(frames, c.n_fft, c.hop)
    n_work = lib.mmk_istft_workspace_floats(batch, frames, c.n_fft)
    work = nan_dev(n_work + woff)[woff:] if n_work else None
    buf = nan_dev(4 + batch * n_out + TAIL)
    native.check(lib.mmk_istft_f32(native.ptr(spec), int(c.polar), batch, frames, c.n_fft, c.hop, native.ptr(work), native.ptr(buf[offset:]),
                                   native.stream_ptr()), "mmk_istft_f32")
    check_written(buf, written_mask(buf.numel(), offset, batch * n_out), f"istft {c.id}")
    return buf[offset:offset + batch * n_out].view(batch, n_out)


@pytest.mark.parametrize("c", sc.istft_cases(), ids=lambda c: c.id)
def test_istft(device, c):
    spec = sc.istft_input(c, sc.all_clips(c))
    dev = spec.cuda()
    got = run_istft(c, dev, c.offset, c.woff)
    clips = sc.ref_clips(c)
    if c.clips is not None:                                   # fixed summation order, independent of the launch geometry
        assert same_bits(run_istft(c, dev, c.offset), got), f"istft {c.id}: two runs differ"
        for b in clips[:2]:
            assert same_bits(run_istft(c, dev[b:b + 1].contiguous(), c.offset)[0], got[b]), f"istft {c.id}: clip {b} differs in a batch of one"
    sc.istft_check(c, spec[clips], got[clips].cpu())


def run_gla(c, mag, init):
    lib = native.lib()
    batch, frames = mag.shape[0], mag.shape[1]
    n_out = lib.mmk_istft_n_samples(frames, c.n_fft, c.hop)
    work = nan_dev(lib.mmk_gla_workspace_floats(batch, frames, c.n_fft, c.hop))
    buf = nan_dev(batch * n_out + TAIL)
    native.check(lib.mmk_gla_f32(native.ptr(mag), native.ptr(init), batch, frames, c.n_fft, c.hop, c.n_iter, 0.99, native.ptr(work),
                                 native.ptr(buf), native.stream_ptr()), "mmk_gla_f32")
    check_written(buf, written_mask(buf.numel(), 0, batch * n_out), f"gla {c.id}")
    return buf[:batch * n_out].view(batch, n_out)


@pytest.mark.parametrize("c", sc.gla_cases(), ids=lambda c: c.id)
def test_griffin_lim(device, c):
    """n_iter 0 and 1, from drawn initial estimates and without them (rand_init=False: all 1 + 0i).  The caps of gla_check hold for both starts
    on these signals: no frame has more than 1 % of its energy in bins whose rebuilt value lies inside its own STFT bound."""
    mag, init = sc.gla_input(c, sc.all_clips(c))
    dmag = mag.cuda()
    dinit = None if init is None else torch.view_as_real(init).contiguous().cuda()
    got = run_gla(c, dmag, dinit)
    clips = sc.ref_clips(c)
    if c.clips is not None:
        assert same_bits(run_gla(c, dmag, dinit), got), f"gla {c.id}: two runs differ"
        for b in clips[:2]:
            one = run_gla(c, dmag[b:b + 1].contiguous(), dinit[b:b + 1].contiguous())
            assert same_bits(one[0], got[b]), f"gla {c.id}: clip {b} differs in a batch of one"
    sc.gla_check(c, mag[clips], None if init is None else init[clips], got[clips].cpu())


@pytest.mark.parametrize("c", sc.resample_cases(), ids=lambda c: c.id)
def test_resample(device, c):
    lib = native.lib()
    orig, new, width, table = resample_filter_bank(c.orig_sr, c.new_sr)
    x = torch.randn(c.batch, c.T, generator=sc.gen(4000 + c.seed))
    xs = c.T + 5                                              # row-strided input and output, NaN between the rows
    xb = nan_dev(c.batch * xs + TAIL)
    xb[:c.batch * xs].view(c.batch, xs)[:, :c.T] = x.cuda()
    n_out = lib.mmk_resample_n_out(c.T, orig, new)
    assert n_out == (new * c.T + orig - 1) // orig
    os_ = n_out + 3
    buf = nan_dev(c.batch * os_ + TAIL)
    native.check(lib.mmk_resample_f32(native.ptr(xb), xs, c.batch, c.T, native.ptr(table.cuda()), orig, new, width, native.ptr(buf), os_,
                                      native.stream_ptr()), "mmk_resample_f32")
    mask = torch.zeros(buf.numel(), dtype=torch.bool)
    mask[:c.batch * os_].view(c.batch, os_)[:, :n_out] = True
    check_written(buf, mask, f"resample {c.id}")
    sc.resample_check(c, x, table, orig, new, width, buf[:c.batch * os_].view(c.batch, os_)[:, :n_out].cpu())
