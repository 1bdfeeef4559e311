"""float64 references and derived error bounds of the HIP building blocks (include/mmk.h), shared by the kernel tests
(test_gpu_kernels_f64.py) and the whole-network check of the transformer step (test_gpu_transformer.py).  u = 2^-24 is the unit
roundoff of fp32; each bound is C u sqrt(chain length) times the magnitudes a chain of fp32 roundings adds, one C per kernel."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24


def check_bound(got, want, bound, what):
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = tuple(int(t[0]) for t in bad.nonzero(as_tuple=True))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the derived bound; at {i}: got "
                             f"{float(got[i]):.9g}, want {float(want[i]):.9g}, error {float(err[i]):.3e} > bound {float(bound[i]):.3e}")


def check_written(buf, mask, what):
    """the non-NaN elements of the output buffer are exactly the ones the call had to write"""
    written = ~torch.isnan(buf.cpu())
    assert torch.equal(written, mask), f"{what}: {int((written & ~mask).sum())} elements written outside the output, " \
                                       f"{int((mask & ~written).sum())} inside it left unwritten"


def check_near_miss(defect, want, bound, what):
    """the reference with one defect must leave the bound somewhere (NaN counts as leaving it)"""
    assert bool((~((defect - want).abs() <= bound)).any()), f"{what}: a near miss stays inside the bound - the bound is too loose"


# f64 reference of every MMK_ACT_* code (nn.Softplus: beta 1, threshold 20, as the kernel) and its Lipschitz constant
# (Mish: max |mish'| = 1.0998 at x = 1.19)
ACT_F = {0: lambda x: x, 1: torch.tanh, 2: torch.sigmoid, 3: F.mish, 4: torch.abs, 5: torch.relu, 6: F.softplus, 7: torch.sin,
         8: torch.cos}
ACT_LIP = {0: 1.0, 1: 1.0, 2: 0.25, 3: 1.1, 4: 1.0, 5: 1.0, 6: 1.0, 7: 1.0, 8: 1.0}


# y = act(x @ w^T + b) with a length-K fmaf chain per element (split K: partial chains added in a fixed order, then the bias):
#   |pre - pre64| <= C_GEMM u sqrt(K) (|x| @ |w|^T + |b|)        (the bias add and the split adds are roundings of that same sum)
#   |y - y64|     <= Lip(act) |pre - pre64| + 4 u |y64|          (output rounding and the libm error of tanhf / expf / log1pf / sinf / cosf:
#                                                                  a few ulp of the result)
# One c for every dot-product kernel (gemm_bias_act, gemm_f32, skinny_linear, linear).
C_GEMM = 2.0


def gemm_bound(x64, w64, b64, K, act, y64):
    s = x64.abs() @ w64.abs().t()
    if b64 is not None:
        s = s + b64.abs()
    return ACT_LIP[act] * C_GEMM * U * math.sqrt(K) * s + 4 * U * y64.abs()


# out_i = sum_j p_ij v_j / sum_j p_ij, p_ij = exp(x_ij - m_i), x_ij = scale (q_i . k_j), over the visible keys j <= q_pos0 + i.
# A relative error e_ij of p_ij moves out_i by at most sum_j w_ij e_ij |v_j - out_i| (w = softmax weights), with
#   e_ij = u (scale sqrt(hd) sum_d |q_id k_jd|      the score: an fmaf chain of hd MFMA steps
#            + |x_ij| + |x_ij - m_i| + 4)            the scale multiply, the max subtraction, expf (a few ulp)
# and the accumulations add u sqrt(n_i + n_sub) (sum_j w_ij |v_jd| + |out_id|): O^T += V^T P^T and the running sum l are chains over the
# n_i visible keys, rescaled by alpha once per 16-key sub-tile (n_sub = ceil(n_keys / 16)); 2 u |out| for the final 1 / l and product.
# |v_j - out_i| <= |v_j| + |out_i|.  One c for every attention case.
C_ATT = 2.0


def attention_ref(q, k, v, q_pos0, scale):
    """q (B, n_q, H, hd), k / v (B, n_keys, H, hd) float64 -> out (B, n_q, H, hd), weights and bound"""
    n_q, n_keys, hd = q.shape[1], k.shape[1], q.shape[3]
    pos = q_pos0 + torch.arange(n_q)
    vis = torch.arange(n_keys)[None, :] <= pos[:, None]                    # (n_q, n_keys)
    x = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    x = x.masked_fill(~vis, -math.inf)
    wts = torch.softmax(x, -1)
    out = torch.einsum("bhij,bjhd->bihd", wts, v)
    return out, wts, x, vis


def attention_bound(q, k, v, out, wts, x, vis, scale):
    hd, n_keys = q.shape[3], k.shape[1]
    A = torch.einsum("bihd,bjhd->bhij", q.abs(), k.abs())
    m = x.max(-1, keepdim=True).values
    xv = torch.where(vis, x, torch.zeros_like(x))
    e = U * (scale * math.sqrt(hd) * A + xv.abs() + (xv - m).abs() + 4)
    we = torch.where(vis, wts * e, torch.zeros_like(wts))
    va = v.abs()
    t1 = torch.einsum("bhij,bjhd->bihd", we, va) + we.sum(-1).permute(0, 2, 1)[..., None] * out.abs()
    n_i = vis.sum(-1).double()                                             # (n_q,)
    chain = torch.sqrt(n_i + math.ceil(n_keys / 16))[None, :, None, None]
    t2 = U * chain * (torch.einsum("bhij,bjhd->bihd", wts, va) + out.abs())
    return C_ATT * (t1 + t2 + 2 * U * out.abs())


# One wave per row: v = y + res (one fp32 rounding), mean = (sum v) / D, var = (sum (v - mean)^2) / D as fmaf, rstd = 1 / sqrtf(var + eps),
# out = (v - mean) rstd w + b.  Each lane adds its ceil(D / 64) columns in turn, then a 6-level butterfly: chains of
# depth = ceil(D / 64) + 6 roundings, bounded here by their worst case u depth sum|terms| (first order):
#   dv   = u |v|                          (with a residual)
#   dm   = u depth mean|v| + mean(dv) + u |mean|
#   dd   = dv + dm + u |d|                 d = v - mean
#   dvar = mean(2 |d| dd + dd^2) + u (depth + 1) var
#   drs  = rstd (dvar / (2 (var + eps)) + 3 u)
#   dout = |w| (dd rstd + |d| drs) + 3 u |d rstd w| + u |out|
C_LN = 2.0
EPS = 1e-5


def ln_ref(v, w, b, unbiased=False, eps=EPS):
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    var = (d * d).sum(-1, keepdim=True) / (v.shape[-1] - (1 if unbiased else 0))
    rstd = 1.0 / torch.sqrt(var + eps)
    return d * rstd * w + b, mean, d, var, rstd


def ln_bound(v, w, with_res, out, mean, d, var, rstd):
    D = v.shape[-1]
    depth = math.ceil(D / 64) + 6
    dv = U * v.abs() if with_res else torch.zeros_like(v)
    dm = U * depth * v.abs().mean(-1, keepdim=True) + dv.mean(-1, keepdim=True) + U * mean.abs()
    dd = dv + dm + U * d.abs()
    dvar = (2 * d.abs() * dd + dd * dd).mean(-1, keepdim=True) + U * (depth + 1) * var
    drs = rstd * (dvar / (2 * (var + EPS)) + 3 * U)
    dout = w.abs() * (dd * rstd + d.abs() * drs) + 3 * U * (d * rstd * w).abs() + U * out.abs()
    return C_LN * dout


# ====================================================================================================================== spectral
# References of the STFT / ISTFT / Griffin-Lim / resample entry points (include/mmk.h: feature functionals): plain float64 torch on the
# CPU (pad, unfold, window, torch.fft.rfft / irfft, fold), never torch.stft / torch.istft - tests/test_spectral_refs.py holds them to a
# float64 DFT-matrix product and to float64 torch.stft / torch.istft.
#
# The error unit of a transform of n_fft points is that of its windowed frame,
#   unit = u (sqrt(log2 n_fft) + 1) ||frame||_2 :
# log2 n_fft butterfly levels, each a rounding of values whose l2 norm is the frame's (a unitary step), random signs: sqrt(levels); the
# + 1 carries the fp32 rounding of the window and twiddle values (one relative u on every term, once).  It is a bound per ELEMENT: one
# output collects the errors of all n_fft inputs, |err_k| <= ||err||_2.
#
# C_FFT: twice the worst error / unit of torch's own fp32 transforms (torch.stft, torch.istft on the CPU) over the inputs of every case
# of tests/spectral_cases.py, rounded up (tests/test_spectral_refs.py repeats the measurement and asserts fp32 torch inside the bounds):
#   torch.stft  fp32, worst |err| / unit by n_fft:   64: 2.02, 128: 1.54, 256: 2.40, 512: 2.89, 1024: 10.28, 2048: 2.58, 4096: 2.27
#   torch.istft fp32, worst |err| / bound(C_FFT = 1): 64: 0.6, 128: 0.4, 256: 0.3, 512: 0.2, 1024: 1.6, 2048: 0.2, 4096: 0.1
C_FFT = 21.0

# polar -> cartesian, relative to |Z|.  Measured like C_FFT: twice the worst error of the fp32 conversion abs * torch.exp(1j * angle) on
# the CPU over the angles of the cases (|angle| up to 3000 rad): worst 1.62 u, twice that rounded up: 4 u -> E_POL_REF.  The kernels use sincos_hw
# (csrc/spectral_util.h): r = x - q 2 pi in two fmaf steps, t = r / 2 pi, v_sin_f32 / v_cos_f32 of t.  Its error beyond a correctly rounded
# sincosf, as an absolute error of the angle (= relative to |Z|):
#   the second fmaf rounds r, |r| <= pi:                       u pi
#   2 pi = 6.28125 + fl(1.9353e-3): the constant's rounding    |q| u 1.94e-3 <= 478 u 1.94e-3 = 0.93 u   at 3000 rad
#   t = r * fl(1 / 2 pi): the constant and the product         2 u pi
#   v_sin_f32 / v_cos_f32 themselves: the ISA manual states no accuracy; 2^-21.41, the absolute error published for the fast sine /
#   cosine intrinsics (__sinf, __cosf) in [-pi, pi], is taken for them                                                    = 6.02 u
#   (a placeholder: another vendor's published figure, until AMD documents one or sincos_hw's own error has been measured against
#   float64 over [-pi, pi]; it is 6 u in a per-frame term of ~100 u and cannot hide a defect the transform term would not)
# and the two products abs * cos, abs * sin: u.
E_POL_REF = 4.0 * U
E_POL = E_POL_REF + (3 * math.pi + 0.93 + 6.02 + 1.0) * U


def hann64(n_fft, periodic=True):
    return torch.hann_window(n_fft, periodic=periodic, dtype=torch.float64)


def stft_ref(x64, n_fft, hop, center, pad="constant", window=None, shift=0):
    """x64 (B, T) float64 -> S (B, frames, n_fft/2 + 1) complex128 and the windowed frames (B, frames, n_fft).
    pad: 'constant' (zeros), 'reflect', or the defect 'edge' (a reflection that repeats the edge sample); shift: the defect 'every frame
    starts `shift` samples late'; window: another window than the periodic Hann."""
    h = n_fft // 2
    if center:
        if pad == "reflect":
            x64 = torch.cat([x64[:, 1:h + 1].flip(-1), x64, x64[:, -h - 1:-1].flip(-1)], -1)
        elif pad == "edge":
            x64 = torch.cat([x64[:, :h].flip(-1), x64, x64[:, -h:].flip(-1)], -1)
        else:
            x64 = F.pad(x64, (h, h))
    if shift:
        x64 = F.pad(x64, (0, shift))[:, shift:]
    fw = x64.unfold(-1, n_fft, hop) * (hann64(n_fft) if window is None else window)
    return torch.fft.rfft(fw, dim=-1), fw


def fft_unit(frames, n_fft):
    """(..., n_fft) -> (...): u (sqrt(log2 n_fft) + 1) ||frame||_2"""
    return U * (math.sqrt(math.log2(n_fft)) + 1) * frames.norm(dim=-1)


def odd_part(fw):
    """the odd samples' share of every bin, sum over odd n of fw[n] exp(-2 pi i k n / n_fft) = W^k O[k] of the last radix-2 step
    X[k] = E[k] + W^k O[k] (and of the untangling pass of a packed real transform): what a wrong twiddle W^k multiplies"""
    fo = fw.clone()
    fo[..., 0::2] = 0
    return torch.fft.rfft(fo, dim=-1)


def stft_want(S, coord):
    if coord == "car":
        return torch.view_as_real(S)
    if coord == "pol":
        return torch.stack([S.abs(), S.angle()], -1)
    return S.angle() if coord == "angle" else S.abs()


def stft_err_bound(val, S, fw, coord, c_fft=C_FFT):
    """error and bound of `val` (the output layout of `coord`) against the spectrum S of the windowed frames fw.
    car: c_fft unit per part.  mag: + 2 u |S| (the square root and the sum of squares).  Phases: bound_car / |S| + 4 u |angle| (atan2f: a few
    ulp), compared modulo 2 pi; where |S| <= bound_car the phase is undetermined and the bound is pi.  Returns err, bound, and the
    share of the phases with the trivial bound."""
    n_fft = fw.shape[-1]
    bcar = (c_fft * fft_unit(fw, n_fft))[..., None].expand(S.shape)
    absS = S.abs()
    want = stft_want(S, coord)
    err = (val.double() - want).abs()
    bmag = bcar + 2 * U * absS
    trivial = absS <= bcar
    bph = torch.where(trivial, torch.full_like(absS, math.pi), bcar / absS.clamp_min(1e-300) + 4 * U * S.angle().abs())
    if coord == "car":
        return err, bcar[..., None].expand(want.shape), 0.0
    if coord == "mag":
        return err, bmag, 0.0
    two_pi = 2 * math.pi
    if coord == "angle":
        err = (torch.remainder(val.double() - want + math.pi, two_pi) - math.pi).abs()
        return err, bph, float(trivial.double().mean())
    err = torch.stack([err[..., 0], (torch.remainder(val[..., 1].double() - want[..., 1] + math.pi, two_pi) - math.pi).abs()], -1)
    return err, torch.stack([bmag, bph], -1), float(trivial.double().mean())


def check_err(err, bound, what):
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = tuple(int(t[0]) for t in bad.nonzero(as_tuple=True))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the derived bound; at {i}: error "
                             f"{float(err[i]):.3e} > bound {float(bound[i]):.3e}")


def check_err_near_miss(err, bound, what):
    assert bool((~(err <= bound)).any()), f"{what}: a near miss stays inside the bound - the bound is too loose"


def _fold(fr, hop):
    """overlap-add of (B, frames, n_fft) at `hop` -> (B, n_fft + hop (frames - 1))"""
    n_frames, n_fft = fr.shape[1], fr.shape[2]
    L = n_fft + hop * (n_frames - 1)
    return F.fold(fr.transpose(1, 2).contiguous(), (1, L), (1, n_fft), stride=(1, hop))[:, 0, 0]


def istft_ref(Z, n_fft, hop, e_rel=0.0, e_extra=None, c_fft=C_FFT, drop=None, env_drop=None, trim=0, unscaled=None):
    """Z (B, frames, n_fft/2 + 1) complex128 -> out (B, hop (frames - 1)) float64 and its bound.
    Per frame e_f = (c_fft u (sqrt(log2 n_fft) + 1) + e_rel) ||y_f||_2 + e_extra[f] for the time-domain frame y_f: the transform, an error of
    the spectrum relative to its bins (e_rel: by Parseval and Cauchy-Schwarz sum_k |Z_k| e_rel / n_fft <= e_rel ||y_f||_2 at every sample),
    and an l2 error of the frame from elsewhere.  The overlap-add of n_cover(t) windowed frames, the envelope's own sum and the division
    round the sum of |w y_f|[t]:  bound[t] = (sum_f w[t - f hop] e_f + u (n_cover(t) + 2) sum_f |w y_f|[t]) / env[t].
    Defects: drop = (f, o): frame f is missing from the sum at its sample o; env_drop = (f, o): the envelope misses frame f there;
    trim: samples the trim is off by; unscaled = f: 1 / n_fft is missing on frame f."""
    y = torch.fft.irfft(Z, n=n_fft, dim=-1)
    w = hann64(n_fft)
    n_out = hop * (Z.shape[1] - 1)
    yw, w2 = y * w, (w * w).expand(y.shape)
    e_f = (c_fft * U * (math.sqrt(math.log2(n_fft)) + 1) + e_rel) * y.norm(dim=-1)
    if e_extra is not None:
        e_f = e_f + e_extra
    num = _fold(w * e_f[..., None], hop) + U * (_fold(torch.ones_like(y), hop) + 2) * _fold(yw.abs(), hop)
    if unscaled is not None:
        yw = yw.clone()
        yw[:, unscaled] *= n_fft
    if drop is not None:
        yw = yw.clone()
        yw[:, drop[0], drop[1]] = 0
    if env_drop is not None:
        w2 = w2.clone()
        w2[:, env_drop[0], env_drop[1]] = 0
    env = _fold(w2, hop)
    lo = n_fft // 2 + trim
    return (_fold(yw, hop) / env)[:, lo:lo + n_out], (num / _fold((w * w).expand(y.shape), hop))[:, n_fft // 2:n_fft // 2 + n_out]


def polar64(abs32, angle32):
    return torch.polar(abs32.double(), angle32.double())


def gla_ref(mag64, init64, n_fft, hop, n_iter, drop=None):
    """torchaudio's Griffin-Lim (include/mmk.h: mmk_gla_f32) for n_iter 0 or 1 from `init` (complex128; ones for rand_init=False).
    n_iter = 0: out = istft(mag init), the ISTFT bound with 2 u for the complex-by-real products.
    n_iter = 1 (tprev = 0): rebuilt = stft(istft(mag init), center, reflect), angles = rebuilt / (|rebuilt| + 1e-16), out = istft(mag angles).
    The STFT bound of the rebuilt spectrum goes through the normalisation as d_angle = min(2, bound_car / |rebuilt|) (two unit vectors
    differ by at most 2), times mag, and by Parseval into frame f as the l2 error sqrt(sum_k c_k (mag d_angle)^2 / n_fft), c_k = 2 but 1
    for DC and Nyquist.  Returns out, bound and, per frame, the share of mag^2 in bins with d_angle = 2.
    Defect: drop = (f, o) in the last overlap-add (istft_ref)."""
    out, bound = istft_ref(mag64 * init64, n_fft, hop, e_rel=2 * U, drop=drop if n_iter == 0 else None)
    if n_iter == 0:
        return out, bound, torch.zeros(mag64.shape[:2], dtype=torch.float64)
    S, fw = stft_ref(out, n_fft, hop, True, "reflect")
    bcar = (C_FFT * fft_unit(fw, n_fft))[..., None]
    absS = S.abs()
    d = torch.where(absS > 0, bcar / absS.clamp_min(1e-300), torch.full_like(absS, 2.0)).clamp_max(2.0)
    ck = torch.full((n_fft // 2 + 1,), 2.0, dtype=torch.float64)
    ck[0] = ck[-1] = 1.0
    e_extra = torch.sqrt((ck * (mag64 * d) ** 2).sum(-1) / n_fft)
    out, bound = istft_ref(mag64 * (S / (absS + 1e-16)), n_fft, hop, e_rel=4 * U, e_extra=e_extra, drop=drop)
    m2 = mag64 * mag64
    return out, bound, (m2 * (d >= 2.0)).sum(-1) / m2.sum(-1).clamp_min(1e-300)


def resample_ref(x64, table64, orig, new, width, phase=0, floor=False):
    """the (new, 2 width + orig) filter bank as a strided correlation over the zero-padded row, cut to ceil(new T / orig):
    out[n new + j] = sum_k table[j][k] x[n orig + k - width].  Returns out, bound (gemm_bound, K = 2 width + orig).
    Defects: phase: filter row j + phase for output phase j; floor: the cut at floor(new T / orig) (the lost sample is NaN)."""
    T = x64.shape[-1]
    taps = 2 * width + orig
    steps = (T + orig - 1) // orig
    fr = F.pad(x64, (width, steps * orig + width + orig - T)).unfold(-1, taps, orig)[:, :steps]      # (B, steps, taps)
    tab = table64.roll(-phase, 0) if phase else table64
    out = (fr @ tab.t()).reshape(x64.shape[0], steps * new)
    bound = gemm_bound(fr.reshape(-1, taps), table64, None, taps, 0, (fr @ table64.t()).reshape(-1, new)).reshape(x64.shape[0], steps * new)
    n_out = (new * T + orig - 1) // orig
    out, bound = out[:, :n_out].clone(), bound[:, :n_out]
    if floor and (new * T) // orig < n_out:
        out[:, (new * T) // orig:] = float("nan")
    return out, bound
