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
