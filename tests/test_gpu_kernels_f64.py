"""The single kernels the plans are built from, each against a float64 reference on the CPU (include/mmk.h: building blocks).

Every case
  * builds its inputs in fp32 with a seeded generator and its reference in float64 on the CPU from those same fp32 values, with plain
    torch ops (never the library, never the GPU);
  * compares element by element with a bound derived from the operands, not with max|out|.  u = 2^-24 is the unit roundoff of fp32;
    v_mfma_f32_16x16x4_f32 is exact fp32 (a k-ordered chain of fmaf), so a chain of n roundings is held to c u sqrt(n) times the sum
    of the magnitudes it adds (the issue's convention for random data; the worst case is c u n);
  * evaluates the same reference with one plausible defect and asserts that the defect BREAKS the bound somewhere: a bound that a near
    miss passes is too loose, and the case fails;
  * pre-fills every output buffer with NaN (padding past the leading dimension, rows past the last one, rows a row map drops) and
    asserts that exactly the specified elements were written.  Inputs are NaN wherever a kernel must not read.
Every split-K case runs twice and must repeat bit for bit."""
import math

import pytest
import torch

from mimikit_amd import native
from tests.f64_bounds import ACT_F, attention_bound, attention_ref, check_bound, check_near_miss, check_written, gemm_bound, ln_bound, ln_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NAN = float("nan")

# biases that put the pre-activations of the act cases on the edges: sigmoid / Mish at -100, the softplus threshold at 20, sin / cos
# at |x| ~ 100, and the unremarkable middle (x @ w^T adds ~N(0, 1) to each)
EDGE_BIAS = [0.0, -100.0, 20.0, 100.0, 0.5, -20.0, 19.5, 20.5, -99.0, 3.0, -3.0, 0.0]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def nan_dev(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


# ================================================================================================================ dot products
def dot_inputs(g, M, N, K, bias, edge_bias=True):
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    if not bias:
        b = None
    elif edge_bias:
        b = torch.tensor([EDGE_BIAS[n % len(EDGE_BIAS)] for n in range(N)]) + 0.25 * torch.randn(N, generator=g)
    else:
        b = torch.randn(N, generator=g)
    return x, w, b


def reference(x, w, b, act):
    pre = x.double() @ w.double().t()
    if b is not None:
        pre = pre + b.double()
    return pre, ACT_F[act](pre)


def check_dot(got, x, w, b, act, what, drop=None):
    """bound check + the near miss 'the last K column dropped' (and, for split K, the K range `drop` of one split)"""
    K = x.shape[1]
    pre, want = reference(x, w, b, act)
    x64, w64 = x.double(), w.double()
    bound = gemm_bound(x64, w64, None if b is None else b.double(), K, act, want)
    check_bound(got, want, bound, what)
    check_near_miss(ACT_F[act](pre - torch.outer(x64[:, -1], w64[:, -1])), want, bound, f"{what}, last K column dropped")
    if drop is not None:
        k0, k1 = drop
        check_near_miss(ACT_F[act](pre - x64[:, k0:k1] @ w64[:, k0:k1].t()), want, bound, f"{what}, K [{k0}, {k1}) dropped")


def a_operand(x, lda):
    """x (M, K) in a NaN-padded device buffer of leading dimension lda"""
    M, K = x.shape
    a = nan_dev(M, lda)
    a[:, :K] = x.cuda()
    return a


# ---------------------------------------------------------------------------------------------------------------- gemm_bias_act
ALL_STAGES = 1 << 20   # more splits than stages: one per 64-column stage


def split_of(M, N, K, k_split):
    """the split the launch runs (mmk_gemm_partial_floats: ks M n_tiles 16 floats, 0 when it does not split) and the K range of its
    last split: workgroup z of a tile takes the 64-column stages [z S / ks, (z + 1) S / ks)"""
    floats = native.gemm_partial_floats(M, N, K, k_split)
    ks = floats // (M * ((N + 15) // 16) * 16) if floats else 1
    S = (K + 63) // 64
    z = ks - 1
    return floats, ks, (64 * (z * S // ks), min(K, 64 * ((z + 1) * S // ks)))


def run_gemm_bias_act(M, N, K, act, k_split, bias=True, lda_pad=0, ldc_pad=0, row_map=None, edge_bias=True, seed=0):
    what = f"gemm_bias_act M={M} N={N} K={K} act={act} k_split={k_split} row_map={row_map}"
    x, w, b = dot_inputs(gen(seed), M, N, K, bias, edge_bias)
    lda = (K + 3) // 4 * 4 + lda_pad
    a = a_operand(x, lda)
    wp = native.pack_weight(w.cuda())
    bd = None if b is None else b.cuda()
    floats, ks, drop = split_of(M, N, K, 0 if k_split is None else k_split)
    partial = torch.empty(floats, device="cuda") if floats else None
    if row_map is None:
        ldc = N + ldc_pad
        mask = torch.zeros(M + 2, ldc, dtype=torch.bool)
        mask[:M, :N] = True
        rm, size, ldc_arg = (0, 0, 0, 0), (M + 2) * ldc, ldc
    else:
        group, kept = row_map
        row_stride = N + ldc_pad
        group_stride = (group + 1) * row_stride        # a spare row slot after every group: must stay NaN
        n_groups = (M + group - 1) // group
        size = n_groups * group_stride
        mask = torch.zeros(size, dtype=torch.bool)
        for m in range(M):
            g, i = divmod(m, group)
            if i < kept:
                mask[g * group_stride + i * row_stride:g * group_stride + i * row_stride + N] = True
        rm, ldc_arg = (group, kept, group_stride, row_stride), 0

    def launch():
        c = nan_dev(size)
        native.gemm_bias_act(a, lda, M, wp, bd, N, K, c, ldc_arg, act, rm, partial, 0 if k_split is None else k_split)
        return c

    c = launch()
    if ks > 1:   # determinism: the partial sums are added in one fixed order
        again = launch()
        assert torch.equal(c.view(torch.int32), again.view(torch.int32)), f"{what}: two runs of a {ks}-way split differ"
    check_written(c.view(mask.shape), mask, what)
    c = c.cpu()
    if row_map is None:
        got = c.view(M + 2, ldc)[:M, :N]
    else:
        keep = torch.tensor([m % group < kept for m in range(M)])
        rows = [c[(m // group) * group_stride + (m % group) * row_stride:][:N] for m in range(M) if m % group < kept]
        got = torch.stack(rows)
        x = x[keep]
    check_dot(got, x, w, b, act, f"{what} (ran {ks}-way)", drop if ks > 1 else None)
    return ks


# the last column: the split that runs.  None / 0 leave the choice to the launch, which doubles the split while the grid stays within
# 512 workgroups (two per CU), at most 8 ways and one stage per split - the value written here is that rule worked out by hand
@pytest.mark.parametrize("M,N,K,k_split,bias,lda_pad,ldc_pad,ks", [
    (128, 16, 16, None, True, 0, 0, 1),      # one stage
    (129, 17, 17, 1, True, 4, 3, 1),
    (191, 1, 63, None, False, 0, 0, 1),
    (256, 64, 64, 1, True, 0, 5, 1),
    (1000, 65, 65, None, True, 8, 0, 2),     # 2 x 16 workgroups, 2 stages
    (128, 100, 100, 2, False, 0, 1, 2),
    (256, 1536, 100, 1, True, 0, 0, 1),
    (129, 100, 513, 2, True, 4, 2, 2),       # 9 stages, the last one ragged (one 16-column chunk of it, one real column): [0, 4) [4, 9)
    (191, 65, 513, 3, True, 0, 0, 3),
    (128, 17, 513, 8, True, 0, 0, 8),        # 8 splits of 9 stages: one takes two
    (256, 16, 513, ALL_STAGES, True, 0, 0, 9),
    (1000, 64, 1024, None, True, 0, 0, 8),   # 1 x 16 workgroups: 8 ways
    (128, 1536, 1024, 0, True, 0, 3, 8),     # 24 x 2 workgroups: 8 ways
    (256, 100, 4096, 3, True, 0, 0, 3),      # 64 stages in 21 + 21 + 22
    (129, 16, 4096, ALL_STAGES, False, 4, 0, 64),
    (1000, 1536, 4096, None, True, 0, 0, 1), # 24 x 16 = 384 workgroups: doubling would pass 512, no split
])
def test_gemm_bias_act_shapes(M, N, K, k_split, bias, lda_pad, ldc_pad, ks):
    assert run_gemm_bias_act(M, N, K, 0, k_split, bias, lda_pad, ldc_pad, edge_bias=False, seed=M * 7 + N * 3 + K) == ks


@pytest.mark.parametrize("act", range(9))
@pytest.mark.parametrize("M,N,K,k_split", [(129, 100, 65, 1), (256, 40, 513, 2)])
def test_gemm_bias_act_every_act(M, N, K, k_split, act):
    run_gemm_bias_act(M, N, K, act, k_split, seed=act)


@pytest.mark.parametrize("M,N,K,k_split,group,kept", [
    (256, 48, 64, 1, 64, 63),                # direct epilogue: the plan's "every row but the window's last" shape
    (260, 48, 513, 3, 65, 64),               # split-reduce epilogue
    (300, 17, 100, 1, 7, 3),                 # a ragged last group
])
def test_gemm_bias_act_row_map(M, N, K, k_split, group, kept):
    assert run_gemm_bias_act(M, N, K, 5, k_split, ldc_pad=3, row_map=(group, kept), seed=group) == max(1, min(k_split, (K + 63) // 64))


def test_gemm_bias_act_refusals():
    w = torch.randn(32, 64, device="cuda")
    wp = native.pack_weight(w)
    a = torch.randn(200 * 68 + 4, device="cuda")
    c = nan_dev(200 * 32)
    with pytest.raises(NotImplementedError):                                     # M = 127
        native.gemm_bias_act(a, 64, 127, wp, None, 32, 64, c, 32)
    with pytest.raises(NotImplementedError):                                     # lda % 4 != 0
        native.gemm_bias_act(a, 66, 128, wp, None, 32, 64, c, 32)
    with pytest.raises(NotImplementedError):                                     # A one float off 16-byte alignment
        native.gemm_bias_act(a[1:], 64, 128, wp, None, 32, 64, c, 32)
    for act in (-1, 9):
        with pytest.raises(ValueError):
            native.gemm_bias_act(a, 64, 128, wp, None, 32, 64, c, 32, act=act)
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all())


# ---------------------------------------------------------------------------------------------------------------- gemm_f32
GEMM_F32_MAX_K = 624     # 64 rows x (K + 4) floats of LDS <= 160 KiB


@pytest.mark.parametrize("batch,M,N,K,odd_ldc", [
    (1, 1, 16, 4, False),
    (3, 63, 100, 17, True),
    (1, 64, 128, 128, False),
    (3, 65, 129, 512, False),
    (1, 1024, 7680, 128, False),
    (1, 64, 16, GEMM_F32_MAX_K, False),
    (3, 65, 100, GEMM_F32_MAX_K, True),
    (1, 1024, 129, 512, True),
])
def test_gemm_f32(batch, M, N, K, odd_ldc):
    what = f"gemm_f32 batch={batch} M={M} N={N} K={K}"
    g = gen(batch * 1000 + M + N + K)
    xs = [torch.randn(M, K, generator=g) for _ in range(batch)]
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    lda = (K + 3) // 4 * 4 + 4
    a_batch = (M + 1) * lda
    a = nan_dev(batch * a_batch)
    for i, x in enumerate(xs):
        a[i * a_batch:(i + 1) * a_batch].view(M + 1, lda)[:M, :K] = x.cuda()
    ldc = N + (1 if odd_ldc else 4) if N % 2 == 0 else N + (2 if odd_ldc else 3)
    assert (ldc % 2 == 1) == odd_ldc
    c_batch = (M + 1) * ldc + 3
    c = nan_dev(batch * c_batch)
    native.gemm_f32(a, lda, a_batch, native.pack_weight(w.cuda()), N, K, c, ldc, c_batch, M, batch)
    mask = torch.zeros(batch * c_batch, dtype=torch.bool)
    for i in range(batch):
        mask[i * c_batch:i * c_batch + (M + 1) * ldc].view(M + 1, ldc)[:M, :N] = True
    check_written(c, mask, what)
    c = c.cpu()
    for i, x in enumerate(xs):
        got = c[i * c_batch:i * c_batch + (M + 1) * ldc].view(M + 1, ldc)[:M, :N]
        check_dot(got, x, w, None, 0, f"{what} [{i}]")


def test_gemm_f32_refuses_k_past_the_lds_stage():
    w = native.pack_weight(torch.randn(16, GEMM_F32_MAX_K + 1, device="cuda"))
    a = torch.zeros(64 * 640, device="cuda")
    c = nan_dev(64 * 16)
    with pytest.raises(NotImplementedError):
        native.gemm_f32(a, 628, 0, w, 16, GEMM_F32_MAX_K + 1, c, 16, 0, 64)
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all())


# ---------------------------------------------------------------------------------------------------------------- skinny_linear
@pytest.mark.parametrize("M,N,K,act,bias", [
    (1, 48, 128, 0, True),                   # K = 128 CPW, CPW 1 .. 8; 16-row blocks RB = ceil(M / 16), 1 .. 4; N / 16 odd
    (15, 100, 256, 1, True),
    (16, 16, 384, 5, True),
    (17, 100, 512, 3, False),
    (33, 48, 640, 0, True),
    (64, 1536, 768, 6, True),
    (64, 100, 896, 4, True),
    (33, 100, 1024, 2, True),
    (17, 48, 1024, 8, True),
    (1, 100, 1024, 7, True),
])
def test_skinny_linear(M, N, K, act, bias):
    what = f"skinny_linear M={M} N={N} K={K} act={act}"
    x, w, b = dot_inputs(gen(M * 100 + K + act), M, N, K, bias)
    lda = K + 4
    a = a_operand(x, lda)
    ldc = N + 3
    c = nan_dev(M + 2, ldc)
    native.skinny_linear(a, lda, M, native.pack_weight(w.cuda()), None if b is None else b.cuda(), N, K, c, ldc, act)
    mask = torch.zeros(M + 2, ldc, dtype=torch.bool)
    mask[:M, :N] = True
    check_written(c, mask, what)
    check_dot(c.cpu()[:M, :N], x, w, b, act, what)


def test_skinny_linear_refusals():
    c = nan_dev(70 * 32)
    a = torch.randn(70 * 128, device="cuda")
    with pytest.raises(NotImplementedError):                                     # K = 100
        native.skinny_linear(a, 100, 4, native.pack_weight(torch.randn(32, 100, device="cuda")), None, 32, 100, c, 32)
    wp = native.pack_weight(torch.randn(32, 128, device="cuda"))
    with pytest.raises(NotImplementedError):                                     # M = 65
        native.skinny_linear(a, 128, 65, wp, None, 32, 128, c, 32)
    for act in (-1, 9):
        with pytest.raises(ValueError):
            native.skinny_linear(a, 128, 4, wp, None, 32, 128, c, 32, act=act)
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all())


# ---------------------------------------------------------------------------------------------------------------- mmk_linear_f32
LINEAR_SHAPES = [(1, 16, 16), (2, 257, 128), (8, 128, 64), (32, 512, 768), (64, 1536, 512), (3, 33, 513), (64, 65, 17), (130, 48, 100),
                 (512, 96, 260)]      # test_gpu_features.py: test_linear_vs_torch


@pytest.mark.parametrize("act", range(9))
@pytest.mark.parametrize("m,n,k", LINEAR_SHAPES)
def test_linear_every_act(m, n, k, act):
    what = f"linear M={m} N={n} K={k} act={act}"
    x, w, b = dot_inputs(gen(m * 1000 + n + act), m, n, k, True)
    ldx = k + 5
    xd = nan_dev(m, ldx)
    xd[:, :k] = x.cuda()
    ldy = n + 3
    y = nan_dev(m + 2, ldy)
    native.check(native.lib().mmk_linear_f32(xd.data_ptr(), ldx, m, native.pack_weight(w.cuda()).data_ptr(), b.cuda().data_ptr(), n, k,
                                             y.data_ptr(), ldy, act, native.stream_ptr()), "mmk_linear_f32")
    mask = torch.zeros(m + 2, ldy, dtype=torch.bool)
    mask[:m, :n] = True
    check_written(y, mask, what)
    check_dot(y.cpu()[:m, :n], x, w, b, act, what)


@pytest.mark.parametrize("act", [-1, 9])
def test_linear_refuses_unknown_act(act):
    x = torch.randn(4, 16, device="cuda")
    with pytest.raises(ValueError):
        native.linear(x, native.pack_weight(torch.randn(16, 16, device="cuda")), None, 16, 16, act)


# ================================================================================================================ attention
def attention_data(g, B, n_q, q_pos0, n_keys, H, hd, data):
    q = torch.randn(B, n_q, H, hd, generator=g)
    k = torch.randn(B, n_keys, H, hd, generator=g)
    v = torch.randn(B, n_keys, H, hd, generator=g)
    if data == "peaked":            # |scale q k| up to ~80: an exp without the max subtraction overflows
        q, k = q * 4.5, k * 4.5
    elif data == "late_max":        # the largest score of every row that sees it sits in the last 64-key tile: the running max jumps there.
        d = torch.randn(hd, generator=g)       # (a second, equal one on the window's last key: masking that key is then visible in a row
        d = d / d.norm()                       #  whose weight it would otherwise hold at e^-30)
        q = q + 3 * d
        k[:, 64 * ((n_keys - 1) // 64)] = 10 * math.sqrt(hd) * d
        k[:, n_keys - 1] = 10 * math.sqrt(hd) * d
    elif data == "equal_keys":
        k[:] = k[:, :1].clone()
    return q, k, v


def place(buf_shape, parts):
    """a NaN host buffer with each (index, tensor) part written into it"""
    buf = torch.full(buf_shape, NAN)
    for idx, t in parts:
        buf[idx] = t
    return buf


def run_attention(hd, H, B, n_q, q_pos0, n_keys, layout, data, o_pad=0, seed=0):
    what = f"attention hd={hd} H={H} B={B} n_q={n_q} q_pos0={q_pos0} n_keys={n_keys} {layout} {data}"
    D = H * hd
    scale = 1.0 / math.sqrt(hd)
    q, k, v = attention_data(gen(seed), B, n_q, q_pos0, n_keys, H, hd, data)
    qf, kf, vf = (t.reshape(*t.shape[:2], D) for t in (q, k, v))
    if layout == "packed":          # the plan's self-attention: one (rows, 3 D) QKV block per clip
        rows = max(n_keys, q_pos0 + n_q)
        qkv = place((B, rows, 3 * D), [((slice(None), slice(q_pos0, q_pos0 + n_q), slice(0, D)), qf),
                                       ((slice(None), slice(0, n_keys), slice(D, 2 * D)), kf),
                                       ((slice(None), slice(0, n_keys), slice(2 * D, 3 * D)), vf)]).cuda()
        qd, kd, vd = qkv[:, q_pos0:], qkv[:, :, D:], qkv[:, :, 2 * D:]
        q_ld, q_cs, kv_ld, kv_cs = 3 * D, rows * 3 * D, 3 * D, rows * 3 * D
    elif layout == "cross":         # the plan's cross-attention: K / V of layer 1 of 3 in one (rows, 2 D L) block
        L = 3
        qd = qf.contiguous().cuda()
        kv = place((B, n_keys, 2 * D * L), [((slice(None), slice(None), slice(2 * D, 3 * D)), kf),
                                            ((slice(None), slice(None), slice(3 * D, 4 * D)), vf)]).cuda()
        kd, vd = kv[:, :, 2 * D:], kv[:, :, 3 * D:]
        q_ld, q_cs, kv_ld, kv_cs = D, n_q * D, 2 * D * L, n_keys * 2 * D * L
    else:                           # separate, NaN-padded rows
        ld = D + 4
        qd = place((B, n_q, ld), [((Ellipsis, slice(0, D)), qf)]).cuda()
        kd = place((B, n_keys, ld), [((Ellipsis, slice(0, D)), kf)]).cuda()
        vd = place((B, n_keys, ld), [((Ellipsis, slice(0, D)), vf)]).cuda()
        q_ld, q_cs, kv_ld, kv_cs = ld, n_q * ld, ld, n_keys * ld
    o_ld = D + o_pad
    out = nan_dev(B, n_q + 2, o_ld)
    native.tr_attention(qd, q_ld, q_cs, kd, vd, kv_ld, kv_cs, out, o_ld, (n_q + 2) * o_ld, n_q, q_pos0, n_keys, H, hd, scale, B)
    mask = torch.zeros(B, n_q + 2, o_ld, dtype=torch.bool)
    mask[:, :n_q, :D] = True
    check_written(out, mask, what)
    got = out.cpu()[:, :n_q, :D].reshape(B, n_q, H, hd)

    q64, k64, v64 = q.double(), k.double(), v.double()
    want, wts, x, vis = attention_ref(q64, k64, v64, q_pos0, scale)
    if data == "peaked":
        assert float(x[:, :, vis].abs().max()) > 40
    bound = attention_bound(q64, k64, v64, want, wts, x, vis, scale)
    check_bound(got, want, bound, what)
    # near miss 1: an off-by-one mask - the last visible key of every row hidden.  Judged on the rows that keep a key (a row that sees
    # key 0 only becomes empty: NaN, trivially outside any bound - all that is left where every row sees one key)
    pos = torch.clamp(q_pos0 + torch.arange(n_q), max=n_keys - 1)
    vis_m = vis & (torch.arange(n_keys)[None, :] != pos[:, None])
    rows = vis_m.any(-1) if bool(vis_m.any()) else torch.ones(n_q, dtype=torch.bool)
    x_m = (torch.einsum("bihd,bjhd->bhij", q64, k64) * scale).masked_fill(~vis_m, -math.inf)
    miss = torch.einsum("bhij,bjhd->bihd", torch.softmax(x_m, -1), v64)
    check_near_miss(miss[:, rows], want[:, rows], bound[:, rows], f"{what}, last visible key masked")
    # near miss 2: scale 1 / hd instead of 1 / sqrt(hd).  No bound can see it where every row's scores are equal (equal keys) or a row
    # has one key: the softmax is then the same for any scale
    if data != "equal_keys" and bool((vis.sum(-1) > 1).any()):
        miss, *_ = attention_ref(q64, k64, v64, q_pos0, 1.0 / hd)
        check_near_miss(miss, want, bound, f"{what}, scale 1/hd")


@pytest.mark.parametrize("hd,H,B,n_q,q_pos0,n_keys,layout,data,o_pad", [
    # full causal windows, every NC instance (nc <= 2, 4, 8, 16, 32) with full and partial nc, partial last output tiles
    (4, 1, 1, 1, 0, 1, "sep", "normal", 0),
    (8, 3, 3, 15, 0, 15, "packed", "normal", 0),
    (12, 4, 1, 16, 0, 16, "packed", "normal", 4),
    (16, 8, 37, 17, 0, 17, "sep", "normal", 0),
    (20, 3, 1, 63, 0, 63, "cross", "normal", 0),
    (32, 8, 3, 64, 0, 64, "packed", "peaked", 0),
    (36, 1, 1, 65, 0, 65, "sep", "late_max", 4),
    (64, 3, 1, 129, 0, 129, "cross", "peaked", 0),
    (68, 1, 3, 300, 0, 300, "packed", "late_max", 0),
    (124, 1, 1, 65, 0, 65, "sep", "equal_keys", 0),
    (128, 3, 1, 129, 0, 129, "sep", "normal", 8),
    (16, 1, 3, 129, 0, 129, "packed", "equal_keys", 0),
    # the last row of a window (the plan's last layer)
    (16, 3, 3, 1, 0, 1, "packed", "normal", 0),
    (32, 3, 3, 1, 63, 64, "packed", "normal", 0),
    (64, 1, 3, 1, 64, 65, "cross", "late_max", 0),
    (128, 3, 3, 1, 2047, 2048, "packed", "late_max", 0),
    (12, 4, 1, 1, 2047, 2048, "cross", "normal", 0),
    # a block in the middle, and rows past the last key (legal: they see every key)
    (16, 3, 3, 5, 40, 64, "sep", "normal", 0),
    (32, 3, 1, 20, 50, 60, "sep", "normal", 4),
])
def test_attention(hd, H, B, n_q, q_pos0, n_keys, layout, data, o_pad):
    run_attention(hd, H, B, n_q, q_pos0, n_keys, layout, data, o_pad, seed=hd * 31 + n_keys)


@pytest.mark.parametrize("hd", [130, 6])
def test_attention_refuses_head_dim(hd):
    x = torch.zeros(4 * hd, device="cuda")
    out = nan_dev(4 * hd)
    with pytest.raises(ValueError):
        native.tr_attention(x, hd, 0, x, x, hd, 0, out, hd, 0, 1, 0, 1, 1, hd, 1.0, 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ================================================================================================================ LayerNorm
def ln_rows(g, rows, D, with_res):
    """y and res by row type r % 4: N(0, 1); mean 1e3 with spread 1; constant (variance 0); magnitude 1e4"""
    y = torch.randn(rows, D, generator=g)
    res = torch.randn(rows, D, generator=g)
    for r in range(rows):
        t = r % 4
        if t == 1:
            res[r] += 1e3
            if not with_res:
                y[r] += 1e3
        elif t == 2:
            y[r], res[r] = 0.3, 0.7
        elif t == 3:
            y[r] *= 1e4
            res[r] *= 1e4
    return y, res


@pytest.mark.parametrize("D,rows,res_mode,res_rf,pad", [
    (1, 5, "none", 1, 0),
    (2, 3, "sep", 1, 3),
    (16, 4, "alias", 1, 0),
    (63, 130, "sep", 1, 1),
    (64, 1, "none", 1, 0),
    (65, 5, "alias", 1, 3),
    (256, 130, "sep", 3, 0),                 # res_ld = rf D: the last row of every window (the plan's last layer)
    (1000, 4, "none", 1, 2),
    (1024, 130, "alias", 1, 0),              # in place, as the plan runs it
    (1024, 3, "sep", 65, 4),
])
def test_add_layer_norm(D, rows, res_mode, res_rf, pad):
    what = f"add+LayerNorm D={D} rows={rows} res={res_mode} rf={res_rf}"
    g = gen(D * 10 + rows)
    with_res = res_mode != "none"
    y, res = ln_rows(g, rows, D, with_res)
    w = 1 + 0.5 * torch.randn(D, generator=g)
    b = 0.5 * torch.randn(D, generator=g)
    y_ld, out_ld = D + 3, D + pad
    yd = place((rows, y_ld), [((slice(None), slice(0, D)), y)]).cuda()
    out = nan_dev(rows + 2, out_ld)
    if res_mode == "alias":
        out[:rows, :D] = res.cuda()
        rd, res_ld = out, out_ld
    elif res_mode == "sep":
        res_ld = res_rf * D + (1 if res_rf == 1 else 0)
        rd = place((rows, res_ld), [((slice(None), slice(0, D)), res)]).cuda()
    else:
        rd, res_ld = None, 0
    native.tr_add_ln(yd, y_ld, rd, res_ld, w.cuda(), b.cuda(), out, out_ld, rows, D)
    mask = torch.zeros(rows + 2, out_ld, dtype=torch.bool)
    mask[:rows, :D] = True
    check_written(out, mask, what)
    got = out.cpu()[:rows, :D]

    v = y.double() + res.double() if with_res else y.double()
    w64, b64 = w.double(), b.double()
    want, mean, d, var, rstd = ln_ref(v, w64, b64)
    bound = ln_bound(v, w64, with_res, want, mean, d, var, rstd)
    check_bound(got, want, bound, what)
    check_near_miss(ln_ref(v, w64, b64, unbiased=True)[0], want, bound, f"{what}, unbiased variance")


def test_add_layer_norm_refuses_1025_columns():
    y = torch.zeros(1025, device="cuda")
    out = nan_dev(1025)
    with pytest.raises(ValueError):
        native.tr_add_ln(y, 1025, None, 0, y, y, out, 1025, 1, 1025)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
