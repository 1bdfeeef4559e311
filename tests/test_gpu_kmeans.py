"""The k-means kernels on the MI355X (csrc/kmeans.hip, include/mmk_kmeans.h) against the float64 restatements and derived bounds of
tests/kmeans_refs.py: the three entry points through the C ABI on strided, misaligned rows (views into longer buffers) with poisoned outputs
and workspace, every call made twice for the same bits; their stream contract by the method of tests/stream_cases.py; and KMeans / lloyd on
device tensors against sklearn's results of tests/golden/kmeans.npz.  Each test prints its worst error / bound."""
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.extract import clusters as CL
from tests import kmeans_refs as R
from tests import stream_cases as S
from tests.f64_bounds import check_written
from tests.neighbors_refs import assert_inside
from tests.strided_inputs import FLOAT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans.npz"))
POISON = -7
NAN = float("nan")


def vector(v_np, device):
    """a float vector one element into its buffer (4-byte aligned only), or None"""
    if v_np is None:
        return None, None
    v = Strided.of(v_np[None], 1, device, row_stride=v_np.shape[0], tail=1)
    return v, v.ptr


def padded(n, dtype, fill, device, before=3, after=4):
    """(buffer, the n elements in its middle)"""
    buf = torch.full((before + n + after,), fill, dtype=dtype, device=device)
    return buf, buf[before:before + n]


def written(buf, n, what, before=3):
    if buf.dtype.is_floating_point:
        mask = torch.zeros(buf.shape, dtype=torch.bool)
        mask[before:before + n] = True
        check_written(buf, mask, what)
    else:
        edge = torch.cat([buf[:before], buf[before + n:]]).cpu()
        assert bool((edge == POISON).all()), f"{what}: written outside the output"


def same_bits(a, b):
    return S.same_bits(a, b)


# ------------------------------------------------------------------------------------------------------------------ assignment
@surround_rule(*FLOAT_SURROUNDS)
def assign_call(x_np, offset_np, centres_np, device, labels_in=None, want_key=True, want_changed=True):
    """mmk_kmeans_assign_f32 on strided, misaligned rows -> (labels int32, key or None, changed or None)"""
    lib = native.lib()
    x, c = Strided.of(x_np, 1, device), Strided.of(centres_np, 2, device)
    obuf, optr = vector(offset_np, device)
    n, d, k = x.rows, x.k, c.rows
    shift = torch.full((k + 3,), NAN, dtype=torch.float32, device=device)
    native.check(lib.mmk_half_neg_sqnorm_f32(c.ptr, c.stride, k, d, shift.data_ptr(), native.stream_ptr(device)))
    lbuf, labels = padded(n, torch.int32, POISON, device, before=1)
    if labels_in is not None:
        labels.copy_(labels_in)
    kbuf, key = padded(n, torch.float32, NAN, device, before=1)
    chbuf, changed = padded(1, torch.int64, POISON, device, before=1, after=1)
    changed.zero_()
    native.check(lib.mmk_kmeans_assign_f32(x.ptr, x.stride, optr, n, d, c.ptr, c.stride, shift.data_ptr(), k, labels.data_ptr(),
                                           key.data_ptr() if want_key else None, changed.data_ptr() if want_changed else None,
                                           native.stream_ptr(device)))
    written(lbuf, n, f"labels {n, d, k}", before=1)
    if want_key:
        written(kbuf, n, f"key {n, d, k}", before=1)
    else:
        assert bool(torch.isnan(kbuf).all()), "key was written though NULL was passed"
    written(chbuf, 1, "changed", before=1)
    assert np.array_equal(x.view.cpu().numpy(), x_np) and np.array_equal(c.view.cpu().numpy(), centres_np), "an input was written"
    return labels, key if want_key else None, int(changed) if want_changed else None


def check_assign(x_np, offset_np, centres_np, device, what):
    """two calls, the same bits; the label rule; the changed count against the poison and against its own labels -> (labels, worst, left)"""
    n = x_np.shape[0]
    labels, key, changed = assign_call(x_np, offset_np, centres_np, device)
    again_l, again_k, _ = assign_call(x_np, offset_np, centres_np, device)
    assert torch.equal(labels, again_l) and same_bits(key, again_k), f"{what}: two calls differ"
    assert changed == n, f"{what}: {changed} of {n} rows changed from the poison"
    xp = R.centred(x_np, offset_np)
    key64, bound = R.key64(xp, centres_np), R.key_bound(xp, centres_np)
    lab = labels.cpu().numpy()
    bad, left = R.label_rule_violations(lab, None, key64, bound)
    assert not bad.any(), f"{what}: rows {np.nonzero(bad)[0][:8]} break the label rule: {lab[bad][:8]}"
    rows = np.arange(n)
    worst = assert_inside(key.cpu().numpy().astype(np.float64), key64[rows, lab], bound[rows, lab] + 1e-300, what)
    # from its own labels nothing changes; from float64's labels with one moved, one does; without key / changed nothing else is written
    l2, _, ch2 = assign_call(x_np, offset_np, centres_np, device, labels_in=labels, want_key=False)
    assert ch2 == 0 and torch.equal(l2, labels), f"{what}: {ch2} rows changed from the call's own labels"
    moved = labels.clone()
    moved[n // 2] = (moved[n // 2] + 1) % max(centres_np.shape[0], 2)
    l3, _, ch3 = assign_call(x_np, offset_np, centres_np, device, labels_in=moved, want_changed=False)
    assert ch3 is None and torch.equal(l3, labels)
    if centres_np.shape[0] > 1:
        assert assign_call(x_np, offset_np, centres_np, device, labels_in=moved)[2] == 1
    return lab, worst, int(left.sum())


@pytest.mark.parametrize("k", R.KS)
def test_assign_against_the_bound(device, k):
    worst, most_left = 0.0, 0.0
    for n in R.NS:
        for d in R.DS:
            x, offset, centres = R.kernel_case(n, d, k)
            _, w, left = check_assign(x, offset, centres, device, f"assign n {n}, d {d}, k {k}")
            assert left <= R.LEFT_CAP * n
            worst, most_left = max(worst, w), max(most_left, left / n)
    x, _, centres = R.kernel_case(257, 33, k, with_offset=False)
    _, w, _ = check_assign(x, None, centres, device, f"assign n 257, d 33, k {k}, no offset")
    print(f"kmeans_assign k {k}: worst key error / bound {max(worst, w):.3f}; at most {most_left:.4f} of a case's rows under the second rule")


@pytest.mark.parametrize("with_offset", (True, False))
def test_assign_special_inputs(device, with_offset):
    x, offset, centres = R.special_case(with_offset)
    lab, worst, _ = check_assign(x, offset, centres, device, f"assign special, offset {with_offset}")
    a, b = R.SAME_CENTRES
    assert lab[10] == a and (lab != b).all(), "of two identical centres the lower index takes the rows"
    assert (lab != R.FAR_CENTRE).all()
    labels, key, _ = assign_call(x, offset, centres, device)
    r0, r1 = R.COPY_ROWS
    assert lab[r0] == lab[r1] and same_bits(key[r0:r0 + 1], key[r1:r1 + 1]), "two identical rows differ in label or key bits"
    zero_key = float(key[R.ZERO_ROW])
    c = centres[lab[R.ZERO_ROW]].astype(np.float64)
    assert zero_key == float(np.float32(-0.5 * (c * c).sum())), "the key of a zero row is not its centre's shift"
    print(f"kmeans_assign special inputs (offset {with_offset}): worst key error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ sums
@surround_rule(*FLOAT_SURROUNDS)
def sums_call(x_np, offset_np, labels_np, k, device, centres_np=None, want_d2=True, want_inertia=True):
    lib = native.lib()
    x = Strided.of(x_np, 1, device)
    obuf, optr = vector(offset_np, device)
    n, d = x.rows, x.k
    labels = Strided.of(labels_np.astype(np.int32)[None], 4, device, row_stride=n, decoy=(0, k)).view[0]      # (contiguous: decoy labels in front and behind)
    n_work = lib.mmk_kmeans_label_sums_workspace_bytes(n, d, k)
    assert 0 < n_work <= (native.KMEANS_MAX_SLABS * (k * (d + 1) + 1)) * 8
    work = torch.full((n_work // 8 + 3,), NAN, dtype=torch.float64, device=device)
    sbuf, sums = padded(k * d, torch.float64, NAN, device)
    cbuf, counts = padded(k, torch.int64, POISON, device)
    dbuf, d2 = padded(n, torch.float64, NAN, device)
    ibuf, inertia = padded(1, torch.float64, NAN, device)
    c = Strided.of(centres_np, 2, device) if centres_np is not None else None
    native.check(lib.mmk_kmeans_label_sums_f64(x.ptr, x.stride, optr, n, d, labels.data_ptr(), k, sums.data_ptr(), counts.data_ptr(),
                                               c.ptr if c else None, c.stride if c else 0, d2.data_ptr() if c and want_d2 else None,
                                               inertia.data_ptr() if c and want_inertia else None, work.data_ptr(), n_work, native.stream_ptr(device)))
    written(sbuf, k * d, f"sums {n, d, k}")
    written(cbuf, k, f"counts {n, d, k}")
    assert bool(torch.isnan(work[n_work // 8:]).all()), "the workspace was written beyond its size"
    assert np.array_equal(x.view.cpu().numpy(), x_np) and np.array_equal(labels.cpu().numpy(), labels_np), "an input was written"
    if c and want_d2:
        written(dbuf, n, "row_d2")
    else:
        assert bool(torch.isnan(dbuf).all()), "row_d2 was written though it was not asked for"
    if c and want_inertia:
        written(ibuf, 1, "inertia")
    else:
        assert bool(torch.isnan(ibuf).all()), "inertia was written though it was not asked for"
    return sums.reshape(k, d), counts, d2 if c and want_d2 else None, inertia[0] if c and want_inertia else None


def check_sums(x_np, offset_np, labels_np, centres_np, device, what):
    k, d = centres_np.shape
    n = x_np.shape[0]
    sums, counts, d2, inertia = sums_call(x_np, offset_np, labels_np, k, device, centres_np)
    a_s, a_c, a_d, a_i = sums_call(x_np, offset_np, labels_np, k, device, centres_np)
    assert same_bits(sums, a_s) and torch.equal(counts, a_c) and same_bits(d2, a_d) and same_bits(inertia.reshape(1), a_i.reshape(1)), f"{what}: two calls differ"
    plain = sums_call(x_np, offset_np, labels_np, k, device)                       # without centres: the same sums, nothing else written
    assert same_bits(plain[0], sums) and torch.equal(plain[1], counts)
    only_i = sums_call(x_np, offset_np, labels_np, k, device, centres_np, want_d2=False)
    assert same_bits(only_i[3].reshape(1), inertia.reshape(1)), "inertia without row_d2 has other bits"
    only_d = sums_call(x_np, offset_np, labels_np, k, device, centres_np, want_inertia=False)
    assert same_bits(only_d[2], d2)
    xp = R.centred(x_np, offset_np)
    want, want_counts, asum = R.label_sums64(xp, labels_np, k)
    assert np.array_equal(counts.cpu().numpy(), want_counts), f"{what}: counts"
    worst = assert_inside(sums.cpu().numpy(), want, R.sums_bound(want_counts, asum) + 1e-300, what + " sums")
    empty = want_counts == 0
    assert not sums.cpu().numpy()[empty].any(), "a label without a row has a sum other than 0"
    want_d2 = R.row_d2_64(xp, labels_np, centres_np)
    worst = max(worst, assert_inside(d2.cpu().numpy(), want_d2, R.d2_bound(want_d2, d) + 1e-300, what + " row_d2"))
    total = float(want_d2.sum())
    worst = max(worst, assert_inside(np.array([float(inertia)]), np.array([total]), np.array([R.total_bound(total, n, d) + 1e-300]), what + " inertia"))
    return worst


@pytest.mark.parametrize("k", R.KS)
def test_label_sums_against_the_bound(device, k):
    worst = 0.0
    for n in R.NS:
        for d in R.DS:
            x, offset, centres = R.kernel_case(n, d, k)
            labels = R.first_argmax(R.key64(R.centred(x, offset), centres))
            worst = max(worst, check_sums(x, offset, labels, centres, device, f"label_sums n {n}, d {d}, k {k}"))
    x, _, centres = R.kernel_case(257, 33, k, with_offset=False)
    labels = R.rng_of(5).integers(0, k, 257)                                        # any labelling, not the nearest centre's
    worst = max(worst, check_sums(x, None, labels, centres, device, f"label_sums n 257, d 33, k {k}, no offset, random labels"))
    print(f"kmeans_label_sums k {k}: worst error / bound {worst:.3f}")


def test_label_sums_special_inputs_and_many_slabs(device):
    x, offset, centres = R.special_case()
    labels = R.first_argmax(R.key64(R.centred(x, offset), centres))
    worst = check_sums(x, offset, labels, centres, device, "label_sums special")
    outside = labels.copy()
    outside[[0, 7]] = [-1, centres.shape[0]]                                       # labels outside [0, k): their rows are left out
    worst = max(worst, check_sums(x, offset, outside, centres, device, "label_sums with labels outside"))
    rng = R.rng_of(6)
    big = (2.0 + rng.standard_normal((70001, 5))).astype(np.float32)              # 1024 slabs, the last ones short; a wave takes 8 rows at once
    c = rng.standard_normal((3, 5)).astype(np.float32)
    mu = big.astype(np.float64).mean(0).astype(np.float32)
    worst = max(worst, check_sums(big, mu, R.first_argmax(R.key64(R.centred(big, mu), c)), c, device, "label_sums 70001 rows"))
    print(f"kmeans_label_sums special inputs, labels outside, 70001 rows: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ seeding step
@surround_rule(*FLOAT_SURROUNDS)
def pp_call(x_np, offset_np, cand_np, closest_np, device):
    lib = native.lib()
    x = Strided.of(x_np, 1, device)
    obuf, optr = vector(offset_np, device)
    n, d = x.rows, x.k
    cand = Strided.of(np.asarray(cand_np, dtype=np.int64)[None], 4, device, row_stride=len(cand_np), decoy=(0, n)).view[0]
    cbuf, closest = padded(n, torch.float64, NAN, device)
    closest.copy_(torch.from_numpy(closest_np))
    pbuf, pot = padded(1, torch.float64, NAN, device)
    hbuf, chosen = padded(1, torch.int64, POISON, device)
    n_work = lib.mmk_kmeans_pp_step_workspace_bytes()
    work = torch.full((n_work // 8 + 3,), NAN, dtype=torch.float64, device=device)
    native.check(lib.mmk_kmeans_pp_step_f64(x.ptr, x.stride, optr, n, d, cand.data_ptr(), cand.shape[0], closest.data_ptr(), pot.data_ptr(),
                                            chosen.data_ptr(), work.data_ptr(), n_work, native.stream_ptr(device)))
    written(cbuf, n, "closest")
    written(pbuf, 1, "pot")
    written(hbuf, 1, "chosen")
    assert bool(torch.isnan(work[n_work // 8:]).all()), "the workspace was written beyond its size"
    assert np.array_equal(x.view.cpu().numpy(), x_np) and cand.cpu().tolist() == list(cand_np), "an input was written"
    return closest, pot[0], int(chosen)


def check_pp(x_np, offset_np, cand, closest_np, device, what):
    n, d = x_np.shape
    closest, pot, chosen = pp_call(x_np, offset_np, cand, closest_np, device)
    a_c, a_p, a_h = pp_call(x_np, offset_np, cand, closest_np, device)
    assert same_bits(closest, a_c) and same_bits(pot.reshape(1), a_p.reshape(1)) and chosen == a_h, f"{what}: two calls differ"
    xp = R.centred(x_np, offset_np)
    _, _, t, pots = R.pp_step64(xp, cand, closest_np)
    pb = np.array([R.total_bound(p, n, d) for p in pots]) + 1e-300
    safe = all(pots[i] - pots[t] > pb[i] + pb[t] for i in range(len(cand)) if cand[i] != cand[t])
    at = list(cand).index(chosen)
    if safe:
        assert chosen == cand[t], f"{what}: row {chosen} was chosen, float64 chooses {cand[t]} by a clear gap"
    else:
        assert pots[at] - pots[t] <= pb[at] + pb[t], f"{what}: the chosen pot is not within the bound of the smallest"
    want = np.minimum(closest_np, ((xp.astype(np.float64) - xp[chosen].astype(np.float64)) ** 2).sum(-1))
    worst = assert_inside(closest.cpu().numpy(), want, R.d2_bound(want, d) + 1e-300, what + " closest")
    worst = max(worst, assert_inside(np.array([float(pot)]), pots[at:at + 1], pb[at:at + 1], what + " pot"))
    same = closest.cpu().numpy() == closest_np
    assert (same | (closest.cpu().numpy() < closest_np)).all(), "closest rose somewhere"
    return worst, closest.cpu().numpy(), float(pot)


def test_pp_step_against_the_bound(device):
    worst = 0.0
    for n in R.NS:
        for d in R.DS:
            x, offset, _ = R.kernel_case(n, d, 16)
            rng = R.rng_of(n + d)
            w, closest, pot = check_pp(x, offset, [int(rng.integers(0, n))], np.full(n, np.inf), device, f"pp_step init n {n}, d {d}")
            cand = rng.integers(0, n, native.KMEANS_PP_MAX_TRIALS).tolist()
            cand[5] = cand[2]                                                        # a repeated candidate
            w2, closest2, _ = check_pp(x, offset, cand, closest, device, f"pp_step 8 candidates n {n}, d {d}")
            w3, _, _ = check_pp(x, None, cand[:3], closest2, device, f"pp_step 3 candidates, no offset, n {n}, d {d}")
            worst = max(worst, w, w2, w3)
    x, offset, _ = R.special_case()
    w, closest, pot = check_pp(x, offset, [R.COPY_ROWS[0]], np.full(200, np.inf), device, "pp_step special")
    assert closest[R.COPY_ROWS[0]] == closest[R.COPY_ROWS[1]] == 0.0
    w2, _, _ = check_pp(x, offset, [R.ZERO_ROW, R.COPY_ROWS[1], R.ZERO_ROW], closest, device, "pp_step special, repeated")
    print(f"kmeans_pp_step: worst error / bound {max(worst, w, w2):.3f}")


def test_wrappers_refuse_what_the_header_refuses(device):
    x = torch.zeros((40, 5), device=device)
    labels = torch.zeros((40,), dtype=torch.int32, device=device)
    with pytest.raises(NotImplementedError, match=str(native.KMEANS_MAX_K)):
        native.kmeans_assign(torch.zeros((300, 5), device=device), None, torch.zeros((native.KMEANS_MAX_K + 1, 5), device=device),
                             torch.zeros((300,), dtype=torch.int32, device=device))
    with pytest.raises(TypeError):
        native.kmeans_assign(x, None, x[:4], labels.long())
    with pytest.raises(ValueError):
        native.kmeans_assign(x, None, x[:4, :3], labels)
    with pytest.raises(NotImplementedError, match=str(native.KMEANS_PP_MAX_TRIALS)):
        native.kmeans_pp_step(x, None, torch.zeros((9,), dtype=torch.int64, device=device), torch.zeros((40,), dtype=torch.float64, device=device),
                              torch.zeros((), dtype=torch.float64, device=device), torch.zeros((), dtype=torch.int64, device=device))
    lib = native.lib()
    assert lib.mmk_kmeans_assign_f32(x.data_ptr(), 5, None, 40, 5, x.data_ptr(), 5, x.data_ptr(), native.KMEANS_MAX_K + 1, labels.data_ptr(), None, None,
                                     native.stream_ptr(device)) == -3
    assert lib.mmk_kmeans_label_sums_f64(x.data_ptr(), 5, None, 40, 5, labels.data_ptr(), 4, x.data_ptr(), x.data_ptr(), None, 0, None, None,
                                         x.data_ptr(), 8, native.stream_ptr(device)) == -4
    assert lib.mmk_kmeans_pp_step_f64(x.data_ptr(), 5, None, 0, 5, x.data_ptr(), 1, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 1 << 20,
                                      native.stream_ptr(device)) == -1
    with pytest.raises(NotImplementedError, match=str(native.KMEANS_MAX_K)):
        mmk.KMeans(n_clusters=native.KMEANS_MAX_K + 1).fit(torch.zeros((300, 5), device=device))
    with pytest.raises(ValueError, match="at least 8 frames"):
        mmk.KMeans(n_clusters=8).fit(x[:7])
    print("kmeans wrappers: worst error / bound 0.000 (refusals)")


# ------------------------------------------------------------------------------------------------------------------ the stream contract
SN, SD, SK = 257, 33, 33          # one past two workgroups' rows, one past a chunk of bins, one past a 32-column product


def _stream_assign():
    def build(seed):
        g = S.gen(seed)
        c = S.uni(S.gen(9), SK, SD)
        return dict(x=S.uni(g, SN, SD) + 1.0, offset=torch.ones(SD), centres=c, shift=(-(c.double() ** 2).sum(-1) / 2).float())

    def call(L, a, s):
        return L.mmk_kmeans_assign_f32(S.P(a["x"]), SD, S.P(a["offset"]), SN, SD, S.P(a["centres"]), SD, S.P(a["shift"]), SK, S.P(a["labels"]), S.P(a["key"]),
                                       S.P(a["changed"]), s)
    return S.Case("mmk_kmeans_assign_f32", build, lambda L, i: dict(labels=((SN,), torch.int32), key=((SN,), torch.float32), changed=((1,), torch.int64)), call)


def _stream_label_sums():
    def build(seed):
        g = S.gen(seed)
        return dict(x=S.uni(g, SN, SD), offset=torch.full((SD,), 0.25), labels=torch.randint(0, SK, (SN,), generator=g).to(torch.int32),
                    centres=S.uni(S.gen(9), SK, SD))

    def call(L, a, s):
        return L.mmk_kmeans_label_sums_f64(S.P(a["x"]), SD, S.P(a["offset"]), SN, SD, S.P(a["labels"]), SK, S.P(a["sums"]), S.P(a["counts"]), S.P(a["centres"]),
                                           SD, S.P(a["row_d2"]), S.P(a["inertia"]), S.P(a["ws"]), a["ws"].numel(), s)
    return S.Case("mmk_kmeans_label_sums_f64", build,
                  lambda L, i: dict(sums=((SK, SD), torch.float64), counts=((SK,), torch.int64), row_d2=((SN,), torch.float64), inertia=((1,), torch.float64)),
                  call, work=lambda L, i: dict(ws=L.mmk_kmeans_label_sums_workspace_bytes(SN, SD, SK)))


def _stream_pp_step():
    def build(seed):
        g = S.gen(seed)
        return dict(x=S.uni(g, SN, SD), offset=torch.full((SD,), 0.25), cand=torch.randint(0, SN, (5,), generator=g),
                    closest=S.uni(g, SN, lo=0.5, hi=30.0).double())

    def call(L, a, s):      # (closest is IN/OUT: the input buffer itself, which every run puts in place again, is updated)
        return L.mmk_kmeans_pp_step_f64(S.P(a["x"]), SD, S.P(a["offset"]), SN, SD, S.P(a["cand"]), 5, S.P(a["closest"]), S.P(a["pot"]), S.P(a["chosen"]),
                                        S.P(a["ws"]), a["ws"].numel(), s)
    return S.Case("mmk_kmeans_pp_step_f64", build, lambda L, i: dict(pot=((1,), torch.float64), chosen=((1,), torch.int64)), call,
                  work=lambda L, i: dict(ws=L.mmk_kmeans_pp_step_workspace_bytes()))


STREAM_CASES = [_stream_assign(), _stream_label_sums(), _stream_pp_step()]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.id for c in STREAM_CASES])
def test_entry_point_behind_a_busy_side_stream(device, case):
    """tests/test_gpu_streams.py's method: the real input twice on the default stream (the same bits), the stale input once (other bits),
    then behind a delay and a late write of the input on a side stream: the default-stream bits, and the call came back while the stream
    was still busy"""
    bound = S.Bound(case, device)
    want = bound.run_default("real")
    again = bound.run_default("real")
    assert not S.differs(want, again), (case.id, "two default-stream calls disagree")
    bound.check_surround(case.id + " on the default stream")
    stale = bound.run_default("stale")
    assert S.differs(want, stale), (case.id, "the stale input gives the real input's bits: the case proves nothing")
    got, busy, host = S.late_input(bound, S.side_stream(device))
    print(f"[streams] {case.id}: host time of the call {host * 1e3:.3f} ms, busy on return: {busy}")
    assert not S.differs(want, got), (case.id, "behind a late input on a side stream the outputs differ from the default-stream run")
    bound.check_surround(case.id + " on the side stream")
    assert busy, (case.id, f"the call waited for its stream (or took {host * 1e3:.1f} ms on the host)")


# ------------------------------------------------------------------------------------------------------------------ end to end
def centre_and_inertia_bounds(x, res):
    """the device's centres (input coordinates) and inertia against the restatement's: kmeans_refs' cerr, the two float32 additions of mu,
    and what cerr moves the inertia by"""
    xp = R.centred(x, res["mu"]).astype(np.float64)
    c, cerr, labels = res["centres_c"].astype(np.float64), res["cerr"], res["labels"]
    cb = cerr * (1 + R.U) + 2 * R.U * np.abs(res["centres"].astype(np.float64)) + 1e-300
    diff = np.abs(xp - c[labels])
    ib = float((2 * diff * cerr[labels] + cerr[labels] ** 2).sum()) + R.total_bound(res["inertia"], *x.shape)
    return cb, ib


def check_fit(got_labels, got_centres, got_inertia, got_iter, x, res, name):
    assert got_labels.device.type == "cuda" and got_labels.dtype == torch.int64 and got_labels.shape == (x.shape[0],)
    assert got_centres.device.type == "cuda" and got_centres.dtype == torch.float32 and type(got_inertia) is float and type(got_iter) is int
    wrong = int((got_labels.cpu().numpy() != G[f"{name}_labels"]).sum())
    print(f"{name}: n_iter {got_iter} (sklearn {int(G[f'{name}_n_iter'])}), {wrong} of {x.shape[0]} labels differ from sklearn's")
    assert wrong == 0 and got_iter == int(G[f"{name}_n_iter"])
    cb, ib = centre_and_inertia_bounds(x, res)
    worst = assert_inside(got_centres.cpu().numpy().astype(np.float64), res["centres"].astype(np.float64), cb, f"{name} centres")
    worst = max(worst, assert_inside(np.array([got_inertia]), np.array([res["inertia"]]), np.array([ib]), f"{name} inertia"))
    return worst


@pytest.mark.parametrize("name", sorted(R.FIT_FIXTURES))
def test_kmeans_against_sklearn(device, name):
    k, seed, _, max_iter = R.FIT_FIXTURES[name][2:]
    x_np = R.fit_corpus(name)
    x = torch.from_numpy(x_np.copy()).to(device)
    km = mmk.KMeans(n_clusters=k, max_iter=max_iter, random_seed=seed).fit(x)
    assert np.array_equal(km.seed_rows_.cpu().numpy(), G[f"{name}_seed_rows"]), f"{name}: seed rows {km.seed_rows_.cpu().tolist()}"
    worst = check_fit(km.labels_, km.cluster_centers_, km.inertia_, km.n_iter_, x_np, R.fit_result(name), name)
    again = mmk.KMeans(n_clusters=k, max_iter=max_iter, random_seed=seed)
    assert torch.equal(again(x), km.labels_) and same_bits(again.cluster_centers_, km.cluster_centers_) and again.inertia_ == km.inertia_
    assert again.n_iter_ == km.n_iter_ and torch.equal(again.seed_rows_, km.seed_rows_)
    assert np.array_equal(x.cpu().numpy(), x_np), "fit wrote its input"
    print(f"KMeans {name}: worst centre / inertia error over bound {worst:.3f}")


@pytest.mark.parametrize("name", sorted(R.LLOYD_FIXTURES))
def test_lloyd_from_an_init_with_an_empty_cluster(device, name):
    x_np, init_np = R.lloyd_corpus(name)
    x, init = torch.from_numpy(x_np.copy()).to(device), torch.from_numpy(init_np.copy()).to(device)
    labels, inertia, centres, n_iter = CL.lloyd(x, init)
    worst = check_fit(labels, centres, inertia, n_iter, x_np, R.lloyd_result(name), name)
    one = CL.lloyd(x, init, max_iter=1)
    want = R.lloyd_from64(x_np, init_np, max_iter=1)
    assert np.array_equal(one[0].cpu().numpy(), want["labels"]) and one[3] == 1, "after one iteration the relocated frame's cluster differs"
    assert int(torch.bincount(one[0], minlength=init.shape[0]).min()) > 0
    l2, i2, c2, n2 = CL.lloyd(x, init)
    assert torch.equal(l2, labels) and i2 == inertia and same_bits(c2, centres) and n2 == n_iter
    print(f"lloyd {name}: worst centre / inertia error over bound {worst:.3f}")


def test_kmeans_after_magspec_and_pca_stays_on_the_device(device):
    g = torch.Generator().manual_seed(3)
    t = torch.arange(48000) / 16000.0
    wave = torch.cat([torch.sin(2 * torch.pi * f * t[:12000]) for f in (220.0, 880.0, 1760.0, 3520.0)]) + 0.05 * torch.randn(48000, generator=g)
    chain = mmk.Compose(mmk.MagSpec(), mmk.PCA(16), mmk.KMeans(n_clusters=4))
    labels = chain(wave.to(device))
    assert labels.device.type == "cuda" and labels.dtype == torch.int64 and labels.dim() == 1
    km = chain.functionals[-1]
    assert km.cluster_centers_.shape == (4, 16) and km.cluster_centers_.device.type == "cuda" and km.n_iter_ >= 1
    low = mmk.Compose(mmk.MagSpec(), mmk.PCA(16))(wave.to(device))
    assert low.device.type == "cuda" and low.shape == (labels.shape[0], 16)
    assert torch.equal(mmk.KMeans(n_clusters=4)(low), labels), "KMeans at the end of a chain differs from KMeans on the chain's output"
    res = R.fit64(low.cpu().numpy(), 4)
    fair = res["ratio"] >= 1.0 and res["margin"] >= 1e-9 and res["shift_margin"] >= 1e-6
    wrong = int((labels.cpu().numpy() != res["labels"]).sum())
    print(f"Compose(MagSpec, PCA(16), KMeans(4)): {labels.shape[0]} frames, sizes {torch.bincount(labels).cpu().tolist()}, n_iter {km.n_iter_}; gap ratio "
          f"{res['ratio']:.2f}, {wrong} labels differ from the float64 restatement on the device's PCA output; worst error / bound 0.000 (integers)")
    assert not fair or (wrong == 0 and km.n_iter_ == res["n_iter"]), "the restatement's conditions hold and the labels differ"
