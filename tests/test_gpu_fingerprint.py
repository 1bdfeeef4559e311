"""The weight fingerprint on the device (csrc/linear.hip: fingerprint_kernel behind mmk_fingerprint_u32 / mmk_fingerprint_buffers_u32)
against the numpy restatement of tests/fingerprint_refs.py, and what hangs on it: a write through .data into any entry of any of the four
networks must lead to a repack where the next generation starts (mimikit_amd/native.py: WeightsTracker)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from oracle.weights import recipe_state_dict
from tests import fingerprint_refs as R
from tests import net_refs as N

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
INVALID = -1          # MMK_ERR_INVALID (include/mmk.h)


def _one(view):
    out = torch.empty(1, dtype=torch.int64, device=view.device)
    native.check(native.lib().mmk_fingerprint_u32(native.ptr(view), view.numel(), native.ptr(out), native.stream_ptr(view.device)), "mmk_fingerprint_u32")
    return R.unsigned(out.item())


def _many(views):
    k = len(views)
    ptrs = (C.c_void_p * k)(*[v.data_ptr() for v in views])
    counts = (C.c_int64 * k)(*[v.numel() for v in views])
    out = torch.empty(1, dtype=torch.int64, device=views[0].device)
    native.check(native.lib().mmk_fingerprint_buffers_u32(ptrs, counts, k, native.ptr(out), native.stream_ptr(views[0].device)),
                 "mmk_fingerprint_buffers_u32")
    return R.unsigned(out.item())


def _words(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32))


def _at(pool, start, off, n):
    """the view of n words that starts `off` words past a 16-byte boundary at or after word `start` of the pool"""
    assert pool.data_ptr() % 16 == 0
    a = -(-start // 4) * 4 + off
    v = pool[a:a + n]
    assert v.numel() == n and (n == 0 or (v.data_ptr() // 4) % 4 == off)      # (an empty view has no address to speak of)
    return v


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------
def test_one_buffer_equals_the_reference_at_every_alignment(device):
    """the 16-byte path with its n % 4 tail (offset 0) and the word path (offsets 1 - 3): the same content at the same positions gives the same
    number, the reference's; all-zero content too, where a workgroup whose sum is 0 skips its atomic"""
    sizes = (0, 1, 3, 4, 5, 8191, 8192, 8193, 2 ** 20 + 3)
    src = _words(max(sizes), 11)
    pool = torch.empty(max(sizes) + 8, dtype=torch.int32, device=device)
    for content in ("random", "zeros"):
        for n in sizes:
            host = src[:n] if content == "random" else torch.zeros(n, dtype=torch.int32)
            want = R.fingerprint(R.words(host))
            for off in (0, 1, 2, 3):
                pool.fill_(-1)
                v = _at(pool, 0, off, n)
                v.copy_(host)
                got = _one(v)
                assert got == want, f"{content}, n={n}, {off} words past a 16-byte boundary: {got:#x}, want {want:#x}"
                assert _one(v) == got                                  # two calls, one number
    assert R.fingerprint(np.zeros(8193, dtype=np.uint32)) != 0


@pytest.mark.parametrize("k", [1, 2, 95, 96, 97, 193])
def test_buffers_equal_their_concatenation(device, k):
    """one launch per 96 buffers, the positions continue from launch to launch; lengths 0, 1, 5, 8193 and 20000 at mixed alignments, empty
    buffers in front, on both sides of the launch boundary and at the end"""
    lengths = [(0, 1, 5, 8193, 20000, 5, 1)[(3 * i + k) % 7] for i in range(k)]
    for i in (0, 95, 96, k - 1):
        if i < k and k > 2:
            lengths[i] = 0
    if k <= 2:
        lengths = [8193, 0][:k]
    total = sum(lengths)
    src = _words(total, 100 + k)
    pool = torch.full((total + 8 * k + 8,), -1, dtype=torch.int32, device=device)
    views, start, pos = [], 0, 0
    for i, n in enumerate(lengths):
        v = _at(pool, start, (i + i // 4) % 4, n)
        v.copy_(src[pos:pos + n])
        views.append(v)
        start, pos = -(-start // 4) * 4 + 3 + n + 1, pos + n
    assert {(v.data_ptr() // 4) % 4 for v in views if v.numel() > 4} == ({0, 1, 2, 3} if k > 4 else {0})
    want = R.fingerprint(R.words(src))
    assert R.fingerprint_buffers([src[a:a + n] for a, n in zip(np.cumsum([0] + lengths[:-1]), lengths)]) == want
    got = _many(views)
    assert got == want, f"{k} buffers: {got:#x}, want {want:#x}"
    assert _many(views) == got
    joined = pool.new_empty(total + 4)[:total]
    joined.copy_(src)
    assert _one(joined) == want
    if k > 2:
        # positions restarting at a launch: what a `pos0` that does not continue would compute
        restart = sum(R.fingerprint_buffers([src[a:a + n] for a, n in list(zip(np.cumsum([0] + lengths[:-1]), lengths))[f:f + R.MAX_BUFFERS]])
                      for f in range(0, k, R.MAX_BUFFERS)) % 2 ** 64
        assert (restart != want) == (sum(lengths[R.MAX_BUFFERS:]) > 0)       # (97 buffers: the second launch has one empty buffer, and is skipped)
        assert k != 193 or restart != want


def test_every_change_moves_the_number(device):
    def flipped(view, i, bit=7):
        mask = (1 << bit) if bit < 31 else -2 ** 31
        view[i] ^= mask
        got = _one(view)
        assert got == R.fingerprint(R.words(view))
        view[i] ^= mask
        return got

    for n in (8192, 8197):                       # the 16-byte path: without a tail, with a tail of one word
        pool = torch.empty(n + 8, dtype=torch.int32, device=device)
        v = _at(pool, 0, 0, n)
        v.copy_(_words(n, n))
        base = _one(v)
        assert base == R.fingerprint(R.words(v))
        seen = {"first word": flipped(v, 0), "last word": flipped(v, n - 1), "first word, top bit": flipped(v, 0, 31),
                "last word of the last 16 bytes": flipped(v, (n & ~3) - 1)}
        w = v.clone()
        assert w.data_ptr() % 16 == 0 and int(w[4000]) != int(w[4001])
        w[4000], w[4001] = v[4001].clone(), v[4000].clone()
        seen["two adjacent words swapped"] = _one(w)
        long = _words(n + 1, 3 * n).to(device)
        a, b = long[:n].clone(), long[1:].clone()                         # the same words one place on, in a buffer of the same alignment
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and torch.equal(a[1:], b[:-1])
        assert _one(b) != _one(a), "a copy shifted by one word"
        for what, got in seen.items():
            assert got != base, f"n={n}: {what}"
        assert _one(v) == base
    # among many buffers
    k, n = 193, 1000
    pool = torch.empty(k * (n + 4), dtype=torch.int32, device=device)
    pool.copy_(_words(pool.numel(), 9))
    views = [_at(pool, i * (n + 4), i % 4 if i % 3 else 0, n - (i % 4 if i % 3 else 0)) for i in range(k)]
    base = _many(views)
    assert base == R.fingerprint_buffers(views)
    views[96][5] ^= 1
    assert _many(views) != base, "one bit in buffer 97 of 193"
    views[96][5] ^= 1
    views[192][-1] ^= 1
    assert _many(views) != base, "one bit in the last word of the last buffer"
    views[192][-1] ^= 1
    assert _many(views) == base
    assert views[3].numel() == views[99].numel() and not torch.equal(views[3], views[99])
    swapped = list(views)
    swapped[3], swapped[99] = views[99], views[3]
    got = _many(swapped)
    assert got != base and got == R.fingerprint_buffers(swapped), "the contents of two buffers of equal length swapped"


def test_refusals(device):
    lib = native.lib()
    buf = torch.zeros(16, dtype=torch.int32, device=device)
    out = torch.zeros(1, dtype=torch.int64, device=device)
    stream = native.stream_ptr(device)
    one = (C.c_void_p * 1)(buf.data_ptr())
    null = (C.c_void_p * 1)(None)
    assert lib.mmk_fingerprint_u32(native.ptr(buf), 16, None, stream) == INVALID
    assert lib.mmk_fingerprint_u32(native.ptr(buf), -1, native.ptr(out), stream) == INVALID
    assert lib.mmk_fingerprint_u32(None, 16, native.ptr(out), stream) == INVALID
    assert lib.mmk_fingerprint_buffers_u32(one, (C.c_int64 * 1)(16), -1, native.ptr(out), stream) == INVALID
    assert lib.mmk_fingerprint_buffers_u32(one, (C.c_int64 * 1)(-16), 1, native.ptr(out), stream) == INVALID
    assert lib.mmk_fingerprint_buffers_u32(null, (C.c_int64 * 1)(16), 1, native.ptr(out), stream) == INVALID
    assert lib.mmk_fingerprint_buffers_u32(None, None, 1, native.ptr(out), stream) == INVALID
    assert lib.mmk_fingerprint_buffers_u32(one, (C.c_int64 * 1)(16), 1, None, stream) == INVALID
    # what is allowed: no buffers at all, and an empty buffer without an address
    assert lib.mmk_fingerprint_buffers_u32(None, None, 0, native.ptr(out), stream) == 0 and int(out.item()) == 0
    assert lib.mmk_fingerprint_u32(None, 0, native.ptr(out), stream) == 0 and int(out.item()) == 0


# ---- the four networks --------------------------------------------------------------------------------------------------------------------------------
def _transformer():
    """the small geometry of tests/test_gpu_transformer.py, filled by the recipe (the positional-encoding table as the network made it)"""
    io = mmk.IOSpec.mulaw_io(mmk.IOSpec.MuLawIOConfig(input_module_type="embedding", mlp_dim=32, n_mlp_layers=1))
    net = mmk.SimpleTransformer.from_config(mmk.SimpleTransformer.Config(io_spec=io, model_dim=64, n_heads=4, feedforward_dim=128, num_layers=2,
                                                                         rf=16)).eval()
    sd = net.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if torch.is_floating_point(v) and v.dim() > 0 and k != "pe.pe"}
    for k, v in recipe_state_dict(shapes, 74, 1.5).items():
        sd[k].copy_(v)
    return net


# kind: (make, clips, prompt length, blocks of steps) - the smallest geometries of tests/net_refs.py; the WaveNet with blocks (8, 8), whose
# state_dict has more entries than one launch of the kernel takes
NETWORKS = {
    "wavenet": (lambda: N._wavenet(32, (8, 8), 32, 21)[0], 2, 511 + 3, (4,)),
    "srnn": (lambda: N._srnn("gru", 128, (16, 4, 1), 78)[0], 2, 2 * 16 + 3, (44,)),
    "s2s": (lambda: N._s2s(128, 2, 1, 7 + 128 + 2)[0], 3, 2, (2, 2, 2)),
    "transformer": (_transformer, 2, 16 + 4, (8,)),
}


def _prompt(kind):
    _, B, P, _ = NETWORKS[kind]
    g = torch.Generator().manual_seed(5)
    return torch.rand(B, P, 65, generator=g) if kind == "s2s" else torch.randint(0, 256, (B, P), generator=g)


def _generate(net, kind, device, prompt=None):
    """one generation from before_generate on: (the classes or frames it wrote, the raw outputs the plan hands back), on the host"""
    _, B, P, parts = NETWORKS[kind]
    prompt = _prompt(kind) if prompt is None else prompt
    hist = torch.cat([prompt, torch.zeros(B, sum(parts), *prompt.shape[2:], dtype=prompt.dtype)], 1).to(device)
    net.before_generate((hist[:, :P],), None)
    t = P
    for nb in parts:
        assert net.generate_block((hist,), t, nb)
        t += nb
    if kind == "s2s":
        raw = hist[:, P:].clone()
    elif kind == "transformer":                   # one teacher-forced step more: the plan's raw head outputs
        net.generate_step((hist[:, t - net.rf:t],), t=t)
        raw = net._plan.last_logits(B).clone()
    else:
        raw = net._plan.last_logits(B).clone()
    net.after_generate((hist,), None)
    return hist[:, P:].cpu(), raw.cpu()


def _candidates(name, entry, kind, raw):
    """[(flat index, prompt or None)]: elements whose ulp can reach the compared outputs `raw`, best first.
    A class embedding: the row of the class the first clip's prompt ends on.  The bias of the head's last layer, one entry per output
    column: an ulp of the bias is lost where the output it is added to is much larger, so the columns whose outputs are smallest against
    their bias.  The input weights of a recurrent layer that reads frames (Seq2Seq's first entry): see _cancelling_frames.  Any other
    entry: the elements of largest magnitude (the largest ulp)."""
    flat = entry.detach().reshape(-1).abs().cpu()
    if kind == "s2s" and name.endswith("weight_ih_l0") and entry.shape[1] == 65:
        return [_cancelling_frames(entry.detach().cpu(), unit) for unit in range(8)]
    out = []
    if "input_module" in name and entry.dim() == 2 and entry.shape[0] == 256:
        last = int(_prompt(kind)[0, -1])
        out.append(last * entry.shape[1] + int(entry[last].abs().argmax()))
    if entry.dim() == 1 and entry.numel() == raw.shape[-1]:
        smallest = raw.reshape(-1, raw.shape[-1]).abs().min(0).values
        out += [int(i) for i in (flat / smallest.clamp_min(1e-30)).topk(4).indices]
    out += [int(i) for i in flat.topk(min(3, flat.numel())).indices]
    return [(j, None) for j in out[:4]]


def _cancelling_frames(w, row, scale=4096.0):
    """An ulp of an input weight w[row, k] of about 0.2 moves a gate's pre-activation of about 1 by a fraction of ITS ulp times the frame's
    bin k, and random frames in [0, 1) let it vanish in the rounding of the sum (measured: four elements of largest magnitude, no output
    bit moved).  So the first clip's frames hold two bins only: `scale` (a power of two: the product with the weight is exact) in the
    row's largest column k and -scale w[row, k] / w[row, m] in its second largest m.  The two products cancel, the pre-activation of
    `row` stays at its bias, and the ulp of w[row, k] arrives in it times 4096 - hundreds of its ulps.  The other rows' gates saturate,
    which stops no signal of this row's unit but where its output gate is shut: hence the rows of several units, until one moves the frames."""
    k, m = (int(i) for i in w[row].abs().topk(2).indices)
    prompt = _prompt("s2s")
    prompt[0] = 0.0
    prompt[0, :, k] = scale
    prompt[0, :, m] = float(-scale * w[row, k].double() / w[row, m].double())
    return row * w.shape[1] + k, prompt


@pytest.mark.parametrize("kind", list(NETWORKS))
def test_one_ulp_through_data_repacks(device, kind):
    """one element of the first fp32 entry, then of a late one (index >= 96 for the WaveNet, the last entry otherwise), moved by one ulp through
    .data - no version counter moves, no storage: only the content fingerprint can see it.  The next generation repacks and computes,
    bit for bit, what a freshly built network with that state_dict computes; written back, the first outputs return; nothing changed,
    nothing is packed"""
    make = NETWORKS[kind][0]
    net = make().to(device)
    names = [k for k, v in net.state_dict(keep_vars=True).items() if v.dtype == torch.float32 and v.numel() > 0]
    if kind == "wavenet":
        assert len(names) > R.MAX_BUFFERS, "the WaveNet's entries fit one launch"
    late = R.MAX_BUFFERS + 1 if kind == "wavenet" else len(names) - 1
    first = _generate(net, kind, device)
    entries = net.state_dict(keep_vars=True)
    want = R.fingerprint_buffers([entries[k] for k in names])
    assert R.unsigned(native.weights_fingerprint(net)) == want
    if kind == "wavenet":                         # positions that start over at the second launch would give another number
        assert sum(R.fingerprint_buffers([entries[k] for k in names[f:f + R.MAX_BUFFERS]]) for f in range(0, len(names), R.MAX_BUFFERS)) % 2 ** 64 != want
    n0 = native.pack_launch_count()
    again = _generate(net, kind, device)
    assert native.pack_launch_count() == n0 and all(torch.equal(a, b) for a, b in zip(first, again))
    for index in (0, late):
        name = names[index]
        entry = entries[name]
        moved = None
        for j, prompt in _candidates(name, entry, kind, first[1]):
            base = first if prompt is None else _generate(net, kind, device, prompt)
            assert native.pack_launch_count() == n0, "a generation with nothing changed packed weights"
            flat = entry.data.view(-1)
            old = flat[j].clone()
            ident = native.weights_identity(net)
            flat[j] = torch.nextafter(old, torch.full_like(old, float("inf")))
            assert native.weights_identity(net) == ident and float(flat[j]) != float(old)      # nothing on the host side has moved
            got = _generate(net, kind, device, prompt)
            n1 = native.pack_launch_count()
            assert n1 > n0, f"{kind}: {name}[{j}] moved by one ulp and nothing was packed"
            if not torch.equal(got[1], base[1]):
                moved = j
                fresh = make()
                fresh.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
                want = _generate(fresh.to(device), kind, device, prompt)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{kind}: {name}[{j}]: not what a fresh network computes"
            n1 = native.pack_launch_count()            # (the fresh network packed its own)
            flat[j] = old
            back = _generate(net, kind, device, prompt)
            n0 = native.pack_launch_count()
            assert n0 > n1 and all(torch.equal(a, b) for a, b in zip(base, back)), f"{kind}: {name}[{j}] written back"
            assert all(torch.equal(a, b) for a, b in zip(base, _generate(net, kind, device, prompt))) and native.pack_launch_count() == n0
            if moved is not None:
                break
        assert moved is not None, f"{kind}: one ulp on {name} (index {index}) moved no compared output: the comparison with a fresh network says nothing"
        print(f"fingerprint, {kind}: entry {index} of {len(names)} ({name}), element {moved}: repacked, outputs moved and equal a fresh network's")
