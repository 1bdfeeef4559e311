"""Bit parity of the kernels built from csrc/frame_walk.h - the nearest-frame and k-best searches (csrc/nn_search.h, neighbors.hip), the
k-means assignment (kmeans.hip) and the novelty scores (novelty.hip) - between two builds of the library, on one MI355X.

    MMK_DIAG_LIB=/path/to/other/libmmk_hip.so timeout -k 10 120 python scripts/walk_parity.py --dump a.npz
    timeout -k 10 120 python scripts/walk_parity.py --dump b.npz
    python scripts/walk_parity.py --compare a.npz b.npz                    (host only)

One process per dump, each under its own time limit.  --dump runs the entry points below on inputs seeded on the CPU and saves every integer
array and the raw int32 bits of every float array; --compare exits 0 only if the two files hold the same arrays, equal element for element
(floats as bits: -0.0 is not 0.0).
  searches  native.nn_cosine, native.nn_cosine_self and native.nn_topk (cosine and euclidean, self_exclude off and on, T = 1, 4, 9, 16).  The
            shapes are the smallest at which the tile walk can go wrong: one row / frame / bin; one row past a query block (128), one frame
            past a span (NN_SPAN) and one bin past a chunk (32); strided rows on a base that is 4-byte but not 16-byte aligned; the diagonal
            of the self-excluding form across a tile, a block and a span edge; one bin, where every cosine clamps to +-1 and the lower index
            must win; exact duplicates and all-zero rows.
  k-means   native.kmeans_assign: labels, key bits and the `changed` count (from labels of 0) for N in 1, 129, 257 by D in 1, 16, 17, 33, 65
            (both sides of the narrow form, one bin past a chunk and past two) by K in 1, 32, 33, 64, 65, 128, 129, 256 (both ends of every
            centre tile), with and without offset; once on strided rows on a base that is 4-byte but not 16-byte aligned; and the planted
            duplicate rows, identical centres and zero row of tests/kmeans_refs.special_case.
  novelty   native.novelty: the raw bits for T in 2, 64, 65, 200 frames (a clip of one frame has no board: it is refused, and the refusal is
            recorded) by 1, 32, 33, 513 bins by half-width sets whose largest is 1, 15, 16, 31 and NOVELTY_MAX_HALF = 32 (both ends of the
            three NB instances), inv_norm given and None; and two clips at a batch stride longer than a clip.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TS = (1, 4, 9, 16)
METRICS = ("cosine", "euclidean")


def rows_of(n, k, seed, strided=False, plant=False):
    """(n, k) seeded normal frames on the CPU.  strided: a view at row stride k + 3 whose first element lies 4 bytes into its buffer.
    plant: exact duplicates of three frames far apart (another tile, another span) and three all-zero rows"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, k, generator=g)
    if plant:
        for src, dst in ((0, 1), (5, n // 2), (7, n - 1)):
            x[dst] = x[src]
        x[[3, n // 3, n - 2]] = 0.0
    if not strided:
        return x
    buf = torch.zeros(n * (k + 3) + 1)
    view = buf[1:].view(n, k + 3)[:, :k]
    view.copy_(x)
    return view


def on_device(x, device):
    """the same bytes at the same row stride and the same offset from a 16-byte boundary"""
    if x.is_contiguous():
        return x.to(device)
    buf = torch.zeros(x.storage_offset() + x.shape[0] * x.stride(0), device=device)
    view = buf.as_strided(x.shape, x.stride(), x.storage_offset())
    view.copy_(x)
    return view


def dump(path):
    from mimikit_amd import native
    device = torch.device("cuda")
    span = native.NN_SPAN
    out = {}

    def keep(name, index, key):
        out[name + ".index"] = index.cpu().numpy()
        out[name + ".key_bits"] = key.cpu().numpy().view(np.int32)

    # (name, query rows, corpus frames, bins, strided, planted)
    plain = (("one", 1, 1, 1, False, False), ("edges", 129, span + 1, 33, False, False), ("strided", 300, 2 * span + 4, 513, True, False),
             ("one_bin", 130, span + 52, 1, False, False), ("planted", 140, span + 100, 33, False, True))
    for name, rows, m, k, strided, plant in plain:
        y = on_device(rows_of(m, k, 11, strided, plant), device)
        xc = rows_of(rows, k, 12, strided, plant)
        if plant:
            xc[:8] = y[:8].cpu()                     # queries that ARE corpus frames (a duplicated one and a zero row among them)
        x = on_device(xc, device)
        keep(f"{name}.nn_cosine", *native.nn_cosine(x, y, native.inv_row_norm(y)))
        for metric in METRICS:
            for t in TS:
                keep(f"{name}.nn_topk_{metric}_{t}", *native.nn_topk(x, y, t, metric))
    for name, rows, k, plant in (("self_2", 2, 33, False), ("self_129", 129, 33, False), ("self_span", span + 129, 33, True),
                                 ("self_one_bin", 131, 1, False)):
        x = on_device(rows_of(rows, k, 13, False, plant), device)
        keep(f"{name}.nn_cosine_self", *native.nn_cosine_self(x))
        for metric in METRICS:
            for t in TS:
                keep(f"{name}.nn_topk_{metric}_{t}", *native.nn_topk(x, x, t, metric, self_exclude=True))
    dump_kmeans(out, device)
    dump_novelty(out, device)
    torch.cuda.synchronize(device)
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays from {native.LIB_PATH}")


def dump_kmeans(out, device):
    from mimikit_amd import native
    from tests import kmeans_refs as R

    def run(name, x, offset, centres):
        n = x.shape[0]
        labels = torch.zeros((n,), dtype=torch.int32, device=device)
        key = torch.full((n,), float("nan"), dtype=torch.float32, device=device)
        changed = torch.zeros((), dtype=torch.int64, device=device)
        native.kmeans_assign(x, offset, centres, labels, changed=changed, key=key)
        out[name + ".labels"] = labels.cpu().numpy()
        out[name + ".key_bits"] = key.cpu().numpy().view(np.int32)
        out[name + ".changed"] = changed.cpu().numpy().reshape(1)

    def dev(a):
        return None if a is None else torch.from_numpy(a.copy()).to(device)

    for n in (1, 129, 257):
        for d in (1, 16, 17, 33, 65):
            for k in (1, 32, 33, 64, 65, 128, 129, 256):
                for with_offset in (False, True):
                    x, offset, centres = R.kernel_case(n, d, k, with_offset)
                    run(f"kmeans.{n}x{d}x{k}.{'offset' if with_offset else 'plain'}", dev(x), dev(offset), dev(centres))
    g = torch.Generator().manual_seed(14)
    run("kmeans.strided", on_device(rows_of(257, 33, 15, strided=True), device), torch.randn(33, generator=g).to(device),
        on_device(rows_of(65, 33, 16, strided=True), device))
    for with_offset in (False, True):
        x, offset, centres = R.special_case(with_offset)
        run(f"kmeans.special.{'offset' if with_offset else 'plain'}", dev(x), dev(offset), dev(centres))


def dump_novelty(out, device):
    from mimikit_amd import native
    top = native.NOVELTY_MAX_HALF
    half_sets = sorted({(1,), (3, 15), (16,), (2, 16, 31), (32,), (1, 15, 16, 31, top)})

    def run(name, x, halves, inv_norm):
        try:
            out[name] = native.novelty(x, halves, inv_norm).cpu().numpy().view(np.int32)
        except ValueError:
            out[name] = np.array([-1], dtype=np.int32)      # refused (one frame)

    for t in (1, 2, 64, 65, 200):
        for bins in (1, 32, 33, 513):
            x = rows_of(t, bins, 17).to(device)
            rx = native.inv_row_norm(x)
            for halves in half_sets:
                tag = f"novelty.{t}x{bins}.h{'_'.join(map(str, halves))}"
                run(tag + ".inv_norm", x, halves, rx)
                run(tag + ".none", x, halves, None)
    # two clips at a batch stride longer than a clip
    buf = torch.zeros((2, 200 + 7, 33))
    buf[:, :200] = rows_of(400, 33, 18).view(2, 200, 33)
    clips = buf.to(device)[:, :200]
    for halves in ((15,), (4, 31), (top,)):
        tag = f"novelty.2x200x33.h{'_'.join(map(str, halves))}"
        run(tag + ".inv_norm", clips, halves, native.inv_row_norm(clips))
        run(tag + ".none", clips, halves, None)


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for name in sorted(set(a.files) & set(b.files)):
        if a[name].shape != b[name].shape or a[name].dtype != b[name].dtype or not np.array_equal(a[name], b[name]):
            bad.append(name)
    for name in bad:
        print(f"DIFFERENT: {name}")
    print(f"{len(a.files)} arrays against {len(b.files)}: {'all equal' if not bad else f'{len(bad)} differ'}")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="FILE.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    args = ap.parse_args()
    if (args.dump is None) == (args.compare is None):
        ap.error("one of --dump FILE.npz and --compare A.npz B.npz")
    sys.exit(compare(*args.compare) if args.compare else dump(args.dump))
