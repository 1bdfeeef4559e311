"""Bit parity of the nearest-frame and k-best searches (csrc/nn_search.h) between two builds of the library, on one MI355X.

    MMK_DIAG_LIB=/path/to/other/libmmk_hip.so timeout -k 10 120 python scripts/nn_search_parity.py --dump a.npz
    timeout -k 10 120 python scripts/nn_search_parity.py --dump b.npz
    python scripts/nn_search_parity.py --compare a.npz b.npz                    (host only)

One process per dump, each under its own time limit.  --dump runs native.nn_cosine, native.nn_cosine_self and native.nn_topk (cosine and
euclidean, self_exclude off and on, T = 1, 4, 9, 16) on inputs seeded on the CPU and saves every index array and the raw int32 bits of every
key array; --compare exits 0 only if the two files hold the same arrays, equal element for element (the keys as bits: -0.0 is not 0.0).
The shapes are the smallest at which the tile walk can go wrong: one row / frame / bin; one row past a query block (128), one frame past a
span (NN_SPAN) and one bin past a chunk (32); strided rows on a base that is 4-byte but not 16-byte aligned; the diagonal of the
self-excluding form across a tile, a block and a span edge; one bin, where every cosine clamps to +-1 and the lower index must win; exact
duplicates and all-zero rows.
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
    torch.cuda.synchronize(device)
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays from {native.LIB_PATH}")


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
