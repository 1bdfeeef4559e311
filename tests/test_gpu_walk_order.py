"""What csrc/frame_walk.h states once, held across the kernels that are built from it: the k-means assignment, the plain and the
self-excluding arg-max and the k-best search sum the bins of a frame pair in ONE order, so the same frames give the same key bits and the
same winner whichever kernel multiplies them.  Every comparison is exact: indices with torch.equal, keys as bits - except against the cosine
form of the k-best search, whose affine key adds a zero shift and turns -0 into +0 (csrc/nn_search.h), where the keys are compared as float
values.  Rows are drawn on the CPU (tests/kmeans_refs.py, seeded torch generators); each case is a handful of launches."""
import pytest
import torch

from mimikit_amd import native
from tests import kmeans_refs as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NS = (1, 129, 257)            # one row; one past a workgroup's 128 rows; one past two
DS = (1, 16, 17, 33)          # one bin; the last narrow load and the first wide one; one past a chunk of 32 bins
KS = (1, 33, 256)             # one centre; one past a 32-centre product; the product-by-product instance


def bits(t):
    return t.contiguous().view(torch.int32)


def assign_against_search(x_np, offset_np, centres_np, device):
    """kmeans_assign's labels and key bits against nn_topk(x', centres, 1, "euclidean"), x' = fl32(x - offset) formed by torch"""
    x = torch.from_numpy(x_np.copy()).to(device)
    centres = torch.from_numpy(centres_np.copy()).to(device)
    offset = None if offset_np is None else torch.from_numpy(offset_np.copy()).to(device)
    n = x.shape[0]
    labels = torch.full((n,), -1, dtype=torch.int32, device=device)
    key = torch.full((n,), float("nan"), dtype=torch.float32, device=device)
    native.kmeans_assign(x, offset, centres, labels, key=key)
    xp = x if offset is None else x - offset[None, :]
    index, want = native.nn_topk(xp, centres, 1, "euclidean")
    what = f"n, d, k = {n, x.shape[1], centres.shape[0]}, offset {'given' if offset is not None else 'None'}"
    assert torch.equal(labels.to(torch.int64), index[:, 0]), f"{what}: labels differ from the search's indices"
    assert torch.equal(bits(key), bits(want[:, 0])), f"{what}: key bits differ from the search's"
    return labels


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_kmeans_assign_is_the_search(device, n, d, k):
    for with_offset in (False, True):
        assign_against_search(*R.kernel_case(n, d, k, with_offset), device)


@pytest.mark.parametrize("with_offset", (False, True))
def test_identical_centres_lower_index_in_both(device, with_offset):
    x, offset, centres = R.special_case(with_offset)
    labels = assign_against_search(x, offset, centres, device).cpu()
    lo, hi = R.SAME_CENTRES
    assert int((labels == lo).sum()) > 0, "no row chose the doubled centre: the case tests nothing"
    assert int((labels == hi).sum()) == 0, "the higher of two identical centres took a row"


def frames(n, k, seed, device):
    return torch.randn(n, k, generator=torch.Generator().manual_seed(seed)).to(device)


@pytest.mark.parametrize("rows, extra, k", ((129, 1, 33), (130, 52, 1)))
def test_nn_cosine_is_the_search(device, rows, extra, k):
    x, y = frames(rows, k, 21, device), frames(native.NN_SPAN + extra, k, 22, device)
    index, cos = native.nn_cosine(x, y, native.inv_row_norm(y))
    want_index, want_cos = native.nn_topk(x, y, 1, "cosine")
    assert torch.equal(index, want_index[:, 0])
    assert torch.equal(cos, want_cos[:, 0])           # as values: the affine key's zero shift makes -0 a +0


@pytest.mark.parametrize("rows, k", ((129, 33), (131, 1)))
def test_nn_cosine_self_is_the_search(device, rows, k):
    x = frames(rows, k, 23, device)
    index, cos = native.nn_cosine_self(x)
    want_index, want_cos = native.nn_topk(x, x, 1, "cosine", self_exclude=True)
    assert torch.equal(index, want_index[:, 0])
    assert torch.equal(cos, want_cos[:, 0])           # as values, as above
