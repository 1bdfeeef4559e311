"""Every capturable entry point inside a replayed graph (tests/graph_cases.py has the tables, the cases and the method).  The float64 suites
establish that the eager default-stream bits are right and tests/test_gpu_streams.py that every launch stays on its stream; a replayed graph
is a stricter caller than either.  In global capture mode the runtime refuses what eager execution tolerates (a launch or memset on the null
stream, a blocking copy, an allocation, a query of the capturing stream); a replay runs the recorded launches with the arguments of capture
time, so a value the host read from the device and folded into a launch is frozen; and a replay finds the workspace as the last replay left
it, where every other test zero-fills it first.  Every comparison is bitwise against the eager call of the same buffers.

  a. every CAPTURED stateless entry point (C ABI, outputs inside NaN / sentinel surrounds): recorded once on a side stream with the stale
     input in place, nothing written by the capture, then replayed on the real input (zeroed workspace), on the stale input (the workspace
     as left) and on the real input again (the workspace as left);
  b. three chains, each recorded as ONE graph with its intermediates left on the device, replayed on two draws with dirty workspaces:
     inverse norms, cosine cost, subsequence DTW; novelty, its finish, the peak picker; one Lloyd step (assignment, label sums);
  c. the Python layer as users capture it: `y = f(x_static)` under torch.cuda.graph for every CAPTURED entry of graph_cases.FUNCTIONALS
     (each public Functional, a Compose of Emphasis, MagSpec and MelSpec, the fitted PCA's transform, discontinuity_scores, the
     neighbour search and cum_entropy), then another draw copied into x_static and a replay.

Every graph is a chain on one stream (no fork, no join), and no test captures a call that is known to wait: each makes an eager call
first, which is also the first spectral call of the process where there is one.

NOT_CAPTURED (tests/graph_cases.py has the reasons): the entry points that wait - mmk_edge_components_i64, mmk_pca_eig_f64,
mmk_nmf_start_f64, mmk_nmf_solve_f64, mmk_fa_fit_f64, the plans' commit / reset / sync_status / inject_sync_error - every other call of a
plan (host-side state, and from 16 steps on a capture of its own), and in the Python layer what fits (PCA, NMF, FactorAnalysis), reads a
flag (nearest_neighbor: `bool((t < 0).any())`) or opens a file.

Found by reading, before the first run: the two NMF half-sweeps (include/mmk_nmf.h: "return without waiting") had neither a stream case nor
any other test off the default stream; they have a Case here (graph_cases.HALF_SWEEP_CASES).  No wrapper uploads a host-built table per
call: the mu-law edges and table (functionals._DEVICE_TABLES), the resample bank (_RESAMPLE_TABLES), the mel bank and the DCT
(features/mel.py: lru_cache per parameters and device) are cached, and F0Filter / AutoConvolve pass their counts by value.  GLA's
__call__ draws its initial phases with torch.rand at every call, which an eager call and a replay do not share: it is captured with the
phases given (`torch_func(x, init=...)`), the launches being the same.

RECORDS of the first runs on an MI355X (records, not thresholds):
  Captured: 67 cases of the 56 CAPTURED entry points (stream_cases.CASES without its two waiting ones, the families' ASYNC cases, the two
  half-sweeps, mmk_gla_f32[256]), the 3 chains, 30 entries of FUNCTIONALS; every capture returned 0 and wrote nothing.
  First run: 42 cases passed in table order, then mmk_gla_f32 (n_fft 1024, initial estimates given) gave other bits in replay A, 4096 of
  4096 outputs.  Nothing in csrc/istft.hip keeps state between calls; the call's only step that is not a kernel was its
  hipMemsetAsync of the previous spectrum.  A probe of the runtime alone - torch fill kernel (ones), hipMemsetAsync(0), copy, on one
  capturing stream, the graph launched three times - showed the memset node right on the first launch of a graph and wrong on every
  later one: of n floats 0 / 2, 750 / 1000, 13851 / 18468 and 786432 / 1048576 read back as zero (three quarters: a 16-byte pattern with
  one word of something else), and the same probe on mmk_gla_f32 showed the previous spectrum holding values up to 3e18 after a second
  launch.  It is the runtime's memset node, not the order of the nodes: the kernels before and behind it ran in order every time.
  Fixed in the entry points, since a caller cannot: every hipMemsetAsync of a stateless entry point is a kernel now - mmk_gla_f32 (both
  paths: fill_complex_kernel), mmk_pack_weight_f32 (launch_fill over the padding; it failed replay B with 480 of 1536 words once
  mmk_gla_f32 passed) and mmk_fingerprint_buffers_u32 (launch_set_i64; it passed only because its kernel adds to a word that the
  wrong pattern happened to leave zero).  The memsets that remain are in entry points that wait (pca_eig, nmf_solve, edge_components)
  and in the plans' commit / reset, none of which is captured.  mmk_gla_f32[256] was added for the general path's device-to-device copy
  (a memcpy node): it replays its bits.
  After the fix: 102 passed in 2.2 s; no replay differed - neither on the dirty workspaces (replays B and A again, the chains) nor in
  the Python layer, where no wrapper uploaded a table or read a value during a capture.
"""
import pytest
import torch

from tests import graph_cases as G
from tests import stream_cases as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_fault():
    """a fault on the device (an illegal access, an abort of the queue) surfaces at the next synchronisation: end the session there
    instead of starting the remaining tests on a device in that state"""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as err:
            pytest.exit(f"the device reported a fault ({err}): nothing more is started on it", returncode=3)


_side = []


def side_stream(device):
    """one side stream for every capture of this file (a capture needs a stream other than the null stream; which hardware queue it
    shares does not matter here: nothing runs beside it)"""
    if not _side:
        _side.append(torch.cuda.Stream(device))
    return _side[0]


CASES = G.captured_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_captured_entry_point_replays_its_eager_bits(device, case):
    bound = S.Bound(case, device)
    record = G.captured(bound, side_stream(device))
    print(f"[graphs] {case.id}: captured, {record['replays']} replays (zeroed, dirty, dirty workspace) equal the eager bits")


@pytest.mark.parametrize("chain", G.CHAINS, ids=[c.id for c in G.CHAINS])
def test_chain_captured_as_one_graph(device, chain):
    G.captured_chain(G.BoundChain(chain, device), side_stream(device))
    print(f"[graphs] chain {chain.id}: {' -> '.join(chain.entries)} as one graph, replays on draws 1, 0, 1 with dirty workspaces equal the eager chain")


@pytest.mark.parametrize("name", G.FUNCTIONALS_CAPTURED)
def test_functional_captured_as_users_capture_it(device, name):
    n_out = G.captured_functional(G.FUNCTIONALS[name], device)
    print(f"[graphs] {name}: captured under torch.cuda.graph, {n_out} output tensor(s) equal the eager call after x_static.copy_(second draw)")


def _on(stream_ptr):
    return torch.cuda.stream(torch.cuda.ExternalStream(stream_ptr) if stream_ptr else torch.cuda.default_stream())


def test_the_method_sees_a_frozen_host_value(device):
    """the method can fail (1): a caller that folds something the host knows about the input into a launch argument - here the filter's
    gain, chosen by which draw is in place - replays with the value of capture time, and replay A reports it"""
    class Folds(S.Bound):
        which = "real"

        def fill(self, which, keep_work=False):
            self.which = which
            super().fill(which, keep_work=keep_work)

        def call(self, stream_ptr):
            a = {**self.inp, **self.out, **self.work}
            batch, n = a["x"].shape
            b0 = 1.0 if self.which == "real" else 0.5
            rc = self.L.mmk_lfilter1_f32(S.P(a["x"]), n, batch, n, b0, -1.0, -0.99, S.P(a["y"]), n, S.P(a["ws"]), stream_ptr)
            assert rc == 0, (rc, self.L.mmk_last_error())
    with pytest.raises(AssertionError, match="replay A"):
        G.captured(Folds(S.BY_ID["mmk_lfilter1_f32"], device), side_stream(device))


def test_the_method_sees_a_word_that_is_expected_zero(device):
    """the method can fail (2): a call whose result is right only while a word of its workspace is zero, and which leaves that word
    non-zero, passes every test that clears the workspace first; replay B, on the workspace as replay A left it, reports it"""
    class Accumulates(S.Bound):
        def __init__(self, case, device):
            super().__init__(case, device)
            self.work["flag"] = torch.zeros(16, dtype=torch.uint8, device=device)

        def call(self, stream_ptr):
            super().call(stream_ptr)
            flag = self.work["flag"].view(torch.float32)[:1]
            with _on(stream_ptr):
                self.out["out"].add_(flag)
                flag.add_(1.0)
    with pytest.raises(AssertionError, match="replay B"):
        G.captured(Accumulates(S.BY_ID["mmk_half_neg_sqnorm_f32"], device), side_stream(device))
