// Labelling the frames of a corpus (mimikit/extract/clusters.py:157-205 HCluster): the pieces of one level besides the nearest-other-frame
// arg-max, which is nn_search_kernel<1, true, NnCosineKey> of nn_search.h (mmk_nn_cosine_self_f32 in neighbors.hip).
//
//   components   the weakly connected components of the functional graph i -> f(i) = nearest[i], numbered by rising smallest member.  Every
//                component of such a graph holds exactly one cycle, so the smallest node ON the cycle names the component:
//                  cc_init_kernel     p[i] = f(i) (clamped into [0, n): an entry outside is the caller's error and must not become an
//                                     address), m[i] = i, cmin[i] = int max
//                  cc_double_kernel   (p, m) <- (p[p], min(m, m[p])) on ping-pong buffers, R = ceil(log2 n) + 1 rounds, one launch each.  After t
//                                     rounds p[i] = f^(2^t)(i) and m[i] = min f^j(i) over 0 <= j < 2^t.  2^R >= 2 n: p[i] lies on the cycle (a
//                                     tail has fewer than n nodes) and m[p[i]] is the minimum over at least n steps from a node of the
//                                     cycle, that is over the whole cycle - whatever its length, self-loops and one chain of n nodes included.
//                  cc_rep_kernel      rep[i] = m[p[i]];  atomicMin(cmin[rep[i]], i): the component's smallest member, which need not lie
//                                     on the cycle.  An integer minimum is the same in any order - the one atomic here, and no float goes
//                                     through it.
//                  cc_count_kernel    node i is a root if cmin[rep[i]] == i; roots per block of 256 nodes
//                  cc_scan_kernel     ONE workgroup: the exclusive prefix sum of the block counts (Hillis-Steele in LDS, chunk by chunk with
//                                     a carry) and the total = the number of components (int64 on the device).  The prefix count is this
//                                     kernel, not a torch.cumsum in the wrapper: the entry point returns finished labels.
//                  cc_rank_kernel     rank[root] = the block's offset + the roots before it in the block (ballot / popcount per wave)
//                  cc_label_kernel    labels[i] = rank[cmin[rep[i]]]
//                Indices are kept in 32 bits: five int32 arrays of n and one of the blocks as workspace.
//   segment_mean out[s] = the mean of the rows x[order[offsets[s] .. offsets[s + 1])]: one workgroup per segment, a lane per bin (consecutive
//                lanes on consecutive bins: every member row is read coalesced), members added in the order given in fp64, one division and
//                ONE rounding to fp32.
//   edge components   (mmk_edge_components_i64; QCluster's graph, mimikit/extract/clusters.py:83) the connected components of an undirected edge
//                list over n nodes - self-loops, repeated and reversed edges allowed, a node without an edge is a singleton - numbered the
//                same way.  parent[i] starts at i and only ever falls, and it only ever takes the number of a node of i's own component:
//                  ec_hook_kernel     a thread per edge (u, v): a = parent[u], b = parent[v]; if they differ, atomicMin(parent[max(a, b)],
//                                     min(a, b)) and the same on the endpoint whose parent was the larger, and the round's flag is raised
//                  ec_jump_kernel     parent[i] <- parent[parent[i]] (twice per round), raising the flag where that moves parent[i]
//                A round that leaves the flag down has written nothing, so it has read ONE state in which every edge joins two nodes of
//                the same parent and every parent is its own parent: parent is constant on a component, at most its smallest member
//                (parent[i] <= i) and a member of it - it IS the smallest member, whatever the order the atomics landed in (integer
//                minima; no float goes through an atomic).  The values are bounded below, so the rounds end.  Convergence is found by
//                the flag, not by a proven count: the entry point runs kEcGroup rounds, lowers the flag before the last of them, copies
//                it to the host and waits for the stream - one synchronisation per group of rounds, which is why this entry point (alone
//                in this file) cannot be captured into a graph.  The numbering is cc_count / cc_scan / cc_rank / cc_label above with
//                rep = parent and cmin = the identity.  Three int32 arrays of n, one of the blocks and the flag as workspace.
// No workgroup waits for another, no scratch, and two calls give the same bits.  NaN in the inputs is not handled.
#include "entry_util.h"

namespace mmk {

constexpr int kCcThreads = 256;

__global__ __launch_bounds__(kCcThreads) void cc_init_kernel(const int64_t* __restrict__ nearest, int32_t n, int32_t* __restrict__ p,
                                                            int32_t* __restrict__ m, int32_t* __restrict__ cmin) {
  const int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t f = nearest[i];
  p[i] = (int32_t)(f < 0 ? 0 : (f >= n ? n - 1 : f));
  m[i] = (int32_t)i;
  cmin[i] = 0x7fffffff;
}

__global__ __launch_bounds__(kCcThreads) void cc_double_kernel(const int32_t* __restrict__ p_in, const int32_t* __restrict__ m_in, int32_t n,
                                                              int32_t* __restrict__ p_out, int32_t* __restrict__ m_out) {
  const int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t q = p_in[i];
  p_out[i] = p_in[q];
  m_out[i] = min(m_in[i], m_in[q]);
}

__global__ __launch_bounds__(kCcThreads) void cc_rep_kernel(const int32_t* __restrict__ p, const int32_t* __restrict__ m, int32_t n,
                                                           int32_t* __restrict__ rep, int32_t* __restrict__ cmin) {
  const int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t r = m[p[i]];
  rep[i] = r;
  atomicMin(&cmin[r], (int32_t)i);
}

__global__ __launch_bounds__(kCcThreads) void cc_count_kernel(const int32_t* __restrict__ rep, const int32_t* __restrict__ cmin, int32_t n,
                                                             int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
  const int root = (i < n && cmin[rep[i < n ? i : 0]] == (int32_t)i) ? 1 : 0;
  const int total = __syncthreads_count(root);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// in place: counts[b] becomes the number of roots in the blocks before b
__global__ __launch_bounds__(kCcThreads) void cc_scan_kernel(int32_t* __restrict__ counts, int32_t n_blocks, int64_t* __restrict__ n_components) {
  __shared__ int32_t scan[2][kCcThreads];
  const int tid = threadIdx.x;
  int32_t carry = 0;
  for (int32_t b0 = 0; b0 < n_blocks; b0 += kCcThreads) {
    const int32_t b = b0 + tid;
    const int32_t v = b < n_blocks ? counts[b] : 0;
    int cur = 0;
    scan[0][tid] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < kCcThreads; off <<= 1) {
      scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= off ? scan[cur][tid - off] : 0);
      cur ^= 1;
      __syncthreads();
    }
    if (b < n_blocks) counts[b] = carry + scan[cur][tid] - v;
    const int32_t next = carry + scan[cur][kCcThreads - 1];
    __syncthreads();        // (the next chunk writes scan[0] again)
    carry = next;
  }
  if (tid == 0) *n_components = carry;
}

__global__ __launch_bounds__(kCcThreads) void cc_rank_kernel(const int32_t* __restrict__ rep, const int32_t* __restrict__ cmin,
                                                            const int32_t* __restrict__ offsets, int32_t n, int32_t* __restrict__ rank) {
  __shared__ int32_t wave_roots[kCcThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * kCcThreads + tid;
  const bool root = i < n && cmin[rep[i < n ? i : 0]] == (int32_t)i;
  const unsigned long long mask = __ballot(root);
  if (lane == 0) wave_roots[wave] = __popcll(mask);
  __syncthreads();
  if (!root) return;
  int32_t before = offsets[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) before += wave_roots[w];
  rank[i] = before;
}

__global__ __launch_bounds__(kCcThreads) void cc_label_kernel(const int32_t* __restrict__ rep, const int32_t* __restrict__ cmin,
                                                             const int32_t* __restrict__ rank, int32_t n, int64_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (i >= n) return;
  labels[i] = rank[cmin[rep[i]]];
}

__global__ __launch_bounds__(256) void segment_mean_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int32_t K,
                                                          const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                          float* __restrict__ out, int64_t out_row_stride) {
  const int64_t s = blockIdx.x;
  // (clamped: a wrong offset or member is the caller's error and gives a wrong mean, never an address outside x or order)
  const int64_t beg = min(max(offsets[s], (int64_t)0), n), end = min(max(offsets[s + 1], beg), n);
  const double count = (double)(end - beg);
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    double acc = 0.0;
    for (int64_t u = beg; u < end; ++u) {
      const int64_t r = min(max(order[u], (int64_t)0), n - 1);      // (one address for the whole wave)
      acc += (double)x[r * x_row_stride + k];
    }
    out[s * out_row_stride + k] = (float)(acc / count);
  }
}

static int cc_blocks(int64_t n) { return (int)((n + kCcThreads - 1) / kCcThreads); }

// ---- components of an undirected edge list ----------------------------------------------------------------------------------------------
constexpr int kEcGroup = 4;       // rounds between two looks at the flag

__global__ __launch_bounds__(kCcThreads) void ec_init_kernel(int32_t n, int32_t* __restrict__ parent, int32_t* __restrict__ ident) {
  const int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (i >= n) return;
  parent[i] = (int32_t)i;
  ident[i] = (int32_t)i;
}

// (an endpoint outside [0, n) is the caller's error: the edge is left out, never used as an address)
__global__ __launch_bounds__(kCcThreads) void ec_hook_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t n_edges,
                                                            int32_t n, int32_t* parent, int32_t* __restrict__ changed) {
  const int64_t e = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (e >= n_edges) return;
  const int64_t u = src[e], v = dst[e];
  if (u < 0 || v < 0 || u >= n || v >= n || u == v) return;
  const int32_t a = parent[u], b = parent[v];
  if (a == b) return;
  const int32_t lo = min(a, b), hi = max(a, b);
  atomicMin(&parent[hi], lo);
  atomicMin(&parent[a > b ? u : v], lo);
  *changed = 1;
}

__global__ __launch_bounds__(kCcThreads) void ec_jump_kernel(int32_t n, int32_t* parent, int32_t* __restrict__ changed) {
  const int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t p = parent[i];
  const int32_t g = parent[p];
  if (g != p) {                   // (g < p: parents only fall)
    atomicMin(&parent[i], g);
    *changed = 1;
  }
}

}  // namespace mmk

extern "C" size_t mmk_nn_components_workspace_bytes(int64_t n) {
  using namespace mmk;
  if (n < 1 || n > 0x7fffffffLL) return 0;
  return ((size_t)5 * (size_t)n + (size_t)cc_blocks(n)) * sizeof(int32_t);
}

extern "C" int mmk_nn_components_i64(const int64_t* nearest, int64_t n, int64_t* labels, int64_t* n_components, void* workspace,
                                     size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (n < 1) return fail(MMK_ERR_INVALID, "nn_components: n = %lld < 1 (nodes)", (long long)n);
  if (n > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "nn_components: n = %lld nodes: indices are kept in 32 bits", (long long)n);
  if (!nearest || !labels || !n_components || !workspace)
    return fail(MMK_ERR_INVALID, "nn_components: bad arguments (null pointer)");
  if (misaligned(nearest, 8) || misaligned(labels, 8) || misaligned(n_components, 8))
    return fail(MMK_ERR_INVALID, "nn_components: nearest, labels and n_components must be 8-byte aligned");
  if (misaligned(workspace, 4)) return fail(MMK_ERR_INVALID, "nn_components: the workspace must be 4-byte aligned");
  MMK_TRY(workspace_check("nn_components", workspace, 4, workspace_bytes, mmk_nn_components_workspace_bytes(n)));
  hipStream_t st = (hipStream_t)stream;
  const int32_t nn = (int32_t)n;
  const int blocks = cc_blocks(n);
  int32_t* w = static_cast<int32_t*>(workspace);
  int32_t* p[2] = {w, w + n};
  int32_t* m[2] = {w + 2 * n, w + 3 * n};
  int32_t* cmin = w + 4 * n;
  int32_t* counts = w + 5 * n;
  const dim3 grid((unsigned)blocks), wg(kCcThreads);
  MMK_TRY(launch(cc_init_kernel, grid, wg, 0, st, nearest, nn, p[0], m[0], cmin));
  int rounds = 1;                                   // ceil(log2 n) + 1
  while (((int64_t)1 << (rounds - 1)) < n) ++rounds;
  int cur = 0;
  for (int r = 0; r < rounds; ++r, cur ^= 1) MMK_TRY(launch(cc_double_kernel, grid, wg, 0, st, p[cur], m[cur], nn, p[cur ^ 1], m[cur ^ 1]));
  int32_t* rep = p[cur ^ 1];                        // the buffers of the round before the last are free again
  int32_t* rank = m[cur ^ 1];
  MMK_TRY(launch(cc_rep_kernel, grid, wg, 0, st, p[cur], m[cur], nn, rep, cmin));
  MMK_TRY(launch(cc_count_kernel, grid, wg, 0, st, rep, cmin, nn, counts));
  MMK_TRY(launch(cc_scan_kernel, dim3(1), wg, 0, st, counts, (int32_t)blocks, n_components));
  MMK_TRY(launch(cc_rank_kernel, grid, wg, 0, st, rep, cmin, counts, nn, rank));
  return launch(cc_label_kernel, grid, wg, 0, st, rep, cmin, rank, nn, labels);
}

extern "C" size_t mmk_edge_components_workspace_bytes(int64_t n) {
  using namespace mmk;
  if (n < 1 || n > 0x7fffffffLL) return 0;
  return ((size_t)3 * (size_t)n + (size_t)cc_blocks(n) + 1) * sizeof(int32_t);
}

extern "C" int mmk_edge_components_i64(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n, int64_t* labels,
                                       int64_t* n_components, void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (n < 1) return fail(MMK_ERR_INVALID, "edge_components: n = %lld < 1 (nodes)", (long long)n);
  if (n_edges < 0) return fail(MMK_ERR_INVALID, "edge_components: n_edges = %lld < 0", (long long)n_edges);
  if (n > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "edge_components: n = %lld nodes: indices are kept in 32 bits", (long long)n);
  if ((n_edges + kCcThreads - 1) / kCcThreads > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "edge_components: %lld edges are more than one launch takes", (long long)n_edges);
  if ((n_edges > 0 && (!src || !dst)) || !labels || !n_components || !workspace)
    return fail(MMK_ERR_INVALID, "edge_components: bad arguments (null pointer)");
  if (misaligned(src, 8) || misaligned(dst, 8) || misaligned(labels, 8) || misaligned(n_components, 8))
    return fail(MMK_ERR_INVALID, "edge_components: src, dst, labels and n_components must be 8-byte aligned");
  if (misaligned(workspace, 4)) return fail(MMK_ERR_INVALID, "edge_components: the workspace must be 4-byte aligned");
  MMK_TRY(workspace_check("edge_components", workspace, 4, workspace_bytes, mmk_edge_components_workspace_bytes(n)));
  hipStream_t st = (hipStream_t)stream;
  const int32_t nn = (int32_t)n;
  const int blocks = cc_blocks(n);
  int32_t* w = static_cast<int32_t*>(workspace);
  int32_t* parent = w;
  int32_t* ident = w + n;
  int32_t* rank = w + 2 * n;
  int32_t* counts = w + 3 * n;
  int32_t* changed = counts + blocks;
  const dim3 grid((unsigned)blocks), wg(kCcThreads);
  const dim3 egrid((unsigned)((n_edges + kCcThreads - 1) / kCcThreads));
  MMK_TRY(launch(ec_init_kernel, grid, wg, 0, st, nn, parent, ident));
  for (bool again = n_edges > 0; again;) {
    for (int r = 0; r < kEcGroup; ++r) {
      if (r == kEcGroup - 1) MMK_HIP(hipMemsetAsync(changed, 0, sizeof(int32_t), st));
      MMK_TRY(launch(ec_hook_kernel, egrid, wg, 0, st, src, dst, n_edges, nn, parent, changed));
      for (int jump = 0; jump < 2; ++jump) MMK_TRY(launch(ec_jump_kernel, grid, wg, 0, st, nn, parent, changed));
    }
    int32_t flag = 0;
    MMK_HIP(hipMemcpyAsync(&flag, changed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MMK_HIP(hipStreamSynchronize(st));
    again = flag != 0;
  }
  MMK_TRY(launch(cc_count_kernel, grid, wg, 0, st, parent, ident, nn, counts));
  MMK_TRY(launch(cc_scan_kernel, dim3(1), wg, 0, st, counts, (int32_t)blocks, n_components));
  MMK_TRY(launch(cc_rank_kernel, grid, wg, 0, st, parent, ident, counts, nn, rank));
  return launch(cc_label_kernel, grid, wg, 0, st, parent, ident, rank, nn, labels);
}

extern "C" int mmk_segment_mean_f32(const float* x, int64_t x_row_stride, int64_t n, int32_t k, const int64_t* order, const int64_t* offsets,
                                    int64_t n_segments, float* out, int64_t out_row_stride, mmk_stream_t stream) {
  using namespace mmk;
  if (n < 1) return fail(MMK_ERR_INVALID, "segment_mean: n = %lld < 1 (rows)", (long long)n);
  if (k < 1) return fail(MMK_ERR_INVALID, "segment_mean: k = %d < 1 (bins)", k);
  if (n_segments < 1 || n_segments > n)
    return fail(MMK_ERR_INVALID, "segment_mean: %lld segments of %lld rows (every segment has a member)", (long long)n_segments, (long long)n);
  if (n_segments > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "segment_mean: %lld segments are more than one launch takes", (long long)n_segments);
  if (!x || !order || !offsets || !out || x_row_stride < 0 || out_row_stride < 0)
    return fail(MMK_ERR_INVALID, "segment_mean: bad arguments (null pointer or negative stride %lld / %lld)", (long long)x_row_stride,
                (long long)out_row_stride);
  if (misaligned(x, 4) || misaligned(out, 4)) return fail(MMK_ERR_INVALID, "segment_mean: x and out must be 4-byte aligned");
  if (misaligned(order, 8) || misaligned(offsets, 8)) return fail(MMK_ERR_INVALID, "segment_mean: order and offsets must be 8-byte aligned");
  const int threads = k <= 64 ? 64 : (k <= 128 ? 128 : 256);
  return launch(segment_mean_kernel, dim3((unsigned)n_segments), dim3(threads), 0, (hipStream_t)stream, x, x_row_stride, n, k, order, offsets,
                out, out_row_stride);
}
