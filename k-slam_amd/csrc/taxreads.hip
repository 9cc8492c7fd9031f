// taxreads.hip -- the reads of chosen taxa, selected on the device (include/kslam_taxreads.h).
//
// When a lane has run the per-read stage, the batch's taxonomy ids -- one per read pair -- lie in device memory next to the
// read pairs they belong to, the uploaded texts and their line index; so does the dense taxonomy tree (SamAnnot: up, depth).
//   once per kslam_set_taxon_reads (taxreads_mask_device): the set S as one byte per node plus a sorted list of unknown ids
//     1. k_tr_seeds     one thread per chosen id: id -> node by binary search in the tree's sorted ids.  A known id marks
//                       seed[node] and mask[node]; with PARENTS the thread walks `up` and marks every node it passes (plain
//                       byte stores of the same value race harmlessly).  An unknown id goes to an item list through an atomic
//                       cursor.  Chosen id 1 with CHILDREN raises all_nonzero.  With PARENTS one more thread handles id 1,
//                       which is in S by rule: it marks the mask only (no seed: the rule gives id 1 no children).
//     2. k_tr_children  (CHILDREN) one thread per node walks `up` for at most depth[node] steps, capped at the node count, and
//                       marks itself at the first seeded ancestor.  It reads seed[] (written by the launch before) and
//                       writes only its own mask byte.
//     3. the unknown items are radix-sorted (radix_sort.hip), run heads flagged and numbered by a scan, and the heads written
//        out: the list the flag pass searches.
//   per batch (taxreads_flag_device):
//     4. k_tr_flags     one thread per read pair: id 0 -> not matched; all_nonzero -> matched; else binary search -> node ->
//                       mask byte; an id without a node -> binary search in the unknown list.  A matched pair marks
//                       flag[r1_read] and, when paired, flag[r2_read], with the bounds check of readsplit.hip's k_rs_flags;
//                       the matched pairs are counted with a ballot and one atomic per wavefront, into one of 32 counters
//                       on cache lines of their own (k_tr_sum adds them up).
//   The lengths, scans and streaming copy are readsplit.hip's (read_split_flagged).
// Bytes, not bits, for seed and mask: marking is then a plain store (bits would need an atomic OR per mark, on the PARENTS walk
// per step), and the flag pass reads ONE byte per read pair behind a binary search that touches ~21 cache lines of the 8-byte-
// per-node id table -- for an NCBI-sized tree (2.5 M nodes) 2.5 MB of mask next to 20 MB of table, all of it L2 / Infinity
// Cache resident either way; packing the mask would save nothing the search does not spend twenty times over.
// Bounds: a node comes out of the table (values < n_nodes, checked again); every walk takes depth[node] steps at most, capped
// at n_nodes, and stops at the first parent that is not a node, so no index leaves [0, n_nodes) whatever the tree holds.
#include "common.h"
#include "../../include/kslam_taxreads.h"

namespace kslam {

namespace {

constexpr int TR_BLOCK = 256;
constexpr uint32_t TR_NONE = 0xFFFFFFFFu;
constexpr unsigned TR_SLOTS = 32, TR_SLOT_STRIDE = 16;   // the matched-pair counters: 32 of them, 128 bytes apart

inline unsigned tr_blocks(uint64_t n) { return (unsigned)((n + TR_BLOCK - 1) / TR_BLOCK); }

// the node of id, TR_NONE when the tree does not know it
__device__ inline uint32_t tr_node_of(uint32_t id, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ nodes, uint64_t n_nodes) {
  uint64_t lo = 0, hi = n_nodes;   // the first key >= id
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= n_nodes || keys[lo] != id) return TR_NONE;
  const uint32_t node = nodes[lo];
  return node < n_nodes ? node : TR_NONE;
}

// n chosen ids, and with add_root one more thread for id 1 (mask only).  items: room for n + 1.
__global__ __launch_bounds__(TR_BLOCK) void k_tr_seeds(const uint32_t *__restrict__ ids, uint64_t n, int add_root, uint32_t mode,
                                                       const uint32_t *__restrict__ keys, const uint32_t *__restrict__ nodes, uint64_t n_nodes,
                                                       const uint32_t *__restrict__ up, const uint32_t *__restrict__ depth,
                                                       uint8_t *__restrict__ seed, uint8_t *__restrict__ mask,
                                                       unsigned long long *__restrict__ items, unsigned long long *__restrict__ cursor,
                                                       int *__restrict__ all_nonzero) {
  const uint64_t i = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (i >= n + (add_root ? 1u : 0u)) return;
  const bool by_rule = i == n;
  const uint32_t id = by_rule ? 1u : ids[i];
  if (id == 0) return;   // (refused on the host; never a seed)
  if (!by_rule && id == 1u && (mode & KSLAM_TAXREADS_CHILDREN)) *all_nonzero = 1;
  const uint32_t node = n_nodes ? tr_node_of(id, keys, nodes, n_nodes) : TR_NONE;
  if (node == TR_NONE) {
    const unsigned long long slot = atomicAdd(cursor, 1ull);
    if (slot < n + 1) items[slot] = (unsigned long long)id << 32;
    return;
  }
  mask[node] = 1;
  if (by_rule) return;
  seed[node] = 1;
  if (mode & KSLAM_TAXREADS_PARENTS) {
    uint64_t steps = depth[node];   // the nodes on the path up, this one included
    if (steps > n_nodes) steps = n_nodes;
    uint32_t at = node;
    for (; steps && at < n_nodes; steps--) {
      mask[at] = 1;
      at = up[at];
    }
  }
}

__global__ __launch_bounds__(TR_BLOCK) void k_tr_children(const uint32_t *__restrict__ up, const uint32_t *__restrict__ depth,
                                                          const uint8_t *__restrict__ seed, uint8_t *__restrict__ mask, uint64_t n_nodes) {
  const uint64_t v = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (v >= n_nodes) return;
  uint64_t steps = depth[v];
  if (steps > n_nodes) steps = n_nodes;
  uint32_t at = (uint32_t)v;
  for (; steps && at < n_nodes; steps--) {
    if (seed[at]) {
      mask[v] = 1;
      return;
    }
    at = up[at];
  }
}

__global__ __launch_bounds__(TR_BLOCK) void k_tr_heads(const uint64_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (i < n) head[i] = i == 0 || (key[i] >> 32) != (key[i - 1] >> 32);
}

__global__ __launch_bounds__(TR_BLOCK) void k_tr_unique(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ head,
                                                        const uint32_t *__restrict__ before, uint32_t *__restrict__ out, uint64_t n_out) {
  const uint64_t i = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (i >= n || !head[i]) return;
  const uint64_t r = before[i];
  if (r < n_out) out[r] = (uint32_t)(key[i] >> 32);
}

// ABLATE (measurement only, `make ABLATE=1`): 1 = without the matched-pair count, 2 = without the marks on the records
template <int ABLATE>
__global__ __launch_bounds__(TR_BLOCK) void k_tr_flags(const kslam_read_pair *__restrict__ groups, const uint32_t *__restrict__ ids, uint64_t n_groups,
                                                       int paired, uint64_t n_total, TaxReadsSel S, uint8_t *__restrict__ flag,
                                                       unsigned long long *__restrict__ n_matched) {
  const uint64_t g = (uint64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  const uint32_t id = g < n_groups ? ids[g] : 0u;   // (no early return: every lane takes part in the ballot)
  bool matched = false;
  if (id) {
    if (S.all_nonzero) matched = true;
    else {
      const uint32_t node = S.n_nodes ? tr_node_of(id, S.keys, S.nodes, S.n_nodes) : TR_NONE;
      if (node != TR_NONE) matched = S.mask[node] != 0;
      else {
        uint64_t lo = 0, hi = S.n_unknown;
        while (lo < hi) {
          const uint64_t mid = lo + (hi - lo) / 2;
          if (S.unknown[mid] < id) lo = mid + 1;
          else hi = mid;
        }
        matched = lo < S.n_unknown && S.unknown[lo] == id;
      }
    }
  }
  if (matched && ABLATE != 2) {
    const uint32_t r1 = groups[g].r1_read, r2 = groups[g].r2_read;
    if (r1 < n_total) flag[r1] = 1;
    if (paired && r2 < n_total) flag[r2] = 1;   // (single end: r2_read is 0 and means nothing)
  }
  // one atomic per wavefront, spread over TR_SLOTS counters on cache lines of their own: 15 625 adds to ONE address take
  // 0.14 ms for a batch of 1 M pairs (some 10 ns each, one after the other), more than the searches do
  const uint64_t m = __ballot(matched);
  if (ABLATE != 1 && (threadIdx.x & 63) == 0 && m)
    atomicAdd(n_matched + TR_SLOT_STRIDE * ((blockIdx.x * (TR_BLOCK / 64) + (threadIdx.x >> 6)) % TR_SLOTS), (unsigned long long)__popcll(m));
}

// the slots' sum into the word behind slot 0's (one wavefront)
__global__ __launch_bounds__(64) void k_tr_sum(unsigned long long *__restrict__ count) {
  unsigned long long v = threadIdx.x < TR_SLOTS ? count[TR_SLOT_STRIDE * threadIdx.x] : 0ull;
  for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
  if (threadIdx.x == 0) count[1] = v;
}

}  // namespace

void taxreads_mask_device(const uint32_t *h_ids, uint64_t n, uint32_t mode, const uint32_t *d_keys, const uint32_t *d_nodes, uint64_t n_nodes,
                          const uint32_t *d_up, const uint32_t *d_depth, TaxReadsMaskWork &W, uint8_t *d_mask, DevBuf &unknown,
                          uint64_t *n_unknown_out, int *all_nonzero_out, hipEvent_t ev[2], hipStream_t s) {
  *n_unknown_out = 0;
  *all_nonzero_out = 0;
  if (n >= (1ull << 32) - 1 || n_nodes >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^32 or more chosen ids or taxonomy nodes"};
  const int add_root = (mode & KSLAM_TAXREADS_PARENTS) ? 1 : 0;
  const uint64_t n_threads = n + add_root, cap = n + 1;
  W.ids.ensure((n + 1) * sizeof(uint32_t));
  W.seed.ensure(n_nodes + 16);
  W.items_a.ensure(cap * sizeof(uint64_t));
  W.items_b.ensure(cap * sizeof(uint64_t));
  W.head.ensure(cap * sizeof(uint32_t));
  W.run.ensure(cap * sizeof(uint32_t));
  W.cursor.ensure(2 * sizeof(uint64_t));   // [0] the items' cursor, [1] all_nonzero
  W.scan_tmp.ensure(scan_tmp_bytes(cap + 1));
  W.totals.ensure(sizeof(uint64_t));
  unsigned long long *cursor = W.cursor.as<unsigned long long>();
  int *all_nonzero = reinterpret_cast<int *>(cursor + 1);
  HIPCHK(hipMemcpyAsync(W.ids.p, h_ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(cursor, 0, 2 * sizeof(uint64_t), s));
  HIPCHK(hipMemsetAsync(W.totals.p, 0, sizeof(uint64_t), s));
  HIPCHK(hipMemsetAsync(W.seed.p, 0, n_nodes + 16, s));
  HIPCHK(hipMemsetAsync(d_mask, 0, n_nodes, s));
  HIPCHK(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(k_tr_seeds, dim3(tr_blocks(n_threads)), dim3(TR_BLOCK), 0, s, W.ids.as<uint32_t>(), n, add_root, mode, d_keys, d_nodes, n_nodes,
                     d_up, d_depth, W.seed.as<uint8_t>(), d_mask, W.items_a.as<unsigned long long>(), cursor, all_nonzero);
  if ((mode & KSLAM_TAXREADS_CHILDREN) && n_nodes)
    hipLaunchKernelGGL(k_tr_children, dim3(tr_blocks(n_nodes)), dim3(TR_BLOCK), 0, s, d_up, d_depth, W.seed.as<uint8_t>(), d_mask, n_nodes);
  HIPCHK(hipGetLastError());
  uint64_t h[2] = {0, 0};
  read_back(h, cursor, sizeof h, s);   // (waits for the stream; h_ids is free again)
  uint64_t n_items = h[0] < cap ? h[0] : cap;
  *all_nonzero_out = (int)(h[1] & 1u);
  uint64_t n_unknown = 0;
  if (n_items) {
    void *sorted = W.items_a.p;
    if (n_items > 1) {
      SortPass passes[4];   // the id is the item's upper word
      for (int p = 0; p < 4; p++) passes[p] = SortPass{1u, (uint32_t)(8 * p), 0u};
      sorted = radix_sort(W.items_a.p, W.items_b.p, n_items, 2, passes, 4, W.sortws, s, nullptr, nullptr, nullptr);
    }
    const uint64_t *key = static_cast<const uint64_t *>(sorted);
    hipLaunchKernelGGL(k_tr_heads, dim3(tr_blocks(n_items)), dim3(TR_BLOCK), 0, s, key, n_items, W.head.as<uint32_t>());
    HIPCHK(hipGetLastError());
    exclusive_scan_u32(W.head.as<uint32_t>(), W.run.as<uint32_t>(), n_items, W.totals.as<uint64_t>(), W.scan_tmp.p, s);
    read_back(&n_unknown, W.totals.p, sizeof n_unknown, s);
    if (n_unknown > n_items) throw StatusError{KSLAM_ERR_INTERNAL, "more distinct unknown ids than items"};
    unknown.ensure((n_unknown + 1) * sizeof(uint32_t));
    hipLaunchKernelGGL(k_tr_unique, dim3(tr_blocks(n_items)), dim3(TR_BLOCK), 0, s, key, n_items, W.head.as<uint32_t>(), W.run.as<uint32_t>(),
                       unknown.as<uint32_t>(), n_unknown);
  } else {
    unknown.ensure(sizeof(uint32_t));
  }
  HIPCHK(hipEventRecord(ev[1], s));
  HIPCHK(hipGetLastError());
  HIPCHK(stream_wait(s));
  *n_unknown_out = n_unknown;
}

void taxreads_flag_device(const kslam_read_pair *d_groups, const uint32_t *d_ids, uint64_t n_groups, int paired, uint64_t n_total,
                          const TaxReadsSel &S, uint8_t *d_flag, TaxReadsFlagWork &W, hipStream_t s) {
  W.ms = 0;
  W.n_matched = 0;
  if (!W.ev[0])
    for (auto &e : W.ev) HIPCHK(hipEventCreate(&e));
  W.count.ensure(TR_SLOTS * TR_SLOT_STRIDE * sizeof(uint64_t));
  HIPCHK(hipMemsetAsync(W.count.p, 0, TR_SLOTS * TR_SLOT_STRIDE * sizeof(uint64_t), s));
  HIPCHK(hipEventRecord(W.ev[0], s));
  int ablate = 0;
#ifdef KSLAM_ABLATE
  if (const char *e = getenv("KSLAM_TAXREADS_ABLATE")) ablate = atoi(e);   // measurement only; the caller's count check then fails
#endif
  const dim3 grid(tr_blocks(n_groups)), block(TR_BLOCK);
  unsigned long long *count = W.count.as<unsigned long long>();
  if (n_groups && ablate == 1) hipLaunchKernelGGL(k_tr_flags<1>, grid, block, 0, s, d_groups, d_ids, n_groups, paired, n_total, S, d_flag, count);
  else if (n_groups && ablate == 2) hipLaunchKernelGGL(k_tr_flags<2>, grid, block, 0, s, d_groups, d_ids, n_groups, paired, n_total, S, d_flag, count);
  else if (n_groups) hipLaunchKernelGGL(k_tr_flags<0>, grid, block, 0, s, d_groups, d_ids, n_groups, paired, n_total, S, d_flag, count);
  if (n_groups) hipLaunchKernelGGL(k_tr_sum, dim3(1), dim3(64), 0, s, count);
  HIPCHK(hipEventRecord(W.ev[1], s));
  HIPCHK(hipGetLastError());
}

void taxreads_flag_finish(TaxReadsFlagWork &W, hipStream_t s) {
  uint64_t n = 0;
  read_back(&n, W.count.as<uint64_t>() + 1, sizeof n, s);   // (k_tr_sum's word; waits for the stream)
  W.n_matched = n;
  HIPCHK(hipEventElapsedTime(&W.ms, W.ev[0], W.ev[1]));
}

}  // namespace kslam
