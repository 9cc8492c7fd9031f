// kreport.hip -- the Kraken-style report's counts, accumulated on the device (include/kslam_kreport.h).
//
// When a lane has run the per-read stage, the batch's taxonomy ids -- one per read pair -- lie in device memory; so does the
// dense taxonomy tree (SamAnnot: up, depth, node_tax).  The state is one 64-bit direct counter per node, the tree's ids sorted
// ascending with their nodes, and a list of (id << 32 | count) items for the ids the tree does not know.  Several lanes count
// into it from their own streams, so every update is a device-scope atomic; every accumulator is an integer add, so the result
// does not depend on who counted what in which order.
//   1. k_kr_count    one thread per read pair: id -> node by binary search in the sorted table.  Real samples are heavily
//                    skewed (a few taxa take most reads), so the lanes of a wavefront that hold the same node are combined
//                    first: the lowest pending lane's node is broadcast, the equal lanes are balloted, the leader adds the
//                    population count, and the rest repeats -- one 64-bit atomicAdd per distinct node per wave.  Unknown ids
//                    go through the same combining into a per-call item buffer through an atomic cursor (at most one item per
//                    lane, so a buffer of n items cannot overflow); the caller appends the items to the state's list.
//   2. on request (kreport_take_device): the clade array is zeroed; k_kr_walk, one thread per node with direct > 0, adds its
//                    direct count to itself and to every ancestor; clade > 0 is flagged, scanned (scan.hip) and the known rows
//                    are compacted in node order.  The unknown items are sorted by id (radix_sort.hip), run heads are flagged
//                    and numbered by a scan, and every item adds its count to its run's row behind the known ones.
// Bounds: a node comes out of the table (values < n_nodes, checked again); the walk takes depth[node] steps at most -- the nodes
// on its path -- and stops at the first parent that is not a node, so no index leaves [0, n_nodes) whatever ids arrive.
#include "common.h"
#include "../../include/kslam_kreport.h"

namespace kslam {

namespace {

constexpr uint32_t KR_NONE = KSLAM_KREPORT_NO_NODE;
constexpr int KR_BLOCK = 256;
constexpr uint64_t KR_SLICE = 1ull << 30;   // ids per launch

struct KrRow {   // kslam_kreport_row as the atomics want it
  uint32_t tax_id, node;
  unsigned long long direct, clade;
};
static_assert(sizeof(KrRow) == sizeof(kslam_kreport_row), "the device row is the ABI's");

inline unsigned kr_blocks(uint64_t n) { return (unsigned)((n + KR_BLOCK - 1) / KR_BLOCK); }

// DRY: only the cursor moves (how many items the call would append); COMBINE = false: the measurement-only variant, one atomic
// per read pair
template <bool DRY, bool COMBINE>
__global__ __launch_bounds__(KR_BLOCK) void k_kr_count(const uint32_t *__restrict__ ids, uint64_t n, KreportTable T,
                                                       unsigned long long *__restrict__ items, unsigned long long *__restrict__ cursor) {
  const uint64_t i = (uint64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t id = i < n ? ids[i] : 0u;   // (no early return: every lane takes part in the ballots)
  uint32_t node = KR_NONE;
  if (id && T.n_nodes) {
    uint64_t lo = 0, hi = T.n_nodes;   // the first key >= id
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (T.keys[mid] < id) lo = mid + 1;
      else hi = mid;
    }
    if (lo < T.n_nodes && T.keys[lo] == id) node = T.nodes[lo];
    if (node >= T.n_nodes) node = KR_NONE;
  }
  const bool known = node != KR_NONE, unknown = id != 0 && !known;
  if (!COMBINE) {
    if (known && !DRY) atomicAdd(T.direct + node, 1ull);
    if (unknown) {
      const unsigned long long slot = atomicAdd(cursor, 1ull);
      if (!DRY) items[slot] = ((unsigned long long)id << 32) | 1ull;
    }
    return;
  }
  uint64_t pending = __ballot(known);
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const uint32_t k0 = __shfl(node, leader);           // (never KR_NONE: the leader is a known lane)
    const uint64_t m = __ballot(node == k0);
    if (lane == leader && !DRY) atomicAdd(T.direct + k0, (unsigned long long)__popcll(m));
    pending &= ~m;
  }
  pending = __ballot(unknown);
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const uint32_t k0 = __shfl(id, leader);
    const uint64_t m = __ballot(unknown && id == k0);
    if (lane == leader) {
      const unsigned long long slot = atomicAdd(cursor, 1ull);
      if (!DRY) items[slot] = ((unsigned long long)k0 << 32) | (unsigned long long)__popcll(m);
    }
    pending &= ~m;
  }
}

__global__ __launch_bounds__(KR_BLOCK) void k_kr_walk(const unsigned long long *__restrict__ direct, const uint32_t *__restrict__ up,
                                                      const uint32_t *__restrict__ depth, unsigned long long *__restrict__ clade, uint64_t n_nodes) {
  const uint64_t v = (uint64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
  if (v >= n_nodes) return;
  const unsigned long long d = direct[v];
  if (!d) return;
  uint64_t steps = depth[v];   // the nodes on the path up, this one included
  if (steps > n_nodes) steps = n_nodes;
  uint32_t at = (uint32_t)v;
  for (; steps && at < n_nodes; steps--) {
    atomicAdd(clade + at, d);
    at = up[at];
  }
}

__global__ __launch_bounds__(KR_BLOCK) void k_kr_flag(const unsigned long long *__restrict__ clade, uint32_t *__restrict__ flag, uint64_t n_nodes) {
  const uint64_t v = (uint64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
  if (v < n_nodes) flag[v] = clade[v] != 0;
}

__global__ __launch_bounds__(KR_BLOCK) void k_kr_rows(const unsigned long long *__restrict__ clade, const unsigned long long *__restrict__ direct,
                                                      const uint32_t *__restrict__ node_tax, const uint32_t *__restrict__ pos,
                                                      KrRow *__restrict__ rows, uint64_t n_nodes, uint64_t n_known) {
  const uint64_t v = (uint64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
  if (v >= n_nodes || !clade[v]) return;
  const uint32_t at = pos[v];
  if (at < n_known) rows[at] = KrRow{node_tax[v], (uint32_t)v, direct[v], clade[v]};
}

__global__ __launch_bounds__(KR_BLOCK) void k_kr_heads(const uint64_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
  if (i < n) head[i] = i == 0 || (key[i] >> 32) != (key[i - 1] >> 32);
}

// rows: the n_runs rows behind the known ones, zeroed
__global__ __launch_bounds__(KR_BLOCK) void k_kr_unknown(const uint64_t *__restrict__ key, uint64_t n, const uint32_t *__restrict__ head,
                                                         const uint32_t *__restrict__ before, KrRow *__restrict__ rows, uint64_t n_runs) {
  const uint64_t i = (uint64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t r = (uint64_t)before[i] + head[i] - 1;   // (item 0 is a head: never negative)
  if (r >= n_runs) return;
  if (head[i]) {
    rows[r].tax_id = (uint32_t)(key[i] >> 32);
    rows[r].node = KR_NONE;
  }
  const unsigned long long count = key[i] & 0xFFFFFFFFull;
  atomicAdd(&rows[r].direct, count);
  atomicAdd(&rows[r].clade, count);
}

template <bool DRY>
void launch_count(bool combine, unsigned grid, hipStream_t s, const uint32_t *d_ids, uint64_t n, const KreportTable &T, unsigned long long *items,
                  unsigned long long *cursor) {
  if (combine) hipLaunchKernelGGL((k_kr_count<DRY, true>), dim3(grid), dim3(KR_BLOCK), 0, s, d_ids, n, T, items, cursor);
  else hipLaunchKernelGGL((k_kr_count<DRY, false>), dim3(grid), dim3(KR_BLOCK), 0, s, d_ids, n, T, items, cursor);
}

}  // namespace

void kreport_count_device(const uint32_t *d_ids, uint64_t n, const KreportTable &T, KreportCountWork &W, bool dry, hipStream_t s) {
  W.ms = 0;
  W.n_new = 0;
  if (!n) return;
  bool combine = true;
#ifdef KSLAM_ABLATE
  if (const char *e = getenv("KSLAM_KREPORT_ABLATE")) combine = e[0] != '1';   // measurement only: one atomic per read pair
#endif
  if (!W.ev[0])
    for (auto &e : W.ev) HIPCHK(hipEventCreate(&e));
  if (!dry) W.items.ensure(n * sizeof(uint64_t));
  W.cursor.ensure(sizeof(uint64_t));
  unsigned long long *cursor = W.cursor.as<unsigned long long>();
  HIPCHK(hipMemsetAsync(cursor, 0, sizeof(uint64_t), s));
  HIPCHK(hipEventRecord(W.ev[0], s));
  for (uint64_t at = 0; at < n; at += KR_SLICE) {
    const uint64_t len = n - at < KR_SLICE ? n - at : KR_SLICE;
    if (dry) launch_count<true>(combine, kr_blocks(len), s, d_ids + at, len, T, nullptr, cursor);
    else launch_count<false>(combine, kr_blocks(len), s, d_ids + at, len, T, W.items.as<unsigned long long>(), cursor);
  }
  HIPCHK(hipEventRecord(W.ev[1], s));
  HIPCHK(hipGetLastError());
  uint64_t n_new = 0;
  read_back(&n_new, cursor, sizeof n_new, s);   // (waits for the stream)
  W.n_new = n_new;
  HIPCHK(hipEventElapsedTime(&W.ms, W.ev[0], W.ev[1]));
}

void kreport_take_device(const KreportTable &T, const uint32_t *d_up, const uint32_t *d_depth, const uint32_t *d_node_tax, const uint64_t *d_items,
                         uint64_t n_items, KreportTakeWork &W, uint64_t *n_known_out, uint64_t *n_unknown_out, hipEvent_t ev[2], hipStream_t s) {
  *n_known_out = *n_unknown_out = 0;
  if (T.n_nodes >= (1ull << 32) || n_items >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^32 or more nodes or unknown-id items"};
  const uint64_t n_scan = T.n_nodes > n_items ? T.n_nodes : n_items;
  W.scan_tmp.ensure(scan_tmp_bytes(n_scan + 1));
  W.totals.ensure(2 * sizeof(uint64_t));
  uint64_t *d_tot = W.totals.as<uint64_t>();
  HIPCHK(hipMemsetAsync(d_tot, 0, 2 * sizeof(uint64_t), s));
  HIPCHK(hipEventRecord(ev[0], s));
  // ---- the known nodes: clade sums, flags, places ----
  uint64_t n_known = 0;
  if (T.n_nodes) {
    W.clade.ensure(T.n_nodes * sizeof(uint64_t));
    W.flag.ensure(T.n_nodes * sizeof(uint32_t));
    W.pos.ensure(T.n_nodes * sizeof(uint32_t));
    HIPCHK(hipMemsetAsync(W.clade.p, 0, T.n_nodes * sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_kr_walk, dim3(kr_blocks(T.n_nodes)), dim3(KR_BLOCK), 0, s, T.direct, d_up, d_depth, W.clade.as<unsigned long long>(), T.n_nodes);
    hipLaunchKernelGGL(k_kr_flag, dim3(kr_blocks(T.n_nodes)), dim3(KR_BLOCK), 0, s, W.clade.as<unsigned long long>(), W.flag.as<uint32_t>(), T.n_nodes);
    HIPCHK(hipGetLastError());
    exclusive_scan_u32(W.flag.as<uint32_t>(), W.pos.as<uint32_t>(), T.n_nodes, d_tot, W.scan_tmp.p, s);
  }
  // ---- the unknown ids: sorted by id, run heads numbered ----
  uint64_t n_unknown = 0;
  const uint64_t *key = nullptr;
  if (n_items) {
    W.keys_a.ensure(n_items * sizeof(uint64_t));
    W.keys_b.ensure(n_items * sizeof(uint64_t));
    W.head.ensure(n_items * sizeof(uint32_t));
    W.run.ensure(n_items * sizeof(uint32_t));
    HIPCHK(hipMemcpyAsync(W.keys_a.p, d_items, n_items * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    void *sorted = W.keys_a.p;
    if (n_items > 1) {
      SortPass passes[4];   // the id is the key's upper word
      for (int p = 0; p < 4; p++) passes[p] = SortPass{1u, (uint32_t)(8 * p), 0u};
      sorted = radix_sort(W.keys_a.p, W.keys_b.p, n_items, 2, passes, 4, W.sortws, s, nullptr, nullptr, nullptr);
    }
    key = static_cast<const uint64_t *>(sorted);
    hipLaunchKernelGGL(k_kr_heads, dim3(kr_blocks(n_items)), dim3(KR_BLOCK), 0, s, key, n_items, W.head.as<uint32_t>());
    HIPCHK(hipGetLastError());
    exclusive_scan_u32(W.head.as<uint32_t>(), W.run.as<uint32_t>(), n_items, d_tot + 1, W.scan_tmp.p, s);
  }
  uint64_t h[2] = {0, 0};
  read_back(h, d_tot, sizeof h, s);
  n_known = h[0];
  n_unknown = h[1];
  // ---- the rows ----
  W.rows.ensure((n_known + n_unknown + 1) * sizeof(KrRow));
  KrRow *rows = W.rows.as<KrRow>();
  if (n_known)
    hipLaunchKernelGGL(k_kr_rows, dim3(kr_blocks(T.n_nodes)), dim3(KR_BLOCK), 0, s, W.clade.as<unsigned long long>(), T.direct, d_node_tax,
                       W.pos.as<uint32_t>(), rows, T.n_nodes, n_known);
  if (n_unknown) {
    HIPCHK(hipMemsetAsync(rows + n_known, 0, n_unknown * sizeof(KrRow), s));
    hipLaunchKernelGGL(k_kr_unknown, dim3(kr_blocks(n_items)), dim3(KR_BLOCK), 0, s, key, n_items, W.head.as<uint32_t>(), W.run.as<uint32_t>(),
                       rows + n_known, n_unknown);
  }
  HIPCHK(hipEventRecord(ev[1], s));
  HIPCHK(hipGetLastError());
  *n_known_out = n_known;
  *n_unknown_out = n_unknown;
}

}  // namespace kslam
