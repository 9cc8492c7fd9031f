// readsplit.hip -- the batch's FASTQ records split by outcome, on the device (include/kslam_readsplit.h).
//
// When a lane has finished a batch, everything the split needs lies in device memory: the two texts as uploaded, their
// line-terminator lists (fastq_index.hip) and the read pairs that survived every stage (pairs.hip).  So:
//   1. k_rs_flags    one thread per read pair: flag[r1_read] = flag[r2_read] = 1 (block layout [R1 | R2]);
//   2. k_rs_lengths  one thread per record: the four lines' spans from the terminator list -- the text is NOT scanned again,
//                    only the records' own terminator bytes are looked at -- give the output length (the lines + 4) and
//                    whether the record is one run of the text as it stands (every line ended by a single "\n");
//   3. two exclusive scans per stream (selected / unselected lengths): where every record goes; the four sizes and the
//      record counts come back in ONE read-back;
//   4. k_rs_copy     a group of 16 lanes (short records) or a wavefront per record: whole-run records move as one span,
//                    the others line by line with a "\n" after each.  A span moves as aligned 16-byte stores fed by
//                    16-byte loads at whatever alignment the source has, with a byte head and tail.
// A pure streaming copy: 2 bytes of traffic per output byte, plus 25 bytes of index per record.
// Steps 2 to 4 also serve a caller that flags the records by a rule of its own (taxreads.hip: the reads of chosen taxa):
// read_split_prepare sizes and zeroes, the caller flags, read_split_flagged does the rest; read_split_device is the two
// around k_rs_flags.
#include "common.h"
#include "fastq_lines.h"
#include "../../include/kslam_readsplit.h"

namespace kslam {

namespace {

constexpr uint64_t RS_RUN = 1ull << 63;   // src[]: the record's output is text[start .. start + len) as it stands

struct __attribute__((packed, aligned(1))) RsBytes16 {
  uint32_t w[4];
};

__global__ __launch_bounds__(256) void k_rs_flags(const kslam_read_pair *__restrict__ groups, uint64_t n_groups, int paired,
                                                  uint64_t n_total, uint8_t *__restrict__ flag) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t r1 = groups[g].r1_read, r2 = groups[g].r2_read;
  if (r1 < n_total) flag[r1] = 1;
  if (paired && r2 < n_total) flag[r2] = 1;   // (single end: r2_read is 0 and means nothing)
}

// tot[0]: selected records of the stream, tot[1]: bit 0 = a record of 4 GiB or more
__global__ __launch_bounds__(256) void k_rs_lengths(FqStream s, const uint8_t *__restrict__ flag, uint32_t *__restrict__ len_sel,
                                                    uint32_t *__restrict__ len_unsel, uint64_t *__restrict__ src,
                                                    unsigned long long *__restrict__ n_sel, unsigned long long *__restrict__ err) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < s.n;
  bool f = false;
  if (live) {
    uint64_t total = 4, a0 = 0;
    bool run = true;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      uint64_t a, b, nx;
      line_span(s, 4 * r + l, &a, &b, &nx);
      if (l == 0) a0 = a;
      total += b - a;
      run = run && nx - b == 1 && s.text[b] == '\n';   // (nx - b == 1: b is a terminator inside the text)
    }
    const uint64_t o = s.first + r;
    f = flag[o] != 0;
    if (total > 0xFFFFFFFFull) { atomicOr(err, 1ull); total = 0; }
    len_sel[o] = f ? (uint32_t)total : 0u;
    len_unsel[o] = f ? 0u : (uint32_t)total;
    src[o] = a0 | (run ? RS_RUN : 0ull);
  }
  const uint64_t m = __ballot(live && f);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_sel, (unsigned long long)__popcll(m));
}

// n bytes from src to dst by the G lanes of a group: a byte head up to dst's 16-byte boundary, 16-byte pieces (aligned
// stores; the loads take the source as it lies), a byte tail.  Reads and writes [0, n) only.
template <int G>
__device__ inline void copy_span(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t lane) {
  const uint64_t to_boundary = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
  const uint64_t head = n < to_boundary ? n : to_boundary;
  if (lane < head) dst[lane] = src[lane];
  dst += head; src += head; n -= head;
  const uint64_t pieces = n >> 4;
  for (uint64_t p = lane; p < pieces; p += G) {
    const RsBytes16 v = *reinterpret_cast<const RsBytes16 *>(src + 16 * p);
    *reinterpret_cast<uint4 *>(dst + 16 * p) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
  }
  const uint64_t tail = n & 15u;
  if (lane < tail) dst[16 * pieces + lane] = src[16 * pieces + lane];
}

template <int G>
__global__ __launch_bounds__(256) void k_rs_copy(FqStream s, const uint8_t *__restrict__ flag, const uint32_t *__restrict__ len_sel,
                                                 const uint32_t *__restrict__ len_unsel, const uint64_t *__restrict__ src,
                                                 const uint64_t *__restrict__ off_sel, const uint64_t *__restrict__ off_unsel,
                                                 uint8_t *__restrict__ d_sel, uint8_t *__restrict__ d_unsel) {
  const uint64_t r = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
  const uint32_t lane = threadIdx.x % G;
  if (r >= s.n) return;
  const uint64_t o = s.first + r;
  const bool f = flag[o] != 0;
  uint8_t *dst = f ? d_sel : d_unsel;
  if (!dst) return;                       // a stream nobody asked for
  dst += f ? off_sel[o] : off_unsel[o];
  const uint64_t v = src[o];
  if (v & RS_RUN) {
    copy_span<G>(dst, s.text + (v & ~RS_RUN), f ? len_sel[o] : len_unsel[o], lane);
    return;
  }
  for (int l = 0; l < 4; l++) {
    uint64_t a, b, nx;
    line_span(s, 4 * r + l, &a, &b, &nx);
    copy_span<G>(dst, s.text + a, b - a, lane);
    if (lane == 0) dst[b - a] = '\n';
    dst += b - a + 1;
  }
}

}  // namespace

uint64_t read_split_prepare(const FqStream st[2], bool single, ReadSplitWork &W, hipStream_t s) {
  const uint64_t n = st[0].n + (single ? 0 : st[1].n);
  if (n >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "2^32 or more records in one batch"};
  W.kernel_ms = 0;
  W.bytes_moved = 0;
  if (!W.ev[0])
    for (auto &e : W.ev) HIPCHK(hipEventCreate(&e));
  W.flag.ensure(n + 16);
  W.len_sel.ensure((n + 1) * sizeof(uint32_t));
  W.len_unsel.ensure((n + 1) * sizeof(uint32_t));
  W.src.ensure((n + 1) * sizeof(uint64_t));
  W.off_sel.ensure((n + 1) * sizeof(uint64_t));
  W.off_unsel.ensure((n + 1) * sizeof(uint64_t));
  W.scan_tmp.ensure(scan_tmp_bytes(std::max<uint64_t>(n, 1)));
  W.totals.ensure(8 * sizeof(uint64_t));
  HIPCHK(hipMemsetAsync(W.totals.p, 0, 8 * sizeof(uint64_t), s));
  HIPCHK(hipMemsetAsync(W.flag.p, 0, n + 16, s));
  return n;
}

void read_split_device(const FqStream st[2], bool single, const kslam_read_pair *d_groups, uint64_t n_groups, uint32_t which,
                       ReadSplitWork &W, uint64_t bytes[4], uint64_t n_records[2], hipStream_t s) {
  for (int k = 0; k < 4; k++) bytes[k] = 0;
  n_records[0] = n_records[1] = 0;
  const uint64_t n = read_split_prepare(st, single, W, s);
  HIPCHK(hipEventRecord(W.ev[0], s));
  if (n_groups)
    hipLaunchKernelGGL(k_rs_flags, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, s, d_groups, n_groups, single ? 0 : 1, n,
                       W.flag.as<uint8_t>());
  read_split_flagged(st, single, which, W, bytes, n_records, s);
}

void read_split_flagged(const FqStream st[2], bool single, uint32_t which, ReadSplitWork &W, uint64_t bytes[4], uint64_t n_records[2],
                        hipStream_t s) {
  const int n_streams = single ? 1 : 2;
  for (int k = 0; k < 4; k++) bytes[k] = 0;
  n_records[0] = n_records[1] = 0;
  uint64_t *tot = W.totals.as<uint64_t>();   // [k] selected bytes of stream k, [2 + k] unselected, [4 + k] selected records, [6] errors
  for (int k = 0; k < n_streams; k++) {
    if (!st[k].n) continue;
    hipLaunchKernelGGL(k_rs_lengths, dim3((unsigned)((st[k].n + 255) / 256)), dim3(256), 0, s, st[k], W.flag.as<uint8_t>(),
                       W.len_sel.as<uint32_t>(), W.len_unsel.as<uint32_t>(), W.src.as<uint64_t>(),
                       reinterpret_cast<unsigned long long *>(tot + 4 + k), reinterpret_cast<unsigned long long *>(tot + 6));
    const uint64_t f = st[k].first;
    if (which & KSLAM_READS_OUT_CLASSIFIED)
      exclusive_scan_u32_to_u64(W.len_sel.as<uint32_t>() + f, W.off_sel.as<uint64_t>() + f, st[k].n, tot + k, W.scan_tmp.p, s);
    if (which & KSLAM_READS_OUT_UNCLASSIFIED)
      exclusive_scan_u32_to_u64(W.len_unsel.as<uint32_t>() + f, W.off_unsel.as<uint64_t>() + f, st[k].n, tot + 2 + k, W.scan_tmp.p, s);
  }
  HIPCHK(hipEventRecord(W.ev[1], s));
  HIPCHK(hipGetLastError());
  uint64_t h[8];
  read_back(h, tot, sizeof h, s);
  if (h[6]) throw StatusError{KSLAM_ERR_UNSUPPORTED, "a FASTQ record of 4 GiB or more"};
  uint64_t moved = 0;
  for (int k = 0; k < n_streams; k++) {
    bytes[k] = h[k];
    bytes[2 + k] = h[2 + k];
    moved += h[k] + h[2 + k];
  }
  n_records[0] = h[4];
  n_records[1] = st[0].n - h[4];
  if (!single && h[5] != h[4]) throw StatusError{KSLAM_ERR_INTERNAL, "read pairs that select R1 and R2 records differently"};
  for (int k = 0; k < 4; k++) W.out[k].ensure(bytes[k] + 64);
  HIPCHK(hipEventRecord(W.ev[2], s));
  for (int k = 0; k < n_streams; k++) {
    if (!st[k].n || !(bytes[k] + bytes[2 + k])) continue;
    uint8_t *d_sel = (which & KSLAM_READS_OUT_CLASSIFIED) ? W.out[k].as<uint8_t>() : nullptr;
    uint8_t *d_unsel = (which & KSLAM_READS_OUT_UNCLASSIFIED) ? W.out[2 + k].as<uint8_t>() : nullptr;
    // short records (150-base reads: some 330 bytes) take 16 lanes each, four to a wavefront; long ones a wavefront
    const uint64_t mean = (bytes[k] + bytes[2 + k]) / st[k].n;
    if (mean <= 512)
      hipLaunchKernelGGL(k_rs_copy<16>, dim3((unsigned)((st[k].n + 15) / 16)), dim3(256), 0, s, st[k], W.flag.as<uint8_t>(),
                         W.len_sel.as<uint32_t>(), W.len_unsel.as<uint32_t>(), W.src.as<uint64_t>(), W.off_sel.as<uint64_t>(),
                         W.off_unsel.as<uint64_t>(), d_sel, d_unsel);
    else
      hipLaunchKernelGGL(k_rs_copy<64>, dim3((unsigned)((st[k].n + 3) / 4)), dim3(256), 0, s, st[k], W.flag.as<uint8_t>(),
                         W.len_sel.as<uint32_t>(), W.len_unsel.as<uint32_t>(), W.src.as<uint64_t>(), W.off_sel.as<uint64_t>(),
                         W.off_unsel.as<uint64_t>(), d_sel, d_unsel);
  }
  HIPCHK(hipEventRecord(W.ev[3], s));
  HIPCHK(hipGetLastError());
  HIPCHK(stream_wait(s));
  float a = 0, b = 0;
  HIPCHK(hipEventElapsedTime(&a, W.ev[0], W.ev[1]));
  HIPCHK(hipEventElapsedTime(&b, W.ev[2], W.ev[3]));
  W.kernel_ms = a + b;
  W.bytes_moved = 2 * moved;
}

}  // namespace kslam
