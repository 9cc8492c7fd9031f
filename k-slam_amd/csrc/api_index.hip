// api_index.hip -- the C ABI, part 2: kslam_set_index (genome k-mer extraction, the ONE-TIME sort of the genome k-mer list,
// key / {meta, offset} columns, bucket table, membership filter: build_index) and the stage-level entry points the parity tests
// use (kslam_extract_kmers / _sort_kmers / _selftest_sort / _find_overlaps).  Replaces GenbankIndex::getKMers + sortKMers of
// every batch (reference src/GenbankTools.h:211-219, src/KMer.h:388-398, src/SLAM.h:64-65) by one build per index.
#include "context.h"

namespace kslam_api {

__global__ void k_split_soa(const uint4 *__restrict__ recs, uint32_t n, uint64_t *__restrict__ key, uint2 *__restrict__ mo) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint4 r = recs[i];
  key[i] = ((uint64_t)r.y << 32) | r.x;
  mo[i] = make_uint2(r.z, r.w);
}

__global__ void k_fill_random(uint4 *recs, uint32_t n, uint64_t seed) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t z = seed + (uint64_t)i * 0x9E3779B97F4A7C15ull;   // splitmix64
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  recs[i] = make_uint4((uint32_t)z, (uint32_t)(z >> 32), i, ~i);
}
__global__ void k_count_inversions(const uint4 *recs, uint32_t n, unsigned long long *out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i + 1 >= n) return;
  const uint4 a = recs[i], b = recs[i + 1];
  const uint64_t ka = ((uint64_t)a.y << 32) | a.x, kb = ((uint64_t)b.y << 32) | b.x;
  // stable LSD: equal keys keep their input order (z = original index)
  if (ka > kb || (ka == kb && a.z > b.z)) atomicAdd(out, 1ull);
}

__global__ void k_to_temp(const kslam_overlap *__restrict__ in, uint64_t n, kslam_overlap_temp *__restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kslam_overlap o = in[i];
  kslam_overlap_temp t;
  t.read = o.read; t.entry = o.entry; t.rel = o.rel; t.revcomp = o.revcomp;
  t.pad[0] = t.pad[1] = t.pad[2] = 0;
  out[i] = t;
}

// passes over the 64-bit k-mer (words x, y of the record), least significant first
void kmer_passes(std::vector<SortPass> &v) {
  for (uint32_t w = 0; w < 2; w++)
    for (uint32_t b = 0; b < 4; b++) v.push_back(SortPass{w, 8 * b, 0});
}
// sortKMers key (KMer.h:392-396): kmer asc, meta desc -> LSD: ~meta bytes, then kmer bytes
void full_key_passes(std::vector<SortPass> &v) {
  for (uint32_t b = 0; b < 4; b++) v.push_back(SortPass{2, 8 * b, 0xFFFFFFFFu});
  kmer_passes(v);
}

struct Planned {
  uint64_t n_kmers = 0, n_segs = 0;
};
Planned plan_host(const uint64_t *off, uint64_t n, uint32_t gap) {
  Planned p;
  for (uint64_t i = 0; i < n; i++) {
    uint64_t len = off[i + 1] - off[i];
    uint64_t k = len >= KSLAM_K ? (len - KSLAM_K) / gap + 1 : 0;
    p.n_kmers += k;
    p.n_segs += (k + SEG_KMERS - 1) / SEG_KMERS;
  }
  return p;
}

// extraction of n sequences d_off[0..n] into d_out (AoS records)
void run_extract(kslam_ctx *c, const uint8_t *d_bases, const uint64_t *d_off, uint64_t n, uint32_t gap, int is_gb,
                 uint64_t n_segs, uint4 *d_out, uint8_t *d_digits, const SortPass *first_pass) {
  hipStream_t s = c->stream;
  c->nk.ensure(n * sizeof(uint32_t) + 4);
  c->nseg.ensure(n * sizeof(uint32_t) + 4);
  c->rec_start.ensure(n * sizeof(uint64_t) + 8);
  c->seg_start.ensure(n * sizeof(uint64_t) + 8);
  c->scan_tmp.ensure(scan_tmp_bytes(n));
  c->totals.ensure(8 * sizeof(uint64_t));
  c->segs.ensure((n_segs + 1) * sizeof(SegEntry));
  extract_plan(d_off, n, gap, c->nk.as<uint32_t>(), c->nseg.as<uint32_t>(), c->rec_start.as<uint64_t>(),
               c->seg_start.as<uint64_t>(), c->totals.as<uint64_t>(), c->scan_tmp.p, s);
  extract_fill_segments(c->nk.as<uint32_t>(), c->rec_start.as<uint64_t>(), c->seg_start.as<uint64_t>(), n, gap,
                        c->segs.as<SegEntry>(), s, n_segs);
  extract_kmers_launch(d_bases, d_off, c->segs.as<SegEntry>(), n_segs, gap, is_gb, 0, d_out, s, d_digits, first_pass);
}

// kslam_set_index / _device, before the upload: the context and its lanes let go of their index (freed here unless a sibling
// still holds it, so that the old and the new one are not resident together) and the new one starts empty
std::shared_ptr<GenomeIndex> new_index(kslam_ctx *c, uint64_t n_entries) {
  c->index.reset();
  for (auto *l : c->lanes) l->c->index.reset();
  release_index_bound_reports(c);
  auto ix = std::make_shared<GenomeIndex>();
  ix->n_entries = n_entries;
  ix->h_goff.assign(n_entries + 1, 0);
  return ix;
}

// builds the uploaded index ixp and hands it to the context and its lanes (no batch may be in flight across kslam_set_index)
void build_index(kslam_ctx *c, std::shared_ptr<GenomeIndex> ixp) {
  GenomeIndex &ix = *ixp;
  hipStream_t s = c->stream;
  const uint64_t n = ix.n_entries;
  ix.max_entry_len = 0;
  for (uint64_t i = 0; i < n; i++) ix.max_entry_len = std::max(ix.max_entry_len, ix.h_goff[i + 1] - ix.h_goff[i]);
  if (n >= (1ull << 30)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^30 entries (KMer.h:65 id field)"};
  if (ix.max_entry_len >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "entry longer than 2^32 bases"};
  ix.g_off.ensure((n + 1) * sizeof(uint64_t));
  HIPCHK(hipMemcpyAsync(ix.g_off.p, ix.h_goff.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  struct Events {       // destroyed on every way out of this function
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } evs;
  for (hipEvent_t &x : evs.e) HIPCHK(hipEventCreate(&x));
  hipEvent_t ev_begin = evs.e[0], e1 = evs.e[1], e2 = evs.e[2], e3 = evs.e[3];
  HIPCHK(hipEventRecord(ev_begin, s));
  ix.g_codes.ensure(ix.h_goff[n] + 64);
  encode_bases(ix.g_bases.as<uint8_t>(), ix.g_codes.as<uint8_t>(), ix.h_goff[n] + 48, s);
  Planned pl = plan_host(ix.h_goff.data(), n, KSLAM_K / 2);  // gap k/2, SLAM.h:64
  if (pl.n_kmers >= (1ull << 32)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^32 genome k-mers"};
  ix.n_gk = pl.n_kmers;
  const uint64_t m = pl.n_kmers;
  c->recs_a.ensure((m + 1) * sizeof(uint4));
  c->recs_b.ensure((m + 1) * sizeof(uint4));
  // sortKMers' order (src/KMer.h:388-398): k-mer ascending, then the meta word DESCENDING.  LSD passes over the meta word
  // first -- but only over what can differ in a list of genome records: the id (n entries: bits 0 .. b - 1), isFromGB = 1
  // everywhere, revComp in bit 30 -- then the 8 bytes of the k-mer.  The id's bytes below its top one take a pass each; its
  // top bits (at most 7 of them) share ONE pass with the revComp bit above them (SortPass::hi_bits): ids of 1 250 entries
  // are 11 bits, so the meta word takes two passes -- id bits 0-7, then {revComp, id bits 8-14} -- and the sort ten.
  // (Round 5: a pass per byte that can differ, three for this database.)
  std::vector<SortPass> passes;
  {
    const uint32_t id_bits = (uint32_t)bits_for(n ? n - 1 : 0);     // <= 30
    uint32_t at = 0;
    while (id_bits - at > 7) {                                        // whole bytes of the id while more than 7 bits remain
      passes.push_back(SortPass{2, at, 0xFFFFFFFFu});
      at += 8;
    }
    SortPass top{2, at, 0xFFFFFFFFu};                                 // the rest of the id below the revComp bit
    top.hi_shift = 30;
    top.hi_bits = 1;
    passes.push_back(top);
  }
  kmer_passes(passes);
  // the extraction writes the first pass's digit of every record next to it: the sort's first histogram reads 1 byte per
  // record instead of 16
  const bool first_digits = c->tune.sort_digit_bytes && passes.size() > 1;
  if (first_digits) c->sortws.digits.ensure(m + 64);
  run_extract(c, ix.g_bases.as<uint8_t>(), ix.g_off.as<uint64_t>(), n, KSLAM_K / 2, 1, pl.n_segs,
              c->recs_a.as<uint4>(), first_digits ? c->sortws.digits.as<uint8_t>() : nullptr, first_digits ? &passes[0] : nullptr);
  c->sortws.use_digit_bytes = c->tune.sort_digit_bytes;
  c->sortws.first_digits_ready = first_digits;
  c->sortws.meta_digits_in_runs = n && m / n >= 64;     // (a database of many tiny entries has as many ids as records in a tile)
  HIPCHK(hipEventRecord(e1, s));
  void *sorted = radix_sort(c->recs_a.p, c->recs_b.p, m, 4, passes.data(), (int)passes.size(), c->sortws, s,
                            nullptr, nullptr, nullptr, /*setup=*/true);
  c->sortws.first_digits_ready = false;
  c->sortws.meta_digits_in_runs = false;
  HIPCHK(hipEventRecord(e2, s));
  ix.gk_key.ensure((m + 1) * sizeof(uint64_t));
  ix.gk_meta.ensure((m + 1) * sizeof(uint2));   // {meta, offset} pairs
  uint32_t bits = 8, max_bits = (uint32_t)c->tune.bucket_bits_max;   // 27: ~2.3 genome k-mers per bucket for a 5 Gb database (537 MB table)
  while (bits < max_bits && (m >> (bits + 2)) != 0) bits++;   // 2 to 4 keys per bucket (measured: 3.06 ms at 27 bits, 3.24 at 26, 3.13 at 28)
  if (c->tune.bucket_bits_exact) bits = (uint32_t)c->tune.bucket_bits_exact;   // tuning
  ix.bucket_bits = bits;
  ix.g_bucket.ensure(((1ull << bits) + 2) * sizeof(uint32_t));
  // membership filter for the read extraction: ~14 bits per genome k-mer (9.3 keys per 128-bit piece),
  // 2^32 bits = 512 MiB for the 312 M k-mers of a 5 Gb database.  KSLAM_FILTER_BITS: log2 of the size
  // in bits, 0 = extract, sort and look up every read k-mer as the reference does.
  uint32_t fb = 20;
  while (fb < 35 && ((uint64_t)1 << fb) < m * 12) fb++;
  if (c->tune.filter_bits >= 0) fb = (uint32_t)c->tune.filter_bits;
  // filter.hip takes line_bits = fb - 10 unsigned and blocks of 2^11 pieces: below 2^20 bits that would wrap
  // (read_tuning clamps KSLAM_FILTER_BITS to [20, 36], the automatic size starts at 20)
  if (fb != 0 && fb < 20)
    throw StatusError{KSLAM_ERR_INTERNAL, "membership filter of 2^" + std::to_string(fb) + " bits: the smallest is 2^20"};
  ix.filter_bits = fb;
  if (fb) ix.g_filter.ensure(filter_bytes(fb));
  // the probe words of the filter's build go through the record buffers of the sort that has just finished: the one that does not
  // hold the sorted list takes them first
  void *other = sorted == c->recs_a.p ? c->recs_b.p : c->recs_a.p;
  bool fused = false;
  if (fb && c->tune.filter_build_sorted)
    fused = split_columns_and_tables(sorted, (uint32_t)m, ix.gk_key.as<uint64_t>(), ix.gk_meta.p, bits, ix.g_bucket.as<uint32_t>(), fb, other, c->sortws, s);
  if (!fused) {
    if (m) hipLaunchKernelGGL(k_split_soa, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, (const uint4 *)sorted,
                              (uint32_t)m, ix.gk_key.as<uint64_t>(), ix.gk_meta.as<uint2>());
    build_bucket_table(ix.gk_key.as<uint64_t>(), (uint32_t)m, bits, ix.g_bucket.as<uint32_t>(), s);
  }
  if (fb) {
    if (c->tune.filter_build_sorted) {
      c->pos.ensure((filter_bytes(fb) / 32768 + 2) * sizeof(uint32_t));
      filter_build_sorted(ix.gk_key.as<uint64_t>(), (uint32_t)m, fb, ix.g_filter.p, other, sorted, c->pos.as<uint32_t>(), c->sortws, s, fused);
    } else {
      filter_build(ix.gk_key.as<uint64_t>(), (uint32_t)m, fb, ix.g_filter.p, s);
    }
  }
  HIPCHK(hipEventRecord(e3, s));
  HIPCHK(stream_wait(s));
  {
    kslam_index_stats &st = ix.stats;
    memset(&st, 0, sizeof st);
    st.n_genome_kmers = m;
    st.sort_passes = (uint32_t)passes.size();
    st.n_entries = (uint32_t)n;
    (void)hipEventElapsedTime(&st.ms_encode_extract, ev_begin, e1);
    (void)hipEventElapsedTime(&st.ms_sort, e1, e2);
    (void)hipEventElapsedTime(&st.ms_tables, e2, e3);
    (void)hipEventElapsedTime(&st.ms_total, ev_begin, e3);
    // the one-time sorts' digit bytes (one per genome k-mer: 312 MB for the 5 Gb database) are not kept for the context's life:
    // a batch's sort allocates what its own record count needs
    c->sortws.digits.release();
  }
  c->index = std::move(ixp);
  c->kept_last = 0;
  for (auto *l : c->lanes) share_index(l->c, c);
}

}  // namespace kslam_api

extern "C" {

kslam_status kslam_index_build_stats(const kslam_ctx *c, kslam_index_stats *out) {
  if (!c || !out) return KSLAM_ERR_ARG;
  if (!c->index) return KSLAM_ERR_STATE;
  *out = c->index->stats;
  return KSLAM_OK;
}

kslam_status kslam_set_index(kslam_ctx *c, uint64_t n_entries, const char *const *bases, const uint64_t *lens) {
  return guarded(c, [&] {
    if (n_entries && (!bases || !lens)) throw StatusError{KSLAM_ERR_ARG, "null bases/lens"};
    auto ixp = new_index(c, n_entries);
    GenomeIndex &ix = *ixp;
    for (uint64_t i = 0; i < n_entries; i++) ix.h_goff[i + 1] = ix.h_goff[i] + lens[i];
    const uint64_t total = ix.h_goff[n_entries];
    ix.g_bases.ensure(total + 64);
    for (uint64_t i = 0; i < n_entries; i++)
      if (lens[i])
        HIPCHK(hipMemcpyAsync(ix.g_bases.as<uint8_t>() + ix.h_goff[i], bases[i], lens[i], hipMemcpyHostToDevice,
                              c->stream));
    HIPCHK(hipMemsetAsync(ix.g_bases.as<uint8_t>() + total, 0, 64, c->stream));
    HIPCHK(stream_wait(c->stream));
    build_index(c, std::move(ixp));
  });
}

kslam_status kslam_set_index_device(kslam_ctx *c, uint64_t n_entries, const void *d_bases,
                                    const uint64_t *h_offsets) {
  return guarded(c, [&] {
    if (n_entries && (!d_bases || !h_offsets)) throw StatusError{KSLAM_ERR_ARG, "null bases/offsets"};
    auto ixp = new_index(c, n_entries);
    GenomeIndex &ix = *ixp;
    const uint64_t o0 = n_entries ? h_offsets[0] : 0;
    for (uint64_t i = 0; i <= n_entries && n_entries; i++) ix.h_goff[i] = h_offsets[i] - o0;
    const uint64_t total = ix.h_goff[n_entries];
    ix.g_bases.ensure(total + 64);
    if (total)
      HIPCHK(hipMemcpyAsync(ix.g_bases.p, (const uint8_t *)d_bases + o0, total, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemsetAsync(ix.g_bases.as<uint8_t>() + total, 0, 64, c->stream));
    build_index(c, std::move(ixp));
  });
}

kslam_status kslam_extract_kmers(kslam_ctx *c, uint64_t n, const char *const *bases, const uint64_t *lens,
                                 int is_from_genbank, uint32_t gap, kslam_kmer *out, uint64_t cap, uint64_t *n_out) {
  return guarded(c, [&] {
    if (!n_out) throw StatusError{KSLAM_ERR_ARG, "null n_out"};
    if (gap == 0 || gap > MAX_GAP) throw StatusError{KSLAM_ERR_UNSUPPORTED, "gap must be in 1..64"};
    if (n >= (1ull << 30)) throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^30 sequences"};
    std::vector<uint64_t> off(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + lens[i];
    Planned pl = plan_host(off.data(), n, gap);
    *n_out = pl.n_kmers;
    if (pl.n_kmers > cap || pl.n_kmers == 0) return;
    hipStream_t s = c->stream;
    DevBuf db, doff, drec;
    db.ensure(off[n] + 64);
    doff.ensure((n + 1) * sizeof(uint64_t));
    drec.ensure(pl.n_kmers * sizeof(uint4));
    for (uint64_t i = 0; i < n; i++)
      if (lens[i]) HIPCHK(hipMemcpyAsync(db.as<uint8_t>() + off[i], bases[i], lens[i], hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(db.as<uint8_t>() + off[n], 0, 64, s));
    HIPCHK(hipMemcpyAsync(doff.p, off.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    run_extract(c, db.as<uint8_t>(), doff.as<uint64_t>(), n, gap, is_from_genbank, pl.n_segs, drec.as<uint4>());
    HIPCHK(hipMemcpyAsync(out, drec.p, pl.n_kmers * sizeof(uint4), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    db.release(); doff.release(); drec.release();
  });
}

kslam_status kslam_sort_kmers(kslam_ctx *c, kslam_kmer *recs, uint64_t n) {
  return guarded(c, [&] {
    if (n == 0) return;
    if (!recs) throw StatusError{KSLAM_ERR_ARG, "null recs"};
    hipStream_t s = c->stream;
    DevBuf a, b;
    a.ensure(n * sizeof(uint4));
    b.ensure(n * sizeof(uint4));
    HIPCHK(hipMemcpyAsync(a.p, recs, n * sizeof(uint4), hipMemcpyHostToDevice, s));
    std::vector<SortPass> passes;
    full_key_passes(passes);
    void *sorted = radix_sort(a.p, b.p, n, 4, passes.data(), (int)passes.size(), c->sortws, s, nullptr, nullptr,
                              nullptr);
    HIPCHK(hipMemcpyAsync(recs, sorted, n * sizeof(uint4), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    a.release(); b.release();
  });
}

kslam_status kslam_selftest_sort(kslam_ctx *c, uint64_t n, uint32_t iters, float *ms_per_sort,
                                 float *ms_per_scatter_launch, uint64_t *n_inversions) {
  return guarded(c, [&] {
    if (n == 0 || n >= (1ull << 32) || iters == 0) throw StatusError{KSLAM_ERR_ARG, "bad n / iters"};
    hipStream_t s = c->stream;
    c->recs_a.ensure((n + 1) * sizeof(uint4));
    c->recs_b.ensure((n + 1) * sizeof(uint4));
    c->cells.ensure(sizeof(uint64_t));
    std::vector<SortPass> passes;
    kmer_passes(passes);
    float tot = 0, tot_sc = 0;
    uint32_t launches = 0;
    const void *sorted = nullptr;
    for (uint32_t it = 0; it < iters; it++) {
      hipLaunchKernelGGL(k_fill_random, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c->recs_a.as<uint4>(),
                         (uint32_t)n, 0x1234567ull + it);
      HIPCHK(hipEventRecord(c->ev[0], s));
      c->sortws.ev_sc0 = c->evs0; c->sortws.ev_sc1 = c->evs1;
      sorted = radix_sort(c->recs_a.p, c->recs_b.p, n, 4, passes.data(), (int)passes.size(), c->sortws, s, c->ev[2],
                          c->ev[3], &launches);
      c->sortws.ev_sc0 = nullptr; c->sortws.ev_sc1 = nullptr;
      HIPCHK(hipEventRecord(c->ev[1], s));
      HIPCHK(stream_wait(s));
      tot += ev_ms(c->ev[0], c->ev[1]);
      for (size_t q = 0; q < passes.size(); q++) tot_sc += ev_ms(c->evs0[q], c->evs1[q]);
    }
    HIPCHK(hipMemsetAsync(c->cells.p, 0, sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_count_inversions, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint4 *)sorted,
                       (uint32_t)n, c->cells.as<unsigned long long>());
    uint64_t inv = 0;
    read_back(&inv, c->cells.p, sizeof inv, s);
    if (ms_per_sort) *ms_per_sort = tot / iters;
    if (ms_per_scatter_launch) *ms_per_scatter_launch = launches ? tot_sc / launches : 0.f;
    if (n_inversions) *n_inversions = inv;
  });
}

kslam_status kslam_find_overlaps(kslam_ctx *c, kslam_overlap_temp **out, uint64_t *n_out, uint64_t *n_raw) {
  if (!out || !n_out) return KSLAM_ERR_ARG;
  *out = nullptr; *n_out = 0;
  return guarded(c, [&] {
    uint64_t raw = 0;
    align_resident(c, true, &raw);
    if (n_raw) *n_raw = raw;
    const uint64_t m = c->n_res;
    kslam_overlap_temp *h = (kslam_overlap_temp *)malloc((m + 1) * sizeof(kslam_overlap_temp));
    if (!h) throw StatusError{KSLAM_ERR_OOM, "host allocation failed"};
    if (m) {
      c->res_tmp.ensure(m * sizeof(kslam_overlap_temp));
      hipLaunchKernelGGL(k_to_temp, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream,
                         c->res_ov.as<kslam_overlap>(), m, c->res_tmp.as<kslam_overlap_temp>());
      HIPCHK(hipMemcpyAsync(h, c->res_tmp.p, m * sizeof(kslam_overlap_temp), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(stream_wait(c->stream));
    }
    *out = h;
    *n_out = m;
  });
}

// ---- test hooks for the shared device primitives (tests/test_gpu_sort_scan.py): radix_sort.hip with any pass list and any
// of its switches, scan.hip's two scans at any alignment, partition_bins; and bgzf.hip's code builder (tests/test_gpu_bgzf_dynamic.py).  Buffers of their own: nothing of the context's
// but sortws is touched, and its switches are put back.
kslam_status kslam_debug_radix_sort(kslam_ctx *c, uint32_t *recs, uint64_t n, uint32_t rec_words, const kslam_sort_pass *passes,
                                    uint32_t n_passes, uint32_t flags, const uint8_t *first_digits) {
  return guarded(c, [&] {
    if (rec_words != 2 && rec_words != 4) throw StatusError{KSLAM_ERR_ARG, "records of 2 or 4 words"};
    if (n_passes > 12) throw StatusError{KSLAM_ERR_ARG, "more than 12 passes"};
    if (n >= (1ull << 32)) throw StatusError{KSLAM_ERR_ARG, "2^32 records or more"};
    if ((n && !recs) || (n_passes && !passes)) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    if (flags & ~15u) throw StatusError{KSLAM_ERR_ARG, "unknown flag"};
    if ((flags & KSLAM_SORT_FIRST_DIGITS) && !first_digits) throw StatusError{KSLAM_ERR_ARG, "first-digits flag without the digit bytes"};
    SortPass pl[12];
    for (uint32_t i = 0; i < n_passes; i++) {
      const kslam_sort_pass &p = passes[i];
      if (p.word > 2) throw StatusError{KSLAM_ERR_ARG, "pass word above 2"};
      if (p.hi_bits > 7) throw StatusError{KSLAM_ERR_ARG, "hi_bits above 7"};
      if ((uint64_t)p.hi_shift + p.hi_bits > 32) throw StatusError{KSLAM_ERR_ARG, "high field beyond the word"};
      const bool key64 = rec_words == 2 && p.word == 2;     // the digit of the whole 64-bit key (radix_sort.hip: digit_of)
      if (key64 && p.hi_bits) throw StatusError{KSLAM_ERR_ARG, "two-field digit of the 64-bit key"};
      if ((uint64_t)p.shift + (8u - p.hi_bits) > (key64 ? 64u : 32u)) throw StatusError{KSLAM_ERR_ARG, "digit beyond the word"};
      pl[i] = SortPass{p.word, p.shift, p.invert};
      pl[i].hi_shift = p.hi_shift;
      pl[i].hi_bits = p.hi_bits;
    }
    if (n == 0) return;
    hipStream_t s = c->stream;
    SortWorkspace &ws = c->sortws;
    DevBuf a, b;
    a.ensure(n * rec_words * sizeof(uint32_t));
    b.ensure(n * rec_words * sizeof(uint32_t));
    HIPCHK(hipMemcpyAsync(a.p, recs, n * rec_words * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    const bool keep_bytes = ws.use_digit_bytes, keep_first = ws.first_digits_ready, keep_runs = ws.meta_digits_in_runs;
    struct Restore {
      SortWorkspace &w; bool bytes, first, runs;
      ~Restore() { w.use_digit_bytes = bytes; w.first_digits_ready = first; w.meta_digits_in_runs = runs; }
    } restore{ws, keep_bytes, keep_first, keep_runs};
    ws.use_digit_bytes = (flags & KSLAM_SORT_DIGIT_BYTES) != 0;
    ws.meta_digits_in_runs = (flags & KSLAM_SORT_META_IN_RUNS) != 0;
    // (the sort reads digit bytes only with the switch on and a second pass to write them for)
    ws.first_digits_ready = (flags & KSLAM_SORT_FIRST_DIGITS) && ws.use_digit_bytes && n_passes > 1;
    if (ws.first_digits_ready) {
      ws.digits.ensure(n + 64);
      HIPCHK(hipMemcpyAsync(ws.digits.p, first_digits, n, hipMemcpyHostToDevice, s));
    }
    void *sorted = radix_sort(a.p, b.p, n, (int)rec_words, pl, (int)n_passes, ws, s, nullptr, nullptr, nullptr,
                              (flags & KSLAM_SORT_SETUP) != 0);
    HIPCHK(hipMemcpyAsync(recs, sorted, n * rec_words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
  });
}

kslam_status kslam_debug_bgzf_code_lengths(kslam_ctx *c, const uint32_t *counts, uint32_t n, uint32_t limit, uint8_t *lengths) {
  return guarded(c, [&] {
    if (!counts || !lengths) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    if (n < 2 || n > 286) throw StatusError{KSLAM_ERR_ARG, "2 to 286 symbols"};
    if (limit < 1 || limit > 15 || (1u << limit) < n) throw StatusError{KSLAM_ERR_ARG, "a limit of 1 to 15 bits that the symbols fit"};
    uint64_t sum = 0;
    for (uint32_t s = 0; s < n; s++) sum += counts[s];
    if (sum >= (1ull << 32)) throw StatusError{KSLAM_ERR_ARG, "counts that sum to 2^32 or more"};
    hipStream_t s = c->stream;
    DevBuf d_counts, d_lengths;
    d_counts.ensure(n * sizeof(uint32_t));
    d_lengths.ensure(n);
    HIPCHK(hipMemcpyAsync(d_counts.p, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    bgzf_code_lengths_device(d_counts.as<uint32_t>(), n, limit, d_lengths.as<uint8_t>(), s);
    HIPCHK(hipMemcpyAsync(lengths, d_lengths.p, n, hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
  });
}

kslam_status kslam_debug_scan(kslam_ctx *c, const uint32_t *in, uint64_t n, void *out, int wide, uint32_t in_skew, uint32_t out_skew,
                              uint64_t *total) {
  return guarded(c, [&] {
    if (wide != 0 && wide != 1) throw StatusError{KSLAM_ERR_ARG, "wide is 0 or 1"};
    if (in_skew > 15 || out_skew > 15) throw StatusError{KSLAM_ERR_ARG, "skew above 15 elements"};
    if (n >= (1ull << 32)) throw StatusError{KSLAM_ERR_ARG, "2^32 elements or more"};
    if (n && (!in || !out)) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    hipStream_t s = c->stream;
    const size_t out_size = wide ? sizeof(uint64_t) : sizeof(uint32_t);
    DevBuf d_in, d_out, d_tmp, d_tot;
    d_in.ensure((n + in_skew + 4) * sizeof(uint32_t));
    d_out.ensure((n + out_skew + 4) * out_size);
    d_tmp.ensure(scan_tmp_bytes(n));
    d_tot.ensure(sizeof(uint64_t));
    const uint32_t *din = d_in.as<uint32_t>() + in_skew;
    if (n) HIPCHK(hipMemcpyAsync((void *)din, in, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_tot.p, 0xFF, sizeof(uint64_t), s));
    uint64_t *dtot = total ? d_tot.as<uint64_t>() : nullptr;
    void *dout = d_out.as<uint8_t>() + (size_t)out_skew * out_size;
    if (wide) exclusive_scan_u32_to_u64(din, (uint64_t *)dout, n, dtot, d_tmp.p, s);
    else exclusive_scan_u32(din, (uint32_t *)dout, n, dtot, d_tmp.p, s);
    if (n) HIPCHK(hipMemcpyAsync(out, dout, n * out_size, hipMemcpyDeviceToHost, s));
    if (total) HIPCHK(hipMemcpyAsync(total, d_tot.p, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
  });
}

kslam_status kslam_debug_partition_bins(kslam_ctx *c, const uint8_t *bins, uint64_t n, uint32_t *lists, uint32_t *counts) {
  return guarded(c, [&] {
    if (!counts || (n && (!bins || !lists))) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    if (n >= (1ull << 32)) throw StatusError{KSLAM_ERR_ARG, "2^32 elements or more"};
    for (int k = 0; k < 8; k++) counts[k] = 0;
    if (n == 0) return;
    hipStream_t s = c->stream;
    DevBuf d_bins, d_lists, d_counts, pos;
    d_bins.ensure(n);
    d_lists.ensure(8 * n * sizeof(uint32_t));     // any list may take every element
    d_counts.ensure(8 * sizeof(uint32_t));
    HIPCHK(hipMemcpyAsync(d_bins.p, bins, n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_counts.p, 0, 8 * sizeof(uint32_t), s));
    BinLists B;
    for (int k = 0; k < 8; k++) B.list[k] = d_lists.as<uint32_t>() + (size_t)k * n;
    B.count = d_counts.as<uint32_t>();
    partition_bins(d_bins.as<uint8_t>(), n, B, pos, s);
    HIPCHK(hipMemcpyAsync(counts, d_counts.p, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
    uint64_t at = 0;
    for (int k = 0; k < 8; k++) at += counts[k];
    if (at > n) throw StatusError{KSLAM_ERR_INTERNAL, "partition_bins: the lists hold more than n elements"};
    at = 0;
    for (int k = 0; k < 8; k++) {
      if (counts[k]) HIPCHK(hipMemcpyAsync(lists + at, B.list[k], (size_t)counts[k] * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      at += counts[k];
    }
    HIPCHK(stream_wait(s));
  });
}

// ---- test hooks for join.hip (tests/test_gpu_join_seams.py): the k-mer join on either route over records the caller supplies,
// and the two routes from sorted overlap keys to the unique rows.  Buffers of their own: nothing of the context's index, reads
// or results is touched.  Everything a kernel would index with is checked on the host first.
static OverlapKeyLayout debug_layout(const kslam_overlap_layout *layout) {
  if (!layout) throw StatusError{KSLAM_ERR_ARG, "null layout"};
  if (layout->bits_read > 31 || layout->bits_entry > 30 || layout->bits_rel < 1 || layout->bits_rel > 31)
    throw StatusError{KSLAM_ERR_ARG, "layout: bits_read <= 31, bits_entry <= 30, bits_rel in 1..31"};
  if (layout->bits_read + layout->bits_entry + layout->bits_rel + 1 > 63) throw StatusError{KSLAM_ERR_ARG, "an overlap key wider than 63 bits"};
  if (layout->rel_bias >= (1u << layout->bits_rel)) throw StatusError{KSLAM_ERR_ARG, "rel_bias beyond bits_rel"};
  OverlapKeyLayout lay;
  lay.bits_read = layout->bits_read; lay.bits_entry = layout->bits_entry; lay.bits_rel = layout->bits_rel;
  lay.rel_bias = layout->rel_bias;
  return lay;
}

kslam_status kslam_debug_join(kslam_ctx *c, const kslam_kmer *genome, uint64_t n_g, uint32_t bucket_bits, const kslam_kmer *reads,
                              uint64_t n_r, uint32_t sorted_top_bits, const uint32_t *read_len, uint64_t n_reads,
                              const kslam_overlap_layout *layout, int route, uint64_t cap, uint64_t *cursor, uint64_t *out,
                              uint32_t *bucket_table) {
  return guarded(c, [&] {
    const OverlapKeyLayout lay = debug_layout(layout);
    if (!cursor || !out || (n_g && !genome) || (n_r && !reads) || (n_reads && !read_len)) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    if (bucket_bits < 8 || bucket_bits > 16) throw StatusError{KSLAM_ERR_ARG, "bucket_bits in 8..16"};
    if (route != 0 && route != 1) throw StatusError{KSLAM_ERR_ARG, "route is 0 (probe) or 1 (merge)"};
    if (n_g >= (1ull << 24) || n_r >= (1ull << 24) || n_reads >= (1ull << 24) || cap >= (1ull << 28))
      throw StatusError{KSLAM_ERR_ARG, "2^24 records or reads or more, or a cap of 2^28 or more"};
    if (route == 1 && (sorted_top_bits == 0 || sorted_top_bits > 64)) throw StatusError{KSLAM_ERR_ARG, "the merge needs sorted_top_bits in 1..64"};
    // the genome side: ascending keys, ids the entry field holds
    int64_t goff_min = INT64_MAX, goff_max = -1;
    for (uint64_t i = 0; i < n_g; i++) {
      if (i && genome[i].kmer < genome[i - 1].kmer) throw StatusError{KSLAM_ERR_ARG, "genome keys are not ascending"};
      if ((uint64_t)(genome[i].meta & 0x3FFFFFFFu) >> lay.bits_entry) throw StatusError{KSLAM_ERR_ARG, "a genome id beyond bits_entry"};
      goff_min = std::min<int64_t>(goff_min, genome[i].offset);
      goff_max = std::max<int64_t>(goff_max, genome[i].offset);
    }
    // the read side: ids inside the length array and the read field, the k-mer inside its read
    const uint32_t gb = std::min(sorted_top_bits, bucket_bits);
    int64_t off_min = INT64_MAX, off_max = -1;
    for (uint64_t i = 0; i < n_r; i++) {
      const uint32_t id = reads[i].meta & 0x3FFFFFFFu;
      if (id >= n_reads) throw StatusError{KSLAM_ERR_ARG, "a read id outside the read-length array"};
      if ((uint64_t)id >> lay.bits_read) throw StatusError{KSLAM_ERR_ARG, "a read id beyond bits_read"};
      if ((uint64_t)reads[i].offset + KSLAM_K > read_len[id]) throw StatusError{KSLAM_ERR_ARG, "a read k-mer that ends beyond its read"};
      const int64_t fwd = reads[i].offset, rev = (int64_t)read_len[id] - reads[i].offset - KSLAM_K;   // Overlap.h:185-189, either strand of the genome record
      off_min = std::min(off_min, std::min(fwd, rev));
      off_max = std::max(off_max, std::max(fwd, rev));
      if (route == 1 && i && (reads[i].kmer >> (64 - gb)) < (reads[i - 1].kmer >> (64 - gb)))
        throw StatusError{KSLAM_ERR_ARG, "the merge needs read records ordered by their top min(sorted_top_bits, bucket_bits) key bits"};
    }
    if (n_g && n_r && (goff_min - off_max + (int64_t)lay.rel_bias < 0 || goff_max - off_min + (int64_t)lay.rel_bias >= (int64_t)(1ull << lay.bits_rel)))
      throw StatusError{KSLAM_ERR_ARG, "offsets and read lengths whose rel + rel_bias the rel field cannot hold"};
    hipStream_t s = c->stream;
    const uint64_t nb = 1ull << bucket_bits;
    // the columns and the table, with the allocation sizes of build_index; the key column's padding word holds all ones, the
    // worst an allocation may hold there
    DevBuf d_g, d_key, d_mo, d_bucket, d_r, d_len, d_out, d_cur;
    d_g.ensure((n_g + 1) * sizeof(uint4));
    d_key.ensure((n_g + 1) * sizeof(uint64_t));
    d_mo.ensure((n_g + 1) * sizeof(uint2));
    d_bucket.ensure((nb + 2) * sizeof(uint32_t));
    d_r.ensure((n_r + 1) * sizeof(uint4));
    d_len.ensure((n_reads + 1) * sizeof(uint32_t));
    d_out.ensure((cap + 64) * sizeof(uint64_t));
    d_cur.ensure(8 * sizeof(uint64_t));
    HIPCHK(hipMemsetAsync(d_key.p, 0xFF, (n_g + 1) * sizeof(uint64_t), s));
    HIPCHK(hipMemsetAsync(d_out.p, KSLAM_DEBUG_SENTINEL_BYTE, (cap + 64) * sizeof(uint64_t), s));
    if (n_g) HIPCHK(hipMemcpyAsync(d_g.p, genome, n_g * sizeof(uint4), hipMemcpyHostToDevice, s));
    if (n_r) HIPCHK(hipMemcpyAsync(d_r.p, reads, n_r * sizeof(uint4), hipMemcpyHostToDevice, s));
    if (n_reads) HIPCHK(hipMemcpyAsync(d_len.p, read_len, n_reads * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (n_g) hipLaunchKernelGGL(k_split_soa, dim3((unsigned)((n_g + 255) / 256)), dim3(256), 0, s, d_g.as<uint4>(), (uint32_t)n_g,
                                d_key.as<uint64_t>(), d_mo.as<uint2>());
    build_bucket_table(d_key.as<uint64_t>(), (uint32_t)n_g, bucket_bits, d_bucket.as<uint32_t>(), s);
    GenomeIndexDev g;
    g.key = d_key.as<uint64_t>(); g.mo = d_mo.as<uint2>(); g.bucket = d_bucket.as<uint32_t>();
    g.bucket_bits = bucket_bits; g.n = (uint32_t)n_g;
    if (route == 1)
      join_fill_merge(d_r.as<uint4>(), (uint32_t)n_r, g, sorted_top_bits, d_len.as<uint32_t>(), d_cur.as<uint64_t>(), cap, lay,
                      d_out.as<uint64_t>(), s);
    else
      join_fill_single_pass(d_r.as<uint4>(), (uint32_t)n_r, g, d_len.as<uint32_t>(), d_cur.as<uint64_t>(), cap, lay, d_out.as<uint64_t>(), s);
    HIPCHK(hipMemcpyAsync(cursor, d_cur.p, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out, d_out.p, (cap + 64) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (bucket_table) HIPCHK(hipMemcpyAsync(bucket_table, d_bucket.p, (nb + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
  });
}

kslam_status kslam_debug_overlap_unique(kslam_ctx *c, const uint64_t *keys, uint64_t n, const kslam_overlap_layout *layout,
                                        uint32_t read_id_base, int route, uint64_t *keys_after, uint64_t *ordered, uint32_t *flags,
                                        uint32_t *big, uint64_t *n_rows, kslam_overlap *rows) {
  return guarded(c, [&] {
    const OverlapKeyLayout lay = debug_layout(layout);
    if (!big || !n_rows || (n && (!keys || !ordered || !flags || !rows))) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    if (route != 0 && route != 1) throw StatusError{KSLAM_ERR_ARG, "route is 0 (sorted keys) or 1 (keys grouped by their high bits)"};
    if (n >= (1ull << 28)) throw StatusError{KSLAM_ERR_ARG, "2^28 keys or more"};
    const uint32_t width = lay.bits_read + lay.bits_entry + lay.bits_rel + 1, low = lay.bits_rel + 1;
    for (uint64_t i = 0; i < n; i++) {
      if (keys[i] >> width) throw StatusError{KSLAM_ERR_ARG, "a key wider than the layout"};
      if ((keys[i] >> (lay.bits_entry + low)) + read_id_base > 0xFFFFFFFFull) throw StatusError{KSLAM_ERR_ARG, "read + read_id_base beyond 32 bits"};
      if (i == 0) continue;
      if (route == 0 && keys[i] < keys[i - 1]) throw StatusError{KSLAM_ERR_ARG, "route 0 needs fully sorted keys"};
      if (route == 1 && (keys[i] >> low) < (keys[i - 1] >> low)) throw StatusError{KSLAM_ERR_ARG, "route 1 needs keys ordered by the bits above rel and revComp"};
    }
    *big = 0;
    *n_rows = 0;
    if (n == 0) return;
    hipStream_t s = c->stream;
    DevBuf d_in, d_ord, d_flags, d_pos, d_tmp, d_tot, d_rows;
    d_in.ensure((n + 1) * sizeof(uint64_t));
    d_ord.ensure((n + 1) * sizeof(uint64_t));
    d_flags.ensure((n + 1) * sizeof(uint32_t));
    d_pos.ensure((n + 1) * sizeof(uint32_t));
    d_tmp.ensure(scan_tmp_bytes(n));
    d_tot.ensure(8 * sizeof(uint64_t));
    HIPCHK(hipMemcpyAsync(d_in.p, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_ord.p, KSLAM_DEBUG_SENTINEL_BYTE, (n + 1) * sizeof(uint64_t), s));
    HIPCHK(hipMemsetAsync(d_flags.p, KSLAM_DEBUG_SENTINEL_BYTE, (n + 1) * sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(d_tot.p, 0, 8 * sizeof(uint64_t), s));
    uint64_t *d_total = d_tot.as<uint64_t>();
    uint32_t *d_big = reinterpret_cast<uint32_t *>(d_total + 3);
    const uint64_t *d_keys = d_in.as<uint64_t>();
    uint64_t back[4] = {0, 0, 0, 0};
    if (route == 1) {
      group_order(d_in.as<uint64_t>(), n, lay, d_ord.as<uint64_t>(), d_flags.as<uint32_t>(), d_big, s);
      d_keys = d_ord.as<uint64_t>();
      read_back(back, d_total, sizeof back, s);
    } else {
      dedupe_flags(d_keys, n, lay, d_flags.as<uint32_t>(), s);
    }
    if (back[3] == 0) {
      exclusive_scan_u32(d_flags.as<uint32_t>(), d_pos.as<uint32_t>(), n, d_total, d_tmp.p, s);
      read_back(back, d_total, sizeof back, s);
      const uint64_t m = back[0];
      if (m > n) throw StatusError{KSLAM_ERR_INTERNAL, "more survivors than keys"};
      d_rows.ensure((m + 1) * sizeof(kslam_overlap));
      dedupe_compact(d_keys, d_flags.as<uint32_t>(), d_pos.as<uint32_t>(), n, lay, read_id_base, d_rows.as<kslam_overlap>(), s);
      if (m) HIPCHK(hipMemcpyAsync(rows, d_rows.p, m * sizeof(kslam_overlap), hipMemcpyDeviceToHost, s));
      *n_rows = m;
    }
    *big = (uint32_t)back[3];
    if (keys_after) HIPCHK(hipMemcpyAsync(keys_after, d_in.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ordered, route == 1 ? d_ord.p : d_in.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(flags, d_flags.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(stream_wait(s));
  });
}

// ---- test hook for build_index (tests/test_gpu_index_build.py): the built index copied to the host, table by table.  Read-only:
// nothing of the context, the index or the sort workspace changes.  Sizes and capacities are settled before the first copy.
kslam_status kslam_debug_index_export(kslam_ctx *c, kslam_index_export *x) {
  if (!c || !x) return KSLAM_ERR_ARG;
  return guarded(c, [&] {
    const GenomeIndex &ix = c->need_index();
    HIPCHK(stream_wait(c->stream));
    const uint64_t n = ix.n_entries, m = ix.n_gk, total = ix.h_goff[n];
    const uint64_t nb = (1ull << ix.bucket_bits) + 1, fbytes = ix.filter_bits ? filter_bytes(ix.filter_bits) : 0;
    x->n_entries = n; x->n_genome_kmers = m; x->n_bases = total; x->n_filter_bytes = fbytes;
    x->bucket_bits = ix.bucket_bits; x->filter_bits = ix.filter_bits;
    if (!x->offsets && !x->codes && !x->keys && !x->meta && !x->bucket && !x->filter) return;   // the sizes alone
    auto room = [](const void *p, uint64_t cap, uint64_t need) { return need == 0 || (p && cap >= need); };
    if (!room(x->offsets, x->cap_offsets, n + 1) || !room(x->codes, x->cap_codes, total) || !room(x->keys, x->cap_records, m) ||
        !room(x->meta, x->cap_records, m) || !room(x->bucket, x->cap_bucket, nb) || !room(x->filter, x->cap_filter, fbytes))
      throw StatusError{KSLAM_ERR_ARG, "index export: a buffer is missing or smaller than its table"};
    hipStream_t s = c->stream;
    auto copy = [&](void *dst, const DevBuf &src, uint64_t bytes) {
      if (bytes > src.cap) throw StatusError{KSLAM_ERR_INTERNAL, "index export: a table larger than its allocation"};
      if (bytes) HIPCHK(hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, s));
    };
    copy(x->offsets, ix.g_off, (n + 1) * sizeof(uint64_t));
    copy(x->codes, ix.g_codes, total);
    copy(x->keys, ix.gk_key, m * sizeof(uint64_t));
    copy(x->meta, ix.gk_meta, m * sizeof(uint2));
    copy(x->bucket, ix.g_bucket, nb * sizeof(uint32_t));
    copy(x->filter, ix.g_filter, fbytes);
    HIPCHK(stream_wait(s));
  });
}

}  // extern "C"
