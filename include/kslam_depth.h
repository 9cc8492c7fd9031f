/*
 * kslam_depth.h -- the depth along every entry (what `samtools depth` or `bedtools genomecov -bg` give over the coordinate-sorted
 * SAM file), accumulated on the GPU from what a lane holds when it has finished a batch (csrc/depth.hip), and written as
 * bedGraph.  Same library as kslam.h.
 *
 * Off by default; with the switch off every byte of every output is what it was.  With it on:
 *   contributing set, skipped records, the walk
 *                      exactly as in kslam_variants.h: a batch contributes its FINAL read pairs with their LIVE alignment
 *                      pairs; every overlap record that at least one live pair names contributes ONCE; a contributing record
 *                      contributes nothing and adds one to n_skipped when entry >= n_entries, or cigar_len == 0, or
 *                      ref_begin < 0, or an M or D run ends past the entry, or an M or I run ends past the read.  The check
 *                      covers the whole CIGAR and is made before anything of the record is emitted.  Operations are M = 0,
 *                      I = 1, D = 2, packed len << 4 | op.  Only the reads' LENGTHS are looked at, never their bases.
 *   intervals          every M operation of length above 0 contributes the CLOSED interval of reference positions it spans.
 *                      depth(entry, pos) is the number of contributing records with an M column at pos -- `samtools depth`
 *                      without -J, and the DP of the VCF rows of kslam_variants.h.  It counts exactly up to 2^32 - 1.
 *   rows               the maximal runs of equal depth above 0 inside one entry: entry, start (0-based), end (exclusive), depth;
 *                      ascending by entry, then start.  Two adjacent runs of one entry never carry the same depth (they are one
 *                      row), and a run never continues from one entry into the next, also when the last base of entry e and
 *                      the first base of entry e + 1 carry the same depth.
 *   filter             min_depth (0 is read as 1) drops the rows below it; the rows that remain are not merged.
 *   stats              n_records, n_skipped, n_intervals: what kslam_variant_stats gives on the same arrays.  n_keys: the stored
 *                      interval boundaries after compaction.  n_rows, covered_bases (the sum of end - start) and max_depth are
 *                      taken BEFORE the filter.
 *   determinism        the state is a multiset of integer boundaries with their net change; the rows do not depend on the
 *                      number of lanes, on the order of the batches, on whether a batch came from its lane or through
 *                      kslam_depth_add, or on how often the state was compacted or taken.  They equal kslam_tail_depth on the
 *                      same arrays, field for field.
 *
 * The state belongs to the context the switch was set on and is shared by its lanes.  It is COMPACTING: 8 bytes per pending
 * boundary (two per interval) until the pending ones exceed a threshold (kslam_depth_set_compact_at), then 16 bytes per DISTINCT
 * boundary whose begins and ends do not cancel -- bounded by the covered part of the index, however many batches pass.  It is
 * emptied at switch-on and by kslam_depth_reset and freed at switch-off, by kslam_set_index and by kslam_destroy.  More than
 * 2^32 - 1 keys in one sort or one merge (the radix sort's and the scan's limit) is outside the envelope: the call that would
 * need it returns KSLAM_ERR_UNSUPPORTED and leaves the state as it was.
 */
#ifndef KSLAM_DEPTH_H_
#define KSLAM_DEPTH_H_
#include "kslam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t entry;
  uint32_t start;   /* 0-based within the entry */
  uint32_t end;     /* exclusive */
  uint32_t depth;
} kslam_depth_row;

typedef struct {
  uint64_t n_records;      /* contributing overlap records (the skipped ones among them) */
  uint64_t n_skipped;
  uint64_t n_intervals;
  uint64_t n_keys;         /* stored boundaries after compaction */
  uint64_t n_rows;         /* before the filter */
  uint64_t covered_bases;  /* before the filter */
  uint64_t max_depth;      /* before the filter */
} kslam_depth_stats;

/* on != 0: the lanes add every batch they finish (a batch whose pseudo-assembly the device left to the host is NOT: hand its
 * final arrays to kslam_depth_add after the host stage).  Needs an index, the device pairing (kslam_set_pairing with
 * stages != 0) and a context created with report_cigar != 0, else KSLAM_ERR_STATE.  Switching on empties the state (on when
 * already on: nothing happens); off frees it.  Set it between batches.  A context of a kslam_multi gets KSLAM_ERR_UNSUPPORTED. */
kslam_status kslam_set_depth(kslam_ctx *ctx, int on);
kslam_status kslam_get_depth(kslam_ctx *ctx, int *on);

/* empties the state and zeroes the counters; KSLAM_ERR_STATE with the switch off */
kslam_status kslam_depth_reset(kslam_ctx *ctx);

/* Host arrays in, uploaded and added like a lane's batch.  read_offsets: read i is read_offsets[i + 1] - read_offsets[i] bases
 * long.  Before anything is launched, KSLAM_ERR_ARG for what kslam_variants_add refuses: a live record's r1 / r2 (not
 * KSLAM_NO_OVERLAP) >= n_overlaps, first + count > n_pairs, groups whose `first` do not ascend or whose slices overlap, 2^32 or
 * more overlap records, read offsets that do not ascend, and an overlap record named by a live pair whose CIGAR slice lies
 * outside the pool or whose `read` is >= n_reads.  KSLAM_ERR_STATE with the switch off.  May be called from any thread; calls
 * are serialised. */
kslam_status kslam_depth_add(kslam_ctx *ctx, const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool,
                             uint64_t n_cigar, const uint64_t *read_offsets, uint64_t n_reads, const kslam_read_pair *read_pairs,
                             uint64_t n_read_pairs, const kslam_paired_overlap *pairs, uint64_t n_pairs);

/* The rows of every batch added so far (it waits for the lanes' streams and compacts what is pending) that pass the filter; the
 * call may be repeated -- without an add in between neither the sort nor the compaction is repeated -- and more batches may
 * follow it.  *rows: a page-locked, library-owned array of *n_rows rows; hand it back with kslam_free_pinned. */
kslam_status kslam_depth_take(kslam_ctx *ctx, uint32_t min_depth, kslam_depth_row **rows, uint64_t *n_rows, kslam_depth_stats *stats);

/* device time (ms), by events: of the last batch added through this context's own stream (kslam_depth_add; the lanes' times
 * are not gathered), of the last compaction that ran (0: none since the switch or the last reset), and of the last take without
 * its compaction */
kslam_status kslam_depth_kernel_ms(kslam_ctx *ctx, double *emit_ms, double *compact_ms, double *take_ms);

/* The number of pending keys (two per interval) above which an add compacts the state; 0 restores the default, 2^27.  A tuning
 * knob: it changes no row.  May be set with the switch on or off; it stays until the context is destroyed. */
kslam_status kslam_depth_set_compact_at(kslam_ctx *ctx, uint64_t n_keys);

/* Host twin (no GPU): the rows of ONE set of arrays (several batches: concatenate them), serially.  *rows: malloc'ed, hand it
 * back with kslam_free.  Argument errors as kslam_depth_add; message: kslam_tail_last_error(). */
kslam_status kslam_tail_depth(const uint64_t *entry_offsets, uint64_t n_entries, const kslam_overlap *overlaps, uint64_t n_overlaps,
                              const uint32_t *cigar_pool, uint64_t n_cigar, const uint64_t *read_offsets, uint64_t n_reads,
                              const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                              uint64_t n_pairs, uint32_t min_depth, kslam_depth_row **rows, uint64_t *n_rows, kslam_depth_stats *stats);

/* The file: bedGraph as `bedtools genomecov -bg` writes it, no track line:
 *   locus \t start \t end \t depth \n
 * 0-based, half-open; locus as the SAM header and the VCF writer spell it.  KSLAM_ERR_ARG, before anything is written, for a
 * row whose entry is not in the view or has an empty locus. */
kslam_status kslam_depth_write(const kslam_index_view *index, const kslam_depth_row *rows, uint64_t n_rows, int fd);

/* kslam_stream_classify (kslam_stream.h) writes the file itself: call this before it with an open descriptor (-1: none).  It
 * holds for the NEXT call alone, which switches the depth on and resets it, feeds the batches left to the host through
 * kslam_depth_add on the host stage's thread, writes the file after the last batch and switches it off. */
kslam_status kslam_stream_set_depth(kslam_ctx *ctx, int fd, uint32_t min_depth);
kslam_status kslam_stream_get_depth(kslam_ctx *ctx, int *fd, uint32_t *min_depth);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_DEPTH_H_ */
