/*
 * kslam_coverage.h -- a per-entry coverage table (breadth against depth, what KrakenUniq added to Kraken and what
 * `samtools coverage` gives for a sorted SAM file), accumulated on the GPU from what a lane holds when it has finished a batch
 * (csrc/coverage.hip).  Same library as kslam.h.
 *
 * Off by default; with the switch off every byte of every output is what it was.  With it on:
 *   contributing set   a batch contributes its FINAL read pairs: the groups read_pairs[i] with their LIVE alignment pairs
 *                      pairs[first .. first + count).  After pseudo-assembly on the device the records keep their places and the
 *                      counts shrink: the records between first + count and the next group's first are dead and contribute
 *                      nothing.  It is the set that gets a _PerRead line; with --just-align the aligned set.  The groups'
 *                      `first` ascend and the slices do not overlap (first + count <= the next group's first).
 *   intervals          every live alignment pair contributes, for each mate that exists (r1, r2 not KSLAM_NO_OVERLAP), the
 *                      CLOSED interval [ref_begin, ref_end] of that overlap record on the overlap record's `entry`.  Coordinates
 *                      are 0-based within the entry, as the SAM writer reads them.  The interval is the reference span: deleted
 *                      reference bases are inside it, the insert between two mates is not.
 *   skipped mates      a mate whose record has entry >= n_entries, ref_begin < 0, ref_end < ref_begin or ref_end >= the entry's
 *                      length contributes nothing and adds one to n_skipped (the SAM writer's rule, host/tail.cpp).  No kernel
 *                      writes outside an entry's bits whatever the records hold.
 *   rows               one per entry of the index; all four fields accumulate over all batches since the switch was turned on
 *                      or kslam_coverage_reset:
 *                        alignments         live alignment pairs whose own `entry` field (kslam_paired_overlap.entry) is this one
 *                        unique_read_pairs  read pairs with count > 0 whose live alignment pairs ALL carry this entry
 *                        aligned_bases      sum of ref_end - ref_begin + 1 over the contributing mates on this entry
 *                        covered_bases      distinct positions of the entry inside at least one contributing interval
 *                      An alignment pair whose own entry is >= n_entries belongs to no row (and is no skipped mate).
 *   determinism        every accumulator is a bitwise OR or an integer add, so the rows do not depend on the number of lanes,
 *                      on the order of the batches, or on whether a batch was marked by its lane or handed in from the host
 *                      (kslam_coverage_add); they equal kslam_tail_coverage on the same arrays, bit for bit.
 *
 * The state -- one bit per base of the index (every entry starts on a 64-bit word: ceil(len / 64) * 8 bytes per entry), 32
 * bytes of counters per entry and the skip counter -- belongs to the context the switch was set on and is shared by its lanes;
 * it is zeroed at switch-on and by kslam_coverage_reset and freed at switch-off, by kslam_set_index and by kslam_destroy.
 */
#ifndef KSLAM_COVERAGE_H_
#define KSLAM_COVERAGE_H_
#include "kslam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint64_t alignments;
  uint64_t unique_read_pairs;
  uint64_t aligned_bases;
  uint64_t covered_bases;
} kslam_entry_coverage;

/* on != 0: the lanes mark every batch they finish (a batch whose pseudo-assembly the device left to the host --
 * pair_stats.stages_done lacks KSLAM_TAIL_PSEUDO_ASM -- is NOT marked: hand its final arrays to kslam_coverage_add after the
 * host stage).  Needs an index and the device pairing (kslam_set_pairing with stages != 0), else KSLAM_ERR_STATE.  Switching
 * on allocates and zeroes the state (on when already on: nothing happens); off frees it.  Set it between batches.  A context of
 * a kslam_multi gets KSLAM_ERR_UNSUPPORTED, as from kslam_set_reads_out. */
kslam_status kslam_set_coverage(kslam_ctx *ctx, int on);
kslam_status kslam_get_coverage(kslam_ctx *ctx, int *on);

/* zeroes the bitmap, the rows and the skip counter; KSLAM_ERR_STATE with the switch off */
kslam_status kslam_coverage_reset(kslam_ctx *ctx);

/* Host arrays in, uploaded and marked like a lane's batch: for the batches left to the host, and for stage-level tests.  Before
 * anything is launched, KSLAM_ERR_ARG for: a live record's r1 / r2 (not KSLAM_NO_OVERLAP) >= n_overlaps, first + count > n_pairs,
 * groups whose `first` do not ascend or whose slices overlap, 2^32 or more overlap records.  KSLAM_ERR_STATE with the switch
 * off.  May be called from any thread; calls are serialised. */
kslam_status kslam_coverage_add(kslam_ctx *ctx, const kslam_overlap *overlaps, uint64_t n_overlaps, const kslam_read_pair *read_pairs,
                                uint64_t n_read_pairs, const kslam_paired_overlap *pairs, uint64_t n_pairs);

/* The table of every batch collected so far (it waits for the lanes' streams): covered_bases is counted from the bitmap at
 * each call, so the call may be repeated.  *rows: a page-locked, library-owned array of *n_entries rows; hand it back with
 * kslam_free_pinned. */
kslam_status kslam_coverage_take(kslam_ctx *ctx, kslam_entry_coverage **rows, uint64_t *n_entries, uint64_t *n_skipped);

/* test hook, like kslam_debug_radix_sort: the n_words = ceil(len / 64) words of one entry's bits (bit b of word w = position
 * 64 w + b); another n_words, or entry >= n_entries: KSLAM_ERR_ARG */
kslam_status kslam_coverage_bitmap(kslam_ctx *ctx, uint64_t entry, uint64_t *words, uint64_t n_words);

/* device time (ms), by events around the launches: the mark passes of the last batch marked through this context's own stream
 * (kslam_coverage_add; the lanes' times are not gathered) and the count pass of the last kslam_coverage_take */
kslam_status kslam_coverage_kernel_ms(kslam_ctx *ctx, double *mark_ms, double *count_ms);

/* Host twin (no GPU): the table of ONE set of arrays (several batches: concatenate them) from host arrays and the entries'
 * lengths, in one serial pass, written to rows[0 .. n_entries) and *n_skipped.  Argument errors as kslam_coverage_add;
 * message: kslam_tail_last_error(). */
kslam_status kslam_tail_coverage(const uint64_t *entry_lengths, uint64_t n_entries, const kslam_overlap *overlaps, uint64_t n_overlaps,
                                 const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                 uint64_t n_pairs, kslam_entry_coverage *rows, uint64_t *n_skipped);

/* The report: one header line, then one line per entry with alignments > 0, in entry order, tab-separated:
 *   #entry  locus  taxid  length  alignments  unique_read_pairs  aligned_bases  covered_bases  breadth  mean_depth
 * breadth = covered_bases / length as %.6f, mean_depth = aligned_bases / length as %.4f (both 0 for an entry of length 0), every
 * other field an integer; locus and taxid from the index view, as the SAM header takes them.  n_entries must be the view's. */
kslam_status kslam_coverage_write(const kslam_index_view *index, const kslam_entry_coverage *rows, uint64_t n_entries, int fd);

/* kslam_stream_classify (kslam_stream.h) writes the report itself: call this before it with an open descriptor (-1: none).  It
 * holds for the NEXT call alone, which switches coverage on and resets it, feeds the batches left to the host through
 * kslam_coverage_add on the host stage's thread, writes the report after the last batch and switches coverage off. */
kslam_status kslam_stream_set_coverage(kslam_ctx *ctx, int fd);
kslam_status kslam_stream_get_coverage(kslam_ctx *ctx, int *fd);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_COVERAGE_H_ */
