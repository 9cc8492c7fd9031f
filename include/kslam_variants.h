/*
 * kslam_variants.h -- a table of single-nucleotide differences between the reads and the entries they align to (what a pileup
 * over the coordinate-sorted SAM file gives), piled up on the GPU from what a lane holds when it has finished a batch
 * (csrc/variants.hip), and written as VCF 4.2 without sample columns.  Same library as kslam.h.
 *
 * Off by default; with the switch off every byte of every output is what it was.  With it on:
 *   contributing set   a batch contributes its FINAL read pairs: the groups read_pairs[i] with their LIVE alignment pairs
 *                      pairs[first .. first + count).  The records between first + count and the next group's first are dead
 *                      and contribute nothing, as in kslam_coverage.h.  Every overlap record that at least one live alignment
 *                      pair names as r1 or r2 (not KSLAM_NO_OVERLAP) contributes ONCE, however many live pairs name it.  This
 *                      differs from the coverage table, which counts an overlap record once per live pair that names it.
 *   skipped records    a contributing overlap record contributes nothing and adds one to n_skipped when
 *                        entry >= n_entries, or cigar_len == 0, or ref_begin < 0, or
 *                        its CIGAR runs past the read or past the entry: an M or D run whose end exceeds the entry's length,
 *                        an M or I run whose end exceeds the read's length.
 *                      The check covers the whole CIGAR and is made before anything of that record is emitted.  No kernel reads
 *                      or writes outside an entry or a read, whatever the records hold.
 *   the walk           starts at reference position ref_begin and at query position max(query_begin, 0).  The query is the read,
 *                      or its reverse complement when revcomp != 0; in the reverse complement only upper-case A/C/G/T are
 *                      complemented, every other byte stays as it is.  Operations are M = 0, I = 1, D = 2, packed
 *                      len << 4 | op; M advances both positions, I the query, D the reference.
 *   intervals          every M operation of length above 0 contributes the CLOSED interval of reference positions it spans on
 *                      the record's entry.  Deleted reference bases and inserted read bases are in no interval, so
 *                      depth(entry, pos) is the number of contributing records with an M column at pos -- what `samtools depth`
 *                      counts without -J.
 *   events             an M column is an event when the entry's byte is one of ACGT, the query byte is one of ACGT and they
 *                      differ.  Upper case only: N, lower case and anything else is no event on either side (the column still
 *                      counts for depth).  An event carries (entry, pos, alt = the query byte, strand = revcomp != 0).
 *   rows               one per distinct (entry, pos, alt) with at least one event, ascending by entry, then pos, then alt in the
 *                      order A < C < G < T: entry, pos (0-based), ref (the entry's byte), alt, alt_fwd and alt_rev (the events of
 *                      each strand), depth.  depth counts both mates of a pair when both cover the site.
 *   filter             kslam_variants_take returns the rows with alt_fwd + alt_rev >= min_alt and depth >= min_depth: integer
 *                      comparisons, no floating point.
 *   determinism        the state is a multiset of integer keys, sorted when the rows are asked for, so the rows do not depend on
 *                      the number of lanes, on the order of the batches, on whether a batch came from its lane or through
 *                      kslam_variants_add, or on how often kslam_variants_take was called before; they equal
 *                      kslam_tail_variants on the same arrays, field for field.
 *
 * The state -- 8 bytes per event, 16 per interval, growing with the batches and not with the database -- belongs to the context
 * the switch was set on and is shared by its lanes; it is emptied at switch-on and by kslam_variants_reset and freed at
 * switch-off, by kslam_set_index and by kslam_destroy.  More than 2^32 - 1 stored events or intervals is outside the envelope
 * (the radix sort's limit): the call that would cross it returns KSLAM_ERR_UNSUPPORTED and leaves the state as it was.  A run
 * longer than that still gets its depth along every entry from kslam_depth.h, whose state is compacted and does not grow.
 */
#ifndef KSLAM_VARIANTS_H_
#define KSLAM_VARIANTS_H_
#include "kslam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t entry;
  uint32_t pos;      /* 0-based within the entry */
  uint8_t ref;       /* the entry's byte at pos */
  uint8_t alt;       /* 'A', 'C', 'G' or 'T' */
  uint8_t pad[2];
  uint32_t alt_fwd;  /* events with revcomp == 0 */
  uint32_t alt_rev;  /* events with revcomp != 0 */
  uint32_t depth;    /* contributing records with an M column at pos */
} kslam_variant_row;

typedef struct {
  uint64_t n_records;   /* contributing overlap records (the skipped ones among them) */
  uint64_t n_skipped;
  uint64_t n_intervals;
  uint64_t n_events;
  uint64_t n_sites;     /* rows before the filter */
} kslam_variant_stats;

/* on != 0: the lanes pile up every batch they finish (a batch whose pseudo-assembly the device left to the host --
 * pair_stats.stages_done lacks KSLAM_TAIL_PSEUDO_ASM -- is NOT: hand its final arrays to kslam_variants_add after the host
 * stage).  Needs an index, the device pairing (kslam_set_pairing with stages != 0) and a context created with
 * report_cigar != 0, else KSLAM_ERR_STATE.  Switching on allocates the state (on when already on: nothing happens); off frees
 * it.  Set it between batches.  A context of a kslam_multi gets KSLAM_ERR_UNSUPPORTED, as from kslam_set_coverage. */
kslam_status kslam_set_variants(kslam_ctx *ctx, int on);
kslam_status kslam_get_variants(kslam_ctx *ctx, int *on);

/* empties the state and zeroes the counters; KSLAM_ERR_STATE with the switch off */
kslam_status kslam_variants_reset(kslam_ctx *ctx);

/* Host arrays in, uploaded and piled up like a lane's batch: for the batches left to the host, and for stage-level tests.
 * read_bases / read_offsets: read i is read_bases[read_offsets[i] .. read_offsets[i + 1]).  Before anything is launched,
 * KSLAM_ERR_ARG for: a live record's r1 / r2 (not KSLAM_NO_OVERLAP) >= n_overlaps, first + count > n_pairs, groups whose `first`
 * do not ascend or whose slices overlap, 2^32 or more overlap records (kslam_coverage_add's refusals), and for an overlap record
 * named by a live pair whose CIGAR slice lies outside the pool or whose `read` is >= n_reads.  KSLAM_ERR_STATE with the switch
 * off.  May be called from any thread; calls are serialised. */
kslam_status kslam_variants_add(kslam_ctx *ctx, const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool,
                                uint64_t n_cigar, const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads,
                                const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                uint64_t n_pairs);

/* The rows of every batch collected so far (it waits for the lanes' streams) that pass the filter; the call may be repeated,
 * and more batches may follow it.  *rows: a page-locked, library-owned array of *n_rows rows; hand it back with
 * kslam_free_pinned. */
kslam_status kslam_variants_take(kslam_ctx *ctx, uint32_t min_alt, uint32_t min_depth, kslam_variant_row **rows, uint64_t *n_rows,
                                 kslam_variant_stats *stats);

/* device time (ms), by events: from the first to the last pass of the last batch piled up through this context's own stream
 * (kslam_variants_add; the lanes' times are not gathered), and of the last kslam_variants_take */
kslam_status kslam_variants_kernel_ms(kslam_ctx *ctx, double *emit_ms, double *take_ms);

/* Host twin (no GPU): the rows of ONE set of arrays (several batches: concatenate them), serially.  *rows: malloc'ed, hand it
 * back with kslam_free.  Argument errors as kslam_variants_add; message: kslam_tail_last_error(). */
kslam_status kslam_tail_variants(const char *entry_bases, const uint64_t *entry_offsets, uint64_t n_entries,
                                 const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                                 const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads,
                                 const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                 uint64_t n_pairs, uint32_t min_alt, uint32_t min_depth, kslam_variant_row **rows, uint64_t *n_rows,
                                 kslam_variant_stats *stats);

/* The file: VCF 4.2, sites only.
 *   ##fileformat=VCFv4.2
 *   ##source=<the first token of kslam_version()>
 *   ##contig=<ID=locus,length=L>      one per entry that has a row, in entry order, locus as the SAM header spells it
 *   ##INFO lines for DP (Integer, 1), AO, SAF, SAR (Integer, A) and AF (Float, A)
 *   #CHROM  POS  ID  REF  ALT  QUAL  FILTER  INFO
 *   locus  pos + 1  .  ref  alt  .  .  DP=depth;AO=alt_fwd + alt_rev;SAF=alt_fwd;SAR=alt_rev;AF=AO / DP as %.6f (0.000000 when DP is 0)
 * Several alts at one site are several lines.  The rows must ascend as kslam_variants_take returns them.  KSLAM_ERR_ARG, before
 * anything is written, for a row whose entry is not in the view or has an empty locus (a VCF line needs a CHROM).  stats may be
 * NULL (it is not written). */
kslam_status kslam_variants_write(const kslam_index_view *index, const kslam_variant_row *rows, uint64_t n_rows,
                                  const kslam_variant_stats *stats, int fd);

/* kslam_stream_classify (kslam_stream.h) writes the file itself: call this before it with an open descriptor (-1: none).  It
 * holds for the NEXT call alone, which switches the variants on and resets them, feeds the batches left to the host through
 * kslam_variants_add on the host stage's thread, writes the file after the last batch and switches them off. */
kslam_status kslam_stream_set_variants(kslam_ctx *ctx, int fd, uint32_t min_alt, uint32_t min_depth);
kslam_status kslam_stream_get_variants(kslam_ctx *ctx, int *fd, uint32_t *min_alt, uint32_t *min_depth);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_VARIANTS_H_ */
