/*
 * kslam_alignqc.h -- an alignment QC report (how good the alignments themselves are: the error rate by cycle and by base
 * quality, the substitution spectrum, the indel lengths, the edit distance and identity per alignment, the insert sizes of the
 * pairs; what `samtools stats` (MPC, IS, ID, IC), Qualimap and Picard make from a second pass over a sorted BAM), tallied per
 * cycle on the GPU from what a lane holds when it has finished a batch (csrc/alignqc.hip).  Same library as kslam.h.
 * kslam_readqc.h reports what went IN, this one what the aligner made of it.
 *
 * Off by default; with the switch off every byte of every output is what it was.  With it on:
 *   contributing set   as kslam_variants.h: a batch contributes its FINAL read pairs, the groups read_pairs[i] with their LIVE
 *                      alignment pairs pairs[first .. first + count); the records between first + count and the next group's
 *                      first are dead.  Every overlap record that at least one live alignment pair names as r1 or r2 (not
 *                      KSLAM_NO_OVERLAP) contributes ONCE, however many live pairs name it (a read that aligns to one place is
 *                      one observation of the sequencer's errors, whatever the pairing made of it).
 *   skipped records    a contributing overlap record adds one to n_records and one to n_skipped, and nothing else, when
 *                        entry >= n_entries, or cigar_len == 0, or ref_begin < 0, or
 *                        its CIGAR runs past the read or past the entry: an M or D run whose end exceeds the entry's length,
 *                        an M or I run whose end exceeds the read's length.
 *                      The check covers the whole CIGAR and is made before anything of that record is counted.  No kernel reads
 *                      outside a read, an entry or the pool, whatever the records hold.
 *   the walk           starts at reference position ref_begin and at query position max(query_begin, 0).  The query is the read,
 *                      or its reverse complement when revcomp != 0; in the reverse complement only upper-case A/C/G/T are
 *                      complemented, every other byte stays as it is.  Operations are M = 0, I = 1, D = 2, packed
 *                      len << 4 | op; M advances both positions, I the query, D the reference; any other operation is passed
 *                      over.
 *   stream             with paired != 0 a record whose read < n_reads / 2 is stream 0, else stream 1; single-end, all records
 *                      are stream 0.
 *   cycle              the index of a base in the read AS SEQUENCED: q for a forward record, len - 1 - q for a reverse one, with
 *                      q the query position of the walk and len the read's length.  The quality byte of a column is the one at
 *                      that index.
 *   cycle rows         C = max_cycles is chosen at switch-on: 0 means 512, 1 .. 65 536 are legal (as kslam_readqc.h).  Every
 *                      per-cycle table has C + 1 rows; row c < C is cycle c, row C pools every cycle at or above C.
 *   per stream         all counters 64-bit:
 *                        n_records           contributing records (the skipped ones among them)
 *                        n_reverse           the non-skipped ones with revcomp != 0
 *                        n_skipped
 *                        n_without_quality   contributing records (skipped or not) of a batch that came without quality column
 *                        m_columns           all M columns
 *                        compared            M columns where the entry's byte and the query byte are both upper-case ACGT
 *                        mismatches          compared columns whose two bytes differ
 *                        ins_events, ins_bases, del_events, del_bases    I / D runs of length >= 1 and their summed lengths
 *                        unaligned_bases     read length - M columns - inserted bases, per non-skipped record
 *                        subst[4][4]         reference base -> read base (A C G T) over the compared columns, in the orientation
 *                                            of the read as sequenced: for a reverse record both bases are complemented.  The
 *                                            diagonal holds the matches; the sum is `compared`.
 *                        ins_len[65], del_len[65]   one count per I / D run of length l >= 1 in entry min(l, 65) - 1
 *                        nm[65]              one count per non-skipped record in entry min(mismatches + ins_bases + del_bases, 64)
 *                                            of that record
 *                        identity[101]       one count per non-skipped record whose denominator compared + ins_bases + del_bases
 *                                            is above 0, in bin 100 * (compared - mismatches) / denominator, integer division
 *                        cycle[c][4]         compared columns; mismatches; inserted bases (each at its own cycle); deletion
 *                                            events, counted at the cycle of query position min(q, len - 1) where the walk stands
 *                                            when it meets the D run (a read of no bases has no cycle: the event is in the
 *                                            scalars and in del_len alone)
 *                        cq_compared[c][95], cq_mismatch[c][95]   compared columns and mismatches by cycle and quality: a quality
 *                                            byte b in 33..126 counts in column b - 33, every other byte in column 94 (as
 *                                            kslam_readqc.h).  Counted only for records of a batch that has a quality column.
 *   per report         n_read_pairs         groups with count > 0
 *                      pairs_both, pairs_r1_only, pairs_r2_only   live alignment pairs by which of r1 / r2 is not
 *                                            KSLAM_NO_OVERLAP (a live pair with neither counts nowhere)
 *                      insert[1002]         one count per live pair with both mates in entry min(insert_size, 1001)
 *                      insert_sum           the sum of those insert sizes
 *                      paired               1 when a batch counted since the last reset was paired (host twin: its argument)
 *   determinism        integer sums only.  The tables do not depend on the number of lanes, on the order of the batches, on whether
 *                      a batch came from its lane or through kslam_align_qc_add, or on how often take was called; they equal
 *                      kslam_tail_align_qc on the same arrays, field for field.
 *
 * What a lane counts: every batch it finishes with its final read pairs on the device (as kslam_set_variants); the quality column
 * is there on the text route (kslam_submit_batch_fastq_text) and on every route that uploaded one.  A batch whose pseudo-assembly
 * the device left to the host is NOT counted by the lane: hand its final arrays to kslam_align_qc_add after the host stage.
 *
 * The tables travel as one block of KSLAM_ALIGN_QC_WORDS(C) 64-bit words:
 *   [0] n_read_pairs [1] pairs_both [2] pairs_r1_only [3] pairs_r2_only [4] insert_sum [5] reserved (0)
 *   [6 .. 1008) insert
 *   then stream 0's KSLAM_ALIGN_QC_STREAM_WORDS(C) words, then stream 1's.  A stream's words:
 *   [0] n_records [1] n_reverse [2] n_skipped [3] n_without_quality [4] m_columns [5] compared [6] mismatches [7] ins_events
 *   [8] ins_bases [9] del_events [10] del_bases [11] unaligned_bases
 *   then subst (16, row-major: reference base first), ins_len (65), del_len (65), nm (65), identity (101),
 *   cycle ((C + 1) * 4, row-major), cq_compared ((C + 1) * 95, row-major), cq_mismatch ((C + 1) * 95, row-major).
 * The pointers of kslam_align_qc_tables point into the block.
 *
 * The file (kslam_align_qc_write) is one JSON document in kslam_read_qc_write's conventions (two spaces per level, ", " between
 * the elements of an array or of a one-line object, keys in this order).  Counts are integers.  Every ratio is "%.6f" of a double
 * division of two of those integers, as a JSON string; a zero denominator prints "0.000000".  Worked example, C = 4, single-end,
 * one entry ACGTACGTAC and one group with one live pair that names both records:
 *   record 0   read ACGATC, quality IIII#I, forward, ref_begin 0, CIGAR 3M 1I 2M: the insertion is the read's A at cycle 3;
 *              the M column of cycle 4 (quality 2) compares entry T with read T, the last one (cycle 5, quality 40) entry A
 *              with read C.  Edit distance 2, identity 100 * 4 / 6 = 66.
 *   record 1   read GTGC, quality 5555 (20), REVERSE, ref_begin 4, CIGAR 2M 1D 2M: the query is GCAC; columns: entry A / query G
 *              (cycle 3), entry C / query C (cycle 2), the deletion of entry G met at query position 2 (cycle 1), entry T /
 *              query A (cycle 1), entry A / query C (cycle 0).  As sequenced both bases are complemented: T>C, a match G>G, A>T
 *              and T>G.  Edit distance 4, identity 100 * 1 / 5 = 20.
 *   the pair   r1 = record 0, r2 = record 1, insert_size 9
 *   {
 *     "kslam_align_qc": 1,
 *     "paired": false,
 *     "max_cycles": 4,
 *     "summary": {
 *       "records": 2,
 *       "reverse": 1,
 *       "skipped": 0,
 *       "without_quality": 0,
 *       "m_columns": 9,
 *       "compared": 9,
 *       "mismatches": 4,
 *       "error_rate": "0.444444",
 *       "ins_events": 1,
 *       "ins_bases": 1,
 *       "del_events": 1,
 *       "del_bases": 1,
 *       "unaligned_bases": 0,
 *       "mean_identity": "0.454545",
 *       "read_pairs": 1,
 *       "pairs_both": 1,
 *       "pairs_r1_only": 0,
 *       "pairs_r2_only": 0,
 *       "insert_size_mean": "9.000000",
 *       "insert_size_median": "9"
 *     },
 *     "read1": {
 *       "records": 2,
 *       "reverse": 1,
 *       "skipped": 0,
 *       "without_quality": 0,
 *       "m_columns": 9,
 *       "compared": 9,
 *       "mismatches": 4,
 *       "error_rate": "0.444444",
 *       "ins_events": 1,
 *       "ins_bases": 1,
 *       "del_events": 1,
 *       "del_bases": 1,
 *       "unaligned_bases": 0,
 *       "mean_identity": "0.454545",
 *       "mismatch_rate_by_cycle": ["0.500000", "0.500000", "0.000000", "1.000000"],
 *       "mismatch_rate_tail": "0.500000",
 *       "compared_by_cycle": [2, 2, 2, 1],
 *       "mismatches_by_cycle": [1, 1, 0, 1],
 *       "inserted_bases_by_cycle": [0, 0, 0, 1],
 *       "deletions_by_cycle": [0, 1],
 *       "tail": [2, 1, 0, 0],
 *       "substitutions": {"A>C": 1, "A>G": 0, "A>T": 1, "C>A": 0, "C>G": 0, "C>T": 0, "G>A": 0, "G>C": 0, "G>T": 0, "T>A": 0, "T>C": 1, "T>G": 1, "matches": 5},
 *       "by_quality": {"2": [1, 0, "0.000000"], "20": [4, 3, "1.249387"], "40": [4, 1, "6.020600"]},
 *       "insertion_lengths": {"1": 1},
 *       "deletion_lengths": {"1": 1},
 *       "edit_distance_counts": {"2": 1, "4": 1},
 *       "identity_counts": {"20": 1, "66": 1}
 *     },
 *     "insert_size_counts": {"9": 1}
 *   }
 * summary: both streams summed, then the pair counters.  error_rate: mismatches / compared.  mean_identity: over all non-skipped
 * records, (compared - mismatches) / (compared + ins_bases + del_bases) of the summed counters.  insert_size_mean: insert_sum /
 * pairs_both.  insert_size_median: the smallest bin b with 2 * (insert[0] + .. + insert[b]) >= pairs_both, as a string of digits,
 * ">1000" when it is the pooled bin, "0" without pairs.  read1 / read2 (read2 for a paired report only): the scalars; the four
 * per-cycle arrays over rows 0 .. C - 1, each cut after its last non-zero count, and mismatch_rate_by_cycle (mismatches /
 * compared per row) cut after the last row that holds a compared column; `tail` is row C's four counters, always four, and
 * mismatch_rate_tail its ratio.  substitutions: the 12 off-diagonal cells "reference>read" in the order above, then the diagonal's
 * sum.  by_quality: per quality value that occurs in cq_compared summed over all rows (keys ascending; column 94 under
 * "invalid"): [compared, mismatches, empirical], empirical = "%.6f" of -10 * log10((double)mismatches / (double)compared) + 0.0
 * (so that a rate of 1 prints "0.000000", not "-0.000000") when both are above 0, else "0.000000".  insertion_lengths, deletion_lengths: the lengths that occur, the pooled entry under ">64".
 * edit_distance_counts: the values that occur, the pooled entry under "64+".  identity_counts: the bins that hold a count.
 * insert_size_counts: the bins that hold a count, the pooled one under ">1000".
 *
 * The state -- the block on the device, 8 * KSLAM_ALIGN_QC_WORDS(C) bytes: 1.6 MB at C = 512, whatever the database or the run --
 * belongs to the context the switch was set on and is shared by its lanes; it is zeroed at switch-on and by kslam_align_qc_reset
 * and freed at switch-off, by kslam_set_index (as the variants' state is: the switch is off afterwards) and by kslam_destroy.
 */
#ifndef KSLAM_ALIGNQC_H_
#define KSLAM_ALIGNQC_H_
#include "kslam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_ALIGN_QC_DEFAULT_CYCLES 512u
#define KSLAM_ALIGN_QC_MAX_CYCLES 65536u
#define KSLAM_ALIGN_QC_QUAL_COLS 95u
#define KSLAM_ALIGN_QC_CYCLE_COLS 4u
#define KSLAM_ALIGN_QC_LEN_BINS 65u
#define KSLAM_ALIGN_QC_NM_BINS 65u
#define KSLAM_ALIGN_QC_IDENTITY_BINS 101u
#define KSLAM_ALIGN_QC_INSERT_BINS 1002u
#define KSLAM_ALIGN_QC_SCALARS 12u
#define KSLAM_ALIGN_QC_REPORT_WORDS (6ull + KSLAM_ALIGN_QC_INSERT_BINS)
/* a stream's 64-bit words for C cycle rows (C as resolved: not 0) */
#define KSLAM_ALIGN_QC_STREAM_WORDS(C) (KSLAM_ALIGN_QC_SCALARS + 16ull + 2 * KSLAM_ALIGN_QC_LEN_BINS + KSLAM_ALIGN_QC_NM_BINS + KSLAM_ALIGN_QC_IDENTITY_BINS + ((uint64_t)(C) + 1) * (KSLAM_ALIGN_QC_CYCLE_COLS + 2 * KSLAM_ALIGN_QC_QUAL_COLS))
/* the whole block */
#define KSLAM_ALIGN_QC_WORDS(C) (KSLAM_ALIGN_QC_REPORT_WORDS + 2 * KSLAM_ALIGN_QC_STREAM_WORDS(C))

typedef struct {
  uint64_t n_records, n_reverse, n_skipped, n_without_quality, m_columns, compared, mismatches, ins_events, ins_bases, del_events, del_bases,
      unaligned_bases;
  const uint64_t *subst;        /* [16] */
  const uint64_t *ins_len;      /* [65] */
  const uint64_t *del_len;      /* [65] */
  const uint64_t *nm;           /* [65] */
  const uint64_t *identity;     /* [101] */
  const uint64_t *cycle;        /* [(C + 1) * 4] */
  const uint64_t *cq_compared;  /* [(C + 1) * 95] */
  const uint64_t *cq_mismatch;  /* [(C + 1) * 95] */
} kslam_align_qc_stream;

typedef struct {
  uint32_t max_cycles;          /* C, resolved */
  int32_t paired;
  uint64_t n_words;             /* KSLAM_ALIGN_QC_WORDS(C) */
  uint64_t *block;              /* n_words words; library-owned */
  uint64_t n_read_pairs, pairs_both, pairs_r1_only, pairs_r2_only, insert_sum;
  const uint64_t *insert;       /* [1002] */
  kslam_align_qc_stream stream[2];
} kslam_align_qc_tables;

/* on != 0: the lanes count every batch they finish.  Needs an index, the device pairing (kslam_set_pairing with stages != 0) and
 * a context created with report_cigar != 0, else KSLAM_ERR_STATE.  Switching on allocates and zeroes the state; on when already
 * on with the same C: nothing happens, with another C: KSLAM_ERR_STATE (switch off first).  max_cycles above 65 536 is
 * KSLAM_ERR_ARG.  Off frees the state (max_cycles is not looked at).  Set it between batches.  A context of a kslam_multi gets
 * KSLAM_ERR_UNSUPPORTED, as from kslam_set_coverage. */
kslam_status kslam_set_align_qc(kslam_ctx *ctx, int on, uint32_t max_cycles);
/* *max_cycles: C as resolved, 0 with the switch off */
kslam_status kslam_get_align_qc(kslam_ctx *ctx, int *on, uint32_t *max_cycles);

/* zeroes the tables and `paired`; KSLAM_ERR_STATE with the switch off */
kslam_status kslam_align_qc_reset(kslam_ctx *ctx);

/* Host arrays in, uploaded and counted like a lane's batch: for the batches left to the host, and for stage-level tests.
 * read_bases / read_offsets: read i is read_bases[read_offsets[i] .. read_offsets[i + 1]); read_quality: the same bytes of the
 * quality column, or NULL for a batch without one.  Before anything is launched, KSLAM_ERR_ARG for kslam_variants_add's refusals
 * (a live record's r1 / r2 >= n_overlaps, first + count > n_pairs, groups whose `first` do not ascend or whose slices overlap,
 * 2^32 or more overlap records, an overlap record named by a live pair whose CIGAR slice lies outside the pool or whose `read` is
 * >= n_reads), for read offsets that do not ascend and for paired != 0 with an odd n_reads.  KSLAM_ERR_STATE with the switch off.
 * May be called from any thread; calls are serialised. */
kslam_status kslam_align_qc_add(kslam_ctx *ctx, const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool,
                                uint64_t n_cigar, const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads,
                                const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                uint64_t n_pairs, const char *read_quality, int paired);

/* The tables of every batch counted so far (it waits for the lanes' streams), copied into page-locked, library-owned memory:
 * hand them back with kslam_align_qc_release.  The call may be repeated and more batches may follow it. */
kslam_status kslam_align_qc_take(kslam_ctx *ctx, kslam_align_qc_tables *tables);
void kslam_align_qc_release(kslam_ctx *ctx, kslam_align_qc_tables *tables);

/* device time (ms), by events around its launches, of the count pass of the last kslam_align_qc_add (the flag, list and pair
 * passes are not in it; the lanes' times are not gathered) */
kslam_status kslam_align_qc_kernel_ms(kslam_ctx *ctx, double *count_ms);

/* Host twin (no GPU): the tables of ONE set of arrays (several batches: concatenate them), serially.  Argument errors as
 * kslam_align_qc_add; max_cycles as for kslam_set_align_qc.  tables->block is malloc'ed: free it with kslam_tail_align_qc_free.
 * message: kslam_tail_last_error(). */
kslam_status kslam_tail_align_qc(const char *entry_bases, const uint64_t *entry_offsets, uint64_t n_entries, const kslam_overlap *overlaps,
                                 uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar, const char *read_bases,
                                 const uint64_t *read_offsets, uint64_t n_reads, const kslam_read_pair *read_pairs, uint64_t n_read_pairs,
                                 const kslam_paired_overlap *pairs, uint64_t n_pairs, const char *read_quality, int paired,
                                 uint32_t max_cycles, kslam_align_qc_tables *tables);
void kslam_tail_align_qc_free(kslam_align_qc_tables *tables);

/* The file described above, from tables as kslam_align_qc_take / kslam_tail_align_qc give them (read from the block alone). */
kslam_status kslam_align_qc_write(const kslam_align_qc_tables *tables, int fd);

/* kslam_stream_classify (kslam_stream.h) writes the report itself: call this before it with an open descriptor (-1: none).  It
 * holds for the NEXT call alone, which switches the report on with max_cycles and resets it, lets the lanes count every batch
 * they finish, feeds the batches left to the host through kslam_align_qc_add on the host stage's thread (with the columns parsed
 * from the batch's text), writes the file after the last batch and switches the report off.  The context needs report_cigar. */
kslam_status kslam_stream_set_align_qc(kslam_ctx *ctx, int fd, uint32_t max_cycles);
kslam_status kslam_stream_get_align_qc(kslam_ctx *ctx, int *fd, uint32_t *max_cycles);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_ALIGNQC_H_ */
