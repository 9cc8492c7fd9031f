/*
 * kslam_readqc.h -- a read QC report (the first table of any sequencing run: reads and bases taken in, read lengths, base
 * content and quality per cycle, mean quality per read, GC content, N bases, broken quality bytes; what FastQC and fastp
 * make), tallied per cycle on the GPU from the columns the lanes already hold (csrc/readqc.hip).  Same library as kslam.h.
 * It is the one report on what went IN: it needs no index, no alignment result and no device pairing.
 *
 * Off by default; with the switch off every byte of every output is what it was.  With it on:
 *   input         every read taken into a batch: the records the batch consumed, whether or not they aligned.  A batch is
 *                 laid out [R1 | R2]: stream 0 is the first half of its reads, stream 1 the second; a single-end batch has
 *                 stream 0 only.  A read is its bases and its quality bytes, which have the same length (the text route
 *                 refuses a record where they differ; kslam_tail_read_qc returns KSLAM_ERR_ARG for one).
 *   cycle rows    C = max_cycles is chosen at switch-on: 0 means 512, 1 .. 65 536 are legal.  Every per-cycle table has C + 1
 *                 rows: row c < C is cycle c (the read's c-th byte, from 0), row C pools every cycle at or above C, so the
 *                 totals stay exact for reads of any length.
 *   per stream    all counters 64-bit:
 *                   n_reads, n_bases
 *                   min_len, max_len     both 0 when n_reads == 0
 *                   len_hist[0 .. C+1]   entry l <= C counts the reads of exactly l bases, entry C + 1 the longer reads
 *                   base[c][k], k = 0..5 A/a, C/c, G/g, T/t, N/n, any other byte -- in that order
 *                   qual[c][q], q = 0..94  a byte b in 33..126 counts in b - 33; every other byte (0x00, 0x7F and above
 *                                        included) counts in column 94
 *                   mean_q[0 .. 93]      one count per read that has at least one quality byte in 33..126: the bin is
 *                                        floor(sum(b - 33) / count) over those bytes, in integer arithmetic
 *                   gc[0 .. 100]         one count per read that has at least one A, C, G or T: with g the number of G and C
 *                                        bases and n the number of A, C, G and T bases (either case) the bin is
 *                                        (200 * g + n) / (2 * n) in integer division: percent, rounded half up
 *   paired        1 when a batch counted since the last reset was paired, else 0 (the host twin: its `paired` argument)
 *   determinism   the tables are integer sums: they do not depend on the number of lanes, on the order of the batches, on
 *                 whether a batch was counted by its lane or handed in through kslam_read_qc_add, or on how often take was
 *                 called; they equal kslam_tail_read_qc on the same reads, field for field.
 *
 * What a lane counts: every batch submitted with kslam_submit_batch_fastq_text (plain or BGZF input alike: the columns are cut
 * from the inflated text), from the bases and quality columns the lane has just cut out of it, on the lane's own stream.  The
 * other submit routes (kslam_submit_batch, _columns, _fastq) are NOT counted by the lane: hand their columns to
 * kslam_read_qc_add.
 *
 * The tables travel as one block of 64-bit words, 2 * words_per_stream of them, stream 0 first.  A stream's words:
 *   [0] n_reads  [1] n_bases  [2] min_len  [3] max_len  then len_hist (C + 2), base ((C + 1) * 6, row-major), qual ((C + 1) * 95,
 *   row-major), mean_q (94), gc (101).  The pointers of kslam_read_qc_stream point into the block.
 *
 * The file (kslam_read_qc_write) is one JSON document, written exactly like this (two spaces per level, ", " between the
 * numbers of an array, keys in this order).  For one paired batch of two reads, R1 = ACGTN with qualities IIII#, R2 = GGC
 * with qualities 5?~, C = 4:
 *   {
 *     "kslam_read_qc": 1,
 *     "paired": true,
 *     "max_cycles": 4,
 *     "summary": {
 *       "total_reads": 2,
 *       "total_bases": 8,
 *       "q20_bases": 7,
 *       "q30_bases": 6,
 *       "q20_rate": "0.875000",
 *       "q30_rate": "0.750000",
 *       "gc_content": "0.714286",
 *       "n_bases": 1,
 *       "other_bases": 0,
 *       "invalid_quality_bytes": 0
 *     },
 *     "read1": {
 *       "total_reads": 1,
 *       "total_bases": 5,
 *       "min_length": 5,
 *       "max_length": 5,
 *       "mean_length": "5.000000",
 *       "q20_bases": 4,
 *       "q30_bases": 4,
 *       "gc_content": "0.500000",
 *       "n_bases": 1,
 *       "other_bases": 0,
 *       "invalid_quality_bytes": 0,
 *       "length_counts": {">4": 1},
 *       "content": {
 *         "A": [1],
 *         "C": [0, 1],
 *         "G": [0, 0, 1],
 *         "T": [0, 0, 0, 1],
 *         "N": [],
 *         "other": [],
 *         "tail": [0, 0, 0, 0, 1, 0]
 *       },
 *       "quality_mean": ["40.000000", "40.000000", "40.000000", "40.000000"],
 *       "quality_tail_mean": "2.000000",
 *       "quality_counts": {"2": [0, 0, 0, 0, 1], "40": [1, 1, 1, 1]},
 *       "mean_quality_counts": {"32": 1},
 *       "gc_counts": {"50": 1}
 *     },
 *     "read2": { ... the same keys ... }
 *   }
 * Counts are integers.  Every ratio is "%.6f" of a double division of two of those integers, as a JSON string; a zero
 * denominator prints "0.000000".  q20_bases / q30_bases: quality bytes in 33..126 with b - 33 >= 20 / >= 30; the rates divide by
 * total_bases.  gc_content: G + C over A + C + G + T.  n_bases, other_bases: columns 4 and 5 of `base`.  invalid_quality_bytes:
 * column 94 of `qual`.  mean_length: n_bases / n_reads.  length_counts: the lengths that occur, ascending, the pooled entry
 * under the key ">C" with C in digits.  content: the per-cycle arrays of rows 0 .. C - 1, each cut after its last non-zero
 * count; `tail` is row C's six counters (A, C, G, T, N, other), always six.  quality_mean: per cycle, sum(q * count) / sum(count)
 * over columns 0..93, cut after the last row of 0 .. C - 1 that holds a quality byte of any column; quality_tail_mean the same
 * ratio for row C.  quality_counts: per quality value that occurs (keys ascending; column 94 under "invalid"), the per-cycle
 * counts over rows 0 .. C -- here the tail row IS the last entry -- cut after the last non-zero count.  mean_quality_counts,
 * gc_counts: the bins that hold a count, ascending.  "read2" is written for a paired run only; `summary` sums the streams.
 * Where a quantity means what fastp's JSON means by it, it has fastp's key name (total_reads, total_bases, q20_bases,
 * q30_bases, q20_rate, q30_rate, gc_content); the document as a whole is this library's own, and nothing here claims that
 * MultiQC's fastp module reads it: that has not been tried.
 *
 * The state -- the two streams' words on the device, 8 * 2 * (4 + (C + 2) + 101 * (C + 1) + 195) bytes: 0.8 MB at C = 512 --
 * belongs to the context the switch was set on and is shared by its lanes; it is zeroed at switch-on and by
 * kslam_read_qc_reset and freed at switch-off and by kslam_destroy.  kslam_set_index leaves it alone.
 */
#ifndef KSLAM_READQC_H_
#define KSLAM_READQC_H_
#include "kslam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_READ_QC_DEFAULT_CYCLES 512u
#define KSLAM_READ_QC_MAX_CYCLES 65536u
#define KSLAM_READ_QC_BASE_COLS 6u
#define KSLAM_READ_QC_QUAL_COLS 95u
#define KSLAM_READ_QC_MEAN_BINS 94u
#define KSLAM_READ_QC_GC_BINS 101u
/* a stream's 64-bit words for C cycle rows (C as resolved: not 0) */
#define KSLAM_READ_QC_WORDS(C) (4ull + ((uint64_t)(C) + 2) + ((uint64_t)(C) + 1) * (KSLAM_READ_QC_BASE_COLS + KSLAM_READ_QC_QUAL_COLS) + KSLAM_READ_QC_MEAN_BINS + KSLAM_READ_QC_GC_BINS)

typedef struct {
  uint64_t n_reads, n_bases, min_len, max_len;
  const uint64_t *len_hist;   /* [C + 2] */
  const uint64_t *base;       /* [(C + 1) * 6] */
  const uint64_t *qual;       /* [(C + 1) * 95] */
  const uint64_t *mean_q;     /* [94] */
  const uint64_t *gc;         /* [101] */
} kslam_read_qc_stream;

typedef struct {
  uint32_t max_cycles;        /* C, resolved */
  int32_t paired;
  uint64_t words_per_stream;  /* KSLAM_READ_QC_WORDS(C) */
  uint64_t *block;            /* 2 * words_per_stream words, stream 0 first; library-owned */
  kslam_read_qc_stream stream[2];
} kslam_read_qc_tables;

/* on != 0: a lane counts every batch that arrives through kslam_submit_batch_fastq_text.  Needs neither an index nor the device
 * pairing.  Switching on allocates and zeroes the state; on when already on with the same C: nothing happens, with another C:
 * KSLAM_ERR_STATE (switch off first).  max_cycles above 65 536 is KSLAM_ERR_ARG.  Off frees the state (max_cycles is not looked
 * at).  Set it between batches.  A context of a kslam_multi gets KSLAM_ERR_UNSUPPORTED, as from kslam_set_coverage. */
kslam_status kslam_set_read_qc(kslam_ctx *ctx, int on, uint32_t max_cycles);
/* *max_cycles: C as resolved, 0 with the switch off */
kslam_status kslam_get_read_qc(kslam_ctx *ctx, int *on, uint32_t *max_cycles);

/* zeroes the tables and `paired`; KSLAM_ERR_STATE with the switch off */
kslam_status kslam_read_qc_reset(kslam_ctx *ctx);

/* Host columns in, uploaded and counted by the same kernel a lane uses: read i is bases[bases_off[i] .. bases_off[i + 1]) and the
 * same bytes of quality (bases_off: n_reads + 1 entries).  paired != 0: the first half of the reads is stream 0, the second
 * stream 1; else all are stream 0.  KSLAM_ERR_ARG for offsets that do not ascend and for paired with an odd n_reads;
 * KSLAM_ERR_STATE with the switch off.  May be called from any thread; calls are serialised. */
kslam_status kslam_read_qc_add(kslam_ctx *ctx, const char *bases, const uint64_t *bases_off, const char *quality, uint64_t n_reads, int paired);

/* The tables of every batch counted so far (it waits for the lanes' streams), copied into page-locked, library-owned memory:
 * hand them back with kslam_read_qc_release.  The call may be repeated and more batches may follow it. */
kslam_status kslam_read_qc_take(kslam_ctx *ctx, kslam_read_qc_tables *tables);
void kslam_read_qc_release(kslam_ctx *ctx, kslam_read_qc_tables *tables);

/* device time (ms), by events around the launches, of the count pass of the last kslam_read_qc_add (the lanes' times are not
 * gathered), and the bytes of bases + quality it read */
kslam_status kslam_read_qc_kernel_ms(kslam_ctx *ctx, double *count_ms, uint64_t *bytes);

/* Host twin (no GPU): the tables of ONE set of reads (several batches: concatenate them per stream), in one serial pass.  Read
 * i is bases[bases_off[i] .. bases_off[i + 1]) with the quality bytes quality[quality_off[i] .. quality_off[i + 1]); a read
 * whose two lengths differ is KSLAM_ERR_ARG, as are offsets that do not ascend and paired with an odd n_reads.  max_cycles as
 * for kslam_set_read_qc.  tables->block is malloc'ed: free it with kslam_tail_read_qc_free.  message: kslam_tail_last_error(). */
kslam_status kslam_tail_read_qc(const char *bases, const uint64_t *bases_off, const char *quality, const uint64_t *quality_off, uint64_t n_reads,
                                int paired, uint32_t max_cycles, kslam_read_qc_tables *tables);
void kslam_tail_read_qc_free(kslam_read_qc_tables *tables);

/* The file described above, from tables as kslam_read_qc_take / kslam_tail_read_qc give them. */
kslam_status kslam_read_qc_write(const kslam_read_qc_tables *tables, int fd);

/* kslam_stream_classify (kslam_stream.h) writes the report itself: call this before it with an open descriptor (-1: none).  It
 * holds for the NEXT call alone, which switches the report on with max_cycles and resets it, lets the lanes count every batch,
 * writes the file after the last batch and switches the report off. */
kslam_status kslam_stream_set_read_qc(kslam_ctx *ctx, int fd, uint32_t max_cycles);
kslam_status kslam_stream_get_read_qc(kslam_ctx *ctx, int *fd, uint32_t *max_cycles);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_READQC_H_ */
