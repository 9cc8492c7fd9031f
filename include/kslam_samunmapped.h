/*
 * kslam_samunmapped.h -- rows for the reads that have no alignment: one FLAG-4 row per read (text, plain or BGZF,
 * include/kslam_bgzf.h) or one unplaced record per read (include/kslam_bam.h), written on the GPU behind the batch's other rows
 * (csrc/samunmapped.hip).  Same library as kslam.h.
 *
 * Off by default: a read pair that ends a batch without a surviving alignment pair leaves no trace in the SAM file, as in the
 * reference (writeSAMOutputPairs, src/SAM.h:443-512), and with the switch off every byte of every output is what it was.
 * With it on, the SAM output of a batch is its rows as before, then:
 *   which reads    among the records the batch consumed (kslam_batch_result.consumed1 / consumed2; the loaded reads of a resident
 *                  batch), every read pair -- single-end: read -- for which the writer emits nothing: one that is not among
 *                  the batch's final read pairs, or whose group reports no row.  The decision is taken after every stage that
 *                  is switched on: a read that aligned and lost to a score screen gets a row here.  A pair of which one mate
 *                  aligned has its 0x4 / 0x8 rows from the writer already and gets nothing new.
 *   order          the input order of the batch's records; for a pair R1's row, then R2's.
 *   text           QNAME FLAG * 0 0 * * 0 0 SEQ QUAL and a newline, no tags.  QNAME is the id the other rows print for that
 *                  read.  FLAG is 77 (0x1 | 0x4 | 0x8 | 0x40) for R1 and 141 (0x1 | 0x4 | 0x8 | 0x80) for R2 of a pair, 4 for a
 *                  single-end read.  RNEXT is "*" in every case, also where the mapped rows of a paired run print "=".
 *   SEQ / QUAL     follow kslam_set_sam_seq (kslam_samseq.h) as a primary row does: off, "*" / "*"; on, the FASTQ record's
 *                  bases and qualities as they stand (0x10 is never set here, nothing is reversed), "*" / "*" for a read of
 *                  length 0, SEQ and "*" for a batch without qualities.
 *   BAM            refID -1, pos -1, mapq 0, bin 4680 (htslib's reg2bin(-1, 0), its value for an unplaced read), n_cigar_op 0,
 *                  the flag above, l_seq as kslam_samseq.h says (0 without that switch), next_refID -1, next_pos -1, tlen 0,
 *                  the read name with its NUL, seq and qual packed by kslam_samseq.h's rules, no tags.  An id longer than 254
 *                  bytes fails the batch and names the lowest such read, among these rows and the mapped ones together.
 * The rows land behind the mapped rows in the same device buffer, so the BGZF / BAM compression and the copy to the host run
 * once over the whole batch.  The per-read lines, the abbreviated report and the XML do not change.
 *
 * Use:  kslam_set_sam_unmapped(ctx, 1) before the batches.  It combines with kslam_set_sam_bgzf, kslam_set_sam_bam,
 * kslam_set_sam_seq and kslam_set_bgzf_deflate and is honoured by the pipelined lanes (kslam_collect_batch), by the resident
 * twins kslam_sam_text and kslam_sam_bam, and by kslam_stream_classify (kslam_stream.h), whose host-formatted batches go
 * through the twin below.
 */
#ifndef KSLAM_SAMUNMAPPED_H_
#define KSLAM_SAMUNMAPPED_H_
#include "kslam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_TEXT_SAM_UNMAPPED 64u   /* kslam_batch_result.text_flags: sam_text was written with the switch below on */

/* on != 0: the rows above follow every batch's rows.  The lanes read the switch batch by batch; during a
 * kslam_stream_classify call it must not change: a batch that comes back formatted the other way fails the call
 * (KSLAM_ERR_STATE), as a change of kslam_set_sam_seq does.  Default off.  A context of a kslam_multi gets
 * KSLAM_ERR_UNSUPPORTED, as from kslam_set_sam_seq. */
kslam_status kslam_set_sam_unmapped(kslam_ctx *ctx, int on);

/* *on = the switch above */
kslam_status kslam_get_sam_unmapped(kslam_ctx *ctx, int *on);

/* The new kernels of the last batch formatted on this context with the switch on (kslam_sam_text / kslam_sam_bam, or a lane
 * of this context): *ms = their device time by events (flags, lengths, scan and the write pass), *bytes_written = the bytes
 * of the new rows before compression, *n_rows = the rows.  All zero before the first such batch. */
kslam_status kslam_sam_unmapped_kernel_ms(kslam_ctx *ctx, double *ms, uint64_t *bytes_written, uint64_t *n_rows);

/* Host twin (no GPU): the bytes the device appends for one batch.  reads: the batch's columns ([R1 block | R2 block] when
 * params->paired; ids always, bases_off -- and bases -- only with seq != 0, quality == NULL: no qualities).  read_pairs: the
 * batch's FINAL read pairs (a group with count == 0 reports no row and counts as absent).  n_consumed_pairs: the read pairs
 * (single-end: reads) the batch consumed, at most reads->n_reads / 2 (single-end: n_reads).  bam != 0: BAM records, else SAM
 * lines; seq != 0: kslam_set_sam_seq on.  *out is malloc'ed (kslam_free), never NULL on success.  BAM with an id longer than
 * 254 bytes among the rows: KSLAM_ERR_ARG naming the lowest such read, *out = NULL.  Errors: kslam_tail_last_error(). */
kslam_status kslam_tail_sam_unmapped(const kslam_tail_params *params, const kslam_reads_view *reads, const kslam_read_pair *read_pairs,
                                     uint64_t n_read_pairs, uint64_t n_consumed_pairs, int bam, int seq, char **out, uint64_t *len);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_SAMUNMAPPED_H_ */
