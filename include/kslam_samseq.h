/*
 * kslam_samseq.h -- SEQ and QUAL in the SAM file: columns 10 and 11 of the text (plain or BGZF, include/kslam_bgzf.h), l_seq /
 * seq / qual of the BAM records (include/kslam_bam.h), written on the GPU from the batch's bases and qualities by the kernels
 * that write the rest of the row (csrc/samtext.hip).  Same library as kslam.h.
 *
 * Off by default: the reference prints "*" in both columns of every row (src/SAM.h:278-290), and with the switch off every
 * byte of every output is what it was.  With it on, nothing else in a row changes, and:
 *   which rows     rows without flag 0x100 -- each mate's primary row, and the rows of an unmapped mate -- carry SEQ and
 *                  QUAL.  Secondary rows (0x100) keep "*" / "*" (l_seq 0), as bwa mem -a and minimap2 write them.  With
 *                  --sam-xa only primary rows exist.
 *   orientation    a row whose FLAG has 0x10 carries the reverse complement of the read's bases and the reversed quality
 *                  string; every other row carries both as the FASTQ record has them.  The FLAG bit decides, also on the
 *                  row of an unmapped mate.  (The row's coordinates are already in that orientation: for a reverse-complement
 *                  overlap the CIGAR is reversed and query_begin / query_end flipped, src/SmithWaterman.h:214-230, so the
 *                  soft clips the row prints are those of the sequence it now carries.)
 *   complement     A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D; W, S, N and every other byte unchanged; the case is kept.
 *                  The FASTQ reader (host/fastq.cpp) copies the bases line as it stands, between the line ends: no case
 *                  folding, nothing replaced or dropped, so lower-case letters, "." or digits reach the writer and leave
 *                  it as they came (forward rows) or through the table above (reverse rows).
 *   text           columns 10 and 11 replace "*\t*".  A read of length 0 keeps "*" / "*".  A batch loaded by columns
 *                  without qualities (no kslam_load_qualities*) writes SEQ and "*" for QUAL.
 *   BAM            l_seq = the read length; seq is (l_seq + 1) / 2 bytes, high nibble first, codes from "=ACMGRSVTWYHKDBN"
 *                  with either case mapping to the same code and every other byte to 15, the last low nibble 0 for an
 *                  odd length; qual is l_seq bytes of quality - 33, or l_seq bytes 0xFF without qualities.  block_size
 *                  covers both; bin and the tags are as in kslam_bam.h.  Secondary rows keep l_seq = 0.
 * One more exception joins kslam_bam.h's about what the BAM decodes to: the records decode (samtools view) to the text
 * byte for byte wherever the bases are upper-case IUPAC letters; a lower-case base decodes as its upper-case letter and any
 * other byte as "N", which is what samtools view -b stores for the text this library writes.
 *
 * Where the bytes come from: the gathered columns of the resident batch (bases, and qualities when the batch has them), for
 * every way a batch is loaded -- kslam_submit_batch_fastq / _fastq_text gather them from the uploaded text before the
 * aligner runs -- so the device reads no FASTQ text at this stage and both record kinds share one source.  The mapping
 * qualities that come back from the host's libm (kslam_samtext.h) are in place before the rows are written, as before.
 *
 * Use:  kslam_set_sam_seq(ctx, 1) before the batches.  It combines with kslam_set_sam_bgzf and kslam_set_sam_bam and is
 * honoured by the pipelined lanes (kslam_collect_batch), by the resident twins kslam_sam_text and kslam_sam_bam, and by
 * kslam_stream_classify (kslam_stream.h), whose host-formatted batches go through the twins below.
 */
#ifndef KSLAM_SAMSEQ_H_
#define KSLAM_SAMSEQ_H_
#include "kslam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_TEXT_SAM_SEQ 32u   /* kslam_batch_result.text_flags: sam_text was written with the switch below on */

/* on != 0: rows without flag 0x100 carry SEQ and QUAL (see above).  The lanes read the switch batch by batch; during a
 * kslam_stream_classify call it must not change: a batch that comes back formatted the other way fails the call
 * (KSLAM_ERR_STATE), as a change of kslam_set_sam_bam does.  Default off.  A context of a kslam_multi gets
 * KSLAM_ERR_UNSUPPORTED, as from kslam_set_sam_bam: a shard's context holds its share of the index, not a batch's rows. */
kslam_status kslam_set_sam_seq(kslam_ctx *ctx, int on);

/* *on = the switch above */
kslam_status kslam_get_sam_seq(kslam_ctx *ctx, int *on);

/* Host twins (no GPU): kslam_tail_sam / kslam_tail_sam_bam and kslam_tail_finish_write_rows / _bam (kslam_tail.h,
 * kslam_bam.h) with the switch on, the same bytes the device writes.  bam != 0: BAM records, else SAM lines.
 * reads->quality == NULL says the batch has no qualities (quality_off is still needed; a batch with CIGARs to walk on the
 * host needs the qualities themselves).  Errors: kslam_tail_last_error(). */
kslam_status kslam_tail_sam_seq(const kslam_tail_params *params, const kslam_reads_view *reads, const kslam_index_view *index,
                                const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                                int bam, char **out, uint64_t *len, kslam_tail_stats *stats);
kslam_status kslam_tail_finish_write_rows_seq(const kslam_tail_params *params, const kslam_reads_view *reads,
                                              const kslam_index_view *index, const kslam_overlap *overlaps, uint64_t n_overlaps,
                                              const uint32_t *cigar_pool, uint64_t n_cigar, const kslam_row_detail *details,
                                              const char *md_pool, uint64_t n_md, kslam_read_pair *read_pairs,
                                              uint64_t n_read_pairs, kslam_paired_overlap *pairs, uint64_t n_pairs, int bam,
                                              kslam_write_fn write, void *user, kslam_tail_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_SAMSEQ_H_ */
