/*
 * kslam_bam.h -- the SAM file as BAM (SAM spec v1, section 4.2): the same records, binary, in BGZF members
 * (include/kslam_bgzf.h), encoded and compressed on the GPU.  Same library as kslam.h.
 *
 * The file is kslam_bam_header's bytes followed by the records of every batch, all of it BGZF, ended by KSLAM_BGZF_EOF.
 * Decoded (samtools view -h), it is the SAM text the plain route writes, byte for byte, with one exception: a mapped row
 * whose text has an empty CIGAR field is stored with n_cigar_op = 0 and decodes as "*".  How the fields are filled:
 *   refID            the row's index entry (the header lists the entries in entry order, so RNAME decodes back)
 *   pos / next_pos   POS - 1 / PNEXT - 1 (-1 for 0)         next_refID   refID for RNEXT "=", -1 for "*"
 *   l_read_name      id length + 1: a read id longer than 254 bytes cannot be encoded (the call fails and names it)
 *   l_seq            0: SEQ and QUAL are "*"                 bin          reg2bin(pos, pos + max(1, M + D lengths))
 *   CIGAR            len << 4 | op, M 0, I 1, D 2, S 4 (the soft clips the text prints)
 *   tags             MD AS XS NM X0 XT XG XP XR as the text has them; Z values end in NUL (XR keeps its quotes); integers
 *                    at htslib's smallest width (C / S / I, c / s / i for negative values), as samtools view -b stores them
 *
 * Use:  kslam_set_sam_bam(ctx, 1) before the batches: the pipelined lanes then write BAM records instead of SAM text and
 * compress them on the device; kslam_collect_batch returns the members in sam_text / sam_text_len with KSLAM_TEXT_SAM_BGZF
 * and KSLAM_TEXT_SAM_BAM in text_flags.  BAM implies BGZF, whatever kslam_set_sam_bgzf says; kslam_set_bgzf_deflate
 * (kslam_bgzf.h) applies to the members of a BAM file as to any others.  The per-read text stays plain.  kslam_stream_classify (kslam_stream.h) writes the whole file when the switch is on.
 */
#ifndef KSLAM_BAM_H_
#define KSLAM_BAM_H_
#include "kslam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_TEXT_SAM_BAM 16u   /* with KSLAM_TEXT_SAM_BGZF: sam_text holds BGZF members whose content is BAM records */

/* on != 0: the pipelined lanes write BAM records, compressed (see above).  Default off.  A context of a kslam_multi gets
 * KSLAM_ERR_UNSUPPORTED. */
kslam_status kslam_set_sam_bam(kslam_ctx *ctx, int on);

/* *on = the switch above */
kslam_status kslam_get_sam_bam(kslam_ctx *ctx, int *on);

/* The BAM header, uncompressed, built on the host: "BAM\1", l_text, sam_header[0 .. len) as it is (normally
 * kslam_sam_header's text), n_ref, and per index entry in entry order l_name, the locus tag with a NUL, l_ref (the entry's
 * base count).  *out is malloc'ed (release with kslam_free), as kslam_sam_header's.  Errors: kslam_tail_last_error(). */
kslam_status kslam_bam_header(const kslam_index_view *index, const char *sam_header, uint64_t len, char **out, uint64_t *out_len);

/* The resident-batch twin of kslam_sam_text (include/kslam_samtext.h): the batch's BAM records, uncompressed.  *bam is
 * page-locked and library-owned (kslam_free_pinned). */
kslam_status kslam_sam_bam(kslam_ctx *ctx, int paired, uint32_t num_alignments, int sam_xa, char **bam, uint64_t *len);

/* Host twins (no GPU): kslam_tail_sam and kslam_tail_finish_write_rows (include/kslam_tail.h) writing BAM records instead
 * of SAM lines, the same bytes the device writes.  stats->sam_bytes counts record bytes.  Errors: kslam_tail_last_error(). */
kslam_status kslam_tail_sam_bam(const kslam_tail_params *params, const kslam_reads_view *reads, const kslam_index_view *index,
                                const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                                char **bam, uint64_t *len, kslam_tail_stats *stats);
kslam_status kslam_tail_finish_write_rows_bam(const kslam_tail_params *params, const kslam_reads_view *reads,
                                              const kslam_index_view *index, const kslam_overlap *overlaps, uint64_t n_overlaps,
                                              const uint32_t *cigar_pool, uint64_t n_cigar, const kslam_row_detail *details,
                                              const char *md_pool, uint64_t n_md, kslam_read_pair *read_pairs,
                                              uint64_t n_read_pairs, kslam_paired_overlap *pairs, uint64_t n_pairs,
                                              kslam_write_fn write, void *user, kslam_tail_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_BAM_H_ */
