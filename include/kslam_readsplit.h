/*
 * kslam_readsplit.h -- the reads themselves, split by outcome: classified and unclassified records written back out as FASTQ
 * (Kraken 2's --classified-out / --unclassified-out), cut out of the uploaded text on the GPU (csrc/readsplit.hip).  Same library
 * as kslam.h.
 *
 * Off by default; with the switch off every byte of every output is what it was.  With it on:
 *   classified     a read pair (single-end: a read) of a batch is classified when it appears in that batch's final read_pairs:
 *                  at least one alignment pair survives every stage the run has switched on.  It is the set that gets a
 *                  _PerRead line; with --just-align the same set, read as "aligned".  Every other record taken into the batch
 *                  is unclassified.
 *   streams        up to four byte streams per batch, in this order: classified R1, classified R2, unclassified R1,
 *                  unclassified R2 (single-end: the two R1 streams only).  Records keep input order; the k-th record of an R1
 *                  stream and of its R2 stream are mates.
 *   record bytes   the content of the record's four lines as the reader's line rule delimits them ("\n", "\r\n", a lone "\r",
 *                  and the one empty line read at the true end of a stream: host/fastq.cpp), each followed by ONE "\n".  An
 *                  LF-terminated file comes out verbatim, header comments and "/1" included; CR and CRLF are normalised to LF;
 *                  an unterminated last record gains its "\n"; a record completed by the end-of-stream empty line gets an empty
 *                  fourth line.  Nothing is validated beyond what the reader validates (no "@" / "+" check).
 *   partition      classified and unclassified are disjoint, and merged back by record number they are exactly the records the
 *                  batch consumed (kslam_batch_result.consumed1 / consumed2).
 *   BGZF           with kslam_set_reads_out_bgzf on, each stream of each batch is compressed on the device into members of at
 *                  most 65 280 input bytes (include/kslam_bgzf.h; kslam_set_bgzf_deflate applies).  A file is then its batches'
 *                  members plus KSLAM_BGZF_EOF.  An empty stream gives no member.
 *
 * The switch is honoured for batches submitted with kslam_submit_batch_fastq_text -- what kslam_stream_classify and SLAM use,
 * and the only route on which the text and its line index are on the device.  Per batch the device runs one flag pass over the
 * read pairs, one pass over the record index for the output lengths, two scans per stream and one streaming copy; only the
 * bytes asked for cross to the host.
 */
#ifndef KSLAM_READSPLIT_H_
#define KSLAM_READSPLIT_H_
#include "kslam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_READS_OUT_CLASSIFIED 1u
#define KSLAM_READS_OUT_UNCLASSIFIED 2u

/* kslam_reads_out.flags */
#define KSLAM_READS_OUT_BGZF 1u         /* data[] hold BGZF members, not plain text */
#define KSLAM_READS_OUT_LEFT_TO_HOST 2u /* nothing was written: the device left the batch's pseudo-assembly to the host
                                           (pair_stats.stages_done lacks KSLAM_TAIL_PSEUDO_ASM), so its final read_pairs exist
                                           only after the host stage; run kslam_tail_split_reads on them */
#define KSLAM_READS_OUT_HOST_MEMORY 4u  /* data[] are malloc'ed (kslam_tail_split_reads), not page-locked */

typedef struct {
  char *data[4];         /* classified R1, classified R2, unclassified R1, unclassified R2; NULL for a stream not asked for */
  uint64_t len[4];       /* their lengths in bytes (compressed bytes with KSLAM_READS_OUT_BGZF) */
  uint64_t n_records[2]; /* records per classified stream, records per unclassified stream (counted whether or not asked for) */
  uint32_t flags;        /* KSLAM_READS_OUT_* flag bits above */
  uint32_t pad_;
} kslam_reads_out;

/* which: a mask of KSLAM_READS_OUT_CLASSIFIED | KSLAM_READS_OUT_UNCLASSIFIED; 0 switches the split off (the default).  A mask
 * above 3 is KSLAM_ERR_ARG.  A non-zero mask needs the device pairing (kslam_set_pairing with stages != 0), else
 * KSLAM_ERR_STATE.  Set it between batches.  A context of a kslam_multi gets KSLAM_ERR_UNSUPPORTED, as from kslam_set_sam_bam. */
kslam_status kslam_set_reads_out(kslam_ctx *ctx, uint32_t which);
kslam_status kslam_get_reads_out(kslam_ctx *ctx, uint32_t *which);

/* on != 0: every stream of every batch leaves the device as BGZF members.  Default off. */
kslam_status kslam_set_reads_out_bgzf(kslam_ctx *ctx, int on);
kslam_status kslam_get_reads_out_bgzf(kslam_ctx *ctx, int *on);

/* The streams of the batch `ticket`, once, after kslam_collect_batch of that ticket (and before its kslam_release_batch, by
 * convention: the two results belong together).  The blocks are page-locked and library-owned; hand them back with
 * kslam_release_reads_out.  A batch submitted any other way than kslam_submit_batch_fastq_text gets KSLAM_ERR_UNSUPPORTED with
 * a message; the batch itself is unaffected.  A ticket that was collected with the switch off, or whose streams were taken
 * already: KSLAM_ERR_STATE.  The library keeps the streams of at most 16 collected batches; older ones nobody asked for are
 * dropped. */
kslam_status kslam_collect_reads_out(kslam_ctx *ctx, uint64_t ticket, kslam_reads_out *out);

/* hands the blocks back (either kind: KSLAM_READS_OUT_HOST_MEMORY says which) and zeroes *out; ctx may be NULL for host memory */
void kslam_release_reads_out(kslam_ctx *ctx, kslam_reads_out *out);

/* Host twin (no GPU): the same plain bytes from host text.  r1 / r2, max_pairs and at_eof as for
 * kslam_submit_batch_fastq_text (r2 == NULL and len2 == 0: single-end); read_pairs: the batch's final read pairs (block layout
 * [R1 | R2]: r2_read == r1_read + the number of pairs).  For a batch flagged KSLAM_READS_OUT_LEFT_TO_HOST, and for a host
 * that formats everything itself.  With BGZF wanted, send each block through kslam_bgzf_compress: both routes then write the
 * same file.  out->data[] are malloc'ed; release with kslam_release_reads_out.  Errors: kslam_tail_last_error(). */
kslam_status kslam_tail_split_reads(const char *r1, uint64_t len1, const char *r2, uint64_t len2, uint64_t max_pairs, int at_eof,
                                    const kslam_read_pair *read_pairs, uint64_t n_read_pairs, uint32_t which,
                                    kslam_reads_out *out);

/* kslam_stream_classify (kslam_stream.h) writes the streams itself: fds[k] is the open descriptor for stream k of
 * kslam_reads_out.data, or -1 for a stream that is not wanted.  Call it before kslam_stream_classify; it holds for the NEXT call
 * alone, which switches the split on for its batches (and off again), writes each batch's blocks in batch order -- on the host
 * stage's thread, not through the SAM writer's queue -- and, with kslam_set_reads_out_bgzf on, ends every file with
 * KSLAM_BGZF_EOF.  A failing write() fails the call.  fds == NULL: none. */
kslam_status kslam_stream_set_reads_out(kslam_ctx *ctx, const int fds[4]);
kslam_status kslam_stream_get_reads_out(kslam_ctx *ctx, int fds[4]);

/* device time (ms) of the last batch's flag, scan and copy kernels on this context, by events around their launches, and the
 * text bytes the copy read plus wrote (tools/readsplit_bench.py); the resident twin below fills them */
kslam_status kslam_reads_out_kernel_ms(kslam_ctx *ctx, double *ms, uint64_t *bytes_moved);

/* The split on THIS context, without the lanes (tests, tools/readsplit_bench.py): uploads the two texts, indexes them on the
 * device and splits by read_pairs (host memory), honouring kslam_set_reads_out_bgzf and kslam_set_bgzf_deflate.  Blocks are
 * page-locked. */
kslam_status kslam_split_reads_text(kslam_ctx *ctx, const char *r1, uint64_t len1, const char *r2, uint64_t len2,
                                    uint64_t max_pairs, int at_eof, const kslam_read_pair *read_pairs, uint64_t n_read_pairs,
                                    uint32_t which, kslam_reads_out *out);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_READSPLIT_H_ */
