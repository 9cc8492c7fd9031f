/*
 * kslam_inflate.h -- BGZF-compressed input (the .fastq.gz that bgzip, htslib and most pipelines write), inflated on the
 * GPU.  Same library as kslam.h; the counterpart of kslam_bgzf.h.
 *
 * A BGZF file is a series of independent gzip members of at most 65 536 bytes, each inflating to at most 65 536 bytes.
 * Every member is inflated by one wavefront (csrc/inflate.hip): RFC 1951 in full -- stored, fixed and dynamic Huffman
 * blocks, any number of blocks per member, distances up to 32 768 -- straight to the member's place in the text, and
 * checked against the member's ISIZE and CRC-32.  The library links no zlib.
 *
 * Use:  if (kslam_bgzf_is_gzip(data, len)) kslam_bgzf_inflate(ctx, data, len, &text, &text_len);  then hand the text to
 * whatever took plain text before (kslam_stream_classify, kslam_submit_batch_fastq_text), and kslam_free_pinned it.
 * A gzip stream that is not BGZF is refused (KSLAM_ERR_UNSUPPORTED): its members cannot be found without inflating it
 * serially; `bgzip` re-blocks such a file.
 */
#ifndef KSLAM_INFLATE_H_
#define KSLAM_INFLATE_H_
#include "kslam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when data starts with the gzip magic 1f 8b, else 0.  Host only. */
int kslam_bgzf_is_gzip(const void *data, uint64_t len);

/* Walks the members of data[0 .. len) by htslib's rule (1f 8b 08, FLG 4, XLEN 6, 'B' 'C', SLEN 2, BSIZE):
 * *n_members = their number (empty members and the EOF marker included), *text_len = the sum of their ISIZE fields.
 * Host only, needs no context; inflates nothing.  An empty input, empty members anywhere and a missing EOF marker are
 * accepted.  KSLAM_ERR_ARG: a truncated last member, a BSIZE that runs past len or is too small for a member, an ISIZE
 * above 65 536 -- the message names the member and its byte offset.  KSLAM_ERR_UNSUPPORTED: gzip without the 'BC' field
 * (plain gzip).  Messages: kslam_tail_last_error(). */
kslam_status kslam_bgzf_scan(const void *data, uint64_t len, uint64_t *n_members, uint64_t *text_len);

/* data[0 .. len) (host memory, BGZF) inflated on the context's device: *out is page-locked and library-owned (hand it back
 * with kslam_free_pinned), *out_len its length.  Works in rounds of KSLAM_INFLATE_ROUND members (environment, read once
 * per process; default 4096), so the device scratch does not grow with the file.  A file the scan refuses returns the
 * scan's status.  A member that does not inflate to its ISIZE and CRC-32 returns KSLAM_ERR_ARG, with the member's index,
 * its byte offset and the kind of error in kslam_last_error(ctx): "bad block type", "stored length check",
 * "code lengths over-subscribed", "code lengths incomplete", "invalid symbol", "distance too far back", "output overrun",
 * "output underrun", "CRC mismatch", "deflate data length".  On any error *out is NULL: partial text is never returned.
 * Not concurrently with another kslam_bgzf_inflate on the same context. */
kslam_status kslam_bgzf_inflate(kslam_ctx *ctx, const void *data, uint64_t len, char **out, uint64_t *out_len);

/* *ms = the device time of the inflate kernels of the last kslam_bgzf_inflate on this context, summed over its rounds
 * (events around each launch; the copies are not in it).  For measurements (tools/inflate_bench.py). */
kslam_status kslam_bgzf_inflate_kernel_ms(kslam_ctx *ctx, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_INFLATE_H_ */
