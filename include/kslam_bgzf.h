/*
 * kslam_bgzf.h -- the SAM file as BGZF (blocked gzip: the framing bgzip and htslib write), compressed on the GPU.
 * Same library as kslam.h.
 *
 * A BGZF file is a series of gzip members of at most 65 536 bytes, each holding at most 65 280 input bytes, ended by the
 * 28-byte empty member KSLAM_BGZF_EOF.  zcat, gzip -d, Python's gzip module and htslib read it; every member can be
 * inflated on its own.  The library writes every member as ONE deflate block: fixed Huffman codes (LZ77 matches inside
 * the member), or stored when that is smaller.  With kslam_set_bgzf_deflate(ctx, KSLAM_BGZF_DEFLATE_DYNAMIC) a member may
 * also carry Huffman codes of its own (BTYPE 10), whichever of the three forms is smallest: the same matches, a smaller
 * file.  The bytes depend on the input and that mode alone.
 *
 * Use:  kslam_set_sam_bgzf(ctx, 1) before the batches: the pipelined lanes then compress the SAM text they format on the
 * device (kslam_set_sam_text) before it leaves the GPU; kslam_collect_batch returns the BGZF members in sam_text /
 * sam_text_len, with KSLAM_TEXT_SAM_BGZF in text_flags.  The per-read text stays plain.  Text formatted on the host (the
 * SAM header, a batch the device hands back without text) goes through kslam_bgzf_compress, so that the whole file is
 * BGZF; the file ends with KSLAM_BGZF_EOF.  kslam_stream_classify (kslam_stream.h) does all of this when the switch is on.
 */
#ifndef KSLAM_BGZF_H_
#define KSLAM_BGZF_H_
#include "kslam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the BGZF end-of-file marker: an empty member */
#define KSLAM_BGZF_EOF_LEN 28
#define KSLAM_BGZF_EOF                                                                                              \
  "\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00"

/* data[0 .. len) (host memory) as BGZF members, on the context's device: *out is page-locked and library-owned (hand it
 * back with kslam_free_pinned), *out_len its length.  Members of 65 280 input bytes from the start of data; len == 0
 * gives *out_len == 0.  No EOF marker is appended.  Not concurrently with another kslam_bgzf_compress on the same
 * context. */
kslam_status kslam_bgzf_compress(kslam_ctx *ctx, const void *data, uint64_t len, char **out, uint64_t *out_len);

/* on != 0: the pipelined lanes compress the device-formatted SAM text (see above).  Default off.  A context of a
 * kslam_multi gets KSLAM_ERR_UNSUPPORTED. */
kslam_status kslam_set_sam_bgzf(kslam_ctx *ctx, int on);

/* *on = the switch above */
kslam_status kslam_get_sam_bgzf(kslam_ctx *ctx, int *on);

/* How the context deflates every member it compresses: kslam_bgzf_compress, the lanes under kslam_set_sam_bgzf and
 * kslam_set_sam_bam, and what kslam_stream_classify sends through them, the header members included. */
#define KSLAM_BGZF_DEFLATE_FIXED 0   /* fixed codes (BTYPE 01), or stored when that is smaller; the default */
#define KSLAM_BGZF_DEFLATE_DYNAMIC 1 /* per member the smallest of stored, fixed and dynamic (BTYPE 10): dynamic only when
                                        strictly smaller than fixed, stored only when strictly smaller than both */
/* Any other mode: KSLAM_ERR_ARG.  A context of a kslam_multi gets KSLAM_ERR_UNSUPPORTED.  Set it between batches, never
 * while one is in flight: a batch is compressed with the mode that holds when its lane reaches the compressor. */
kslam_status kslam_set_bgzf_deflate(kslam_ctx *ctx, int mode);

/* *mode = the mode above */
kslam_status kslam_get_bgzf_deflate(kslam_ctx *ctx, int *mode);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_BGZF_H_ */
