/*
 * kslam_gunzip.h -- plain gzip input (RFC 1952: what gzip, pigz, the sequencers' converters, SRA downloads and
 * `cat a.gz b.gz` write), inflated in parallel on the GPU.  Same library as kslam.h; the counterpart of kslam_inflate.h,
 * which reads BGZF only and is not changed by this header.
 *
 * The blocks of a plain gzip file cannot be located without inflating it.  The file is therefore cut into chunks of
 * compressed bytes, and (csrc/gunzip.hip)
 *   1 find     every chunk but the first is searched, bit by bit, for a deflate block header (the rule is below);
 *   2 count    from every start found, and from the first member's first block, one wavefront decodes lengths only until a
 *              block of its ends exactly on a later start; the host then follows these links from the file's first block:
 *              the starts on that chain are live, every other one was false and is dropped;
 *   3 decode   one wavefront per live start decodes into 16-bit symbols, in which a match that reaches before the start
 *              is a marker into the 32 KiB of text before it;
 *   4 window   one workgroup resolves the last 32 768 symbols of each live stretch in order, so that the text before
 *              every start is final;
 *   5 resolve  all other symbols become bytes;
 *   6 check    CRC-32 and ISIZE of every member against its trailer; the text goes to page-locked memory.
 * Stages 3 to 6 run in rounds, so the device scratch does not grow with the text.
 *
 * THE FINDER'S RULE.  The start of chunk k (k >= 1; its bytes are [k * chunk, (k + 1) * chunk) of the file) is the LOWEST bit
 * offset p inside the chunk at which all of this holds: BFINAL = 0, BTYPE = 2 (dynamic Huffman), HLIT <= 29, HDIST <= 29, the
 * code-length code is complete, the code lengths decode without error, the end-of-block symbol has a code, and both codes
 * are neither over-subscribed nor incomplete (zlib's rule) -- and none of it reads a bit past the end of the file.  A
 * chunk without such an offset has no start and is decoded by the wave of its predecessor.
 *
 * LIMITS.  Stored and fixed blocks are never starts: a file made only of them (gzip -1 of short inputs, level 0) is decoded
 * by ONE wavefront, which is correct and slow; so is a BGZF file whose members are one final block each (kslam_bgzf_inflate
 * is the path for those).  One wavefront addresses at most 2^32 bits: deflate data that goes on for more than 512 MiB
 * without a start that a wave could be started on gives KSLAM_ERR_UNSUPPORTED.  A stretch of text between two live starts that is
 * longer than the round (kslam_gunzip_set_round) raises the round to its length for that call.
 */
#ifndef KSLAM_GUNZIP_H_
#define KSLAM_GUNZIP_H_
#include "kslam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_GUNZIP_CHUNK_DEFAULT (32u * 1024u)         /* compressed bytes per chunk: the measured best (profiles/gunzip.json) */
#define KSLAM_GUNZIP_CHUNK_MIN 1024u
#define KSLAM_GUNZIP_ROUND_DEFAULT (256u * 1024u * 1024u) /* symbols (= text bytes) per round: 768 MiB of scratch */

typedef struct kslam_gunzip_stats {
  uint64_t members;         /* gzip members, empty ones included */
  uint64_t chunks;          /* ceil(len / chunk) */
  uint64_t starts_found;    /* chunks in which the finder's rule held somewhere */
  uint64_t starts_live;     /* of those, the ones on the chain: true block starts */
  uint64_t starts_dropped;  /* found - live: false starts */
  uint64_t rounds;
  uint64_t text_len;
  double find_ms, count_ms, decode_ms, window_ms, resolve_ms, check_ms;   /* device time of each stage, summed over the rounds */
} kslam_gunzip_stats;

/* The RFC 1952 member header at data[0 .. len): *deflate_at = the offset of the member's deflate data (10 without optional
 * fields; FEXTRA, FNAME, FCOMMENT and FHCRC are walked over).  Host only, needs no context.  KSLAM_ERR_ARG with
 * "not a gzip member" (fewer than 2 bytes, or no magic 1f 8b) or "gzip header" (the header is cut short, the method is not
 * 8, a reserved FLG bit is set) in kslam_tail_last_error(). */
kslam_status kslam_gunzip_header(const void *data, uint64_t len, uint64_t *deflate_at);

/* data[0 .. len) (host memory, any RFC 1952 file: one member or many, optional header fields, BGZF included) inflated on
 * the context's device: *out is page-locked and library-owned (hand it back with kslam_free_pinned), *out_len its length.
 * Which files are accepted is Python's gzip.decompress: members follow each other, zero bytes behind a member are
 * skipped, anything else behind a member is refused; an empty input gives an empty text.  Stricter than it in one point:
 * reserved FLG bits are refused.  On any error *out is NULL -- partial text is never returned -- and kslam_last_error(ctx)
 * names the member, the byte offset of its header and the kind: those of kslam_bgzf_inflate (kslam_inflate.h), "gzip header" and
 * "not a gzip member"; status KSLAM_ERR_ARG, or KSLAM_ERR_UNSUPPORTED for the 2^32-bit limit above.  Not concurrently with
 * another call on the same context. */
kslam_status kslam_gunzip_inflate(kslam_ctx *ctx, const void *data, uint64_t len, char **out, uint64_t *out_len);

/* Compressed bytes per chunk for the calls that follow on this context: a multiple of 4, at least KSLAM_GUNZIP_CHUNK_MIN, at
 * most 2^28; anything else is KSLAM_ERR_ARG.  0 restores the default.  Changes the speed and the stats, never the text. */
kslam_status kslam_gunzip_set_chunk(kslam_ctx *ctx, uint64_t bytes);

/* Symbols of scratch per round (one symbol per text byte; the device holds 3 bytes per symbol): at least the chunk size in
 * force, else KSLAM_ERR_ARG.  0 restores the default. */
kslam_status kslam_gunzip_set_round(kslam_ctx *ctx, uint64_t symbols);

/* The figures of the last kslam_gunzip_inflate on this context that got as far as its text (all zero before the first). */
kslam_status kslam_gunzip_last_stats(kslam_ctx *ctx, kslam_gunzip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_GUNZIP_H_ */
