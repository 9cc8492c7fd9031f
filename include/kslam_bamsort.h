/*
 * kslam_bamsort.h -- the SAM file as a coordinate-sorted BAM with its BAI index (SAM spec v1, sections 4.2 and 5.2): the
 * records of kslam_bam.h held on the GPU while the batches run, then sorted, moved into order, compressed and indexed there.
 * Same library as kslam.h.  Opt-in: with the switch off every output is what it is without this header.
 *
 * THE SORTED RECORD STREAM.  Input: batches, each a byte string of whole BAM records (block_size chains) as the lanes or
 * the host twins of kslam_bam.h write them -- whatever kslam_set_sam_seq, kslam_set_sam_unmapped, num_alignments and sam_xa
 * make of them -- and each with an ordinal seq: its place in submission order, 0-based, counted from switch-on or reset.
 * Output: the stable sort of all records by (refID as unsigned: -1 sorts last; pos + 1 as unsigned: pos -1 sorts in front of
 * its reference's others), ties by seq, then by position inside the batch.  That is "the records of the unsorted BAM file
 * of the same run, stably sorted by that key"; it does not depend on the number of lanes, on which lane finished first,
 * on the slice size or on whether a batch came from its lane or through kslam_bam_sort_add.
 *
 * THE FILE.  bgzf(BAM header) + bgzf(sorted record stream) + KSLAM_BGZF_EOF, where bgzf(x) are the members of 65 280 input
 * bytes cut from the start of x that kslam_bgzf_compress gives under the context's deflate mode, and the BAM header is
 * kslam_tail_bam_sort_header's: "BAM\1", the SAM header text with its sort order rewritten -- a first line that starts with
 * "@HD" gets SO:coordinate as the value of its SO: field, or "\tSO:coordinate" appended when it has none; otherwise
 * "@HD\tVN:1.0\tSO:coordinate\n" is put in front -- and the reference list, read from the text's @SQ lines (SN, LN) in their
 * order.  For kslam_sam_header's text these are the bytes of kslam_bam_header over the rewritten text.
 *
 * THE INDEX (BAI), byte-determined.  "BAI\1", n_ref, then per reference in entry order its bins, its linear index; at the end
 * n_no_coor (u64), the records with refID < 0.  For a record with refID >= 0 and pos >= 0: beg = pos, end = pos + max(1, reflen),
 * reflen = the lengths of CIGAR ops 0, 2, 3, 7, 8, counted as 0 when FLAG has 0x4 or n_cigar_op == 0; bin = reg2bin(beg, end)
 * (the stored bin field of the library's own records).  A record's start virtual offset is coffset << 16 | uoffset: coffset the
 * file offset of the member that holds the record's first byte (the header's members included), uoffset the byte's offset inside
 * that member's input.  Its end virtual offset is the start virtual offset of the byte behind it: the next record's start, for
 * the last record offset 0 of the EOF member; a position at a member's end is always written as offset 0 of the next member.
 * Per reference the bins ascend by number; a bin's chunks are the maximal runs of file-consecutive records with the same
 * (refID, bin), one chunk (start of first, end of last) per run, in file order, not merged further.  Behind the real bins comes
 * pseudo-bin 37450 with two chunks: (start of the reference's first record, end of its last), then (n_mapped: FLAG without 0x4,
 * n_unmapped).  A record with refID >= 0 and pos < 0 is counted in the pseudo-bin and lies inside its span, but enters no bin
 * and no window.  Linear index: n_intv = 1 + max((end - 1) >> 14) over the reference's records, ioffset[w] the smallest start
 * virtual offset of a record with beg >> 14 <= w <= (end - 1) >> 14; a window no record overlaps takes the value of the next
 * higher window that has one.  A reference without records has n_bin = 0 and n_intv = 0.
 *
 * LIMITS, each refused by name and leaving the state as it was.  An index entry longer than 2^29 bases: kslam_set_bam_sort
 * returns KSLAM_ERR_UNSUPPORTED (BAI cannot address it).  More than 2^32 - 1 records in one sort: kslam_bam_sort_take returns
 * KSLAM_ERR_UNSUPPORTED.  An append for which device memory cannot be had: KSLAM_ERR_OOM, the message saying how many bytes
 * are held and how many were asked for; the batches added before stay intact.  Everything is held in device memory: spilling
 * to host memory or to disk is out of scope.  A context of a kslam_multi gets KSLAM_ERR_UNSUPPORTED.
 */
#ifndef KSLAM_BAMSORT_H_
#define KSLAM_BAMSORT_H_
#include "kslam.h"
#include "kslam_bam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_TEXT_SAM_HELD 128u /* with KSLAM_TEXT_SAM_BAM: the batch's records stayed on the device (sam_text_len == 0) */

typedef struct {
  uint64_t n_records;        /* records in the file */
  uint64_t n_no_coor;        /* of them with refID < 0 */
  uint64_t record_bytes;     /* the sorted record stream */
  uint64_t compressed_bytes; /* its members (without the header's and the EOF marker) */
  uint64_t n_members;        /* of the record stream */
  uint64_t n_chunks;         /* in the index, the pseudo-bins' not counted */
  uint64_t bytes_held;       /* device memory of the store */
} kslam_bam_sort_stats;

/* on != 0: needs kslam_set_index; from then on the pipelined lanes write BAM records (as under kslam_set_sam_bam) and, instead
 * of compressing and fetching them, append them to this context's store on the device: kslam_collect_batch returns
 * sam_text_len == 0 with KSLAM_TEXT_SAM_BAM | KSLAM_TEXT_SAM_HELD in text_flags, and the batch's ordinal is its ticket counted
 * from switch-on or reset.  A batch the device leaves to the host (no KSLAM_TEXT_SAM in text_flags) is not appended: its
 * records go in through kslam_bam_sort_add.  on == 0 frees the store.  Between batches, never while one is in flight. */
kslam_status kslam_set_bam_sort(kslam_ctx *ctx, int on);

/* *on = the switch above */
kslam_status kslam_get_bam_sort(kslam_ctx *ctx, int *on);

/* One batch's records from host memory (kslam_tail_finish_write_rows_bam's output, or any whole BAM records) as ordinal seq.
 * KSLAM_ERR_ARG, before anything is launched, for: a block_size chain that does not end exactly at len, a record shorter than
 * its fixed part, read name and CIGAR, a refID >= n_ref or a record that reaches past its entry's end, a seq already present.
 * Calls are serialised and may come from any thread. */
kslam_status kslam_bam_sort_add(kslam_ctx *ctx, uint64_t seq, const void *records, uint64_t len);

/* Forgets every batch (the store's memory is kept) and starts the ordinals again at the next ticket. */
kslam_status kslam_bam_sort_reset(kslam_ctx *ctx);

/* Tuning knobs that change no byte; 0 restores the default.  slice: the bytes of the sorted stream gathered and compressed at
 * a time, rounded down to whole members of 65 280 bytes, at least one (default: 16 448 members, about 1 GiB).  segment: the
 * records per walk segment of kslam_bam_sort_add's record index (default 64).  gather: the lanes that copy one record -- 16 or
 * 64, or 1: the one-thread-per-record baseline (default: by the mean record length). */
kslam_status kslam_bam_sort_set_slice(kslam_ctx *ctx, uint64_t bytes);
kslam_status kslam_bam_sort_set_segment(kslam_ctx *ctx, uint32_t records);
kslam_status kslam_bam_sort_set_gather(kslam_ctx *ctx, uint32_t lanes);

/* Device time by events, in ms: ms[0] the last append (kslam_bam_sort_add's, or a lane's), then of the last take ms[1] sort,
 * ms[2] gather, ms[3] compress, ms[4] index. */
kslam_status kslam_bam_sort_kernel_ms(kslam_ctx *ctx, double ms[5]);

/* Waits for the lanes, orders the batches by seq (KSLAM_ERR_STATE when an ordinal is missing), sorts, and per slice gathers the
 * records into sorted order, compresses them and hands the members to write_bam: the whole file as defined above, sam_header
 * [0 .. len) being the SAM header text.  Then the index to write_bai (NULL: no index).  Repeatable; more batches may follow. */
kslam_status kslam_bam_sort_take(kslam_ctx *ctx, const char *sam_header, uint64_t len, kslam_write_fn write_bam, void *user_bam,
                                 kslam_write_fn write_bai, void *user_bai, kslam_bam_sort_stats *stats);

/* For the NEXT kslam_stream_classify on ctx alone (kslam_stream.h), like the other stream setters: on != 0 makes the file on
 * sam_fd (which the call then needs: KSLAM_ERR_ARG without) the coordinate-sorted BAM, whatever kslam_set_sam_bam says, and
 * bai_fd >= 0 receives its index (-1: none).  The call switches the sort on and resets it; the lanes hold their batches, the
 * batches formatted on the host go in through kslam_bam_sort_add with their ordinal; nothing is written to sam_fd or bai_fd until
 * the last batch is in.  Then the whole file and the index are written, in front of the other report files, and the sort is
 * switched off.  A call that fails in a batch leaves both descriptors empty.  stats->sam_bytes counts the record members'
 * compressed bytes. */
kslam_status kslam_stream_set_bam_sort(kslam_ctx *ctx, int on, int bai_fd);
kslam_status kslam_stream_get_bam_sort(kslam_ctx *ctx, int *on, int *bai_fd);

/* Host twins (no GPU); errors: kslam_tail_last_error(), results malloc'ed (kslam_free).
 * kslam_tail_bam_sort_header: the BAM header of the sorted file, uncompressed (see THE FILE).
 * kslam_tail_bam_sort: the batches' bytes in seq order -> the sorted record stream.
 * kslam_tail_bai: the sorted record stream, n_ref, the compressed size of every record member and the compressed length of the
 * header's members -> the BAI bytes. */
kslam_status kslam_tail_bam_sort_header(const char *sam_header, uint64_t len, char **out, uint64_t *out_len);
kslam_status kslam_tail_bam_sort(const char *const *batches, const uint64_t *lens, uint64_t n_batches, char **out, uint64_t *out_len);
kslam_status kslam_tail_bai(const char *stream, uint64_t len, uint32_t n_ref, const uint32_t *member_sizes, uint64_t n_members,
                            uint64_t header_compressed_len, char **out, uint64_t *out_len);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_BAMSORT_H_ */
