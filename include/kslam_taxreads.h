/*
 * kslam_taxreads.h -- the reads of chosen taxa, written back out as FASTQ: KrakenTools' extract_kraken_reads.py
 * (-t ... --include-children / --include-parents / --exclude) without a second pass over the input, selected on the GPU where
 * the taxonomy ids are made (csrc/taxreads.hip).  Same library as kslam.h.
 *
 * Off by default; with the switch off every byte of every output and every kernel is what it was.  With it on:
 *   input          per batch: the records the batch consumed, its FINAL read pairs and the taxonomy id of each read pair -- the
 *                  tax_ids that kslam_collect_batch / kslam_sam_text / kslam_tail_classify return.
 *   chosen ids     a list of n >= 1 taxonomy ids.  Duplicates are allowed.  Id 0 is KSLAM_ERR_ARG ("no taxon" is the job of
 *                  --unclassified-out, include/kslam_readsplit.h).  Ids the tree does not know are legal.
 *   set S          starts as the chosen ids.
 *                  With KSLAM_TAXREADS_CHILDREN: also every id in the CLADE of a chosen id, exactly as include/kslam_kreport.h
 *                  defines clade: every node from which following `up` reaches the chosen id's node.  For chosen id 1, the
 *                  synthetic root, that is every non-zero id, including ids the tree does not know.  An unknown chosen id has
 *                  no children.
 *                  With KSLAM_TAXREADS_PARENTS: also every node on the `up` path from each chosen known id, and always id 1.
 *                  `up` stops below the root (kslam_taxonomy.h: "a parent id of 1 ends it"), so id 1 is added by rule and not by
 *                  walking.  An unknown chosen id adds only id 1.
 *   matched        a read pair is matched when its id is non-zero and in S.  A read pair whose id the tree does not know is
 *                  therefore matched only when that id is itself chosen, or when id 1 is chosen with CHILDREN.
 *   selected       without KSLAM_TAXREADS_EXCLUDE: the records of the matched read pairs (single-end: reads).  With it: every
 *                  record the batch consumed that does NOT belong to a matched pair; reads without any alignment are therefore
 *                  included.  This is KrakenTools' rule, and it is what decontamination wants.
 *   streams        two byte streams, selected R1 and selected R2 (single-end: R1 only).  Records keep input order; the k-th
 *                  records of the two streams are mates.
 *   record bytes   exactly those of include/kslam_readsplit.h: the four lines as the reader's line rule delimits them, each
 *                  followed by ONE "\n" (LF normalisation, the unterminated last record, the end-of-stream empty line).
 *   BGZF           with kslam_set_reads_out_bgzf on, each stream of each batch is compressed on the device into BGZF members
 *                  (kslam_set_bgzf_deflate applies).  An empty stream gives no member.  A file is its batches' members plus
 *                  KSLAM_BGZF_EOF.
 *   cross-property with CHILDREN, and with neither PARENTS nor EXCLUDE, the number of read pairs selected for ONE chosen id
 *                  over a run equals that id's clade count in kslam_kreport_take for the same run (for chosen id 1: the
 *                  synthetic root's clade, the sum of all direct counts).
 *
 * Example, on the tree and the ids of the example in include/kslam_kreport.h (1; 131567 -> 1; 2 -> 131567; 1224 -> 2;
 * 562 -> 1224; 83333 -> 562; 10239 -> 1; 10760 -> 10239).  Ten read pairs carry the ids 562 x 3, 83333 x 2, 2, 10760, 999999 and
 * 0 x 2:
 *    chosen   mode                   selected pairs
 *    562      -                      3
 *    562      CHILDREN               5
 *    562      PARENTS                4   (S = 562, 1224, 2, 131567, 1)
 *    562      CHILDREN | PARENTS     6
 *    2        CHILDREN               6
 *    10239    CHILDREN               1
 *    999999   CHILDREN               1
 *    1        CHILDREN               8
 *    562      CHILDREN | EXCLUDE     5, among them the two pairs with id 0
 * (tests/golden/taxreads_small.json holds the bytes.)
 *
 * The state -- the chosen ids, the id -> node table (the tree's ids sorted ascending with their nodes), one mask byte per node
 * (1: the node's id is in S) and the sorted list of the chosen ids the tree does not know -- is built once per
 * kslam_set_taxon_reads, belongs to the context the call was made on and is read by its lanes.  Per batch the device runs one
 * flag pass over the read pairs and the length pass, scans and streaming copy of the reads split; only the selected bytes cross
 * to the host.
 */
#ifndef KSLAM_TAXREADS_H_
#define KSLAM_TAXREADS_H_
#include "kslam.h"
#include "kslam_readsplit.h"
#include "kslam_taxonomy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_TAXREADS_CHILDREN 1u
#define KSLAM_TAXREADS_PARENTS 2u
#define KSLAM_TAXREADS_EXCLUDE 4u

/* Chooses the taxa and builds S on the device.  n == 0 switches the selection off and frees the state (ids may be NULL, mode
 * is not looked at).  KSLAM_ERR_ARG: an id of 0, mode bits above 7, ids == NULL with n > 0.  It needs annotations that hold a
 * tree (kslam_set_sam_annotations with a taxdb) and the device pairing (kslam_set_pairing with stages != 0), else
 * KSLAM_ERR_STATE.  A context of a kslam_multi gets KSLAM_ERR_UNSUPPORTED.  The state is freed, and the switch goes off, where
 * the Kraken-style report's does: kslam_set_sam_annotations, kslam_set_index, kslam_destroy.  Set it between batches. */
kslam_status kslam_set_taxon_reads(kslam_ctx *ctx, const uint32_t *ids, uint64_t n, uint32_t mode);
/* the chosen ids as they were set (*ids: malloc'ed, kslam_free; NULL and *n == 0 with the switch off) and the mode */
kslam_status kslam_get_taxon_reads(kslam_ctx *ctx, uint32_t **ids, uint64_t *n, uint32_t *mode);

/* The selected streams of the batch `ticket`, once, after kslam_collect_batch of that ticket.  out->data[0] / data[1] are the
 * selected R1 / R2 records, data[2] and data[3] are NULL; n_records[0] counts the selected records of a stream and
 * n_records[1] the others.  The lanes select a batch when the switch is on, the batch came through
 * kslam_submit_batch_fastq_text and the per-read stage made its ids on the device (kslam_set_sam_text with want_per_read).  A
 * batch whose ids are made on the host (pseudo-assembly left to the host, no per-read stage) comes back with
 * KSLAM_READS_OUT_LEFT_TO_HOST and no data: run kslam_tail_taxon_reads on it.  A batch submitted any other way than as FASTQ
 * text gets KSLAM_ERR_UNSUPPORTED; a ticket collected with the switch off, or taken already, KSLAM_ERR_STATE.  The library
 * keeps the streams of at most 16 collected batches.  Hand the blocks back with kslam_release_reads_out. */
kslam_status kslam_collect_taxon_reads(kslam_ctx *ctx, uint64_t ticket, kslam_reads_out *out);

/* Host twin (no GPU): the same plain bytes from host text, the tree through the public kslam_taxdb_* accessors.  r1 / r2,
 * max_pairs and at_eof as for kslam_tail_split_reads; pair_tax_ids[g] is the id of read_pairs[g].  n == 0, an id of 0 and
 * mode bits above 7 are KSLAM_ERR_ARG.  out as above, with KSLAM_READS_OUT_HOST_MEMORY.  Errors: kslam_tail_last_error(). */
kslam_status kslam_tail_taxon_reads(const kslam_taxdb *taxdb, const uint32_t *ids, uint64_t n, uint32_t mode, const char *r1, uint64_t len1,
                                    const char *r2, uint64_t len2, uint64_t max_pairs, int at_eof, const kslam_read_pair *read_pairs,
                                    const uint32_t *pair_tax_ids, uint64_t n_read_pairs, kslam_reads_out *out);

/* The selection on THIS context, without the lanes (tests, tools/taxreads_bench.py): uploads the texts, indexes them on the
 * device, flags by read_pairs and pair_tax_ids (host memory) with the S of kslam_set_taxon_reads and copies, honouring
 * kslam_set_reads_out_bgzf and kslam_set_bgzf_deflate.  Blocks are page-locked.  KSLAM_ERR_STATE with the switch off. */
kslam_status kslam_taxon_reads_text(kslam_ctx *ctx, const char *r1, uint64_t len1, const char *r2, uint64_t len2, uint64_t max_pairs,
                                    int at_eof, const kslam_read_pair *read_pairs, const uint32_t *pair_tax_ids, uint64_t n_read_pairs,
                                    kslam_reads_out *out);

/* The device-built S, copied to the host: *mask has one byte per node of the tree (1: the node's id is in S), *unknown_ids the
 * chosen ids the tree does not know, ascending and distinct (with PARENTS and a tree without a node for id 1 that includes id
 * 1), *all_nonzero is 1 when id 1 was chosen with CHILDREN.  Both arrays are malloc'ed (kslam_free). */
kslam_status kslam_taxon_reads_mask(kslam_ctx *ctx, uint8_t **mask, uint64_t *n_nodes, uint32_t **unknown_ids, uint64_t *n_unknown,
                                    int *all_nonzero);

/* device time (ms), by events around the launches: the mask pass of the last kslam_set_taxon_reads, and the flag pass and the
 * lengths + scans + copy of the last kslam_taxon_reads_text on this context (the lanes' times are not gathered); bytes_moved:
 * the text bytes that copy read plus wrote */
kslam_status kslam_taxon_reads_kernel_ms(kslam_ctx *ctx, double *mask_ms, double *flag_ms, double *copy_ms, uint64_t *bytes_moved);

/* kslam_stream_classify (kslam_stream.h) writes the streams itself: fds[0] / fds[1] are the open descriptors for the selected
 * R1 / R2 records (-1: not wanted; fds == NULL: none).  It holds for the NEXT call alone.  The chosen ids and the mode are those
 * set with kslam_set_taxon_reads before that call, which sets them again behind its own kslam_set_sam_annotations, writes each
 * batch's blocks in batch order on the host stage's thread, runs kslam_tail_taxon_reads after kslam_tail_classify for every
 * batch that arrives KSLAM_READS_OUT_LEFT_TO_HOST, ends the files with KSLAM_BGZF_EOF under kslam_set_reads_out_bgzf and
 * switches the selection off when it returns.  Without a taxdb, or without chosen ids, that call returns KSLAM_ERR_STATE. */
kslam_status kslam_stream_set_taxon_reads(kslam_ctx *ctx, const int fds[2]);
kslam_status kslam_stream_get_taxon_reads(kslam_ctx *ctx, int fds[2]);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_TAXREADS_H_ */
