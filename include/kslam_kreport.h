/*
 * kslam_kreport.h -- a Kraken-style report (the six-column table Bracken, Pavian, Krona's importers and MultiQC read: percent,
 * clade reads, direct reads, rank code, taxonomy id, indented name), counted per taxon on the GPU from the taxonomy ids the
 * lanes make (csrc/kreport.hip).  Same library as kslam.h.
 *
 * Off by default; with the switch off every byte of every output is what it was.  With it on:
 *   input         per batch, the taxonomy id per read pair of the batch's FINAL read pairs: the tax_ids that kslam_collect_batch /
 *                 kslam_sam_text / kslam_tail_classify return.  An id of 0 contributes nothing (that covers the groups with
 *                 count == 0); every other id adds one to that id's DIRECT count.  The _abbreviated file's quirk of dropping one
 *                 record when nothing is unclassified (kslam_taxonomy_summary) is deliberately not reproduced: every read pair counts.
 *   tree          the dense forest of kslam_taxdb_dense.  Nodes past kslam_taxdb_size (parents the file never defines) are
 *                 ordinary nodes with empty name and rank.  An id the tree does not know (kslam_taxdb_node gives 0xFFFFFFFF) is
 *                 treated as a top-level node of its own with empty name and rank.
 *   clade         the clade count of a node is its direct count plus the direct counts of all nodes below it, following `up`.
 *                 A synthetic ROOT row (taxonomy id 1) is the parent of every top-level node (up == none) and of every unknown
 *                 id; its name is that of the tree's node for id 1 if there is one, else "root".  Root's clade is the sum of all
 *                 direct counts, root's direct count is the direct count of id 1: the tree's own node for id 1, if present, is
 *                 folded into the root row and is not listed again (nor is id 1 when the tree does not know it).
 *   rows          (kslam_kreport_take) one row per node or unknown id with clade > 0: {tax_id, node (0xFFFFFFFF for an unknown
 *                 id), direct, clade} with 64-bit counts.  Known nodes first, in ascending node order; unknown ids follow in
 *                 ascending id order.  The synthetic root is not a row: the writer makes it.
 *   file          (kslam_kreport_write) one line per row plus the `unclassified` and root lines:
 *                   pct \t clade \t direct \t code \t taxid \t indent name \n
 *                 pct is "%6.2f" of 100.0 * clade / total in double; total is the run's read pairs (n_pairs of the stream's
 *                 statistics, what _abbreviated divides by).  First line, written only when its count is greater than 0:
 *                 unclassified = total - sum of direct, with code U, id 0 and no indent.  total smaller than that sum is
 *                 KSLAM_ERR_ARG, returned before anything is written.  Then root at indent 0, then depth-first order; a node's
 *                 children are ordered by clade descending, ties by taxonomy id ascending; indent is two spaces per level (root
 *                 is level 0); lines with clade 0 are not written.
 *   rank code     Kraken 2's rule: root is R; a node whose rank text is exactly superkingdom or domain takes D, kingdom K,
 *                 phylum P, class C, order O, family F, genus G, species S; any other rank inherits its parent's letter with
 *                 the parent's number + 1 appended (R1, S1, S2; a number of 0 is not printed).
 *   determinism   every accumulator is an integer add, so the rows do not depend on the number of lanes, on the order of the
 *                 batches, on whether a batch was counted by its lane or handed in through kslam_kreport_add, or on how often
 *                 take was called; they equal kslam_tail_kreport on the same ids, field for field.
 *
 * Example: a taxDB of 1 (parent 1, "root", no rank), 131567 (1, "cellular organisms", no rank), 2 (131567, "Bacteria",
 * superkingdom), 1224 (2, "Proteobacteria", phylum), 562 (1224, "Escherichia coli", species), 83333 (562, "Escherichia coli K-12",
 * strain), 10239 (1, "Viruses", superkingdom), 10760 (10239, "Escherichia phage T7", species); ids 562 x 3, 83333 x 2, 2, 10760,
 * 999999 and 0 x 2; total 10 (tabs shown as " | "):
 *    20.00 | 2 | 2 | U  | 0      | unclassified
 *    80.00 | 8 | 0 | R  | 1      | root
 *    60.00 | 6 | 0 | R1 | 131567 |   cellular organisms
 *    60.00 | 6 | 1 | D  | 2      |     Bacteria
 *    50.00 | 5 | 0 | P  | 1224   |       Proteobacteria
 *    50.00 | 5 | 3 | S  | 562    |         Escherichia coli
 *    20.00 | 2 | 2 | S1 | 83333  |           Escherichia coli K-12
 *    10.00 | 1 | 0 | D  | 10239  |   Viruses
 *    10.00 | 1 | 1 | S  | 10760  |     Escherichia phage T7
 *    10.00 | 1 | 1 | R1 | 999999 |   (two spaces of indent, an empty name)
 * (tests/golden/kreport_small.json holds the bytes.)
 *
 * The state -- one 64-bit direct counter per node, the id -> node table (the tree's ids sorted ascending with their nodes) and
 * a list of (id, count) items for unknown ids, which grows by at most 8 bytes per read pair with an unknown id -- belongs to the
 * context the switch was set on and is shared by its lanes; it is zeroed at switch-on and by kslam_kreport_reset and freed at
 * switch-off, by kslam_set_sam_annotations and kslam_set_index (they replace the device tree) and by kslam_destroy.
 */
#ifndef KSLAM_KREPORT_H_
#define KSLAM_KREPORT_H_
#include "kslam.h"
#include "kslam_taxonomy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_KREPORT_NO_NODE 0xFFFFFFFFu

typedef struct {
  uint32_t tax_id;
  uint32_t node;     /* the tree's node, KSLAM_KREPORT_NO_NODE for an id the tree does not know */
  uint64_t direct;
  uint64_t clade;
} kslam_kreport_row;

typedef struct {
  uint64_t n_ids;          /* non-zero ids counted */
  uint64_t n_unknown_ids;  /* distinct ids the tree does not know */
  uint64_t n_rows;
} kslam_kreport_stats;

/* on != 0: a lane counts every batch whose taxonomy ids it computed itself (the per-read stage ran for it: kslam_set_sam_text
 * with want_per_read); the ids of every other batch are made on the host: hand them to kslam_kreport_add.  Needs annotations
 * that hold a tree (kslam_set_sam_annotations with a taxdb), else KSLAM_ERR_STATE.  Switching on allocates and zeroes the state
 * (on when already on: nothing happens); off frees it.  Set it between batches.  A context of a kslam_multi gets
 * KSLAM_ERR_UNSUPPORTED, as from kslam_set_coverage. */
kslam_status kslam_set_kreport(kslam_ctx *ctx, int on);
kslam_status kslam_get_kreport(kslam_ctx *ctx, int *on);

/* zeroes the counters and empties the list of unknown ids; KSLAM_ERR_STATE with the switch off */
kslam_status kslam_kreport_reset(kslam_ctx *ctx);

/* Host ids in, uploaded and counted by the same kernel a lane uses: for the batches whose ids were made on the host, and for
 * stage-level tests.  Any id is legal input.  A call that would take the list of unknown ids past 2^32 - 1 items returns
 * KSLAM_ERR_UNSUPPORTED and leaves the state as it was.  KSLAM_ERR_STATE with the switch off.  May be called from any thread;
 * calls are serialised. */
kslam_status kslam_kreport_add(kslam_ctx *ctx, const uint32_t *tax_ids, uint64_t n);

/* The rows of every batch counted so far (it waits for the lanes' streams); the clade sums are made at each call, so the call
 * may be repeated and more batches may follow it.  *rows: a page-locked, library-owned array of *n_rows rows; hand it back with
 * kslam_free_pinned.  Only the rows travel to the host. */
kslam_status kslam_kreport_take(kslam_ctx *ctx, kslam_kreport_row **rows, uint64_t *n_rows, kslam_kreport_stats *stats);

/* device time (ms), by events around the launches: the count pass of the last batch counted through this context's own stream
 * (kslam_kreport_add; the lanes' times are not gathered) and the kernels of the last kslam_kreport_take */
kslam_status kslam_kreport_kernel_ms(kslam_ctx *ctx, double *add_ms, double *take_ms);

/* Host twin (no GPU): the rows of ONE set of ids (several batches: concatenate them), in one serial pass; *rows is malloc'ed
 * (kslam_free).  message: kslam_tail_last_error(). */
kslam_status kslam_tail_kreport(const kslam_taxdb *taxdb, const uint32_t *tax_ids, uint64_t n, kslam_kreport_row **rows, uint64_t *n_rows,
                                kslam_kreport_stats *stats);

/* The file described above, from rows as kslam_kreport_take / kslam_tail_kreport give them.  KSLAM_ERR_ARG before anything is
 * written: total_read_pairs smaller than the sum of the direct counts, a row whose node is not one of the tree's, a known row
 * whose ancestors are not all among the rows. */
kslam_status kslam_kreport_write(const kslam_taxdb *taxdb, const kslam_kreport_row *rows, uint64_t n_rows, uint64_t total_read_pairs, int fd);

/* kslam_stream_classify (kslam_stream.h) writes the report itself: call this before it with an open descriptor (-1: none).  It
 * holds for the NEXT call alone, which switches the report on and resets it, feeds every batch that arrives without
 * KSLAM_TEXT_PER_READ (its ids are kslam_tail_classify's) through kslam_kreport_add on the host stage's thread, writes the file
 * after the last batch and switches the report off.  Without a taxdb that call returns KSLAM_ERR_STATE. */
kslam_status kslam_stream_set_kreport(kslam_ctx *ctx, int fd);
kslam_status kslam_stream_get_kreport(kslam_ctx *ctx, int *fd);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_KREPORT_H_ */
