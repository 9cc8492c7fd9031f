/*
 * kslam_genes.h -- a per-gene abundance table (what featureCounts / HTSeq give for a SAM file and a GFF: reads per gene, from
 * which RPK and TPM follow), counted on the GPU from what a lane holds when it has finished a batch (csrc/genes.hip).  Same
 * library as kslam.h.
 *
 * Off by default; with the switch off every byte of every output is what it was.  With it on:
 *   contributing set   exactly the coverage table's (kslam_coverage.h): a batch contributes its FINAL read pairs: the groups
 *                      read_pairs[i] with their LIVE alignment pairs pairs[first .. first + count).  The records between
 *                      first + count and the next group's first are dead and contribute nothing.  The groups' `first` ascend
 *                      and the slices do not overlap (first + count <= the next group's first).
 *   gene of a record   GenbankEntry::getGene (src/GenbankTools.h:170-185) applied to the record's OWN fields pairs[j].entry,
 *                      pairs[j].ref_start, pairs[j].ref_end -- what the SAM writer and the XML report pass.  Among the genes g
 *                      of that entry, shared(g) = min(ref_end, gene_stop[g]) - max(ref_start, gene_start[g]); the chosen gene
 *                      has the strictly largest shared greater than 0; among genes with equal shared the lowest gene index
 *                      wins (file order: the reference's loop keeps the first).  No gene with shared > 0: the record has no
 *                      gene.  The subtraction and the comparison are done in 64 bits, so the result equals the SAM writer's
 *                      (best_gene, 32-bit like the reference) whenever the 32-bit subtraction does not overflow: for every
 *                      gene and interval inside +-2^30.  A record with entry >= n_entries belongs to no gene and adds one to
 *                      n_skipped.
 *   rows               one per gene of the index view; all fields are 64-bit and accumulate over all batches since the switch
 *                      was turned on or kslam_genes_reset:
 *                        alignments         live alignment pairs whose gene is this one (a read pair counts once per
 *                                           alignment pair)
 *                        unique_read_pairs  read pairs with count > 0 whose live alignment pairs ALL have this gene (none of
 *                                           them gene-less or skipped)
 *                        overlap_bases      the sum of shared(g) over the records counted in alignments
 *   statistics         n_alignments (live records seen) = n_in_gene + n_no_gene + n_skipped; n_rows = rows of the take
 *   take               only the rows with alignments > 0 travel to the host, in ascending gene index order: flagged, scanned
 *                      and compacted on the device.  The take may be repeated and more batches may follow it.
 *   file               (kslam_genes_write) one header line, then one line per row in row order, tab-separated:
 *                        #entry  locus  taxid  gene  start  stop  length  name  protein_id  product  alignments
 *                        unique_read_pairs  overlap_bases  rpk  tpm
 *                      entry, gene (the index within the view), start, stop, length = stop - start and the three counts are
 *                      integers; locus, taxid, name, protein_id and product come from the index view, as the SAM header and
 *                      tags take them (an empty field stays empty).  rpk = alignments * 1000.0 / length in double, 0 when
 *                      length <= 0, printed %.4f; tpm = rpk * 1e6 / S with S the sum of the rows' rpk added in row order, 0
 *                      when S == 0, printed %.4f.
 *   determinism        every accumulator is an integer add, so the rows do not depend on the number of lanes, on the order of
 *                      the batches, on whether a batch was counted by its lane or handed in through kslam_genes_add, or on how
 *                      often take was called; they equal kslam_tail_genes on the same arrays, field for field.
 *
 * The state -- a lookup index of 16 bytes per gene (per entry the genes ordered by start, with their stops and the running
 * maximum of the stops), 32 bytes of counters per gene and four statistics counters -- belongs to the context the switch was
 * set on and is shared by its lanes; the index is built and the counters are zeroed at switch-on, kslam_genes_reset zeroes the
 * counters, and everything is freed at switch-off, by kslam_set_sam_annotations and kslam_set_index (they replace the gene
 * columns) and by kslam_destroy.
 */
#ifndef KSLAM_GENES_H_
#define KSLAM_GENES_H_
#include "kslam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint64_t gene; /* index into the view's gene columns */
  uint64_t alignments;
  uint64_t unique_read_pairs;
  uint64_t overlap_bases;
} kslam_gene_row;

typedef struct {
  uint64_t n_alignments;
  uint64_t n_in_gene;
  uint64_t n_no_gene;
  uint64_t n_skipped;
  uint64_t n_rows;
} kslam_gene_stats;

/* on != 0: the lanes count every batch they finish (a batch whose pseudo-assembly the device left to the host --
 * pair_stats.stages_done lacks KSLAM_TAIL_PSEUDO_ASM -- is NOT counted: hand its final arrays to kslam_genes_add after the host
 * stage).  Needs an index, the device pairing (kslam_set_pairing with stages != 0) and annotations
 * (kslam_set_sam_annotations), else KSLAM_ERR_STATE; n_genes == 0 is legal (the table is empty), n_genes >= 2^32 - 2 is
 * KSLAM_ERR_UNSUPPORTED, gene_first not ascending from 0 to n_genes is KSLAM_ERR_ARG.  Switching on builds the lookup index and
 * zeroes the counters (on when already on: nothing happens); off frees the state.  Set it between batches.  A context of a
 * kslam_multi gets KSLAM_ERR_UNSUPPORTED, as from kslam_set_coverage. */
kslam_status kslam_set_genes(kslam_ctx *ctx, int on);
kslam_status kslam_get_genes(kslam_ctx *ctx, int *on);

/* zeroes the rows and the statistics; KSLAM_ERR_STATE with the switch off */
kslam_status kslam_genes_reset(kslam_ctx *ctx);

/* Host arrays in, uploaded and counted like a lane's batch: for the batches left to the host, and for stage-level tests.  Before
 * anything is launched, KSLAM_ERR_ARG for: first + count > n_pairs, groups whose `first` do not ascend or whose slices overlap.
 * KSLAM_ERR_STATE with the switch off.  May be called from any thread; calls are serialised. */
kslam_status kslam_genes_add(kslam_ctx *ctx, const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                             uint64_t n_pairs);

/* The rows of every batch counted so far (it waits for the lanes' streams).  *rows: a page-locked, library-owned array of
 * *n_rows rows; hand it back with kslam_free_pinned.  Only the rows and the statistics travel to the host. */
kslam_status kslam_genes_take(kslam_ctx *ctx, kslam_gene_row **rows, uint64_t *n_rows, kslam_gene_stats *stats);

/* test hook, like kslam_debug_radix_sort: the device function the count pass uses (linear != 0: the linear walk over all genes
 * of the entry, kept as a cross-check and for measurement) on n host triples.  genes_out[i] = the gene, -1 for none, -2 for
 * entries[i] >= n_entries; shared_out (may be NULL) = shared of that gene, 0 without one.  KSLAM_ERR_STATE with the switch off. */
kslam_status kslam_genes_lookup(kslam_ctx *ctx, const uint32_t *entries, const int32_t *starts, const int32_t *stops, uint64_t n,
                                int64_t *genes_out, int64_t *shared_out, int linear);

/* device time (ms), by events around the launches: the index build of the last switch-on, the count passes of the last batch
 * counted through this context's own stream (kslam_genes_add; the lanes' times are not gathered) and the last take's kernels */
kslam_status kslam_genes_kernel_ms(kslam_ctx *ctx, double *build_ms, double *count_ms, double *take_ms);

/* Host twin (no GPU): the rows of ONE set of arrays (several batches: concatenate them) in one serial pass that uses the linear
 * walk; *rows is malloc'ed (kslam_free).  Argument errors as kslam_genes_add; message: kslam_tail_last_error(). */
kslam_status kslam_tail_genes(const kslam_index_view *index, const kslam_read_pair *read_pairs, uint64_t n_read_pairs,
                              const kslam_paired_overlap *pairs, uint64_t n_pairs, kslam_gene_row **rows, uint64_t *n_rows,
                              kslam_gene_stats *stats);

/* The file described above, from rows as kslam_genes_take / kslam_tail_genes give them.  A row whose gene is not one of the
 * view's: KSLAM_ERR_ARG, returned before anything is written. */
kslam_status kslam_genes_write(const kslam_index_view *index, const kslam_gene_row *rows, uint64_t n_rows, int fd);

/* kslam_stream_classify (kslam_stream.h) writes the file itself: call this before it with an open descriptor (-1: none).  It
 * holds for the NEXT call alone, which sets the annotations, switches the table on and resets it, feeds the batches left to the
 * host through kslam_genes_add on the host stage's thread, writes the file after the last batch and switches the table off. */
kslam_status kslam_stream_set_genes(kslam_ctx *ctx, int fd);
kslam_status kslam_stream_get_genes(kslam_ctx *ctx, int *fd);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_GENES_H_ */
