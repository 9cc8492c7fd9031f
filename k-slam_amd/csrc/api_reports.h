// api_reports.h -- what the opt-in reports behind the C ABI share (api_coverage.hip, api_variants.hip, api_indels.hip, api_depth.hip,
// api_kreport.hip, api_genes.hip, api_readqc.hip, api_alignqc.hip, api_consensus.hip, api_bamsort.hip; the reads of chosen taxa, api_taxreads.hip, are released with
// them): their entry points for the lanes, the lists of what an index or a tree takes with it, and the shell of their ABI
// functions.  Each file keeps what is its own: its table layout, its switch-on preconditions, its zeroing, its take.
// Included from context.h, behind the context.
#pragma once

namespace kslam_api {

// ---- api_coverage.hip
// frees the coverage state of c and switches it off (kslam_set_coverage(c, 0), kslam_set_index)
void coverage_release(kslam_ctx *c);
// the batch `lane` has just finished (lane->pres over lane->res_ov) into owner's table, on lane's stream
void coverage_mark_resident(kslam_ctx *owner, kslam_ctx *lane);

// ---- api_variants.hip
// frees the variants state of c and switches it off (kslam_set_variants(c, 0), kslam_set_index)
void variants_release(kslam_ctx *c);
// the batch `lane` has just finished (lane->pres over lane->res_ov, lane->res_cig and lane's reads) into owner's state, on lane's stream
void variants_emit_resident(kslam_ctx *owner, kslam_ctx *lane);

// ---- api_indels.hip
// frees the indel state of c and switches it off (kslam_set_indels(c, 0), kslam_set_index)
void indels_release(kslam_ctx *c);
// the batch `lane` has just finished (as variants_emit_resident sees it) into owner's state, on lane's stream
void indels_emit_resident(kslam_ctx *owner, kslam_ctx *lane);

// ---- api_depth.hip
// frees the depth state of c and switches it off (kslam_set_depth(c, 0), kslam_set_index)
void depth_release(kslam_ctx *c);
// the batch `lane` has just finished into owner's state, on lane's stream
void depth_emit_resident(kslam_ctx *owner, kslam_ctx *lane);

// ---- api_kreport.hip
// frees the report state of c and switches it off (kslam_set_kreport(c, 0), kslam_set_sam_annotations, kslam_set_index)
void kreport_release(kslam_ctx *c);
// the n taxonomy ids `lane` has just computed (lane->samw.tax_ids) into owner's state, on lane's stream
void kreport_count_resident(kslam_ctx *owner, kslam_ctx *lane, uint64_t n);
// the id -> node table of c's device tree (c->annot), uploaded into the two buffers; waits for c's stream
void id_node_table(kslam_ctx *c, DevBuf &d_keys, DevBuf &d_nodes);

// ---- api_genes.hip
// frees the gene table of c and switches it off (kslam_set_genes(c, 0), kslam_set_sam_annotations, kslam_set_index)
void genes_release(kslam_ctx *c);
// the batch `lane` has just finished (lane->pres) into owner's table, on lane's stream
void genes_count_resident(kslam_ctx *owner, kslam_ctx *lane);

// ---- api_readqc.hip
// frees the read QC state of c and switches it off (kslam_set_read_qc(c, 0, 0))
void readqc_release(kslam_ctx *c);
// the batch resident on `lane` (lane->r_bases, r_qual, r_off: the columns cut out of the text it uploaded) into owner's tables,
// on lane's stream; does not wait
void readqc_count_resident(kslam_ctx *owner, kslam_ctx *lane, bool single);

// ---- api_alignqc.hip
// frees the alignment QC state of c and switches it off (kslam_set_align_qc(c, 0, 0), kslam_set_index)
void alignqc_release(kslam_ctx *c);
// the batch `lane` has just finished (lane->pres over lane->res_ov, lane->res_cig, lane's reads and, when it holds one, its quality
// column) into owner's tables, on lane's stream
void alignqc_count_resident(kslam_ctx *owner, kslam_ctx *lane, bool single);

// ---- api_consensus.hip
// frees the consensus state of c and switches it off (kslam_set_consensus(c, 0), kslam_set_index)
void consensus_release(kslam_ctx *c);
// the batch `lane` has just finished (as variants_emit_resident sees it) into owner's state, on lane's stream
void consensus_emit_resident(kslam_ctx *owner, kslam_ctx *lane);

// ---- api_bamsort.hip
// frees the held records of c and switches the sort off (kslam_set_bam_sort(c, 0), kslam_set_index)
void bamsort_release(kslam_ctx *c);
// ... and the state itself (kslam_destroy)
void bamsort_destroy(kslam_ctx *c);
// the BAM records `lane` has just written (lane->samw.text[0 .. total_bytes): the mapped rows of n_groups read pairs in front of
// mapped_bytes, the rows of the reads without alignment behind it) into owner's store as batch `ticket`, on lane's stream
void bamsort_append_resident(kslam_ctx *owner, kslam_ctx *lane, uint64_t ticket, uint64_t n_groups, uint64_t mapped_bytes, uint64_t n_unmapped_rows,
                             uint64_t total_bytes);

// ---- api_taxreads.hip
// frees the selection of c and switches it off (kslam_set_taxon_reads(c, NULL, 0, 0), kslam_set_sam_annotations, kslam_set_index)
void taxreads_release(kslam_ctx *c);
// the batch resident on c (indexed by fastq_index_device: c->fqw) selected by owner's S: d_ids[g] is the taxonomy id of
// d_groups[g].  Blocks from c's page-locked pool: out->data[0] / [1] the selected R1 / R2.
void taxreads_resident(kslam_ctx *owner, kslam_ctx *c, bool single, const kslam_read_pair *d_groups, const uint32_t *d_ids, uint64_t n_groups,
                       bool bgzf, int deflate, kslam_reads_out *out);

// ---- what goes with the annotations, and with the index ----
// kslam_set_sam_annotations: the state laid out for the old tree's nodes and the old gene columns
inline void release_tree_bound_reports(kslam_ctx *c) {
  kreport_release(c);    // (include/kslam_kreport.h) the counters were laid out for the old tree's nodes
  taxreads_release(c);   // (include/kslam_taxreads.h) the mask was laid out for them too
  genes_release(c);      // (include/kslam_genes.h) the lookup index was built from the old gene columns
}
// kslam_set_index: the state laid out for the old index's entries
inline void release_index_bound_reports(kslam_ctx *c) {
  coverage_release(c);   // (include/kslam_coverage.h) the table was laid out for the old index's entries
  variants_release(c);   // (include/kslam_variants.h) the keys hold the old index's base positions
  indels_release(c);     // (include/kslam_indels.h) likewise
  depth_release(c);      // (include/kslam_depth.h) likewise, and the spare position per entry besides
  kreport_release(c);    // (include/kslam_kreport.h) the annotations, and the tree with them, belong to the old index's entries
  taxreads_release(c);   // (include/kslam_taxreads.h) likewise
  genes_release(c);      // (include/kslam_genes.h) likewise: the gene columns belong to the old index's entries
  alignqc_release(c);    // (include/kslam_alignqc.h) its counts are of alignments to the old index's entries
  consensus_release(c);  // (include/kslam_consensus.h) the keys hold the old index's base positions
  bamsort_release(c);    // (include/kslam_bamsort.h) the held records name the old index's entries
}

// ---- the batch a lane has just finished, as the reports' kernels see it ----
// lane->pres over lane->res_ov, lane->res_cig and lane's reads against ix; with_bases: the reads' and the entries' bases too
inline VariantInputs resident_inputs(const kslam_ctx *lane, const GenomeIndex &ix, bool with_bases) {
  return VariantInputs{lane->res_ov.as<kslam_overlap>(), lane->n_res, lane->pres.d_groups, lane->pres.n_read_pairs, lane->pres.d_pairs,
                       lane->pres.n_pairs, lane->res_cig.as<uint32_t>(), lane->n_cig, with_bases ? lane->r_bases.as<uint8_t>() : nullptr,
                       lane->r_off.as<uint64_t>(), lane->n_reads, with_bases ? ix.g_bases.as<uint8_t>() : nullptr, ix.g_off.as<uint64_t>(),
                       ix.n_entries};
}

// ---- the shell of a report's ABI functions ----
// every lane's marks, appends and counts are in memory before anybody reads, sorts, zeroes or frees a report's state
inline void wait_for_lanes(kslam_ctx *c) {
  for (auto *l : c->lanes) HIPCHK(hipStreamSynchronize(l->c->stream));
}

inline void need_on(const std::atomic<bool> &on, const char *message) {
  if (!on.load(std::memory_order_acquire)) throw StatusError{KSLAM_ERR_STATE, message};
}

// "<the report is> not available on the contexts of a kslam_multi": true, with the refusal in c->err, on such a context.  The
// switch throws it, kslam_stream_set_* returns it.
inline bool refused_in_multi(kslam_ctx *c, const char *report_is) {
  if (c->in_multi) c->err = std::string(report_is) + " not available on the contexts of a kslam_multi";
  return c->in_multi;
}

// kslam_get_*: is the report of c (a member of kslam_ctx) switched on?  With max_cycles: what it was switched on with, 0 when off.
template <typename Report> kslam_status get_switch(kslam_ctx *c, Report kslam_ctx::*report, int *on) {
  if (!c || !on) return KSLAM_ERR_ARG;
  *on = (c->*report).on.load(std::memory_order_acquire) ? 1 : 0;
  return KSLAM_OK;
}
template <typename Report> kslam_status get_switch(kslam_ctx *c, Report kslam_ctx::*report, int *on, uint32_t *max_cycles) {
  if (!c || !on || !max_cycles) return KSLAM_ERR_ARG;
  std::lock_guard<std::mutex> lk((c->*report).mu);
  get_switch(c, report, on);
  *max_cycles = *on ? (c->*report).C : 0;
  return KSLAM_OK;
}

// kslam_*_take of a report that hands rows over: the outputs start empty, `fill(h)` runs guarded -- it takes h from c's page-locked
// pool (pinned_get), fills it and sets *n_rows and *stats -- and a failure hands h back and leaves the outputs empty.
template <typename Row, typename Stats, typename Fill> kslam_status take_rows(kslam_ctx *c, Row **rows, uint64_t *n_rows, Stats *stats, Fill &&fill) {
  if (rows) *rows = nullptr;
  if (n_rows) *n_rows = 0;
  if (stats) memset(stats, 0, sizeof *stats);
  Row *h = nullptr;
  const kslam_status st = guarded(c, [&] {
    if (!rows || !n_rows || !stats) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    fill(h);
  });
  if (st != KSLAM_OK) {
    if (h) pinned_put(c, h);
    if (n_rows) *n_rows = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return st;
  }
  *rows = h;
  return KSLAM_OK;
}

}  // namespace kslam_api
