/*
 * kslam_indels.h -- a table of the insertions and deletions the reads carry against the entries they align to, every one shifted
 * to its leftmost equivalent position (`bcftools norm`'s rule) before it is counted, piled up on the GPU from what a lane holds
 * when it has finished a batch (csrc/indels.hip), and written as VCF 4.2 without sample columns.  The report stands beside the
 * SNV table (kslam_variants.h) and has its life cycle; neither depends on the other's switch.  Same library as kslam.h.
 *
 * Off by default; with the switch off every byte of every output is what it was.  With it on:
 *   contributing set   a batch contributes its FINAL read pairs: the groups read_pairs[i] with their LIVE alignment pairs
 *                      pairs[first .. first + count).  The records between first + count and the next group's first are dead
 *                      and contribute nothing.  Every overlap record that at least one live alignment pair names as r1 or r2
 *                      (not KSLAM_NO_OVERLAP) contributes ONCE, however many live pairs name it.
 *   skipped records    a contributing overlap record contributes nothing and adds one to n_skipped when
 *                        entry >= n_entries, or cigar_len == 0, or ref_begin < 0, or
 *                        its CIGAR runs past the read or past the entry: an M or D run whose end exceeds the entry's length,
 *                        an M or I run whose end exceeds the read's length.
 *                      The check covers the whole CIGAR and is made before anything of that record is emitted.  No kernel reads
 *                      or writes outside an entry or a read, whatever the records hold.
 *   the walk           starts at reference position ref_begin and at query position max(query_begin, 0).  The query is the read,
 *                      or its reverse complement when revcomp != 0; in the reverse complement only upper-case A/C/G/T are
 *                      complemented, every other byte stays as it is.  Operations are M = 0, I = 1, D = 2, packed
 *                      len << 4 | op; M advances both positions, I the query, D the reference.
 *   intervals          every M operation of length above 0 contributes the CLOSED interval of reference positions it spans on
 *                      the record's entry, as in the SNV table.  The state keeps interval arrays of its own.
 *   raw events         p is the reference position the walk stands at, 0-based in the entry; strand = revcomp != 0.
 *                        deletion   a D run of length len >= 1 deletes the entry's bytes p .. p + len - 1.  It is counted when
 *                                   p > ref_begin (anchored: the record consumed a reference position before it) and
 *                                   len <= KSLAM_INDEL_MAX_DEL; else it adds one to n_unanchored, or (anchored) to n_long_del.
 *                        insertion  an I run of length len >= 1 inserts the oriented query bytes s[0 .. len) in front of p.  It
 *                                   is counted when p > ref_begin and len <= KSLAM_INDEL_MAX_INS and every inserted byte is
 *                                   upper-case A/C/G/T; else it adds one to n_unanchored, or (anchored) to n_unrepresentable.
 *   normalisation      of every counted raw event, against the bytes `ref` of the record's entry ALONE and the allele, never the
 *                      read:
 *                        deletion   while p >= 2 and ref[p - 1] == ref[p + len - 1] and that byte is upper-case A/C/G/T: p -= 1
 *                        insertion  while p >= 2 and ref[p - 1] == s[len - 1]: s = s[len - 1] + s[0 .. len - 1), p -= 1
 *                      There is NO cap on the number of steps: a cap would make the canonical form depend on where a read
 *                      happened to put the gap.  The loop never looks at another entry's bytes; p >= 2 keeps the anchor
 *                      p - 1 >= 0 inside the entry after the last step (an event is never stepped from p == 1, so an entry's
 *                      first base can be an anchor but is never deleted or inserted in front of by a shift).  N, lower case
 *                      and any other byte stops the shift, whichever side of the comparison it stands on.  The event is keyed
 *                      at anchor = p - 1.
 *   rows               one per distinct (entry, anchor, kind, len, bases), ascending by entry, then anchor, then kind (deletion
 *                      0 before insertion 1), then len, then bases (as a number: 2 bits per base, A 0 C 1 G 2 T 3, the first
 *                      base highest): entry, pos = anchor, kind, len, bases (0 for a deletion), alt_fwd and alt_rev (the events
 *                      of each strand), depth.  depth is the number of contributing records with an M column at the anchor: the
 *                      SNV table's depth at that position.  A read whose own gap lay to the right of where normalisation puts
 *                      it may have no M column at the new anchor (it may not even reach it), so alt_fwd + alt_rev CAN EXCEED
 *                      depth.  The table reports both as counted and clamps nothing.
 *   filter             kslam_indels_take returns the rows with alt_fwd + alt_rev >= min_alt and depth >= min_depth: integer
 *                      comparisons, no floating point.
 *   determinism        the state is a multiset of integer keys, sorted when the rows are asked for, so the rows do not depend on
 *                      the number of lanes, on the order of the batches, on whether a batch came from its lane or through
 *                      kslam_indels_add, or on how often kslam_indels_take was called before; they equal kslam_tail_indels on
 *                      the same arrays, field for field.
 *
 * The state -- 8 bytes per deletion, 16 per insertion, 16 per interval, growing with the batches and not with the database --
 * belongs to the context the switch was set on and is shared by its lanes; it is emptied at switch-on and by kslam_indels_reset
 * and freed at switch-off, by kslam_set_index and by kslam_destroy.  More than 2^32 - 1 stored keys of one kind is outside the
 * envelope (the radix sort's limit): the call that would cross it returns KSLAM_ERR_UNSUPPORTED and leaves the state as it was.
 * An index of 2^47 or more bases is refused at switch-on (a deletion key holds the position above 17 bits).
 *
 * SNV rows and indel rows are two files.  Merging them into one is out of scope here: `bcftools concat -a` does it.
 */
#ifndef KSLAM_INDELS_H_
#define KSLAM_INDELS_H_
#include "kslam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_INDEL_MAX_DEL 65536u   /* the longest D run that is counted */
#define KSLAM_INDEL_MAX_INS 32u      /* the longest I run that is counted (KSLAM_CONSENSUS_MAX_INS's limit, restated) */
#define KSLAM_INDEL_DEL 0
#define KSLAM_INDEL_INS 1

typedef struct {
  uint32_t entry;
  uint32_t pos;      /* the anchor, 0-based within the entry: the base in front of the deleted / inserted bases */
  uint8_t kind;      /* KSLAM_INDEL_DEL or KSLAM_INDEL_INS */
  uint8_t pad[3];
  uint32_t len;      /* deleted or inserted bases */
  uint64_t bases;    /* insertion: the inserted bases at 2 bits each, the first one highest; deletion: 0 */
  uint32_t alt_fwd;  /* events with revcomp == 0 */
  uint32_t alt_rev;  /* events with revcomp != 0 */
  uint32_t depth;    /* contributing records with an M column at pos; may be below alt_fwd + alt_rev (see above) */
  uint32_t pad2;
} kslam_indel_row;

typedef struct {
  uint64_t n_records;          /* contributing overlap records (the skipped ones among them) */
  uint64_t n_skipped;
  uint64_t n_intervals;
  uint64_t n_deletions;        /* counted D runs */
  uint64_t n_insertions;       /* counted I runs */
  uint64_t n_unanchored;       /* D and I runs in front of the record's first reference position */
  uint64_t n_long_del;         /* anchored D runs longer than KSLAM_INDEL_MAX_DEL */
  uint64_t n_unrepresentable;  /* anchored I runs longer than KSLAM_INDEL_MAX_INS or with a byte outside ACGT */
  uint64_t n_sites;            /* rows before the filter */
} kslam_indel_stats;

/* on != 0: the lanes pile up every batch they finish (a batch whose pseudo-assembly the device left to the host --
 * pair_stats.stages_done lacks KSLAM_TAIL_PSEUDO_ASM -- is NOT: hand its final arrays to kslam_indels_add after the host
 * stage).  Needs an index, the device pairing (kslam_set_pairing with stages != 0) and a context created with
 * report_cigar != 0, else KSLAM_ERR_STATE.  Switching on allocates the state (on when already on: nothing happens); off frees
 * it.  Set it between batches.  A context of a kslam_multi gets KSLAM_ERR_UNSUPPORTED, as from kslam_set_variants. */
kslam_status kslam_set_indels(kslam_ctx *ctx, int on);
kslam_status kslam_get_indels(kslam_ctx *ctx, int *on);

/* empties the state and zeroes the counters; KSLAM_ERR_STATE with the switch off */
kslam_status kslam_indels_reset(kslam_ctx *ctx);

/* Host arrays in, uploaded and piled up like a lane's batch: for the batches left to the host, and for stage-level tests.
 * Arguments and the KSLAM_ERR_ARG refusals made before anything is launched: those of kslam_variants_add.  KSLAM_ERR_STATE with
 * the switch off.  May be called from any thread; calls are serialised. */
kslam_status kslam_indels_add(kslam_ctx *ctx, const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool,
                              uint64_t n_cigar, const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads,
                              const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                              uint64_t n_pairs);

/* The rows of every batch collected so far (it waits for the lanes' streams) that pass the filter; the call may be repeated,
 * and more batches may follow it.  *rows: a page-locked, library-owned array of *n_rows rows; hand it back with
 * kslam_free_pinned. */
kslam_status kslam_indels_take(kslam_ctx *ctx, uint32_t min_alt, uint32_t min_depth, kslam_indel_row **rows, uint64_t *n_rows,
                               kslam_indel_stats *stats);

/* device time (ms), by events: from the first to the last pass of the last batch piled up through this context's own stream
 * (kslam_indels_add; the lanes' times are not gathered), and of the last kslam_indels_take */
kslam_status kslam_indels_kernel_ms(kslam_ctx *ctx, double *emit_ms, double *take_ms);

/* Host twin (no GPU): the rows of ONE set of arrays (several batches: concatenate them), serially.  *rows: malloc'ed, hand it
 * back with kslam_free.  Argument errors as kslam_indels_add; message: kslam_tail_last_error(). */
kslam_status kslam_tail_indels(const char *entry_bases, const uint64_t *entry_offsets, uint64_t n_entries,
                               const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                               const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads,
                               const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                               uint64_t n_pairs, uint32_t min_alt, uint32_t min_depth, kslam_indel_row **rows, uint64_t *n_rows,
                               kslam_indel_stats *stats);

/* The file: VCF 4.2, sites only.
 *   ##fileformat=VCFv4.2
 *   ##source=<the first token of kslam_version()>
 *   ##contig=<ID=locus,length=L>      one per entry that has a row, in entry order, locus as the SAM header spells it
 *   ##INFO lines for DP (Integer, 1), AO, SAF, SAR (Integer, A), AF (Float, A), TYPE (String, A: del / ins), LEN (Integer, A)
 *   #CHROM  POS  ID  REF  ALT  QUAL  FILTER  INFO
 *   deletion   locus  pos + 1  .  <the anchor byte and the len deleted bytes of the entry>  <the anchor byte>  .  .
 *              DP=depth;AO=alt_fwd + alt_rev;SAF=alt_fwd;SAR=alt_rev;AF=AO / DP as %.6f;TYPE=del;LEN=len
 *   insertion  REF is the anchor byte, ALT the anchor byte followed by the inserted bases; TYPE=ins
 * The entry's bytes are written as the entry holds them.  AF is 0.000000 when DP is 0 and is not clamped (AO may exceed DP).
 * The rows must ascend as kslam_indels_take returns them.  KSLAM_ERR_ARG, before anything is written, for a row whose entry is
 * not in the view or has an empty locus, whose pos lies outside the entry, whose kind or len (an insertion's: 1 .. 32) is none,
 * and for a deletion whose pos + len runs past the entry.  stats may be NULL (it is not written). */
kslam_status kslam_indels_write(const kslam_index_view *index, const kslam_indel_row *rows, uint64_t n_rows,
                                const kslam_indel_stats *stats, int fd);

/* kslam_stream_classify (kslam_stream.h) writes the file itself: call this before it with an open descriptor (-1: none).  It
 * holds for the NEXT call alone, which switches the indels on and resets them, feeds the batches left to the host through
 * kslam_indels_add on the host stage's thread, writes the file after the last batch and switches them off. */
kslam_status kslam_stream_set_indels(kslam_ctx *ctx, int fd, uint32_t min_alt, uint32_t min_depth);
kslam_status kslam_stream_get_indels(kslam_ctx *ctx, int *fd, uint32_t *min_alt, uint32_t *min_depth);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_INDELS_H_ */
