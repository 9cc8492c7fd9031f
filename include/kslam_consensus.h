/*
 * kslam_consensus.h -- the consensus sequence of every entry the reads align to (what `samtools consensus`, `bcftools consensus`
 * or `ivar consensus` give after a pile-up over the coordinate-sorted SAM file), called on the GPU from what a lane holds when it
 * has finished a batch (csrc/consensus.hip), and written as FASTA.  It is the other half of the pile-up behind kslam_variants.h:
 * that table has no indels, no votes for non-ACGT columns and no deletion depth.  Same library as kslam.h.
 *
 * Off by default; with the switch off every byte of every output is what it was.  All integer, no floating point on the device.
 *   contributing set   as kslam_variants.h: every overlap record that at least one LIVE alignment pair of a FINAL read pair names
 *                      as r1 or r2 contributes ONCE.
 *   skipped records    as kslam_variants.h: entry >= n_entries, cigar_len == 0, ref_begin < 0, or a CIGAR that runs past the read
 *                      or past the entry.  The check covers the whole CIGAR and is made before anything of that record is emitted;
 *                      a skipped record adds one to n_skipped and nothing else.  No kernel reads or writes outside an entry, a
 *                      read or the CIGAR pool, whatever the records hold.
 *   the walk           as kslam_variants.h: from ref_begin and max(query_begin, 0); the query is the read, or its reverse
 *                      complement when revcomp != 0 (only upper-case A/C/G/T are complemented); M = 0, I = 1, D = 2, packed
 *                      len << 4 | op.  g = g_off[entry] + pos numbers the bases of the whole index.
 *   what a record contributes
 *     M interval       one closed interval of g per M run of length above 0
 *     D interval       one closed interval of g per D run of length above 0
 *     event            one per M column whose query byte differs from the entry's byte (a plain byte comparison), keyed
 *                      (g << 3) | code with code A 0, C 1, G 2, T 3 (upper case) and 4 for anything else.  No strand bit.
 *     insertion        one per I run of length len above 0.  Its anchor is the g of the last reference position the record
 *                      consumed before the run, by M or by D.  A run before any consumed position is UNANCHORED: it is counted
 *                      in n_ins_unanchored and not stored.  An anchored run with len > 32, or with a query byte (after
 *                      complementing) that is not upper-case A/C/G/T, is UNREPRESENTABLE: it is counted in
 *                      n_ins_unrepresentable and not stored, so that read votes "no insertion" there.  A stored insertion is a
 *                      16-byte key: (anchor << 6) | (len - 1), and the bases at 2 bits each, the first base in the highest of
 *                      the 2 * len bits (32 bases is what one 64-bit word holds; the word's numeric order among runs of one
 *                      length is the strings' order).  Every I run is an insertion of its own: two I runs in a row are two
 *                      insertions at one anchor.
 *   per position, over all batches piled up
 *     m(g), dl(g)      the M / D intervals containing g;   d(g) = m(g) + dl(g)
 *     ev(g, code)      the events at g with that code;     refc(g) = m(g) - the sum of ev(g, code) over the five codes
 *     vote(g, b)       for b in A C G T: ev(g, b), plus refc(g) when the entry's byte at g is upper-case b.  Non-ACGT query bytes
 *                      vote for nothing, and so do the refc(g) columns of an entry byte that is not upper-case A/C/G/T.
 *   the call           parameters: min_depth (>= 1), call_permille (500 .. 999), fill (N or REF), min_covered.  A candidate with
 *                      count c wins at g when c * 1000 > d(g) * call_permille; with a permille of at least 500 at most one of
 *                      A, C, G, T and deletion can win, so there are no ties and no order dependence.
 *                        d(g) < min_depth   UNCOVERED: `N`, or the entry's byte as it is under fill = REF
 *                        otherwise          COVERED.  A base wins: that base in upper case, and one substitution when it differs
 *                                           from the entry's byte.  Deletion (by dl(g)) wins: nothing, and one deleted position.
 *                                           Nothing wins: `N`, and one ambiguous position.
 *                      After a covered position's own output come the stored insertions anchored at g: when a distinct pair
 *                      (len, bases) has a count c with c * 1000 > d(g) * call_permille -- the denominator is the depth at the
 *                      anchor, as `ivar consensus` has it -- its bases are emitted, one insertion and len inserted bases are
 *                      counted.  This does not depend on what was called at g itself.  (Two I runs in a row share an anchor, so
 *                      two pairs can pass; then the one with the smaller len, among equal lengths the one whose string sorts
 *                      first, is emitted, and it alone is counted.)
 *   rows               an entry is reported when its covered positions number at least min_covered and at least 1.  Its sequence
 *                      spans the whole entry, from position 0 to its length; entries ascend.
 *   determinism        the state is multisets of integer keys, so the result does not depend on the number of lanes, on the
 *                      order of the batches, on whether a batch came from its lane or through kslam_consensus_add, on the slice
 *                      size, or on how often kslam_consensus_take was called before; it equals kslam_tail_consensus on the same
 *                      arrays, byte for byte and field for field.
 *
 * The state -- 8 bytes per event, 16 per M or D run, 16 per stored insertion, growing with the batches and not with the database
 * -- belongs to the context the switch was set on and is shared by its lanes; it is emptied at switch-on and by
 * kslam_consensus_reset and freed at switch-off, by kslam_set_index and by kslam_destroy.  More than 2^32 - 1 stored keys of any
 * one kind is outside the envelope (the radix sort's limit): the call that would cross it returns KSLAM_ERR_UNSUPPORTED and leaves
 * the state as it was.  An index of 2^57 or more bases is refused at switch-on (the anchor is shifted by 6 in the insertion key).
 */
#ifndef KSLAM_CONSENSUS_H_
#define KSLAM_CONSENSUS_H_
#include "kslam.h"
#include "kslam_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KSLAM_CONSENSUS_FILL_N 0u
#define KSLAM_CONSENSUS_FILL_REF 1u
#define KSLAM_CONSENSUS_MAX_INS 32u               /* bases of a stored insertion */
#define KSLAM_CONSENSUS_DEFAULT_SLICE (1ull << 26) /* positions called per pass of kslam_consensus_take */

typedef struct kslam_consensus_params {
  uint32_t min_depth;      /* >= 1 */
  uint32_t call_permille;  /* 500 .. 999 */
  uint32_t fill;           /* KSLAM_CONSENSUS_FILL_N or _REF */
  uint32_t min_covered;    /* 0 is as 1 */
} kslam_consensus_params;

typedef struct kslam_consensus_row {
  uint32_t entry;
  uint32_t pad;
  uint64_t seq_off;         /* the entry's sequence is seq[seq_off .. seq_off + seq_len) */
  uint64_t seq_len;
  uint64_t entry_len;
  uint64_t covered;         /* positions with d >= min_depth */
  uint64_t substitutions;   /* called bases that differ from the entry's byte */
  uint64_t deleted;         /* positions at which deletion won */
  uint64_t insertions;      /* anchors at which an insertion won */
  uint64_t inserted_bases;
  uint64_t ambiguous;       /* covered positions at which nothing won */
} kslam_consensus_row;

typedef struct kslam_consensus_stats {
  uint64_t n_records;              /* contributing overlap records (the skipped ones among them) */
  uint64_t n_skipped;
  uint64_t n_intervals;            /* M runs */
  uint64_t n_del_intervals;        /* D runs */
  uint64_t n_events;
  uint64_t n_insertions;           /* stored */
  uint64_t n_ins_unanchored;
  uint64_t n_ins_unrepresentable;
  uint64_t n_entries_touched;      /* entries holding at least one M or D interval */
  uint64_t n_entries_reported;
} kslam_consensus_stats;

/* on != 0: the lanes pile up every batch they finish (a batch whose pseudo-assembly the device left to the host is NOT: hand its
 * final arrays to kslam_consensus_add after the host stage).  Needs an index, the device pairing (kslam_set_pairing with
 * stages != 0) and a context created with report_cigar != 0, else KSLAM_ERR_STATE.  Switching on allocates the state (on when
 * already on: nothing happens); off frees it.  Set it between batches.  A context of a kslam_multi gets KSLAM_ERR_UNSUPPORTED. */
kslam_status kslam_set_consensus(kslam_ctx *ctx, int on);
kslam_status kslam_get_consensus(kslam_ctx *ctx, int *on);

/* empties the state and zeroes the counters; KSLAM_ERR_STATE with the switch off */
kslam_status kslam_consensus_reset(kslam_ctx *ctx);

/* Host arrays in, uploaded and piled up like a lane's batch: for the batches left to the host, and for stage-level tests.
 * Arguments and refusals (KSLAM_ERR_ARG before anything is launched, KSLAM_ERR_STATE with the switch off) as kslam_variants_add.
 * May be called from any thread; calls are serialised. */
kslam_status kslam_consensus_add(kslam_ctx *ctx, const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool,
                                 uint64_t n_cigar, const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads,
                                 const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                 uint64_t n_pairs);

/* kslam_consensus_take calls the touched entries in slices: whole touched entries whose lengths add up to at most `slice`
 * positions (an entry longer than that is a slice by itself).  slice = 0 puts the default back.  The result does not depend on
 * it; it bounds the work memory (17 bytes per position of a slice).  KSLAM_ERR_STATE with the switch off. */
kslam_status kslam_consensus_set_slice(kslam_ctx *ctx, uint64_t slice);

/* The consensus of every batch collected so far (it waits for the lanes' streams); the call may be repeated, with other
 * parameters too, and more batches may follow it.  *rows: a page-locked, library-owned array of *n_rows rows; *seq: one
 * page-locked byte array holding their sequences back to back (not terminated).  Hand both back with kslam_free_pinned.
 * KSLAM_ERR_ARG for parameters outside their ranges. */
kslam_status kslam_consensus_take(kslam_ctx *ctx, const kslam_consensus_params *params, kslam_consensus_row **rows, uint64_t *n_rows,
                                  char **seq, kslam_consensus_stats *stats);

/* device time (ms), by events: of the last batch piled up through this context's own stream (kslam_consensus_add; the lanes'
 * times are not gathered), and of the last kslam_consensus_take (its sorts, call, scan and write passes; not the copies) */
kslam_status kslam_consensus_kernel_ms(kslam_ctx *ctx, double *emit_ms, double *take_ms);

/* Host twin (no GPU): the consensus of ONE set of arrays (several batches: concatenate them), serially, with dense counters per
 * touched entry.  *rows and *seq: malloc'ed, hand them back with kslam_free.  Argument errors as kslam_consensus_add and
 * kslam_consensus_take; message: kslam_tail_last_error(). */
kslam_status kslam_tail_consensus(const char *entry_bases, const uint64_t *entry_offsets, uint64_t n_entries,
                                  const kslam_overlap *overlaps, uint64_t n_overlaps, const uint32_t *cigar_pool, uint64_t n_cigar,
                                  const char *read_bases, const uint64_t *read_offsets, uint64_t n_reads,
                                  const kslam_read_pair *read_pairs, uint64_t n_read_pairs, const kslam_paired_overlap *pairs,
                                  uint64_t n_pairs, const kslam_consensus_params *params, kslam_consensus_row **rows, uint64_t *n_rows,
                                  char **seq, kslam_consensus_stats *stats);

/* The file: FASTA, one record per row.
 *   >LOCUS kslam_consensus entry_length=L covered=.. substitutions=.. deletions=.. insertions=.. ambiguous=..
 *   the sequence in lines of 60 (no sequence line when it is empty)
 * LOCUS as the SAM header spells it; deletions = the row's deleted positions.  KSLAM_ERR_ARG, before anything is written, for a
 * row whose entry is not in the view or has an empty locus. */
kslam_status kslam_consensus_write(const kslam_index_view *index, const kslam_consensus_row *rows, uint64_t n_rows, const char *seq,
                                   int fd);

/* kslam_stream_classify (kslam_stream.h) writes the file itself: call this before it with an open descriptor (-1: none).  It
 * holds for the NEXT call alone, which switches the consensus on and resets it, feeds the batches left to the host through
 * kslam_consensus_add on the host stage's thread, writes the file after the last batch and switches it off.  params == NULL:
 * the defaults (1, 500, N, 1).  KSLAM_ERR_ARG for parameters outside their ranges. */
kslam_status kslam_stream_set_consensus(kslam_ctx *ctx, int fd, const kslam_consensus_params *params);
kslam_status kslam_stream_get_consensus(kslam_ctx *ctx, int *fd, kslam_consensus_params *params);

#ifdef __cplusplus
}
#endif
#endif /* KSLAM_CONSENSUS_H_ */
