// consensus.h -- the consensus caller's device side as the ABI sees it (include/kslam_consensus.h; kernels: consensus.hip).
// The state -- six append-only arrays of keys -- belongs to the context the switch was set on (context.h: kslam_ctx::Consensus);
// each lane counts its batch with an EmitWork of its own (common.h) and appends under the state's lock.
#pragma once
#include "common.h"
#include "../../include/kslam_consensus.h"

namespace kslam {

enum { CNS_EV = 0, CNS_M = 1, CNS_D = 2, CNS_INS = 3, CNS_KINDS = 4 };   // the kinds of keys a record emits (EmitWork's n[kind])

struct ConsensusKeys {                // the state's arrays (or where a batch's keys go)
  uint64_t *ev;                       // (g << 3) | code
  uint64_t *mb, *me;                  // g of the first / last column of an M run
  uint64_t *db, *de;                  // of a D run
  uint64_t *ins;                      // two words per insertion: [0] the bases, [1] (anchor << 6) | (len - 1)
};

struct ConsensusTakeWork {
  SortWorkspace sortws;
  DevBuf alt;                         // the sorts' second buffer
  DevBuf tflag, tpos, tlist;          // u32 per entry: touched, its place in the list; the list
  DevBuf tstart;                      // u64 [n_touched + 1]: positions of the touched entries before this one
  DevBuf obase;                       // u64 per touched entry of a slice: where its sequence goes in `seq` (~0: not reported)
  DevBuf len, off, call, insidx;      // per position of a slice: output bytes (u32), their place (u64), the byte called for the
                                      // position itself (u8, 0: none), the winning insertion's record (u32, ~0: none)
  DevBuf counters;                    // u64 [2][4] per touched entry of a slice (wave_add.h's rows)
  DevBuf seq;                         // the reported entries' sequences, back to back
  DevBuf scan_tmp, totals;
};

struct ConsensusCall {                // one take, as the host sees it
  std::vector<kslam_consensus_row> rows;
  uint64_t seq_bytes = 0, n_touched = 0;
};

// the contributing list, the counting walk and the four scans; fills W.n_list / n / n_skipped / ... (waits for the stream)
void consensus_count_device(const VariantInputs &in, EmitWork &W, hipStream_t s);
// the writing walk: the keys of the batch counted last, from `at` on (the caller made room for W.n[kind] of each); waits for
// the stream and fills W.ms
void consensus_write_device(const VariantInputs &in, EmitWork &W, const ConsensusKeys &at, hipStream_t s);
// sorts the six arrays in place (insertions: by key, then by bases)
void consensus_sort_device(ConsensusTakeWork &T, DevBuf &ev, DevBuf &mb, DevBuf &me, DevBuf &db, DevBuf &de, DevBuf &ins, const uint64_t n[CNS_KINDS],
                           uint64_t total_bases, hipStream_t s);
// over SORTED arrays: the touched entries, then slice by slice the call pass, the scan and the write pass; the reported entries'
// rows into out.rows and their sequences into T.seq (device).  Waits for the stream.
void consensus_take_device(ConsensusTakeWork &T, const ConsensusKeys &K, const uint64_t n[CNS_KINDS], const uint64_t *d_goff, const uint8_t *d_gbases,
                           const std::vector<uint64_t> &h_goff, uint64_t n_entries, const kslam_consensus_params &P, uint64_t slice,
                           ConsensusCall &out, hipStream_t s);

}  // namespace kslam
