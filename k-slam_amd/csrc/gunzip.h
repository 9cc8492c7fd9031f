// gunzip.h -- interface of gunzip.hip (plain gzip inflated on the device, include/kslam_gunzip.h)
#pragma once
#include "common.h"
#include "../host/gunzip.hpp"

namespace kslam {

constexpr uint32_t GUNZIP_WAVES = 4;                 // waves per workgroup of the find, count and decode kernels
constexpr uint32_t GUNZIP_WINDOW = 32768;            // deflate's window: how far back a match may reach
constexpr uint64_t GUNZIP_SPAN_BYTES = (1ull << 29) - 64;   // compressed bytes one wave can address (32-bit bit positions)
constexpr uint64_t GUNZIP_NO_START = ~0ull;
constexpr uint32_t GUNZIP_CRC_PIECE = 65536;         // text bytes per workgroup of the CRC pass

struct GunzipDecodeSpan {   // one live start of a round
  uint64_t bit;             // where its first block header begins, in bits from the start of the file
  uint64_t stop_bit;        // the block start it ends on (the next live start); GUNZIP_NO_START: the end of the file
  uint64_t sym_off;         // its first symbol inside the round's scratch (= its first byte inside the round's text)
  uint64_t n_out;           // its symbols, as the count pass found them
  uint64_t member_slot;     // where the members that end inside it go in the round's member table
  uint64_t n_members;
  uint64_t out;             // its first byte inside the whole text
};

struct GunzipMemberEnd {    // written by the decode pass for every member that ends in the round
  uint64_t trailer_at;      // byte offset of its CRC-32 / ISIZE trailer in the file
  uint64_t out_end;         // the text offset behind its last byte
};

struct GunzipCrcSeg {       // the part of one member that lies inside the round
  uint64_t off, len;        // inside the round's text
  uint32_t prev_crc;        // CRC-32 of the member's text before it (0 when it begins in this round)
  uint32_t pad;
};

struct GunzipWork {   // scratch, grown once and kept by the context
  DevBuf in, found, starts, links, spans, sym, text, win, members, segs, crcs, first_bad;
};

// Stage 1.  d_found[k] (k in [1, n_chunks)) = the lowest bit offset in chunk k that the finder's rule accepts, or GUNZIP_NO_START;
// d_found[0] is left alone.  d_in: the file, 4-byte aligned, 64 readable bytes behind it.
void gunzip_find_device(const uint8_t *d_in, uint64_t len, uint64_t chunk, uint64_t n_chunks, uint64_t *d_found, hipStream_t s);
// Stage 2.  One wave per start first .. first + n_run - 1 of d_starts[0 .. n_starts) (bit offsets, ascending); each writes
// d_links[its number].  budget_bits: a wave that has consumed more at a block start gives up (0: never).
void gunzip_count_device(const uint8_t *d_in, uint64_t len, const uint64_t *d_starts, uint32_t n_starts, uint32_t first, uint32_t n_run,
                         uint64_t budget_bits, kslam_host::GunzipLink *d_links, hipStream_t s);
// Stage 3.  One wave per span: symbols to d_sym, member ends to d_members.  *d_first_bad (u64, ~0 before) takes the minimum of
// (span number << 8 | kind) over the spans that did not decode as the count pass said they would.
void gunzip_decode_device(const uint8_t *d_in, uint64_t len, const GunzipDecodeSpan *d_spans, uint32_t n, uint16_t *d_sym,
                          GunzipMemberEnd *d_members, uint64_t *d_first_bad, hipStream_t s);
// Stage 4.  The last GUNZIP_WINDOW symbols of every span, in order, to d_text (the round's text; the GUNZIP_WINDOW bytes before
// d_text hold the text before the round).
void gunzip_window_device(const GunzipDecodeSpan *d_spans, uint32_t n, const uint16_t *d_sym, uint8_t *d_text, hipStream_t s);
// Stage 5.  Every other symbol of the round's n_text to d_text.
void gunzip_resolve_device(const GunzipDecodeSpan *d_spans, uint32_t n, const uint16_t *d_sym, uint8_t *d_text, uint64_t n_text, hipStream_t s);
// Stage 6.  d_crc[i] = CRC-32 of (what came before segment i, prev_crc) followed by its bytes; d_crc is cleared here.
void gunzip_crc_device(const uint8_t *d_text, const GunzipCrcSeg *d_segs, uint32_t n, uint64_t longest, uint32_t *d_crc, hipStream_t s);

}  // namespace kslam
