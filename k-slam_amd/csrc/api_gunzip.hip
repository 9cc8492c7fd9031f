// api_gunzip.hip -- the C ABI, plain gzip input (include/kslam_gunzip.h; kernels: gunzip.hip; the chain walk: host/gunzip.cpp).
// kslam_gunzip_inflate runs the stages in order: the file goes to the device once and stays there; find and count run over
// the whole file, the host follows the chain, and decode / window / resolve / check then run in rounds of live starts whose
// text fits the round's scratch.  Nothing leaves for the caller's buffer before its members' CRC-32 and ISIZE have held.
#include "context.h"
#include "gzip_header.h"

namespace kslam_api {

namespace {

using namespace kslam_host;

uint64_t chunk_of(const kslam_ctx *c) { return c->gz.chunk ? c->gz.chunk : (uint64_t)KSLAM_GUNZIP_CHUNK_DEFAULT; }
uint64_t round_of(const kslam_ctx *c) { return std::max(c->gz.round ? c->gz.round : (uint64_t)KSLAM_GUNZIP_ROUND_DEFAULT, chunk_of(c)); }
uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

[[noreturn]] void refuse(uint64_t member, uint64_t at, uint32_t kind) {
  const char *name = gunzip_kind_name(kind);
  throw StatusError{kind == GZK_SPAN ? KSLAM_ERR_UNSUPPORTED : KSLAM_ERR_ARG, gunzip_error_text(member, at, name ? name : inflate_error_name(kind))};
}

template <typename T> void download(std::vector<T> &dst, const void *d_src, size_t n, hipStream_t s) {
  dst.resize(n);
  if (n) HIPCHK(hipMemcpyAsync(dst.data(), d_src, n * sizeof(T), hipMemcpyDeviceToHost, s));
  HIPCHK(stream_wait(s));
}

}  // namespace

}  // namespace kslam_api

using namespace kslam_api;

extern "C" {

kslam_status kslam_gunzip_inflate(kslam_ctx *c, const void *data, uint64_t len, char **out, uint64_t *out_len) {
  if (out) *out = nullptr;
  if (out_len) *out_len = 0;
  char *h = nullptr;
  const kslam_status st = guarded(c, [&] {
    if (!out || !out_len || (len && !data)) throw StatusError{KSLAM_ERR_ARG, "null argument"};
    const uint8_t *src = static_cast<const uint8_t *>(data);
    kslam_gunzip_stats S{};
    GunzipWork &W = c->gzw;
    hipStream_t s = c->stream;
    if (!len) {
      h = (char *)pinned_get(c, 64);
      c->gz.stats = S;
      *out = h;
      return;
    }
    uint64_t deflate_at = 0;
    if (const uint32_t herr = gzip_header_walk(src, 0, len, &deflate_at)) refuse(0, 0, herr == GZH_HEADER ? GZK_HEADER : GZK_NOT_MEMBER);
    if (deflate_at >= len) refuse(0, 0, INF_DATA_LENGTH);
    const uint64_t chunk = chunk_of(c), n_chunks = (len + chunk - 1) / chunk;
    S.chunks = n_chunks;
    W.in.ensure(len + 64);   // 4-byte aligned, and the readers' last words may reach behind the bytes
    HIPCHK(hipMemcpyAsync(W.in.p, src, len, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(W.in.as<uint8_t>() + len, 0, 64, s));
    const uint8_t *d_in = W.in.as<uint8_t>();

    // ---- 1 find ----
    std::vector<uint64_t> starts{deflate_at * 8};
    bool first_found = false;
    if (n_chunks > 1) {
      W.found.ensure(n_chunks * sizeof(uint64_t));
      HIPCHK(hipEventRecord(c->ev[0], s));
      gunzip_find_device(d_in, len, chunk, n_chunks, W.found.as<uint64_t>(), s);
      HIPCHK(hipEventRecord(c->ev[1], s));
      std::vector<uint64_t> found;
      download(found, W.found.p, n_chunks, s);
      S.find_ms = ev_ms(c->ev[0], c->ev[1]);
      for (uint64_t k = 1; k < n_chunks; k++) {
        if (found[k] == GUNZIP_NO_START) continue;
        S.starts_found++;
        if (found[k] == starts[0]) first_found = true;
        else starts.push_back(found[k]);
      }
      std::sort(starts.begin(), starts.end());   // (a start inside the first member's header comes before its first block)
    }
    if (starts.size() > 0x7fffffffu) throw StatusError{KSLAM_ERR_UNSUPPORTED, "more than 2^31 block starts: raise kslam_gunzip_set_chunk"};
    const uint32_t n_starts = (uint32_t)starts.size();
    const uint32_t first = (uint32_t)(std::lower_bound(starts.begin(), starts.end(), deflate_at * 8) - starts.begin());

    // ---- 2 count, and the chain ----
    W.starts.ensure(starts.size() * sizeof(uint64_t));
    W.links.ensure(starts.size() * sizeof(GunzipLink));
    HIPCHK(hipMemcpyAsync(W.starts.p, starts.data(), starts.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(W.links.p, 0, starts.size() * sizeof(GunzipLink), s));
    HIPCHK(hipEventRecord(c->ev[2], s));
    // a wave on a false start may decode garbage for a long time: four chunks without meeting a start, and it gives up
    gunzip_count_device(d_in, len, W.starts.as<uint64_t>(), n_starts, 0, n_starts, 4 * chunk * 8, W.links.as<GunzipLink>(), s);
    HIPCHK(hipEventRecord(c->ev[3], s));
    std::vector<GunzipLink> links;
    download(links, W.links.p, starts.size(), s);
    S.count_ms = ev_ms(c->ev[2], c->ev[3]);
    GunzipChain chain;
    for (uint32_t last_broken = ~0u;;) {
      chain = gunzip_chain_walk(links.data(), n_starts, first);
      if (chain.state != GunzipChain::BROKEN) break;
      // a live wave gave up: the same start once more, to wherever it leads.  The links behind it stand.
      const uint32_t b = chain.broken_at;
      if (b >= n_starts || b == last_broken) throw StatusError{KSLAM_ERR_INTERNAL, "gunzip: the chain of block starts does not close at start " + std::to_string(b)};
      last_broken = b;
      HIPCHK(hipEventRecord(c->ev[2], s));
      gunzip_count_device(d_in, len, W.starts.as<uint64_t>(), n_starts, b, 1, 0, W.links.as<GunzipLink>(), s);
      HIPCHK(hipEventRecord(c->ev[3], s));
      HIPCHK(hipMemcpyAsync(&links[b], W.links.as<GunzipLink>() + b, sizeof(GunzipLink), hipMemcpyDeviceToHost, s));
      HIPCHK(stream_wait(s));
      S.count_ms += ev_ms(c->ev[2], c->ev[3]);
    }
    if (chain.state == GunzipChain::FAILED) refuse(chain.bad_member, chain.bad_at, chain.bad_kind);
    const std::vector<GunzipSpan> &spans = chain.spans;
    S.members = chain.members;
    S.text_len = chain.text_len;
    S.starts_live = spans.size() - 1 + (first_found ? 1 : 0);
    S.starts_dropped = S.starts_found - S.starts_live;

    // ---- 3 to 6, in rounds ----
    h = (char *)pinned_get(c, chain.text_len + 64);
    W.win.ensure(GUNZIP_WINDOW);
    W.first_bad.ensure(sizeof(uint64_t));
    HIPCHK(hipMemsetAsync(W.win.p, 0, GUNZIP_WINDOW, s));
    const uint64_t round_syms = round_of(c);
    uint64_t member = 0, member_at = 0, member_start = 0;   // the member that is open at the round's first byte: number, header, first text byte
    uint32_t open_crc = 0;                                  // CRC-32 of its text before the round
    std::vector<GunzipDecodeSpan> dspans;
    std::vector<GunzipMemberEnd> ends;
    std::vector<GunzipCrcSeg> segs;
    std::vector<uint32_t> crcs;
    for (size_t i = 0; i < spans.size();) {
      size_t j = i;
      uint64_t n_text = 0, n_mem = 0;
      dspans.clear();
      do {   // at least one stretch, however long
        const uint64_t stop = j + 1 < spans.size() ? starts[spans[j + 1].start] : GUNZIP_NO_START;
        dspans.push_back(GunzipDecodeSpan{starts[spans[j].start], stop, n_text, spans[j].n_out, n_mem, spans[j].n_members, spans[j].out});
        n_text += spans[j].n_out;
        n_mem += spans[j].n_members;
        j++;
      } while (j < spans.size() && n_text + spans[j].n_out <= round_syms);
      const uint64_t r0 = spans[i].out, r1 = r0 + n_text;
      const uint32_t n = (uint32_t)dspans.size();
      W.spans.ensure(dspans.size() * sizeof(GunzipDecodeSpan));
      W.sym.ensure((n_text + 64) * sizeof(uint16_t));
      W.text.ensure(GUNZIP_WINDOW + n_text + 64);
      W.members.ensure((n_mem + 1) * sizeof(GunzipMemberEnd));
      uint8_t *d_text = W.text.as<uint8_t>() + GUNZIP_WINDOW;
      HIPCHK(hipMemcpyAsync(W.spans.p, dspans.data(), dspans.size() * sizeof(GunzipDecodeSpan), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(W.text.p, W.win.p, GUNZIP_WINDOW, hipMemcpyDeviceToDevice, s));   // the 32 KiB of text before the round
      HIPCHK(hipMemsetAsync(W.first_bad.p, 0xff, sizeof(uint64_t), s));
      HIPCHK(hipEventRecord(c->ev[4], s));
      gunzip_decode_device(d_in, len, W.spans.as<GunzipDecodeSpan>(), n, W.sym.as<uint16_t>(), W.members.as<GunzipMemberEnd>(), W.first_bad.as<uint64_t>(), s);
      HIPCHK(hipEventRecord(c->ev[5], s));
      uint64_t bad = 0;
      read_back(&bad, W.first_bad.p, sizeof bad, s);
      if (bad != ~0ull)   // the count pass decoded the same bits and found them sound
        throw StatusError{KSLAM_ERR_INTERNAL, "gunzip: the decode pass stopped at start " + std::to_string(spans[i + (bad >> 8)].start) + " (" +
                                                  inflate_error_name((uint32_t)(bad & 0xffu)) + ") where the count pass went through"};
      HIPCHK(hipEventRecord(c->ev[6], s));
      gunzip_window_device(W.spans.as<GunzipDecodeSpan>(), n, W.sym.as<uint16_t>(), d_text, s);
      HIPCHK(hipEventRecord(c->ev[7], s));
      gunzip_resolve_device(W.spans.as<GunzipDecodeSpan>(), n, W.sym.as<uint16_t>(), d_text, n_text, s);
      HIPCHK(hipEventRecord(c->ev[8], s));
      download(ends, W.members.p, n_mem, s);

      // ---- 6 check: the members' parts inside [r0, r1) ----
      segs.clear();
      uint64_t ms = member_start, longest = 0;
      for (const GunzipMemberEnd &e : ends) {
        if (e.out_end < std::max(ms, r0) || e.out_end > r1 || e.trailer_at + 8 > len) throw StatusError{KSLAM_ERR_INTERNAL, "gunzip: a member's end lies outside its round"};
        const uint64_t a = std::max(ms, r0);
        segs.push_back(GunzipCrcSeg{a - r0, e.out_end - a, ms < r0 ? open_crc : 0u, 0});
        ms = e.out_end;
      }
      const bool open = ms < r1;   // a member goes on into the next round
      if (open) {
        const uint64_t a = std::max(ms, r0);
        segs.push_back(GunzipCrcSeg{a - r0, r1 - a, ms < r0 ? open_crc : 0u, 0});
      }
      for (const GunzipCrcSeg &g : segs) longest = std::max(longest, g.len);
      crcs.clear();
      if (!segs.empty()) {
        W.segs.ensure(segs.size() * sizeof(GunzipCrcSeg));
        W.crcs.ensure(segs.size() * sizeof(uint32_t));
        HIPCHK(hipMemcpyAsync(W.segs.p, segs.data(), segs.size() * sizeof(GunzipCrcSeg), hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(c->ev[9], s));
        gunzip_crc_device(d_text, W.segs.as<GunzipCrcSeg>(), (uint32_t)segs.size(), longest, W.crcs.as<uint32_t>(), s);
        HIPCHK(hipEventRecord(c->ev[10], s));
        download(crcs, W.crcs.p, segs.size(), s);
        S.check_ms += ev_ms(c->ev[9], c->ev[10]);
      }
      uint64_t m_start = member_start;
      for (size_t k = 0; k < ends.size(); k++) {
        const uint8_t *t = src + ends[k].trailer_at;
        const uint32_t produced = (uint32_t)(ends[k].out_end - m_start), isize = le32(t + 4);
        if (crcs[k] != le32(t)) refuse(member, member_at, INF_CRC);
        if (produced != isize) refuse(member, member_at, produced < isize ? INF_OUTPUT_UNDERRUN : INF_OUTPUT_OVERRUN);
        m_start = ends[k].out_end;
        member++;
        member_at = ends[k].trailer_at + 8;
        while (member_at < len && src[member_at] == 0) member_at++;   // zero bytes behind a member are skipped
      }
      member_start = m_start;
      open_crc = open ? crcs.back() : 0u;
      if (n_text) HIPCHK(hipMemcpyAsync(h + r0, d_text, n_text, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(W.win.p, W.text.as<uint8_t>() + n_text, GUNZIP_WINDOW, hipMemcpyDeviceToDevice, s));   // the last 32 KiB, older text included
      HIPCHK(stream_wait(s));   // the next round overwrites the scratch
      S.decode_ms += ev_ms(c->ev[4], c->ev[5]);
      S.window_ms += ev_ms(c->ev[6], c->ev[7]);
      S.resolve_ms += ev_ms(c->ev[7], c->ev[8]);
      S.rounds++;
      i = j;
    }
    if (member != chain.members) throw StatusError{KSLAM_ERR_INTERNAL, "gunzip: the rounds checked " + std::to_string(member) + " members of " + std::to_string(chain.members)};
    c->gz.stats = S;
    *out = h;
    *out_len = chain.text_len;
  });
  if (st != KSLAM_OK && h) pinned_put(c, h);
  if (st != KSLAM_OK && out) *out = nullptr;
  return st;
}

kslam_status kslam_gunzip_set_chunk(kslam_ctx *c, uint64_t bytes) {
  return guarded(c, [&] {
    if (bytes && (bytes % 4 || bytes < KSLAM_GUNZIP_CHUNK_MIN || bytes > (1ull << 28)))
      throw StatusError{KSLAM_ERR_ARG, "kslam_gunzip_set_chunk: " + std::to_string(bytes) + " is not a multiple of 4 between 1024 and 2^28"};
    c->gz.chunk = bytes;
  });
}

kslam_status kslam_gunzip_set_round(kslam_ctx *c, uint64_t symbols) {
  return guarded(c, [&] {
    if (symbols && symbols < chunk_of(c))
      throw StatusError{KSLAM_ERR_ARG, "kslam_gunzip_set_round: " + std::to_string(symbols) + " symbols are less than one chunk (" + std::to_string(chunk_of(c)) + ")"};
    c->gz.round = symbols;
  });
}

kslam_status kslam_gunzip_last_stats(kslam_ctx *c, kslam_gunzip_stats *stats) {
  if (!c || !stats) return KSLAM_ERR_ARG;
  *stats = c->gz.stats;
  return KSLAM_OK;
}

}  // extern "C"
