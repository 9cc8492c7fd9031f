// gunzip_check.cpp -- the host side of plain gzip input (k-slam_amd/host/gunzip.cpp) run alone, for a sanitizer build:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o gunzip_check
//       tools/gunzip_check.cpp k-slam_amd/host/gunzip.cpp -lpthread     (one line)
//   ./gunzip_check
//
// It walks member headers of every shape at every truncation length (each piece in a heap block of exactly its size, so
// that a read one byte too far is an error the sanitizer sees), and follows hand-made link tables: a plain chain, false
// starts beside it, starts the chain jumps over, a chain that breaks (abandoned, never run, pointing backwards or out of the
// table), errors on and off the chain, and a match that reaches before its member.  Prints "gunzip_check: ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/kslam_gunzip.h"
#include "../k-slam_amd/csrc/gzip_header.h"
#include "../k-slam_amd/host/gunzip.hpp"
#include "../k-slam_amd/host/workers.hpp"   // g_err: what kslam_tail_last_error() hands out

using namespace kslam_host;

namespace {

int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      failures++;                                                        \
    }                                                                    \
  } while (0)

std::vector<uint8_t> make_header(uint32_t flags, size_t extra, size_t name, size_t comment) {
  std::vector<uint8_t> h = {0x1f, 0x8b, 8, (uint8_t)flags, 0, 0, 0, 0, 0, 0xff};
  if (flags & 4) {
    h.push_back((uint8_t)(extra & 0xff));
    h.push_back((uint8_t)(extra >> 8));
    for (size_t i = 0; i < extra; i++) h.push_back((uint8_t)(i * 7 + 1));
  }
  if (flags & 8) {
    h.insert(h.end(), name, 'n');
    h.push_back(0);
  }
  if (flags & 16) {
    h.insert(h.end(), comment, 'c');
    h.push_back(0);
  }
  if (flags & 2) {
    h.push_back(0x12);
    h.push_back(0x34);
  }
  return h;
}

// data[0 .. n) in a heap block of exactly n bytes
kslam_status header_of(const std::vector<uint8_t> &data, size_t n, uint64_t *at) {
  uint8_t *p = static_cast<uint8_t *>(std::malloc(n ? n : 1));
  if (n) std::memcpy(p, data.data(), n);
  const kslam_status st = kslam_gunzip_header(n ? p : nullptr, n, at);
  std::free(p);
  return st;
}

void check_headers() {
  const size_t sizes[][3] = {{0, 0, 0}, {3, 4, 1}, {300, 70, 13}, {65535, 1, 1}};
  for (uint32_t flags = 0; flags < 32; flags += 2)
    for (const auto &s : sizes) {
      std::vector<uint8_t> h = make_header(flags, s[0], s[1], s[2]);
      const size_t whole = h.size();
      h.push_back(0x03);   // deflate data behind it
      h.push_back(0x00);
      uint64_t at = 0;
      CHECK(header_of(h, h.size(), &at) == KSLAM_OK && at == whole);
      CHECK(header_of(h, whole, &at) == KSLAM_OK && at == whole);
      const size_t step = whole > 2000 ? 97 : 1;   // the long FEXTRA field: not every one of its 65 535 bytes
      for (size_t cut = 0; cut < whole; cut += (cut < 16 || cut + 16 >= whole) ? 1 : step) {
        CHECK(header_of(h, cut, &at) == KSLAM_ERR_ARG && at == 0);
        const std::string msg = g_err;
        CHECK(msg.find(cut < 2 ? "not a gzip member" : "gzip header") != std::string::npos);
      }
    }
  std::vector<uint8_t> h = make_header(0, 0, 0, 0);
  uint64_t at = 0;
  for (uint32_t bit : {0x20u, 0x40u, 0x80u}) {
    h[3] = (uint8_t)bit;
    CHECK(header_of(h, h.size(), &at) == KSLAM_ERR_ARG);
  }
  h[3] = 0;
  h[2] = 7;
  CHECK(header_of(h, h.size(), &at) == KSLAM_ERR_ARG);
  h[2] = 8;
  h[1] = 0x8c;
  CHECK(header_of(h, h.size(), &at) == KSLAM_ERR_ARG);
  CHECK(kslam_gunzip_header(h.data(), h.size(), nullptr) == KSLAM_ERR_ARG);
  // the walk from the middle of a buffer, as the device uses it
  std::vector<uint8_t> two = make_header(8, 0, 5, 0);
  const size_t first = two.size();
  const std::vector<uint8_t> second = make_header(4 | 2, 9, 0, 0);
  two.insert(two.end(), second.begin(), second.end());
  CHECK(kslam::gzip_header_walk(two.data(), first, two.size(), &at) == kslam::GZH_OK && at == two.size());
  CHECK(kslam::gzip_header_walk(two.data(), first, two.size() - 1, &at) == kslam::GZH_HEADER);
  CHECK(kslam::gzip_header_walk(two.data(), two.size(), two.size(), &at) == kslam::GZH_NOT_MEMBER);
}

GunzipLink hit(uint32_t next, uint64_t out, uint64_t members = 0, uint64_t member_at = 0, uint64_t member_out = 0, uint32_t need_back = 0) {
  GunzipLink l{};
  l.status = GZL_HIT;
  l.next = next;
  l.out_bytes = out;
  l.members = members;
  l.member_at = member_at;
  l.member_out = member_out;
  l.need_back = need_back;
  return l;
}
GunzipLink eof(uint64_t out, uint64_t members) {
  GunzipLink l = hit(0, out, members);
  l.status = GZL_EOF;
  return l;
}
GunzipLink error(uint32_t kind, uint64_t members = 0, uint64_t member_at = 0) {
  GunzipLink l{};
  l.status = GZL_ERROR;
  l.kind = kind;
  l.members = members;
  l.member_at = member_at;
  return l;
}
GunzipLink with_status(uint32_t status) {
  GunzipLink l{};
  l.status = status;
  return l;
}

void check_chains() {
  {   // one start: the whole file on one wave
    const GunzipLink t[] = {eof(1000, 3)};
    const GunzipChain c = gunzip_chain_walk(t, 1, 0);
    CHECK(c.state == GunzipChain::COMPLETE && c.spans.size() == 1 && c.members == 3 && c.text_len == 1000);
    CHECK(c.spans[0].out == 0 && c.spans[0].n_out == 1000 && c.spans[0].member0 == 0 && c.spans[0].n_members == 3);
  }
  {   // 0 -> 2 -> 3 -> end; start 1 is false (its wave died), start 4 is false and claims a link to 5; 5 does not exist
    const GunzipLink t[] = {hit(2, 100), error(5), hit(3, 50, 2, 777, 20), eof(30, 1), hit(5, 9)};
    const GunzipChain c = gunzip_chain_walk(t, 5, 0);
    CHECK(c.state == GunzipChain::COMPLETE && c.spans.size() == 3 && c.members == 3 && c.text_len == 180);
    CHECK(c.spans[1].start == 2 && c.spans[1].out == 100 && c.spans[1].member0 == 0 && c.spans[1].n_members == 2);
    CHECK(c.spans[2].start == 3 && c.spans[2].out == 150 && c.spans[2].member0 == 2 && c.spans[2].n_members == 1);
  }
  {   // a start found inside the first member's header sorts before the first block: the walk begins at 1
    const GunzipLink t[] = {error(1), hit(2, 10), eof(5, 1)};
    const GunzipChain c = gunzip_chain_walk(t, 3, 1);
    CHECK(c.state == GunzipChain::COMPLETE && c.spans.size() == 2 && c.spans[0].start == 1 && c.text_len == 15);
  }
  {   // a false start that ends on a true one: never looked at, because nothing links TO it
    const GunzipLink t[] = {hit(2, 100), hit(2, 12345), eof(1, 1)};
    const GunzipChain c = gunzip_chain_walk(t, 3, 0);
    CHECK(c.state == GunzipChain::COMPLETE && c.text_len == 101 && c.spans.size() == 2);
  }
  // broken chains: abandoned, never run, pointing at itself, backwards, out of the table; and a first start beyond the table
  for (int k = 0; k < 5; k++) {
    GunzipLink t[] = {hit(1, 10), hit(2, 10), eof(10, 1)};
    if (k == 0) t[1] = with_status(GZL_ABANDONED);
    if (k == 1) t[1] = with_status(GZL_NONE);
    if (k == 2) t[1].next = 1;
    if (k == 3) t[1].next = 0;
    if (k == 4) t[1].next = 3;
    const GunzipChain c = gunzip_chain_walk(t, 3, 0);
    CHECK(c.state == GunzipChain::BROKEN && c.broken_at == 1);
    t[1] = hit(2, 10);   // the wave ran again, to the end: the chain closes
    const GunzipChain d = gunzip_chain_walk(t, 3, 0);
    CHECK(d.state == GunzipChain::COMPLETE && d.text_len == 30);
  }
  CHECK(gunzip_chain_walk(nullptr, 0, 0).state == GunzipChain::BROKEN);
  {   // an unknown status is no link
    const GunzipLink t[] = {with_status(99)};
    CHECK(gunzip_chain_walk(t, 1, 0).state == GunzipChain::BROKEN);
  }
  {   // an error on the chain is the file's: in the member the wave started in (no member ended on the way) ...
    const GunzipLink t[] = {hit(1, 100, 1, 400, 60), error(5)};
    const GunzipChain c = gunzip_chain_walk(t, 2, 0);
    CHECK(c.state == GunzipChain::FAILED && c.bad_member == 1 && c.bad_at == 400 && c.bad_kind == 5);
  }
  {   // ... or in one that began on the way
    const GunzipLink t[] = {hit(1, 100, 1, 400, 60), error(GZK_NOT_MEMBER, 2, 900)};
    const GunzipChain c = gunzip_chain_walk(t, 2, 0);
    CHECK(c.state == GunzipChain::FAILED && c.bad_member == 3 && c.bad_at == 900 && c.bad_kind == GZK_NOT_MEMBER);
    CHECK(std::string(gunzip_kind_name(c.bad_kind)) == "not a gzip member" && gunzip_kind_name(5) == nullptr);
    CHECK(gunzip_error_text(3, 900, "x") == "gzip member 3 (byte offset 900): x");
  }
  {   // a match before the wave's first byte: fine while it stays inside its member (40 bytes of it came before), refused beyond
    GunzipLink t[] = {hit(1, 100, 1, 400, 60), hit(2, 10, 0, 0, 0, 40), eof(1, 1)};
    CHECK(gunzip_chain_walk(t, 3, 0).state == GunzipChain::COMPLETE);
    t[1].need_back = 41;
    const GunzipChain c = gunzip_chain_walk(t, 3, 0);
    CHECK(c.state == GunzipChain::FAILED && c.bad_member == 1 && c.bad_at == 400 && c.bad_kind == GZK_DISTANCE);
    t[1].need_back = 0;
    t[0].need_back = 1;   // the file's first wave stands at its member's first byte
    CHECK(gunzip_chain_walk(t, 3, 0).state == GunzipChain::FAILED);
  }
}

}  // namespace

int main() {
  check_headers();
  check_chains();
  if (failures) {
    std::fprintf(stderr, "gunzip_check: %d checks failed\n", failures);
    return 1;
  }
  std::puts("gunzip_check: ok");
  return 0;
}
