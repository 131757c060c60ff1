// table_images_check.cpp — CPU check of the device table images
// (erasure-coding-crust_amd/csrc/table_images.hpp), built by
// tests/test_table_images.py with g++ against gf_field.cpp and
// table_images.cpp.  Prints "image <name> <bytes> <sha256>" for each of the six
// images (compared with tests/golden/table_images.json, recorded from the
// upload loops these builders replaced), and reads entries of the tower images
// back from their slots with the address arithmetic written out here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gf_field.hpp"
#include "table_images.hpp"

using namespace ecamd;

// SHA-256 (FIPS 180-4) of n bytes, as lower-case hex
static std::string sha256(const uint8_t *data, size_t n) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
      0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
      0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
      0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
      0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  std::vector<uint8_t> m(data, data + n);
  m.push_back(0x80);
  while (m.size() % 64 != 56) m.push_back(0);
  for (int s = 56; s >= 0; s -= 8) m.push_back(uint8_t((uint64_t(n) * 8) >> s));
  const auto rotr = [](uint32_t x, int r) { return (x >> r) | (x << (32 - r)); };
  for (size_t off = 0; off < m.size(); off += 64) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
      w[i] = uint32_t(m[off + 4 * i]) << 24 | uint32_t(m[off + 4 * i + 1]) << 16 | uint32_t(m[off + 4 * i + 2]) << 8 |
             m[off + 4 * i + 3];
    for (int i = 16; i < 64; ++i)
      w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] +
             (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
    uint32_t v[8];
    std::memcpy(v, h, sizeof v);
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = v[7] + (rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) +
                          K[i] + w[i];
      const uint32_t t2 = (rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
      for (int j = 7; j > 0; --j) v[j] = v[j - 1];
      v[4] += t1;
      v[0] = t1 + t2;
    }
    for (int i = 0; i < 8; ++i) h[i] += v[i];
  }
  char hex[65];
  for (int i = 0; i < 8; ++i) std::snprintf(hex + 8 * i, 9, "%08x", h[i]);
  return hex;
}

template <typename V>
static void report(const char *name, const V &v) {
  const size_t bytes = v.size() * sizeof(v[0]);
  std::printf("image %s %zu %s\n", name, bytes, sha256(reinterpret_cast<const uint8_t *>(v.data()), bytes).c_str());
}

int main() {
  const Field &f = field();
  const std::vector<uint8_t> tower = tower_images(f);
  report("tower", tower);
  report("f9", f9_images(f));
  report("compact", compact_image(f));
  report("eimg512", eimg512_images(f));
  report("eimg256", eimg256_images(f));
  report("mslot", mslot_tables(f));
  // entry i of tower image q, read back as a kernel finds it (LdsTabs<1024>:
  // 5 planes of 1024 16-byte slots, the slot within its group of 16 XORed with
  // i ^ i >> 4 ^ i >> 8): the subfield or the general tower table of
  // skews[1024 q + i], by the tower_sub_min rule
  int fails = 0;
  if (tower.size() != size_t(4) * 81920) return 1;
  for (uint32_t q = 0; q < 4; ++q)
    for (uint32_t i : {0u, 1u, 15u, 16u, 255u, 256u, 1022u}) {
      const uint32_t c = f.skews[1024 * q + i];
      const size_t at = size_t(q) * 81920 + (i / 16) * 256 + ((i ^ (i >> 4) ^ (i >> 8)) % 16) * 16;
      uint32_t got[20];
      for (uint32_t plane = 0; plane < 5; ++plane) std::memcpy(&got[4 * plane], &tower[at + plane * 16384], 16);
      bool same;
      if (__builtin_ctz(1024 * q + i + 1) >= tower_sub_min(int(q))) {
        const MulTabSub u = f.sub_tab(c);
        same = std::memcmp(got, u.w, 20) == 0;
      } else {
        const MulTab g = f.tower_tab(c);
        same = std::memcmp(got, g.w, 80) == 0;
      }
      if (!same) {
        std::printf("FAIL tower image %u entry %u\n", q, i);
        ++fails;
      }
    }
  if (fails) return 1;
  std::printf("tower slots ok\n");
  return 0;
}
