// table_images.hpp — layout of the device table images and their host
// builders: the contract between the host and every fast kernel.  No HIP
// header: this and table_images.cpp also build with a plain C++17 compiler
// (tests/cpp/table_images_check.cpp pins every byte without a device).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "gf_field.hpp"

#ifdef __HIPCC__
#define ECAMD_HOST_DEVICE __host__ __device__
#else
#define ECAMD_HOST_DEVICE
#endif

namespace ecamd {

// LDS images of the multiply tables of one 1023-skew set, in the swizzled
// LdsTabs<1024> layout: set q = skews[1024 q + i], i < 1023 (q = 0..3), i.e.
// the tables of an FFT / IFFT of size <= 1024 at index 1024 q.  A kernel loads
// a set with one coalesced 80 KB copy instead of a 1023-entry gather.
constexpr size_t kTabImageBytes = 5 * 1024 * 16;
constexpr int kTabImages = 4;

// The LdsTabs slot of entry i: its byte offset inside plane 0, and the entry
// whose slot is 16-byte chunk `chunk` of a plane.  The kernels keep their own
// wording of the two (ec_device.hpp LdsTabs::addr, dec_n4096.hip
// n4096_out_image: calling these changed their code), hence the assertion.
constexpr uint32_t lds_tab_slot(uint32_t i) { return ((i >> 4) << 8) + (((i ^ (i >> 4) ^ (i >> 8)) & 15) << 4); }
constexpr uint32_t lds_tab_entry(uint32_t chunk) {
  return (chunk & ~15u) | ((chunk ^ (chunk >> 4) ^ (chunk >> 8)) & 15u);
}
constexpr bool lds_tab_round_trip() {
  for (uint32_t i = 0; i < 1024; ++i)
    if (lds_tab_entry(lds_tab_slot(i) >> 4) != i) return false;
  return true;
}
static_assert(lds_tab_round_trip(), "lds_tab_entry inverts lds_tab_slot over i < 1024");

// Tower images: the same slots in tower coordinates.  Entry
// i of set q is a subfield table (MulTabSub: plane 0 = w[0..3], dword 0 of
// plane 1 = w[4]) when its stage ctz(1024 q + i + 1) >= tower_sub_min(q) --
// every such skew is < 256 -- and a general tower table (Field::tower_tab)
// below; a kernel reading set q uses mul_acc_sub at exactly those stages.
constexpr int tower_sub_min(int q) { return q == 0 ? 2 : q == 1 ? 3 : 4; }

// F9 variants of tower image 0: entry i holds a MulTabF9
// (plane q = w[4q .. 4q + 3]) where f9_slot(kind, i), the tower image's table
// elsewhere.  Kind 0 (reconstruct_n1024): the stage-1 entries (i = 1 mod 4,
// elements 0..510); kind 1 (encode_k256): also the stage-0 entries
// 256..510 (elements 256..510, its coset-256 FFT).  Their elements' high
// tower coordinate is 0 or 1 (tests/cpp/tower_check.cpp).
constexpr int kF9Images = 2;
constexpr bool f9_slot(int kind, uint32_t i) {
  return i % 4 == 1 || (kind == 1 && i % 2 == 0 && i >= 256 && i < 512);
}

// Element-indexed compact image (the n = 1024 encode).  The
// skew of a stage-m butterfly at position pos of an FFT / IFFT at index `off`
// (additive_fft.hpp:99-141) is the element 2 x, x = (pos + off) >> (m + 1)
// (skews[i] = log(((i + 1) >> ctz(i + 1)) - 1); checked against the oracle),
// so a table set can be indexed by x instead of by skew slot.  For the
// k = 256 / n = 1024 encode x < 512, and the element's tower coordinates put
// it in one of three kinds: x < 128 subfield (MulTabSub), 128 <= x < 256 F9
// (MulTabF9), 256 <= x < 512 general (Field::tower_tab).  Plane q of entry x
// sits at base(kind, q) | cimg_lin(x ^ kind_bit), cimg_lin GF(2)-linear (the
// LdsTabs swizzle applied to x), so every table address is a per-lane base XOR
// a wave-uniform value; 32 KB instead of the 80 KB skew-slot image.
constexpr uint32_t kCImgGen = 0, kCImgGenPlane = 4096;      // 5 planes x 256 entries
constexpr uint32_t kCImgF9 = 20480, kCImgF9Plane = 2048;    // 4 planes x 128 entries
constexpr uint32_t kCImgSub0 = 28672, kCImgSub1 = 30720;    // plane 0 / dword 0 of plane 1, 128 entries
constexpr uint32_t kCImgBytes = 32768;
ECAMD_HOST_DEVICE constexpr uint32_t cimg_lin(uint32_t x) {
  return ((x >> 4) << 8) | (((x ^ (x >> 4) ^ (x >> 8)) & 15) << 4);
}

// Per-coset extension images of the k = 512 encode (enc_k512w.hip; n = 2048 /
// 4096): the general tables its FFT_512 at coset j (index 512 j, j = 1..7)
// needs beyond the compact image's subfield and F9 entries, element-indexed
// like it: stage m (0, 1, 2) entry e = x - (512 j >> (m + 1)), e < 256 >> m,
// plane q at kEImg512Stage[m] + q * (4096 >> m) + cimg_lin(e).  Coset 1 uses
// stage 0's part (20 KB), cosets 2-3 stages 0-1 (30 KB), cosets 4-7 all.
constexpr uint32_t kEImg512Bytes = 35840, kEImg512Cosets = 7;
constexpr uint32_t kEImg512Stage[3] = {0, 20480, 30720};

// The same for the k = 256, n = 2048 encode (enc_kw.hip): stage 0 of cosets
// j = 4..7 (elements 128 j + e, e < 128), plane q at q * 2048 + cimg_lin(e).
constexpr uint32_t kEImg256Bytes = 10240, kEImg256Cosets = 4;

// One builder per image (DevTables, ec_kernels.hpp).  The F9 and compact
// builders return an empty vector if Field::f9_tab refuses one of their
// constants (tower_check: never).
std::vector<uint8_t> tower_images(const Field &f);    // kTabImages x kTabImageBytes
std::vector<uint8_t> f9_images(const Field &f);       // kF9Images x kTabImageBytes
std::vector<uint8_t> compact_image(const Field &f);   // kCImgBytes
std::vector<uint8_t> eimg512_images(const Field &f);  // kEImg512Cosets x kEImg512Bytes
std::vector<uint8_t> eimg256_images(const Field &f);  // kEImg256Cosets x kEImg256Bytes
std::vector<MulTab> mslot_tables(const Field &f);     // [i] = mtab[skews[i]]: by skew slot, one load

}  // namespace ecamd
