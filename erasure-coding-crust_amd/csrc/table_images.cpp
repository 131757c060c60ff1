// table_images.cpp — the host builders of the device table images.
#include "table_images.hpp"

#include <cstring>

namespace ecamd {
namespace {
// planes 0 .. n - 1 of a table (plane q = w[4 q .. 4 q + 3]) to dst + q * stride
void put(uint8_t *dst, const uint32_t *w, uint32_t n, size_t stride) {
  for (uint32_t q = 0; q < n; ++q) std::memcpy(dst + q * stride, w + 4 * q, 16);
}
// a subfield table: plane 0 to p0, dword 0 of plane 1 to p1
void put_sub(uint8_t *p0, uint8_t *p1, const MulTabSub &u) {
  std::memcpy(p0, &u.w[0], 16);
  std::memcpy(p1, &u.w[4], 4);
}
// tower image q to dst (kTabImageBytes of zeroes)
void tower_image(const Field &f, int q, uint8_t *dst) {
  for (uint32_t i = 0; i < 1023; ++i) {
    const uint32_t c = f.skews[1024 * q + i];
    uint8_t *slot = dst + lds_tab_slot(i);
    if (__builtin_ctz(1024 * q + i + 1) >= tower_sub_min(q)) put_sub(slot, slot + 16384, f.sub_tab(c));
    else put(slot, f.tower_tab(c).w, 5, 16384);
  }
}
}  // namespace

std::vector<uint8_t> tower_images(const Field &f) {
  std::vector<uint8_t> img(kTabImages * kTabImageBytes, 0);
  for (int q = 0; q < kTabImages; ++q) tower_image(f, q, &img[size_t(q) * kTabImageBytes]);
  return img;
}

std::vector<uint8_t> f9_images(const Field &f) {
  std::vector<uint8_t> img(kF9Images * kTabImageBytes, 0);
  for (int kind = 0; kind < kF9Images; ++kind) {
    uint8_t *dst = &img[size_t(kind) * kTabImageBytes];
    tower_image(f, 0, dst);
    for (uint32_t i = 0; i < 1023; ++i) {
      if (!f9_slot(kind, i)) continue;
      MulTabF9 t9;
      if (!f.f9_tab(f.skews[i], &t9)) return {};
      put(dst + lds_tab_slot(i), t9.w, 4, 16384);
    }
  }
  return img;
}

std::vector<uint8_t> compact_image(const Field &f) {
  std::vector<uint8_t> cimg(kCImgBytes, 0);
  for (uint32_t x = 0; x < 512; ++x) {  // entry x = element 2 x
    const uint32_t e = 2 * x, c = e == 0 ? kZeroTab : f.log[e];
    MulTabF9 t9;
    if (x < 128) {
      put_sub(&cimg[kCImgSub0 | cimg_lin(x)], &cimg[kCImgSub1 | cimg_lin(x)], f.sub_tab(c));
    } else if (x < 256) {
      if (!f.f9_tab(c, &t9)) return {};  // (tower(e) >> 8 == 1 for 256 <= e < 512)
      put(&cimg[kCImgF9 | cimg_lin(x ^ 128)], t9.w, 4, kCImgF9Plane);
    } else {
      put(&cimg[kCImgGen | cimg_lin(x ^ 256)], f.tower_tab(c).w, 5, kCImgGenPlane);
    }
  }
  return cimg;
}

std::vector<uint8_t> eimg512_images(const Field &f) {
  std::vector<uint8_t> eimg(kEImg512Cosets * kEImg512Bytes, 0);
  for (uint32_t j = 1; j <= kEImg512Cosets; ++j)
    for (uint32_t m = 0; m < 3; ++m)
      for (uint32_t e = 0; e < (256u >> m); ++e) {  // general tower tables of the elements x
        const uint32_t x = ((512 * j) >> (m + 1)) + e;
        put(&eimg[(j - 1) * kEImg512Bytes + kEImg512Stage[m] + cimg_lin(e)], f.tower_tab(f.log[2 * x]).w, 5,
            4096 >> m);
      }
  return eimg;
}

std::vector<uint8_t> eimg256_images(const Field &f) {
  std::vector<uint8_t> eimg(kEImg256Cosets * kEImg256Bytes, 0);
  for (uint32_t j = 4; j < 4 + kEImg256Cosets; ++j)
    for (uint32_t e = 0; e < 128; ++e)
      put(&eimg[(j - 4) * kEImg256Bytes + cimg_lin(e)], f.tower_tab(f.log[2 * (128 * j + e)]).w, 5, 2048);
  return eimg;
}

std::vector<MulTab> mslot_tables(const Field &f) {
  std::vector<MulTab> ms(f.skews.size());
  for (size_t i = 0; i < ms.size(); ++i) ms[i] = f.mtab[f.skews[i]];
  return ms;
}

}  // namespace ecamd
