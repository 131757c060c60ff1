// enc_k256w_body.hpp — what the k = 256, n = 1024 encode's one kernel body
// (enc_k256w_tile.inc) needs at namespace scope: its LDS map,
// staging swizzle and row-store geometry.  The body is shared by encode_k256w
// (enc_k256w.hip: the uniform batch) and encode_k256w_ragged
// (enc_k256w_ragged.hip: items of unequal length, ragged.hpp).  It is
// parameterised by a geometry policy (enc_w_common.hpp: the contract, the
// ticket protocol, and the uniform batch's UniformGeo).
#pragma once

#include "enc_w_common.hpp"

namespace ecamd {
namespace {
namespace k256w {

constexpr int K = 256;
constexpr int TILE = 8 * WAVES;  // pieces per tile
constexpr uint32_t XCH0 = kCImgBytes;      // the waves' regions follow the tables
constexpr uint32_t SLOT = XCH0 + WAVES * XCH_BYTES;  // the next tile's ticket (dynamic schedule)
template <typename Geo>
constexpr int lds_bytes() {
  static_assert(2 * (SLOT + Geo::SLOT_BYTES) <= 160 * 1024, "two workgroups per CU");
  return int(SLOT + Geo::SLOT_BYTES);
}

// ---- own-region staging: wave w stages its 8 pieces x 256 rows in its own
// 4 KB region, 16 B per row (half = instance); row v in 256-B block v >> 4 at
// 16-B slot (v ^ (v >> 4) ^ 2w) & 15.  The row reads (lane = row-in-8 << 3 |
// source wave c) hit 16 distinct slots in every ds_read_b128 lane group; the
// layout-A writes are 2-way (the minimum for 8-B writes of one instance).
__host__ __device__ constexpr uint32_t soff8(uint32_t v, uint32_t w) {
  return ((v >> 4) << 8) | (((v ^ (v >> 4) ^ (w << 1)) & 15) << 4);
}

__device__ __forceinline__ void stage_own8(const State &s, uint8_t *xch, uint32_t q, uint32_t inst,
                                           uint32_t wave) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
    *reinterpret_cast<uint2 *>(xch + soff8(posA(q, r), wave) + 8 * inst) = to_be(s.l[r], s.h[r]);
}

// the row stores' geometry (enc_w_common.hpp store_own): lane = (row in 8,
// source wave c = 16-B chunk of pieces [8c, 8c + 8)); row v = it * 64 + wave *
// 8 + lane / 8, 8 lanes per 128-B row segment
struct Rows {
  static constexpr int TILE = k256w::TILE, K = k256w::K;
  static constexpr uint32_t VSTEP = 8 * WAVES;
  __device__ static __forceinline__ RowLane lane_role(uint32_t wave, uint32_t lane) {
    const uint32_t c = lane & 7;
    const uint32_t v0 = wave * 8 + (lane >> 3);
    return {v0, c, XCH0 + c * XCH_BYTES + soff8(v0, c)};
  }
  __device__ static __forceinline__ v4u read(uint32_t a, int it) { return lds_r128(a ^ soff8(uint32_t(it) * VSTEP, 0)); }
};

}  // namespace k256w
}  // namespace
}  // namespace ecamd
