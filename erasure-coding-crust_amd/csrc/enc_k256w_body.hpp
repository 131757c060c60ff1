// enc_k256w_body.hpp — what the k = 256, n = 1024 encode's one kernel body
// (enc_k256w_tile.inc) needs at namespace scope: its LDS map,
// staging swizzle, row-store geometry and the geometry policies.  The body is
// shared by encode_k256w (enc_k256w.hip: the uniform batch) and
// encode_k256w_ragged (enc_k256w_ragged.hip: items of unequal length,
// ragged.hpp).  It is parameterised by a geometry policy that
// says, for a tile ticket, which payload bytes, shard rows, piece count and
// pitch the tile works on, and how the ticket travels from the thread that
// takes it to the other waves.  The transforms, the staging, the row stores
// and the order of barriers do not depend on it.
//
// A geometry policy Geo provides (all values wave-uniform):
//   Tile, ticket(T)         what a wave keeps of a ticket between reading it
//                           from LDS and the end of its tile; ticket(T) <
//                           Pre::total means a tile of the launch
//   SLOT_BYTES              LDS bytes at SLOT the policy publishes tickets in
//   Pre, prepare()          what the policy works out once per launch; total:
//                           the launch's tiles
//   publishes(tid0)         the threads that take part in publishing a ticket
//                           (thread 0, or all of wave 0); the call sites are
//                           reached by whole waves, wave 0 always among them
//   first(slot, tid0)       those threads: take and publish the workgroup's
//                           first ticket
//   next_ticket(T)          thread 0: the ticket after tile T's
//   publish(slot, ticket, tid0)
//                           those threads: resolve and store thread 0's ticket
//   read(slot).t            the published Tile (after a barrier)
//   Loc, loc(pre, T)        where a valid tile's payload bytes are, as far as
//                           it is worked out when the tile is read
//   loc_or_none(pre, T)     the same for a tile that may be past the end: then
//                           a place for which the fetch loads nothing
//   fetch(pre, Loc)         the payload fetch's geometry (Fetch)
//   At, at(pre, T), piece0(At), rows(At), npieces(pre, T), sstride(T)
//                           geometry of a valid tile's transforms and stores
#pragma once

#include <type_traits>

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

using LdsWord = __attribute__((address_space(3))) volatile uint32_t;

// what the payload fetch of a tile needs: the item's payload, its length in
// bytes and pieces, the tile's first piece
struct Fetch {
  const uint8_t *P;
  uint64_t plen, npieces, piece0;
};

// The uniform batch: payload b at b * pstride, its rows at b * nv * sstride,
// every payload plen bytes: ticket cur is tile cur % tiles_pp of payload
// cur / tiles_pp.  Without a counter (no scratch) a static grid stride
// (slower: the two workgroups of a CU drift apart).
struct UniformGeo {
  const uint8_t *payloads;
  uint64_t plen_, pstride;
  uint8_t *shards;
  uint64_t slen, sstride_;
  int nv;
  uint32_t batch;
  uint32_t *tick;
  using Tile = uint32_t;  // the ticket itself
  static constexpr uint32_t SLOT_BYTES = 16;
  struct Pre {  // per launch: pieces and tiles per payload, tiles of the launch
    uint64_t npieces;
    uint32_t tiles_pp, total;
  };
  __device__ __forceinline__ Pre prepare() const {
    const uint64_t npieces = slen / 2;
    const uint32_t tiles_pp = uint32_t((npieces + TILE - 1) / TILE);
    return {npieces, tiles_pp, tiles_pp * batch};  // < 2^32 (launch_encode_k256w)
  }
  __device__ __forceinline__ bool publishes(uint32_t tid0) const { return tid0 == 0; }
  __device__ __forceinline__ void first(LdsWord *slot, uint32_t) const {
    *slot = tick ? atomicAdd(tick, 1u) : blockIdx.x;
  }
  __device__ __forceinline__ uint32_t next_ticket(Tile c) const {
    return tick ? atomicAdd(tick, 1u) : c + gridDim.x;
  }
  __device__ __forceinline__ void publish(LdsWord *slot, uint32_t ticket, uint32_t) const { *slot = ticket; }
  struct Read {
    Tile t;
  };
  __device__ __forceinline__ Read read(LdsWord *slot) const { return {uint32_t(__builtin_amdgcn_readfirstlane(*slot))}; }
  __device__ __forceinline__ uint32_t ticket(Tile c) const { return c; }
  struct Loc {
    uint64_t b, i;  // payload, tile in the payload
  };
  __device__ __forceinline__ Loc loc(const Pre &p, Tile c) const { return {c / p.tiles_pp, c % p.tiles_pp}; }
  // past the end: the zero path, no loads
  __device__ __forceinline__ Loc loc_or_none(const Pre &p, Tile c) const {
    return {c < p.total ? uint64_t(c / p.tiles_pp) : uint64_t(0),
            uint64_t(c < p.total ? c % p.tiles_pp : p.tiles_pp)};
  }
  __device__ __forceinline__ Fetch fetch(const Pre &p, Loc l) const {
    return {payloads + l.b * pstride, plen_, p.npieces, l.i * TILE};
  }
  struct At {
    uint64_t b, piece0;  // a valid tile's payload and first piece
  };
  __device__ __forceinline__ At at(const Pre &p, Tile c) const { return {c / p.tiles_pp, uint64_t(c % p.tiles_pp) * TILE}; }
  __device__ __forceinline__ uint64_t piece0(At a) const { return a.piece0; }
  __device__ __forceinline__ uint64_t npieces(const Pre &p, Tile) const { return p.npieces; }
  __device__ __forceinline__ uint64_t sstride(Tile) const { return sstride_; }
  __device__ __forceinline__ uint8_t *rows(At a) const { return shards + a.b * uint64_t(nv) * sstride_; }
};

}  // namespace k256w
}  // namespace
}  // namespace ecamd
