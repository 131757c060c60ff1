// dec_n1024x_body.hpp — what reconstruct_n1024x's one kernel body
// (dec_n1024x_tile.inc; dec_n1024x.hip's header comment and DESIGN.md describe
// the kernel) needs at namespace scope: the two forms' LDS maps, the IFFT
// passes, and the geometry policies.  The body is shared by
// reconstruct_n1024x<12 / 16> (the uniform batch) and
// reconstruct_n1024x_ragged (dec_n1024x_ragged.hip: items of unequal length,
// ragged.hpp).  It is parameterised by a geometry policy that says, for a
// tile ticket, which item it belongs to (the item indexes the gather order and
// the present / locator rows exactly as the payload index does), where the
// item's shard rows and output bytes are, its shard length and pitch, and how
// a ticket travels from the thread that takes it to the other waves.
//
// A geometry policy Geo provides (all values wave-uniform):
//   Tile                   what a wave keeps of a ticket; Tile::ticket <
//                          Pre::total means a tile of the launch
//   Pre, prepare()         what the policy works out once per launch; total:
//                          the launch's tiles
//   first_ticket()         thread 0, before the table image is copied: the
//                          first ticket it takes from the counter
//   settle_first(slot, taken, tid0)
//                          after the image's barrier, every thread (taken:
//                          thread 0's first ticket): settles the workgroup's
//                          first tile
//   second_ticket(taken, tid0)
//                          thread 0's ticket for the tile after the first,
//                          published next
//   first_tile(slot)       the workgroup's first tile
//   next_ticket()          thread 0: a further ticket
//   publishes(tid0), publish(slot, ticket, tid0)
//                          the threads for which publishes() holds (thread 0,
//                          or all of wave 0, which always reaches the tile's
//                          end with every lane active) resolve and store
//                          thread 0's ticket
//   read(slot)             the published Tile (after a barrier)
//   item(pre, T)           the item of a valid tile
//   where(pre, T)          a valid tile's geometry (Where)
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "dec_n1024_common.hpp"
#include "ec_device.hpp"
#include "ec_kernels.hpp"
#include "cimg.hpp"

namespace ecamd {
namespace {
using namespace n1024;
constexpr int TAB_REGION = int(kCImgBytes);  // the element-indexed compact image
static_assert(TAB_REGION % 8192 == 0, "regions 8 KB aligned: region addresses are base | rz");
constexpr uint32_t STG_PITCH = 112;
// the two forms' sizes and LDS maps
template <int WAVES>
struct Form {
  static_assert(WAVES == 12 || WAVES == 16, "three or four waves per SIMD");
  static constexpr int THREADS = 64 * WAVES;
  static constexpr int COLS = 4 * WAVES;     // shard columns per tile
  static constexpr int ROW_WORDS = COLS / 2;  // dwords of a row segment (96 B / 128 B)
  // gather slots per thread: tid and, with 768 threads, 768 + tid below 1024
  static constexpr int SLOTS = (N + THREADS - 1) / THREADS;
  // 12 waves: phase 5's received rows y < 256 staged after the regions, row
  // slot (y & 3) << 6 | y >> 2 at a 112-B pitch, so that its reads
  // (y = 4 lane + q) are at most 2-way; then the tile schedule's LDS word.
  // 16 waves: nothing after the regions, the schedule word in the image
  static constexpr bool STAGED = WAVES == 12;
  static constexpr uint32_t STG = uint32_t(TAB_REGION + WAVES * REG_BYTES);
  static constexpr uint32_t SLOT = STAGED ? STG + 256 * STG_PITCH : kCImgSub1 + 4;
  static constexpr int LDS_BYTES = STAGED ? int(SLOT + 16) : int(STG);
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};
template <int WAVES>
__device__ __forceinline__ uint32_t stg_row(uint32_t y) {
  return Form<WAVES>::STG + (((y & 3) << 6) | (y >> 2)) * STG_PITCH;
}

// Region address of position v (8-byte cells, GF(2)-linear): conflict-free
// for the reads (2 x 32 lanes) and writes (4 x 16 lanes) of the three layouts
// below (scripts/search_raddr.py's condition; raddr, tf1024.hpp, is 2-way on
// layout A' reads)
__host__ __device__ constexpr uint32_t rz(uint32_t v) {
  return ((v >> 5) << 8) | (((v ^ (v >> 4) ^ (v >> 5)) & 31) << 3);
}

// The IFFT's three register layouts (lane bits / register bits -> position bits):
//  A' lane = p2..p7, r = (p0, p1, p8, p9): stages 0, 1.  The element of a
//     butterfly, x = pos >> (m + 1) (its table: the compact image entry x,
//     cimg.hpp), has its kind bits (x >= 128: F9, x >= 256: general) in p8,
//     p9, i.e. in the register index: every multiply takes the cheapest form
//     its element allows (stage 0: 2 subfield + 2 F9 + 4 general per lane,
//     stage 1: 4 subfield + 4 F9), where the round-5 layout (p0..p3 in
//     registers) had p8, p9 in the lane and used the general form for all of
//     stage 0 and the F9 form for all of stage 1.
//  B' lane = (p0, p1, p6..p9), r = p2..p5: stages 2-5 (subfield).
//  C  lane = p0..p5, r = (p8, p9, p6, p7): stages 6-9, every element
//     wave-uniform (x = 0: b ^= a only), then the derivative and the FFT.
__device__ __forceinline__ uint32_t posA2_reg(int r) { return uint32_t(r & 3) | (uint32_t(r >> 2) << 8); }
__device__ __forceinline__ uint32_t posB2_lane(uint32_t lane) { return (lane & 3) | ((lane >> 2) << 6); }
__device__ __forceinline__ uint32_t posC_reg(int r) {
  return (uint32_t((r >> 2) & 3) << 6) | (uint32_t(r & 3) << 8);
}

// IFFT stages 0 and 1 in layout A'
__device__ __forceinline__ void ipassA2(S16 &s, uint32_t lane) {
  const uint32_t l0 = cimg_lin(lane << 1), l1 = cimg_lin(lane);
  SubTab S0, S1;
  F9Tab F0, F1;
  Tab G0, G1;
  // stage 0, pair (r, r + 1): x = ((r >> 1) & 1) | lane << 1 | (r >> 2) << 7
  ctab(l0, cimg_lin(0), S0);
  ctab(l0, cimg_lin(1), S1);
  ctab(l0, cimg_lin(128), F0);
  ib(s, 0, 1, S0);
  ctab(l0, cimg_lin(129), F1);
  ib(s, 2, 3, S1);
  ctab(l0, cimg_lin(256), G0);
  ib(s, 4, 5, F0);
  ctab(l0, cimg_lin(257), G1);
  ib(s, 6, 7, F1);
  ib(s, 8, 9, G0);
  ctab(l0, cimg_lin(384), G0);
  ib(s, 10, 11, G1);
  ctab(l0, cimg_lin(385), G1);
  ctab(l1, cimg_lin(0), S0);
  ib(s, 12, 13, G0);
  ctab(l1, cimg_lin(64), S1);
  ib(s, 14, 15, G1);
  // stage 1, pair (r, r + 2): x = lane | (r >> 2) << 6
  ctab(l1, cimg_lin(128), F0);
  ib(s, 0, 2, S0);
  ib(s, 1, 3, S0);
  ctab(l1, cimg_lin(192), F1);
  ib(s, 4, 6, S1);
  ib(s, 5, 7, S1);
  ib(s, 8, 10, F0);
  ib(s, 9, 11, F0);
  ib(s, 12, 14, F1);
  ib(s, 13, 15, F1);
}

// IFFT stages 2-5 in layout B': radix 16 over r = p2..p5, 15 subfield tables
// (stage 2 + t, block blk: x = lane part >> (3 + t) | blk >> (1 + t)) through
// a ring of R slots, table k requested R - 1 tables ahead of its use
constexpr int tk(int k) { return k < 8 ? 0 : k < 12 ? 1 : k < 14 ? 2 : 3; }
constexpr int bk(int k) { return k < 8 ? 2 * k : k < 12 ? 4 * (k - 8) : k < 14 ? 8 * (k - 12) : 0; }
constexpr int RING_B = 3;
__device__ __forceinline__ void ipassB2(S16 &s, uint32_t lane) {
  const uint32_t ph = (lane >> 2) << 6;  // p6..p9 of the lane part
  const uint32_t lt[4] = {cimg_lin(ph >> 3), cimg_lin(ph >> 4), cimg_lin(ph >> 5), cimg_lin(ph >> 6)};
  SubTab ring[RING_B];
  const auto fetch = [&](int k, SubTab &U) __attribute__((always_inline)) {
    ctab(lt[tk(k)], cimg_lin(uint32_t(bk(k)) >> (1 + tk(k))), U);
  };
#pragma unroll
  for (int k = 0; k < RING_B - 1; ++k) fetch(k, ring[k]);
#pragma unroll
  for (int k = 0; k < 15; ++k) {
    if (k + RING_B - 1 < 15) fetch(k + RING_B - 1, ring[(k + RING_B - 1) % RING_B]);
    const int blk = bk(k), d = 1 << tk(k);
#pragma unroll
    for (int i = 0; i < d; ++i) ib(s, blk + i, blk + i + d, ring[k % RING_B]);
  }
}

// IFFT stages 6-9 in layout C (r bit 0 = p8, 1 = p9, 2 = p6, 3 = p7): the
// elements are wave-uniform (broadcast table reads); x = 0 is b ^= a only
// (the skew 0xFFFF, additive_fft.hpp:110-112)
__device__ __forceinline__ void ipassC2(S16 &s) {
  SubTab X1, X2, X3, X4;
  ctab(0u, cimg_lin(1), X1);
  ctab(0u, cimg_lin(2), X2);
  ctab(0u, cimg_lin(3), X3);
  ctab(0u, cimg_lin(4), X4);
  // stage 6, pair (r, r | 4): x = p7 | p8 << 1 | p9 << 2
  bx(s, 0, 4);
  ib(s, 8, 12, X1);
  ib(s, 1, 5, X2);
  ib(s, 9, 13, X3);
  ib(s, 2, 6, X4);
  ctab(0u, cimg_lin(5), X4);
  ib(s, 10, 14, X4);
  ctab(0u, cimg_lin(6), X4);
  ib(s, 3, 7, X4);
  ctab(0u, cimg_lin(7), X4);
  ib(s, 11, 15, X4);
  // stage 7, pair (r, r | 8): x = p8 | p9 << 1
  bx(s, 0, 8);
  bx(s, 4, 12);
  ib(s, 1, 9, X1);
  ib(s, 5, 13, X1);
  ib(s, 2, 10, X2);
  ib(s, 6, 14, X2);
  ib(s, 3, 11, X3);
  ib(s, 7, 15, X3);
  // stage 8, pair (r, r | 1): x = p9
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    bx(s, 4 * q, 4 * q + 1);
    ib(s, 4 * q + 2, 4 * q + 3, X1);
  }
  // stage 9, pair (r, r | 2): x = 0
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    bx(s, 4 * q, 4 * q + 2);
    bx(s, 4 * q + 1, 4 * q + 3);
  }
}

// bytes [0, avail) (avail < 4 ROW_WORDS) of a 16-B aligned row slice into
// w[ROW_WORDS], zero beyond: whole dwords at immediate offsets under a uniform
// count, the last one masked (an aligned dword holding a wanted byte never
// crosses a page)
template <int ROW_WORDS>
__device__ __forceinline__ void load_row_tail(const uint8_t *row, uint32_t avail, uint32_t (&w)[ROW_WORDS]) {
  const uint32_t nw = (avail + 3) / 4;  // wave-uniform
  const uint32_t last = (avail & 3) ? (1u << (8 * (avail & 3))) - 1 : ~0u;
  const uint32_t *r = reinterpret_cast<const uint32_t *>(row);
#pragma unroll
  for (int j = 0; j < ROW_WORDS; ++j) {
    w[j] = 0;
    if (uint32_t(j) < nw) w[j] = r[j] & (uint32_t(j) + 1 == nw ? last : ~0u);
  }
}


// a tile's geometry: its first column, the item's shard length in bytes and
// columns and its row pitch, the item's row 0 and its output
struct Where {
  uint64_t col0, slen, ncols, sstride;
  const uint8_t *SH;
  uint8_t *O;
};

// The uniform batch: item b's rows at b * nv * sstride, its output at
// b * ostride, every item slen bytes per shard: ticket cur is tile
// cur % tiles_pp of item cur / tiles_pp.  A workgroup's first tile is
// blockIdx.x, every later one gridDim.x + a ticket from the counter.
template <int WAVES>
struct UniformGeo {
  static constexpr int COLS = Form<WAVES>::COLS;
  const uint8_t *shards;
  uint64_t slen, sstride;
  uint8_t *out;
  uint64_t ostride;
  int nv;
  uint32_t batch;
  uint32_t *tick;
  struct Tile {
    uint32_t ticket;
  };
  struct Pre {  // per launch: columns and tiles per item, tiles of the launch
    uint64_t ncols;
    uint32_t tiles_pp;
    uint64_t total;
  };
  __device__ __forceinline__ Pre prepare() const {
    const uint64_t ncols = slen / 2;
    const uint32_t tiles_pp = uint32_t((ncols + COLS - 1) / COLS);
    return {ncols, tiles_pp, uint64_t(tiles_pp) * batch};
  }
  __device__ __forceinline__ uint32_t first_ticket() const { return gridDim.x + atomicAdd(tick, 1u); }
  __device__ __forceinline__ uint32_t next_ticket() const { return gridDim.x + atomicAdd(tick, 1u); }
  __device__ __forceinline__ void settle_first(volatile uint32_t *, uint32_t, uint32_t) const {}
  __device__ __forceinline__ uint32_t second_ticket(uint32_t taken, uint32_t) const { return taken; }
  __device__ __forceinline__ Tile first_tile(volatile uint32_t *) const { return {blockIdx.x}; }
  __device__ __forceinline__ bool publishes(uint32_t tid0) const { return tid0 == 0; }
  __device__ __forceinline__ void publish(volatile uint32_t *slot, uint32_t ticket, uint32_t) const {
    *slot = ticket;
  }
  __device__ __forceinline__ Tile read(volatile uint32_t *slot) const {
    return {uint32_t(__builtin_amdgcn_readfirstlane(*slot))};
  }
  __device__ __forceinline__ uint64_t item(const Pre &p, Tile c) const { return c.ticket / p.tiles_pp; }
  __device__ __forceinline__ Where where(const Pre &p, Tile c) const {
    const uint32_t bq = c.ticket / p.tiles_pp;
    const uint64_t b = bq, col0 = uint64_t(c.ticket - bq * p.tiles_pp) * COLS;
    return {col0, slen, p.ncols, sstride, shards + b * uint64_t(nv) * sstride, out + b * ostride};
  }
};

}  // namespace
}  // namespace ecamd
