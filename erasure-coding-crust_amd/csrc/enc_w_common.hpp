// enc_w_common.hpp — the one copy of what the two-workgroups-per-CU encode
// kernels share (enc_k256w.hip, enc_kw.hip, enc_k512w.hip; DESIGN.md §5.1,
// §5.7): 8-wave workgroups on the compact table image (cimg.hpp), radix-8
// register passes in tower coordinates, wave-private LDS exchanges
// (enc_k256_common.hpp), the payload fetch of a lane, the row stores out of
// the waves' own regions, the tile schedule (the geometry policy's contract,
// the ticket protocol, the uniform batch's policy UniformGeo) and the
// launchers' tail.  Each kernel keeps its tile loop with its barrier sequence,
// its passes and table kinds, its LDS map and its staging swizzle (soff*).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "ec_device.hpp"
#include "ec_kernels.hpp"
#include "cimg.hpp"
#include "enc_k256_common.hpp"

namespace ecamd {
namespace {

constexpr int WAVES = 8;
constexpr int THREADS = 64 * WAVES;
constexpr uint32_t XCH_BYTES = 4096;  // per-wave exchange / staging region
static_assert(kCImgBytes % (16 * THREADS) == 0, "whole image chunks per thread");

// the compact image (32 KB) -> LDS address 0, every load issued before the
// first store
__device__ __forceinline__ void copy_cimg(uint8_t *lds, const uint8_t *cimg, uint32_t tid0) {
  constexpr int kPer = int(kCImgBytes / 16 / THREADS);
  v4u v[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) v[k] = reinterpret_cast<const v4u *>(cimg)[tid0 + k * THREADS];
#pragma unroll
  for (int k = 0; k < kPer; ++k) reinterpret_cast<v4u *>(lds)[tid0 + k * THREADS] = v[k];
}

// Element index of a stage-m butterfly whose a-position is pos, in a transform
// at index off (a multiple of k): x = (pos + off) >> (m + 1) (ec_kernels.hpp).
// A radix-8 pass over position bits b0..b0+2 held in registers (pos = base |
// r << b0, base without those bits): stage b0 block rr (registers 2rr, 2rr+1)
// x = base >> (b0+1) | rr; stage b0+1 block hh (registers 4hh + {0,1}, + 2)
// x = base >> (b0+2) | hh; stage b0+2: x = base >> (b0+3); each | off >> (m+1).
// Lane parts l0..l2 = cimg_lin of the three base shifts (3 VGPRs per pass).
struct XLanes {
  uint32_t l0, l1, l2;
};
template <int B0>
__device__ __forceinline__ XLanes xlanes(uint32_t base) {
  return {cimg_lin(base >> (B0 + 1)), cimg_lin(base >> (B0 + 2)), cimg_lin(base >> (B0 + 3))};
}

// inverse radix-8 pass at index 0 whose every element is subfield (x < 128)
template <int B0>
__device__ __forceinline__ void ipass(State &s, uint32_t base) {
  const XLanes x = xlanes<B0>(base);
  SubTab Ta0, Tb0, Ta1, Tb1, Ta2;
  ctab(x.l0, cimg_lin(0), Ta0);
  ctab(x.l0, cimg_lin(1), Tb0);
  ibfly(s, 0, 1, Ta0);
  ctab(x.l0, cimg_lin(2), Ta0);
  ibfly(s, 2, 3, Tb0);
  ctab(x.l0, cimg_lin(3), Tb0);
  ibfly(s, 4, 5, Ta0);
  ctab(x.l1, cimg_lin(0), Ta1);
  ibfly(s, 6, 7, Tb0);
  ctab(x.l1, cimg_lin(1), Tb1);
  ibfly(s, 0, 2, Ta1);
  ibfly(s, 1, 3, Ta1);
  ctab(x.l2, cimg_lin(0), Ta2);
  ibfly(s, 4, 6, Tb1);
  ibfly(s, 5, 7, Tb1);
#pragma unroll
  for (int r = 0; r < 4; ++r) ibfly(s, r, r + 4, Ta2);
}

// Table kinds of a stage: the compact image's subfield / F9 / general entries
// (SubTab, F9Tab, Tab: the kind is the table type), or an extension kind of
// the kernel: a struct derived from ExtKind whose BASE / PLANE give the LDS
// address and plane pitch of a general table image brought in per coset.
struct ExtKind {};
template <typename K_>
using TabOf = std::conditional_t<std::is_base_of_v<ExtKind, K_>, Tab, K_>;

// table of element x = lane part lt ^ block part r ^ uniform part u (each the
// cimg_lin of its bits): compact-image kinds at their element address, an
// extension table at the coset-local one (u, the coset's offset bits, dropped)
template <typename K_>
__device__ __forceinline__ void ftab(uint32_t lt, uint32_t r, uint32_t u, TabOf<K_> &T) {
  if constexpr (std::is_base_of_v<ExtKind, K_>) {
    const uint32_t a = lt ^ r;
#pragma unroll
    for (int q = 4; q >= 0; --q) {
      const v4u v = lds_r128(a + K_::BASE + uint32_t(q) * K_::PLANE);
      T.t[4 * q] = v.x;
      T.t[4 * q + 1] = v.y;
      T.t[4 * q + 2] = v.z;
      T.t[4 * q + 3] = v.w;
    }
  } else {
    ctab(lt, r ^ u, T);
  }
}

// forward radix-8 pass at index off over position bits B0..B0+2: stages B0+2,
// B0+1, B0 with table kinds K2, K1, K0 (the elements' kinds, known per coset:
// DESIGN.md §5.1).  u0..u2: the uniform parts (scalar for a run-time coset)
template <int B0, typename K2, typename K1, typename K0>
__device__ __forceinline__ void fpass(State &s, uint32_t base, uint32_t off) {
  const XLanes x = xlanes<B0>(base);
  const uint32_t u0 = cimg_lin(off >> (B0 + 1)), u1 = cimg_lin(off >> (B0 + 2)), u2 = cimg_lin(off >> (B0 + 3));
  TabOf<K2> Ta2;
  TabOf<K1> Ta1, Tb1;
  TabOf<K0> Ta0, Tb0;
  ftab<K2>(x.l2, 0u, u2, Ta2);
  ftab<K1>(x.l1, 0u, u1, Tb1);
#pragma unroll
  for (int r = 0; r < 4; ++r) fbfly(s, r, r + 4, Ta2);
  ftab<K1>(x.l1, cimg_lin(1), u1, Ta1);
  fbfly(s, 0, 2, Tb1);
  fbfly(s, 1, 3, Tb1);
  ftab<K0>(x.l0, 0u, u0, Tb0);
  fbfly(s, 4, 6, Ta1);
  fbfly(s, 5, 7, Ta1);
  ftab<K0>(x.l0, cimg_lin(1), u0, Ta0);
  fbfly(s, 0, 1, Tb0);
  ftab<K0>(x.l0, cimg_lin(2), u0, Tb0);
  fbfly(s, 2, 3, Ta0);
  ftab<K0>(x.l0, cimg_lin(3), u0, Ta0);
  fbfly(s, 4, 5, Tb0);
  fbfly(s, 6, 7, Ta0);
}

// ---- layout C for k = 256 (register bit 0 = p6, bit 1 = p7, bit 2 = p5): the
// elements of stages 6, 7 are lane-uniform.  IFFT at index 0: stage 7 (x = 0)
// and stage 6's p7 = 0 block (x = 0) are b ^= a only (the skew 0xFFFF of
// additive_fft.hpp:110-112); stage 6's p7 = 1 block has x = 1.
__device__ __forceinline__ void ipassC(State &s) {
  SubTab Tb;
  ctab(0u, cimg_lin(1), Tb);
  bxor(s, 0, 1);
  bxor(s, 4, 5);
  ibfly(s, 2, 3, Tb);
  ibfly(s, 6, 7, Tb);
  bxor(s, 0, 2);
  bxor(s, 1, 3);
  bxor(s, 4, 6);
  bxor(s, 5, 7);
}

// FFT stages 7, 6 at index off, reading the IFFT coefficients c and writing s:
// stage 7 x = off >> 8, stage 6 x = off >> 7 | p7
__device__ __forceinline__ void fpassC(State &s, const State &c, uint32_t off) {
  SubTab Ta, Tb;
  ctab(0u, cimg_lin(off >> 8), Ta);
  ctab(0u, cimg_lin(off >> 7), Tb);
  fbfly_from(s, c, 0, 2, Ta);
  fbfly_from(s, c, 1, 3, Ta);
  fbfly_from(s, c, 4, 6, Ta);
  fbfly_from(s, c, 5, 7, Ta);
  ctab(0u, cimg_lin((off >> 7) | 1u), Ta);
  fbfly(s, 0, 1, Tb);
  fbfly(s, 4, 5, Tb);
  fbfly(s, 2, 3, Ta);
  fbfly(s, 6, 7, Ta);
}

// wave-private exchange (enc_k256_common.hpp exchange) at the wave's region
// folded into the lane bases xb (bits >= 12): the bases are laundered here, so
// the 16 cell addresses are formed at the exchange (one XOR each) instead of
// being hoisted out of the tile loop and kept live (spilled) across it
template <Layout FROM, Layout TO>
__device__ __forceinline__ void xchg(State &s, XBase xb) {
  asm volatile("" : "+v"(xb.a), "+v"(xb.b), "+v"(xb.c));
#pragma unroll
  for (int r = 0; r < 8; ++r) lds_st2(xcell<FROM>(xb, r), make_uint2(s.l[r], s.h[r]));
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint2 v = lds_ld2(xcell<TO>(xb, r));
    s.l[r] = v.x;
    s.h[r] = v.y;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---- payload fetch: a lane's 4 x 16 payload bytes, zero past plen.  FP: the
// payload; pw: the wave's first piece (uniform) of its wp; the lane takes
// pieces pw + 4 g + u (g: its byte-planar group in the wave, u = 0..3), bytes
// 16 q .. 16 q + 15 of each (2 K bytes a piece).  Whole wave inside the
// payload: 4 loads in flight; the payload's edge: piece by piece, byte by byte
// at plen; a wave past the end: zeros, no loads (every path assigns d: no
// value is carried across a tile).
template <int K>
__device__ __forceinline__ void fetch_pieces(const uint8_t *FP, uint64_t plen, uint64_t npieces, uint64_t pw,
                                             uint32_t wp, uint32_t g, uint32_t q, v4u (&d)[4]) {
  if ((pw + wp) * 2 * K <= plen) {
    const uint8_t *src = FP + (pw + 4 * g) * 2 * K + 16 * q;
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] = *reinterpret_cast<const v4u *>(src + u * 2 * K);
  } else if (pw < npieces) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t off = (pw + 4 * g + u) * 2 * K + 16 * q;
      uint32_t w[4] = {0, 0, 0, 0};
      if (off + 16 <= plen) {
        const v4u x = *reinterpret_cast<const v4u *>(FP + off);
        w[0] = x.x;
        w[1] = x.y;
        w[2] = x.z;
        w[3] = x.w;
      } else {
        for (uint64_t e = off; e < plen && e < off + 16; ++e)
          w[(e - off) >> 2] |= uint32_t(FP[e]) << (8 * ((e - off) & 3));
      }
      d[u] = v4u{w[0], w[1], w[2], w[3]};
    }
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] = v4u{0, 0, 0, 0};
  }
}

// 4 x 16 payload bytes (4 pieces, positions 8q..8q+7) -> byte-planar State:
// 4x4 byte transposes, dword j of each piece = (hi_{2j}, lo_{2j}, hi_{2j+1}, lo_{2j+1})
__device__ __forceinline__ void to_state(const v4u (&d)[4], State &s) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t D0 = d[0][j], D1 = d[1][j], D2 = d[2][j], D3 = d[3][j];
    const uint32_t t0 = vperm(D1, D0, 0x05010400u), t1 = vperm(D1, D0, 0x07030602u);
    const uint32_t u0 = vperm(D3, D2, 0x05010400u), u1 = vperm(D3, D2, 0x07030602u);
    s.h[2 * j] = vperm(u0, t0, 0x05040100u);
    s.l[2 * j] = vperm(u0, t0, 0x07060302u);
    s.h[2 * j + 1] = vperm(u1, t1, 0x05040100u);
    s.l[2 * j + 1] = vperm(u1, t1, 0x07060302u);
  }
}

// ---- row stores, all waves: rows [s0, s0 + K) of the tile from the 8 regions
// -> shards, 16 B (pieces 8c .. 8c + 7 of one row) per lane and iteration, 4
// iterations.  The kernel's geometry G gives
//   TILE, K        pieces per tile, rows per store phase;
//   VSTEP          rows per iteration (all waves): K / 4;
//   lane_role(wave, lane)   the lane's first row v0, its chunk c and the LDS
//                  address a of that row's chunk;
//   read(a, it)    the 16 bytes of row v0 + it * VSTEP (the staging swizzles
//                  are GF(2)-linear in v = it * VSTEP | v0: one XOR on a), as
//                  a v4u or what converts to one (the slow path converts
//                  only the rows it stores).
// Fast path (uniform): 16-B aligned rows, the whole tile inside the payload,
// all K rows below n_validators -- one streaming 16-B store per lane and row.
struct RowLane {
  uint32_t v0, c, a;
};
// Which rows of a store phase are written: every row (the encodes), or the rows
// whose bit is set in a 1024-bit mask in LDS (word y >> 5, bit y & 31: the
// masked encode, enc_k256w_missing.hip).  MASKED false compiles to nothing.
struct AllRows {
  static constexpr bool MASKED = false;
};
struct LdsRowMask {
  static constexpr bool MASKED = true;
  uint32_t base;  // LDS address of the mask's word 0
  __device__ __forceinline__ bool wanted(uint32_t row) const {
    return (lds_r32(base + ((row >> 5) << 2)) >> (row & 31)) & 1u;
  }
};
template <typename G>
__device__ __forceinline__ bool store_fast(const uint8_t *SH, uint64_t sstride, uint32_t s0, int nv,
                                           uint64_t piece0, uint64_t npieces) {
  return ((sstride | reinterpret_cast<uintptr_t>(SH)) & 15) == 0 && piece0 + G::TILE <= npieces &&
         int(s0) + int(G::K) <= nv;
}

// `then` runs at the end of each path: code that waits for a load issued
// before the stores is placed there, so the compiler's wait on the fast path
// counts its 4 stores (vmcnt(4)) instead of the minimum over every path.
template <typename G, typename Then, typename Mask = AllRows>
__device__ __forceinline__ void store_own(uint8_t *SH, uint64_t sstride, uint32_t s0, int nv,
                                          uint64_t piece0, uint64_t npieces, uint32_t wave,
                                          uint32_t lane, Then &&then, Mask mask = {}) {
  static_assert(G::K == 4 * G::VSTEP, "4 stores per lane: the vmcnt(4) waits count them");
  asm volatile("" : "+v"(lane));  // recomputed here, not kept live across the FFTs
  const RowLane rl = G::lane_role(wave, lane);
  const uint32_t v0 = rl.v0, c = rl.c, a = rl.a;
  if (store_fast<G>(SH, sstride, s0, nv, piece0, npieces)) {
    uint8_t *dst = SH + uint64_t(s0 + v0) * sstride + 2 * (piece0 + 8 * c);
    const uint64_t dstep = uint64_t(G::VSTEP) * sstride;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const v4u val = G::read(a, it);
      if constexpr (Mask::MASKED) {
        if (!mask.wanted(s0 + uint32_t(it) * G::VSTEP + v0)) continue;
      }
      __builtin_nontemporal_store(val, reinterpret_cast<v4u *>(dst + it * dstep));  // written once
    }
    then();
    asm volatile("; store_own fast path end" ::: "memory");  // distinct tails: `then` is not merged
    return;
  }
  const uint64_t p = piece0 + 8 * c;
  const bool wide = ((sstride | reinterpret_cast<uintptr_t>(SH)) & 15) == 0;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const uint32_t v = uint32_t(it) * G::VSTEP + v0;
    const auto raw = G::read(a, it);  // a v4u only below: not assembled for rows that are cut
    const uint32_t shard = s0 + v;
    if (int(shard) >= nv) continue;
    if constexpr (Mask::MASKED) {
      if (!mask.wanted(shard)) continue;
    }
    uint8_t *dst = SH + uint64_t(shard) * sstride + 2 * p;
    const v4u val = raw;
    if (p + 8 <= npieces) {
      if (wide) {
        *reinterpret_cast<v4u *>(dst) = val;
      } else {
        reinterpret_cast<uint2 *>(dst)[0] = make_uint2(val.x, val.y);
        reinterpret_cast<uint2 *>(dst)[1] = make_uint2(val.z, val.w);
      }
    } else if (p < npieces) {
      const uint32_t w[4] = {val.x, val.y, val.z, val.w};
      for (uint64_t e = 0; e < npieces - p; ++e)
        *reinterpret_cast<uint16_t *>(dst + 2 * e) = uint16_t(w[e >> 1] >> (16 * (e & 1)));
    }
  }
  then();
  asm volatile("; store_own slow path end" ::: "memory");
}

// a store phase: the row stores (LDS reads + global stores) at raised issue priority
template <typename G, typename Then, typename Mask = AllRows>
__device__ __forceinline__ void store_rows(uint8_t *SH, uint64_t sstride, uint32_t s0, int nv, uint64_t piece0,
                                           uint64_t npieces, uint32_t wave, uint32_t lane, Then &&then,
                                           Mask mask = {}) {
  __builtin_amdgcn_s_setprio(1);
  store_own<G>(SH, sstride, s0, nv, piece0, npieces, wave, lane, then, mask);
  __builtin_amdgcn_s_setprio(0);
}

// ---- the tile schedule.  The kernels are persistent: a workgroup works on
// tile tickets until one is past the launch's last tile.  A tile loop is
// written against a geometry policy that says, for a ticket, which payload
// bytes, shard rows, piece count and pitch the tile works on, and how the
// ticket travels from the thread that takes it to the other waves; the
// transforms, the staging, the row stores and the order of barriers do not
// depend on it.  UniformGeo below: the uniform batch (encode_k256w, encode_kw,
// encode_k512w); the ragged batch: enc_k256w_ragged.hip.
//
// A geometry policy Geo provides (all values wave-uniform):
//   Tile, ticket(T)      what a wave keeps of a ticket from reading it to the
//                        end of its tile; ticket(T) < Pre::total: a tile of
//                        the launch
//   SLOT_BYTES           LDS bytes at the kernel's SLOT the tickets are published in
//   Pre, prepare()       worked out once per launch; total: the launch's tiles
//   publishes(tid0)      the threads that take part in publishing a ticket
//                        (thread 0, or all of wave 0); the call sites are
//                        reached by whole waves, wave 0 always among them
//   first(slot, tid0)    those threads: take and publish the first ticket
//   next_ticket(T)       thread 0: the ticket after tile T's
//   publish(slot, ticket, tid0)  those threads: resolve and store thread 0's ticket
//   read(slot).t         the published Tile (after a barrier)
//   Loc, loc(pre, T)     where a valid tile's payload bytes are
//   loc_or_none(pre, T)  the same for a tile that may be past the end: then a
//                        place for which the fetch loads nothing
//   fetch(pre, Loc)      the payload fetch's geometry (Fetch)
//   At, at(pre, T), piece0(At), rows(At), npieces(pre, T), sstride(T)
//                        geometry of a valid tile's transforms and stores
//   MASKED               false: every phase of a tile runs and every row is
//                        stored.  true (enc_k256w_missing.hip, which states the
//                        schedule of a tile with skipped phases): also
//                        phases(T), row_mask(T), read through tile_phases /
//                        tile_mask below
//
// The ticket protocol.  Tiles come from the launch's counter (zeroed before the
// launch), so the two workgroups of a CU, which the issue arbiter serves at
// unequal rates, finish together: with a static grid-stride split the faster
// one ended up to 2.8 ms before the slower one of a 7 ms launch
// (scripts/variants/clk_run.py).  A ticket is
//  * taken by thread 0 at the start of the tile before its own (next_ticket:
//    the atomic's latency hides behind that tile);
//  * published in the LDS slot after that tile's systematic stores (the store
//    phase's `then`: the wait for the atomic's return counts only the stores
//    issued after it on the fast path, store_own);
//  * read by every wave in that tile's last coset (fetch_next), at least one
//    barrier later (the one after IFFT pass A);
//  * rewritten only after the next tile's systematic stores, past that tile's
//    start barrier, by which every wave has read it.
// The first ticket is published before the kernel's first __syncthreads.
//
// what the payload fetch of a tile needs: the item's payload, its length in
// bytes and pieces, the tile's first piece
struct Fetch {
  const uint8_t *P;
  uint64_t plen, npieces, piece0;
};

// The uniform batch in tiles of TILE pieces: payload b at b * pstride, its
// rows at b * nv * sstride, every payload plen bytes: ticket cur is tile
// cur % tiles_pp of payload cur / tiles_pp.  Without a counter (no scratch) a
// static grid stride (slower: the two workgroups of a CU drift apart).
template <int TILE>
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
  static constexpr bool MASKED = false;
  struct Pre {  // per launch: pieces and tiles per payload, tiles of the launch
    uint64_t npieces;
    uint32_t tiles_pp, total;
  };
  __device__ __forceinline__ Pre prepare() const {
    const uint64_t npieces = slen / 2;
    const uint32_t tiles_pp = uint32_t((npieces + TILE - 1) / TILE);
    return {npieces, tiles_pp, tiles_pp * batch};  // < 2^32 (launch_w)
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

// What a tile loop asks a MASKED policy, in a form that compiles for every
// policy (the loops are textual fragments inside non-template kernels): the
// tile's phase flags (bit 0: the systematic rows, bits 1..3: the cosets 256,
// 512, 768) and its row mask.
template <typename Geo>
__device__ __forceinline__ uint32_t tile_phases(const Geo &geo, const typename Geo::Tile &t) {
  if constexpr (Geo::MASKED)
    return geo.phases(t);
  else
    return 0xFu;
}
template <typename Geo>
__device__ __forceinline__ auto tile_mask(const Geo &geo, const typename Geo::Tile &t) {
  if constexpr (Geo::MASKED)
    return geo.row_mask(t);
  else
    return AllRows{};
}

}  // namespace

// ---- the launchers' tail: the kernel prepared for its dynamic LDS, the tile
// count (payload pieces in tiles of `tile`) below 2^32 - 4 CUs (the kernels
// count tiles, and the static schedule's cur + gridDim.x, in 32 bits), the
// tile counter (`scratch`: kTileCounterBytes) zeroed in stream
// order, grid = min(tiles, two workgroups per CU).  No scratch: the static
// schedule (a missing counter costs speed, not an error).  `tabs`: the
// kernel's table images, passed between batch and the counter.
template <typename Kern, typename... Tabs>
hipError_t launch_w(Kern kern, int lds_bytes, size_t tile, const CodeParams &p, const EncodeCall &c, void *scratch,
                    hipStream_t s, Tabs... tabs) {
  int cus = 0;
  if (const hipError_t e = prepare_kernel(reinterpret_cast<const void *>(kern), lds_bytes, &cus); e != hipSuccess)
    return e;
  const size_t sl = shard_len(p.k, c.plen);
  const size_t tiles = (sl / 2 + tile - 1) / tile * c.batch;
  if (tiles >= (size_t(1) << 32) - size_t(4) * cus) return hipErrorInvalidValue;
  uint32_t *tick = static_cast<uint32_t *>(scratch);
  if (tick)
    if (const hipError_t e = launch_zero_counters(tick, sizeof(uint32_t), s); e != hipSuccess) return e;
  const size_t slots = 2 * size_t(cus);
  const unsigned grid = unsigned(tiles < slots ? tiles : slots);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), lds_bytes, s, c.payloads, uint64_t(c.plen),
                     uint64_t(c.pstride), c.shards, uint64_t(sl), uint64_t(c.sstride), int(p.nv),
                     uint32_t(c.batch), tabs..., tick);
  return hipGetLastError();
}

}  // namespace ecamd
