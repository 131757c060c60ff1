// enc_k256w_ragged.hip — encode_k256w_ragged: the k = 256, n = 1024 encode
// (n_validators 766..1024) over a ragged batch (ragged.hpp, ec_amd.h
// ECCR_AMD_encode_ragged): one persistent launch whose tile queue spans items
// of every length.  The tile body is encode_k256w's (enc_k256w_body.hpp, one
// copy); this file holds the ragged geometry policy only.
//
// Tile ticket t belongs to the item i with tile_first[i] <= t <
// tile_first[i + 1] (the plan kernel's prefix, ragged.hip).  The lookup is
// done off the tile's critical path, one tile ahead, where the uniform kernel
// publishes its ticket: wave 0, which holds the ticket thread 0 took at the
// tile's start, finds the item with a 64-ary search of tile_first (one
// coalesced probe per lane and round: ragged_find_item), loads the item's
// record with scalar loads, and thread 0 stores the resolved tile -- ticket,
// tile in the item, the item's payload and row addresses, lengths, pitch: 12
// words -- in the LDS slot.  What the lookup needs (the buffers, the item
// array, the prefix) it loads from the plan's header (RaggedHdr) there.  Every wave reads those words where the uniform kernel reads
// its ticket (LDS broadcast reads into SGPRs); no other wave touches
// tile_first or the item array, so no wave walks dependent global loads at a
// tile's start.
//
// A tile is 64 pieces whatever the item's length, so an item of one piece
// (a payload up to 512 bytes) keeps one of eight waves busy and items under
// 8 pieces waste most of a tile.  That is accepted here: the ragged calls are
// for mixed batches, where the long items dominate; a uniform batch of tiny
// payloads is better served by ECCR_AMD_encode_batch, whose dispatch picks the
// packed kernel (encode_k256_packed) for it.
#include "enc_k256w_body.hpp"
#include "ragged.hpp"

namespace ecamd {
namespace {
namespace k256w {

struct RaggedGeo {
  const RaggedHdr *hdr;  // read where a ticket is resolved only (ragged.hpp)
  uint32_t *tick;
  // a resolved tile, as published (every member wave-uniform: SGPRs)
  struct Tile {
    uint32_t ticket, tile;  // the ticket; the tile's index in its item
    const uint8_t *P;       // the item's payload
    uint64_t plen;
    uint8_t *SH;            // the item's row 0
    uint64_t sstride, npieces;
  };
  using Loc = Tile;
  using At = Tile;
  static constexpr uint32_t SLOT_BYTES = 64;  // 12 words
  static constexpr bool MASKED = false;
  struct Pre {
    uint32_t total;  // tiles of the launch: the plan's last prefix entry
  };
  __device__ __forceinline__ Pre prepare() const { return {hdr->total}; }
  __device__ __forceinline__ uint32_t ticket(const Tile &c) const { return c.ticket; }
  __device__ __forceinline__ uint32_t next_ticket(const Tile &) const { return atomicAdd(tick, 1u); }
  // Wave 0 (all 64 lanes: the call sites are reached by whole waves) resolves
  // thread 0's ticket and thread 0 stores the tile.  A ticket past the end is
  // stored with an empty geometry (no pieces: the payload fetch loads nothing).
  __device__ __forceinline__ bool publishes(uint32_t tid0) const {
    return __builtin_amdgcn_readfirstlane(tid0 >> 6) == 0;
  }
  __device__ __forceinline__ void publish(LdsWord *slot, uint32_t ticket, uint32_t tid0) const {
    const uint32_t t = uint32_t(__builtin_amdgcn_readfirstlane(int(ticket)));
    const RaggedHdr h = *hdr;
    uint32_t tile = 0;
    RaggedItem it = {0, 0, 0, 0, 0};
    uint64_t np = 0;
    if (t < h.total) {
      const uint32_t *first = ragged_global_ptr<const uint32_t>(reinterpret_cast<uintptr_t>(h.tile_first));
      const uint32_t i = ragged_find_item(first, h.batch, t, tid0);
      tile = t - first[i];
      it = ragged_global_ptr<const RaggedItem>(reinterpret_cast<uintptr_t>(h.items))[i];
      np = (it.payload_len / 2 + (it.payload_len & 1) + K - 1) / K;  // shard_len / 2
    }
    if (tid0 == 0) {
      const uint64_t pp = uint64_t(reinterpret_cast<uintptr_t>(h.in)) + it.payload_off;
      const uint64_t sh = uint64_t(reinterpret_cast<uintptr_t>(h.out)) + it.shard_off;
      slot[0] = t;
      slot[1] = tile;
      slot[2] = uint32_t(pp);
      slot[3] = uint32_t(pp >> 32);
      slot[4] = uint32_t(it.payload_len);
      slot[5] = uint32_t(it.payload_len >> 32);
      slot[6] = uint32_t(sh);
      slot[7] = uint32_t(sh >> 32);
      slot[8] = uint32_t(it.shard_stride);
      slot[9] = uint32_t(it.shard_stride >> 32);
      slot[10] = uint32_t(np);
      slot[11] = uint32_t(np >> 32);
    }
  }
  __device__ __forceinline__ void first(LdsWord *slot, uint32_t tid0) const {
    uint32_t ticket = 0;
    if (tid0 == 0) ticket = atomicAdd(tick, 1u);
    publish(slot, ticket, tid0);
  }
  struct Read {
    Tile t;
  };
  __device__ __forceinline__ Read read(LdsWord *slot) const {
    uint32_t w[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) w[j] = uint32_t(__builtin_amdgcn_readfirstlane(int(slot[j])));
    const auto u64 = [&](int j) { return uint64_t(w[j]) | (uint64_t(w[j + 1]) << 32); };
    return {{w[0], w[1], ragged_global_ptr<const uint8_t>(u64(2)), u64(4), ragged_global_ptr<uint8_t>(u64(6)), u64(8),
             u64(10)}};
  }
  __device__ __forceinline__ Loc loc(const Pre &, const Tile &c) const { return c; }
  __device__ __forceinline__ Loc loc_or_none(const Pre &, const Tile &c) const { return c; }
  // 16-B aligned pieces: payload_off is a multiple of 16 on a 16-B aligned base
  __device__ __forceinline__ Fetch fetch(const Pre &, const Loc &l) const {
    return {l.P, l.plen, l.npieces, uint64_t(l.tile) * TILE};
  }
  __device__ __forceinline__ At at(const Pre &, const Tile &c) const { return c; }
  __device__ __forceinline__ uint64_t piece0(const At &c) const { return uint64_t(c.tile) * TILE; }
  __device__ __forceinline__ uint64_t npieces(const Pre &, const Tile &c) const { return c.npieces; }
  __device__ __forceinline__ uint64_t sstride(const Tile &c) const { return c.sstride; }
  // 16-B aligned row slices: shard_off and shard_stride are multiples of 16 on
  // a 16-B aligned base (store_own's fast path tests it again)
  __device__ __forceinline__ uint8_t *rows(const At &c) const { return c.SH; }
};

}  // namespace k256w
}  // namespace

__global__ void __launch_bounds__(THREADS, 4) encode_k256w_ragged(const RaggedHdr *__restrict__ hdr, int nv,
                                                                  const uint8_t *__restrict__ cimg,
                                                                  uint32_t *__restrict__ tick) {
  const k256w::RaggedGeo geo{hdr, tick};
#include "enc_k256w_tile.inc"
}

// `ws` planned by launch_ragged_plan (tile 64) in stream order before this.
// The grid is sized from the most tiles the call can have (the host does not
// know the items): workgroups beyond the real count take a ticket past the end
// and leave.
hipError_t launch_encode_k256w_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                      hipStream_t s) {
  if (!t.cimg || !ws) return hipErrorInvalidValue;
  if (p.nv <= 2 * k256w::K || p.nv > 1024) return hipErrorInvalidValue;  // cosets 256, 512 (, 768)
  constexpr int kLds = k256w::lds_bytes<k256w::RaggedGeo>();
  int cus = 0;
  if (const hipError_t e = prepare_kernel(reinterpret_cast<const void *>(&encode_k256w_ragged), kLds, &cus);
      e != hipSuccess)
    return e;
  const size_t most = (shard_len(p.k, c.max_len) / 2 + k256w::TILE - 1) / k256w::TILE * c.batch;
  if (most + 4096 >= (size_t(1) << 32)) return hipErrorInvalidValue;  // 32-bit tile tickets
  const size_t slots = 2 * size_t(cus);
  hipLaunchKernelGGL(encode_k256w_ragged, dim3(unsigned(most < slots ? most : slots)), dim3(THREADS), kLds, s,
                     ragged_hdr(ws), int(p.nv), t.cimg, ragged_tick(ws));
  return hipGetLastError();
}

}  // namespace ecamd
