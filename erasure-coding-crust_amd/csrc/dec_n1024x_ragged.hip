// dec_n1024x_ragged.hip — reconstruct_n1024x_ragged: the n = 1024, k = 256
// reconstruct (n_validators 766..1024) over a ragged batch (ragged.hpp,
// ec_amd.h ECCR_AMD_reconstruct_ragged): one persistent launch whose tile
// queue spans items of every shard length.  The kernel body is
// reconstruct_n1024x's (dec_n1024x_tile.inc, one copy) in its 16-wave,
// 64-column form for every item size; this file holds the ragged geometry
// policy only.
//
// Tile ticket t belongs to the item i with tile_first[i] <= t <
// tile_first[i + 1] (the plan kernel's prefix, ragged.hip).  The lookup is done
// off the tile's critical path where the uniform kernel publishes its ticket,
// at a tile's end for the tile after next: wave 0, which holds the ticket
// thread 0 took at the tile's start, finds the item with a 64-ary search of
// tile_first (one coalesced probe per lane and round: ragged_find_item), loads
// the item's record with scalar loads, and thread 0 stores the resolved tile
// -- ticket, item, tile in the item, the item's row and output addresses,
// shard length, pitch: 11 words -- in LDS.  What the lookup needs (the buffers,
// the item array, the prefix) it loads from the plan's header (RaggedHdr)
// then and there: kept as kernel arguments they would sit in SGPRs through
// every tile, and the 16-wave form then spills (SGPRs into a VGPR, and a
// VGPR in turn).  Every wave reads those words where the uniform
// kernel reads its ticket (LDS broadcast reads into SGPRs), a tile before it
// works on them: no other wave touches tile_first or the item array, so no wave
// walks dependent global loads at a tile's start.
//
// The 16-wave form uses all 160 KB of LDS; like its schedule word, the words
// live in dwords of the compact image's 128 kCImgSub1 entries that no table
// fetch reads (ctab reads dword 0 of those 16-B entries only): word j of a
// published tile in dword 1 of entry j, word j of the workgroup's first tile
// (resolved once, behind a barrier of its own) in dword 2 of entry j.
//
// Per-item metadata -- the gather order, the present and locator rows -- is
// indexed by the item exactly as the uniform kernel indexes it by the payload
// (d_pattern included); launch_gather_order is the uniform launcher's.
//
// A tile is 64 columns whatever the item's shard length, so an item of one
// column keeps one of sixteen waves busy in phases 2-5 (every wave gathers).
// That is accepted here: the ragged calls are for mixed batches; a uniform
// batch of tiny payloads is better served by ECCR_AMD_reconstruct_batch, whose
// dispatch picks the packed kernel (reconstruct_n1024_packed) for it.
#include "dec_n1024x_body.hpp"
#include "ragged.hpp"

namespace ecamd {
namespace {

constexpr int kRaggedWaves = 16;

struct RaggedGeo {
  static constexpr int COLS = Form<kRaggedWaves>::COLS;
  const RaggedHdr *hdr;  // read where a ticket is resolved only (ragged.hpp)
  uint32_t *tick;
  // a resolved tile, as published (every member wave-uniform: SGPRs)
  struct Tile {
    uint32_t ticket, item, tile;  // the ticket; its item; the tile's index in the item
    const uint8_t *SH;            // the item's row 0
    uint64_t slen, sstride;
    uint8_t *O;                   // the item's output
  };
  static constexpr int kWords = 11;
  // the words are read and written as LDS (ds instructions), not through the
  // body's generic pointer (flat instructions): LdsWord, ec_device.hpp
  __device__ static __forceinline__ LdsWord *lds_words(volatile uint32_t *slot) { return (LdsWord *)slot; }
  struct Pre {
    uint64_t total;  // tiles of the launch
  };
  __device__ __forceinline__ Pre prepare() const { return {hdr->total}; }
  // every ticket comes from the counter (the host does not know how many tiles
  // there are, so no tile is implied by a workgroup's index)
  __device__ __forceinline__ uint32_t first_ticket() const { return atomicAdd(tick, 1u); }
  __device__ __forceinline__ uint32_t next_ticket() const { return atomicAdd(tick, 1u); }
  __device__ __forceinline__ uint32_t second_ticket(uint32_t taken, uint32_t tid0) const {
    if (tid0 == 0) taken = atomicAdd(tick, 1u);
    return taken;
  }
  // all of wave 0 (the call sites are reached by wave 0 with every lane active)
  __device__ __forceinline__ bool publishes(uint32_t tid0) const {
    return __builtin_amdgcn_readfirstlane(tid0 >> 6) == 0;
  }
  // `slot`: dword 1 of entry 0; words 16 B apart.  A ticket past the end is
  // stored as it is with an empty geometry; nobody works on it.
  __device__ __forceinline__ void publish(volatile uint32_t *slot_, uint32_t ticket, uint32_t tid0) const {
    const uint32_t t = uint32_t(__builtin_amdgcn_readfirstlane(int(ticket)));
    const RaggedHdr h = *hdr;
    uint32_t i = 0, tile = 0;
    RaggedItem it = {0, 0, 0, 0, 0};
    if (t < h.total) {
      const uint32_t *first = ragged_global_ptr<const uint32_t>(reinterpret_cast<uintptr_t>(h.tile_first));
      i = ragged_find_item(first, h.batch, t, tid0);
      tile = t - first[i];
      it = ragged_global_ptr<const RaggedItem>(reinterpret_cast<uintptr_t>(h.items))[i];
    }
    if (tid0 == 0) {
      LdsWord *slot = lds_words(slot_);
      const uint64_t sh = uint64_t(reinterpret_cast<uintptr_t>(h.in)) + it.shard_off;
      const uint64_t o = uint64_t(reinterpret_cast<uintptr_t>(h.out)) + it.payload_off;
      slot[0] = t;
      slot[4] = i;
      slot[8] = tile;
      slot[12] = uint32_t(sh);
      slot[16] = uint32_t(sh >> 32);
      slot[20] = uint32_t(it.shard_len);
      slot[24] = uint32_t(it.shard_len >> 32);
      slot[28] = uint32_t(it.shard_stride);
      slot[32] = uint32_t(it.shard_stride >> 32);
      slot[36] = uint32_t(o);
      slot[40] = uint32_t(o >> 32);
    }
  }
  __device__ __forceinline__ Tile read(volatile uint32_t *slot_) const {
    LdsWord *slot = lds_words(slot_);
    uint32_t w[kWords];
#pragma unroll
    for (int j = 0; j < kWords; ++j) w[j] = uint32_t(__builtin_amdgcn_readfirstlane(int(slot[4 * j])));
    const auto u64 = [&](int j) { return uint64_t(w[j]) | (uint64_t(w[j + 1]) << 32); };
    return {w[0], w[1], w[2], ragged_global_ptr<const uint8_t>(u64(3)), u64(5), u64(7),
            ragged_global_ptr<uint8_t>(u64(9))};
  }
  // the workgroup's first tile: resolved like any other, into the entries'
  // dword 2, and read by every wave behind a barrier of its own
  __device__ __forceinline__ void settle_first(volatile uint32_t *slot, uint32_t taken, uint32_t tid0) const {
    if (publishes(tid0)) publish(slot + 1, taken, tid0);
    __syncthreads();
  }
  __device__ __forceinline__ Tile first_tile(volatile uint32_t *slot) const { return read(slot + 1); }
  __device__ __forceinline__ uint64_t item(const Pre &, const Tile &c) const { return c.item; }
  // Row slices are 16-B aligned: shard_off and shard_stride are multiples of 16
  // on a 16-B aligned base and a tile starts at a multiple of 128 bytes, so
  // load_row_tail's masked last dword never crosses a page.  Phase 5's 8-B
  // read of a received data row y < k at the wave's columns may run up to 6
  // bytes past shard_len: it stays inside the row's pitch or runs into the same
  // item's next row, which exists because y < 256 < 766 <= n_validators, so it
  // never leaves the item.  The output is 8-B aligned (payload_off).
  __device__ __forceinline__ Where where(const Pre &, const Tile &c) const {
    return {uint64_t(c.tile) * COLS, c.slen, c.slen / 2, c.sstride, c.SH, c.O};
  }
};
static_assert(kCImgSub1 + 16 * RaggedGeo::kWords <= kCImgBytes, "the words' entries are kCImgSub1 entries");

}  // namespace

__global__ void __launch_bounds__(64 * kRaggedWaves) reconstruct_n1024x_ragged(
    const RaggedHdr *__restrict__ hdr, const uint8_t *__restrict__ present, const uint16_t *__restrict__ elog,
    const uint32_t *__restrict__ pattern, const uint32_t *__restrict__ order, uint32_t *tick, DevTables t) {
  constexpr int WAVES = kRaggedWaves;
  const RaggedGeo geo{hdr, tick};
#include "dec_n1024x_tile.inc"
}

// `ws` planned by launch_ragged_plan (tile 64) in stream order before this; the
// gather order follows the plan in it.  The grid is sized from the most tiles
// the call can have (the host does not know the items): workgroups beyond the
// real count take tickets past the end and leave.
hipError_t launch_reconstruct_n1024x_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                            hipStream_t s) {
  using F = Form<kRaggedWaves>;
  int cus = 0;
  if (!t.cimg || !ws) return hipErrorInvalidValue;
  if (const hipError_t e =
          prepare_kernel(reinterpret_cast<const void *>(&reconstruct_n1024x_ragged), F::LDS_BYTES, &cus);
      e != hipSuccess)
    return e;
  const size_t most = (c.max_len / 2 + F::COLS - 1) / F::COLS * c.batch;
  if (most + 4096 >= (size_t(1) << 32)) return hipErrorInvalidValue;  // 32-bit tile tickets
  uint32_t *order = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(ws) + ragged_scratch_offset(c.batch));
  if (const hipError_t e = launch_gather_order(p, c.present, c.err_log, c.pattern, c.batch, order, s);
      e != hipSuccess)
    return e;
  const unsigned grid = unsigned(most < size_t(cus) ? most : size_t(cus));
  hipLaunchKernelGGL(reconstruct_n1024x_ragged, dim3(grid), dim3(F::THREADS), F::LDS_BYTES, s, ragged_hdr(ws),
                     c.present, c.err_log, c.pattern, order, ragged_tick(ws), t);
  return hipGetLastError();
}

}  // namespace ecamd
