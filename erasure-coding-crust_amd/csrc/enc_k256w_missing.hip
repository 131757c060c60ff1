// enc_k256w_missing.hip — encode_k256w_missing: the k = 256, n = 1024 encode
// (n_validators 766..1024) that writes only the rows a payload's pattern marks
// missing (ec_amd.h ECCR_AMD_encode_missing_batch, the second stage of
// ECCR_AMD_repair_batch).  The tile body is encode_k256w's
// (enc_k256w_tile.inc, one copy); this file holds the masked geometry policy
// and the launcher.
//
// What a tile is told.  The plan kernel (row_mask.hip) turns each payload's
// row of d_present (row b, or row d_pattern[b]; no other row is read) into a
// record of kRowMaskWords words: a 1024-bit mask of the rows
// to write (bit y: y < n_validators and present[y] == 0) and a word of phase
// flags (bit 0: a systematic row is wanted; bits 1..3: a row of coset 256, 512,
// 768).  Where the uniform kernel publishes the next tile's ticket, wave 0
// resolves that ticket's payload and copies the payload's record
// into LDS behind the ticket (one coalesced load); the ticket, the flags and
// the number of the mask buffer are read together by every wave.  There are
// two mask buffers: a tile's stores still test its own mask while the next
// tile's is being published.
//
// The schedule of a tile with skipped phases (enc_k256w_tile.inc, `M`).  The
// phases are the systematic rows and the cosets 256, 512, 768, in this order;
// a phase whose flag is clear does not run: no staging, no barrier of its own,
// no store, and for a coset no FFT.  The IFFT (with its barrier) runs iff a
// coset runs.  Every decision is read from the tile's one flag word, so it is
// uniform for the workgroup, and a wave without pieces takes the barriers of
// exactly the phases that run (the idle block tests the same flags).  Of the
// ticket protocol (enc_w_common.hpp):
//  * taken: thread 0, at the tile's start, as ever;
//  * published: behind the systematic stores, as in the uniform kernel, when
//    they and at least one coset run; in every other tile (no systematic rows,
//    or nothing but them, or nothing) right after the tile-start barrier, so
//    that the taken ticket is never kept in a register across a transform;
//  * a barrier: the IFFT's and the cosets' when a coset runs; the systematic
//    staging barrier when only the systematic rows do (published in front of
//    it, read behind it); a barrier of the tile's end when nothing runs;
//  * read, with the next tile's payload fetch: coset 768, when it runs, is the
//    last phase whatever else ran, and ends the tile as the uniform kernel's
//    last coset does (fetch_next in front of its staging barrier, the next
//    State behind its stores: store_last).  A tile without coset 768 ends with
//    tile_end: read, fetch and State behind the stores of whatever ran last.
//    (A last phase known only at run time would keep the fetched registers
//    and the next State alive across every phase -- the compiler cannot see
//    that exactly one phase is the last -- which does not fit 128 VGPRs;
//    profiles/repair/asm_identity.txt);
//  * rewritten only after the next tile-start barrier: every publication sits
//    behind one.
// Each of the four happens exactly once per tile whatever the flags.  The mask
// buffer a publication writes is the one the tile before this one stored
// under, whose last test precedes this tile's start barrier.
//
// A ticket past the end is published with flags 0; nothing of the plan is read
// for it.  d_pattern is read by the plan kernel only, and trusted as the
// reconstruct trusts it (it names rows that exist).
//
// publish / first run with all of wave 0 active: they make the ticket uniform
// with readfirstlane and load one word per lane.  The call sites are a store
// phase's `then`, behind per-lane branches of store_own (the row mask, rows at
// or above n_validators), and the tile start: like RaggedGeo's, they rely on
// the wave having reconverged there, which every path of store_own does
// before it calls `then`.
#include "enc_k256w_body.hpp"

namespace ecamd {
namespace {
namespace k256w {

struct MissingGeo {
  UniformGeo<TILE> u;          // the uniform batch's division of tickets into payloads and tiles
  uint32_t tiles_pp, total;    // u.prepare()'s, from the host: the publication needs no division chain
  const uint32_t *plan;        // [batch][kRowMaskWords]: payload b's record
  static constexpr bool MASKED = true;
  // LDS behind the kernel's SLOT: word 0 the ticket, 1 the mask buffer of its
  // tile, 2 its phase flags; from byte 16 two buffers of MASK_PITCH bytes
  static constexpr uint32_t MASK0 = 16, MASK_PITCH = 144;
  static constexpr uint32_t SLOT_BYTES = MASK0 + 2 * MASK_PITCH;
  static_assert(kRowMaskWords * 4 <= MASK_PITCH && MASK_PITCH % 16 == 0, "a record per buffer");
  struct Tile {
    uint32_t ticket, buf, flags;
  };
  using Pre = UniformGeo<TILE>::Pre;
  using Loc = UniformGeo<TILE>::Loc;
  using At = UniformGeo<TILE>::At;
  __device__ __forceinline__ Pre prepare() const { return {u.slen / 2, tiles_pp, total}; }
  __device__ __forceinline__ uint32_t ticket(const Tile &c) const { return c.ticket; }
  __device__ __forceinline__ uint32_t phases(const Tile &c) const { return c.flags; }
  __device__ __forceinline__ LdsRowMask row_mask(const Tile &c) const {
    return {SLOT + MASK0 + c.buf * MASK_PITCH};
  }
  __device__ __forceinline__ uint32_t next_ticket(const Tile &) const { return atomicAdd(u.tick, 1u); }
  // all of wave 0 (the call sites are reached by whole waves): lane j < 33
  // brings word j of the record
  __device__ __forceinline__ bool publishes(uint32_t tid0) const {
    return __builtin_amdgcn_readfirstlane(tid0 >> 6) == 0;
  }
  __device__ __forceinline__ void publish_to(LdsWord *slot, uint32_t ticket, uint32_t tid0, uint32_t buf) const {
    const uint32_t t = uint32_t(__builtin_amdgcn_readfirstlane(int(ticket)));
    asm volatile("" : "+v"(tid0));  // per-lane addresses formed here, not hoisted out of the tile loop and spilled
    uint32_t w = 0;
    if (t < total && tid0 < kRowMaskWords) {
      const uint64_t b = t / tiles_pp;
      w = plan[b * kRowMaskWords + tid0];
    }
    if (tid0 < MASK_PITCH / 4) slot[(MASK0 + buf * MASK_PITCH) / 4 + tid0] = w;
    if (tid0 == kRowMaskWords - 1) slot[2] = w;
    if (tid0 == 0) {
      slot[0] = t;
      slot[1] = buf;
    }
  }
  // the other buffer than the published tile's (slot[1]: this wave's own last store there)
  __device__ __forceinline__ void publish(LdsWord *slot, uint32_t ticket, uint32_t tid0) const {
    publish_to(slot, ticket, tid0, uint32_t(__builtin_amdgcn_readfirstlane(int(slot[1]))) ^ 1u);
  }
  __device__ __forceinline__ void first(LdsWord *slot, uint32_t tid0) const {
    uint32_t ticket = 0;
    if (tid0 == 0) ticket = atomicAdd(u.tick, 1u);
    publish_to(slot, ticket, tid0, 0u);
  }
  struct Read {
    Tile t;
  };
  __device__ __forceinline__ Read read(LdsWord *slot) const {
    return {{uint32_t(__builtin_amdgcn_readfirstlane(int(slot[0]))),
             uint32_t(__builtin_amdgcn_readfirstlane(int(slot[1]))),
             uint32_t(__builtin_amdgcn_readfirstlane(int(slot[2])))}};
  }
  __device__ __forceinline__ Loc loc(const Pre &p, const Tile &c) const { return u.loc(p, c.ticket); }
  __device__ __forceinline__ Loc loc_or_none(const Pre &p, const Tile &c) const { return u.loc_or_none(p, c.ticket); }
  __device__ __forceinline__ Fetch fetch(const Pre &p, Loc l) const { return u.fetch(p, l); }
  __device__ __forceinline__ At at(const Pre &p, const Tile &c) const { return u.at(p, c.ticket); }
  __device__ __forceinline__ uint64_t piece0(At a) const { return a.piece0; }
  // (made opaque per tile: its copy for the lanes' compares is formed where it
  // is used instead of being hoisted out of the tile loop and spilled)
  __device__ __forceinline__ uint64_t npieces(const Pre &p, const Tile &) const {
    uint64_t np = p.npieces;
    asm volatile("" : "+s"(np));
    return np;
  }
  __device__ __forceinline__ uint64_t sstride(const Tile &) const { return u.sstride_; }
  __device__ __forceinline__ uint8_t *rows(At a) const { return u.rows(a); }
};

}  // namespace k256w
}  // namespace

__global__ void __launch_bounds__(THREADS, 4) encode_k256w_missing(const uint8_t *__restrict__ payloads,
                                                                   uint64_t plen, uint64_t pstride,
                                                                   uint8_t *__restrict__ shards, uint64_t slen,
                                                                   uint64_t sstride, int nv, uint32_t batch,
                                                                   uint32_t tiles_pp, uint32_t total,
                                                                   const uint8_t *__restrict__ cimg,
                                                                   const uint32_t *__restrict__ plan,
                                                                   uint32_t *__restrict__ tick) {
  const k256w::MissingGeo geo{{payloads, plen, pstride, shards, slen, sstride, nv, batch, tick},
                              tiles_pp, total, plan};
#include "enc_k256w_tile.inc"
}

// scratch (required: no static schedule): the tile counter's block, then the
// plan (encode_missing_scratch_bytes).  The plan kernel and the counter's
// zeroing run in stream order before the encode, on every call and replay.
hipError_t launch_encode_k256w_missing(const CodeParams &p, const DevTables &t, const MissingCall &c, void *scratch,
                                       hipStream_t s) {
  if (!t.cimg || !scratch || !c.present) return hipErrorInvalidValue;
  if (p.nv <= 2 * k256w::K || p.nv > 1024) return hipErrorInvalidValue;  // cosets 256, 512 (, 768)
  constexpr int kLds = k256w::lds_bytes<k256w::MissingGeo>();
  int cus = 0;
  if (const hipError_t e = prepare_kernel(reinterpret_cast<const void *>(&encode_k256w_missing), kLds, &cus);
      e != hipSuccess)
    return e;
  const EncodeCall &ec = c.enc;
  const size_t sl = shard_len(p.k, ec.plen);
  const size_t tiles_pp = (sl / 2 + k256w::TILE - 1) / k256w::TILE;
  const size_t tiles = tiles_pp * ec.batch;
  if (tiles >= (size_t(1) << 32) - size_t(4) * cus) return hipErrorInvalidValue;  // 32-bit tickets (launch_w)
  uint32_t *tick = static_cast<uint32_t *>(scratch);
  uint32_t *plan = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(scratch) + kTileCounterBytes);
  if (const hipError_t e = launch_row_mask_plan(p, c.present, c.pattern, ec.batch, plan, s); e != hipSuccess)
    return e;
  if (const hipError_t e = launch_zero_counters(tick, sizeof(uint32_t), s); e != hipSuccess) return e;
  const size_t slots = 2 * size_t(cus);
  hipLaunchKernelGGL(encode_k256w_missing, dim3(unsigned(tiles < slots ? tiles : slots)), dim3(THREADS), kLds, s,
                     ec.payloads, uint64_t(ec.plen), uint64_t(ec.pstride), ec.shards, uint64_t(sl),
                     uint64_t(ec.sstride), int(p.nv), uint32_t(ec.batch), uint32_t(tiles_pp), uint32_t(tiles),
                     t.cimg, plan, tick);
  return hipGetLastError();
}

}  // namespace ecamd
