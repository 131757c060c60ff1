// ragged.hpp — ragged device batches (ec_amd.h ECCR_AMD_*_ragged): the item
// record, its validation (one function for the host's ECCR_AMD_ragged_check
// and the device's plan kernel), the workspace layout of a ragged call and
// the tile -> item lookup of the persistent kernels.
//
// A ragged call runs two kernels: ragged_plan (ragged.hip), which validates
// the items, counts each item's tiles for the kernel that follows and writes
// their exclusive prefix tile_first[batch + 1], the zeroed tile counter and
// d_status; then the encode / reconstruct kernel, for which tile ticket t
// belongs to the item i with tile_first[i] <= t < tile_first[i + 1].  An item
// that breaks the contract has no tiles: nothing of it is read or written.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ec_kernels.hpp"

namespace ecamd {

struct RaggedItem {  // == ECCR_AMD_RaggedItem
  uint64_t payload_off, payload_len, shard_off, shard_len, shard_stride;
};
static_assert(sizeof(RaggedItem) == 40, "ECCR_AMD_RaggedItem layout");

// The shard length an item runs with, 0 where it breaks the contract (length
// 0 or above max_len, odd shard_len, a pitch below the shard length, an
// offset or pitch that is no multiple of 16).  k = 2^logk.
__host__ __device__ inline uint64_t ragged_shard_len(const RaggedItem &it, uint64_t max_len, bool reconstruct,
                                                     uint32_t logk) {
  uint64_t sl;
  if (reconstruct) {
    sl = it.shard_len;
    if (sl == 0 || sl > max_len || (sl & 1)) return 0;
  } else {
    if (it.payload_len == 0 || it.payload_len > max_len) return 0;
    const uint64_t syms = it.payload_len / 2 + (it.payload_len & 1);  // gf_field.hpp shard_len
    sl = ((syms + (uint64_t(1) << logk) - 1) >> logk) * 2;
  }
  if (it.shard_stride < sl) return 0;
  if ((it.payload_off | it.shard_off | it.shard_stride) & 15) return 0;
  return sl;
}

// tiles of `tile` pieces / columns of an item of shard length sl (0: none)
__host__ __device__ inline uint32_t ragged_tiles(uint64_t sl, uint32_t tile) {
  return uint32_t((sl / 2 + tile - 1) / tile);
}

// What the persistent kernels' publishing wave needs to resolve a ticket,
// written by the plan kernel into the workspace.  The kernels take one pointer
// to it and load from it where a ticket is resolved, instead of keeping five
// kernel arguments in SGPRs through every tile (reconstruct_n1024x's 16-wave
// form has none to spare).
struct RaggedHdr {
  const uint8_t *in;   // encode: d_payloads; reconstruct: d_shards
  uint8_t *out;        // encode: d_shards; reconstruct: d_out
  const RaggedItem *items;
  const uint32_t *tile_first;
  uint32_t batch, total;  // total = tile_first[batch]
};

// One ragged call, built where it enters the library: the input and output
// buffers the items' offsets are relative to (encode: payloads in, shard rows
// out; reconstruct and systematic: shard rows in, payloads out), the device
// item array, the stated maximum length (payload_len for an encode, shard_len
// otherwise), the nullable status words, and the reconstruct's pattern rows.
struct RaggedCall {
  const uint8_t *in;
  const RaggedItem *items;
  size_t batch, max_len;
  uint8_t *out;
  uint32_t *status;
  const uint8_t *present = nullptr;  // the reconstruct alone, as in ReconCall
  const uint16_t *err_log = nullptr;
  const uint32_t *pattern = nullptr;
};

// ---- workspace of a ragged call: 256 B of counters (word 0: the tile
// counter; byte 64: the RaggedHdr), tile_first[batch + 1], then the kernel's
// own scratch (the gather order of reconstruct_n1024x_ragged; the generic
// kernels' transform buffers where n does not fit LDS), each part 256-B aligned
constexpr size_t kRaggedCounterBytes = 256, kRaggedHdrOffset = 64;
static_assert(kRaggedHdrOffset + sizeof(RaggedHdr) <= kRaggedCounterBytes, "the header fits the counter block");
inline RaggedHdr *ragged_hdr(void *ws) {
  return reinterpret_cast<RaggedHdr *>(static_cast<uint8_t *>(ws) + kRaggedHdrOffset);
}
inline size_t ragged_first_bytes(size_t batch) { return ((batch + 1) * 4 + 255) / 256 * 256; }
inline size_t ragged_scratch_offset(size_t batch) { return kRaggedCounterBytes + ragged_first_bytes(batch); }
inline uint32_t *ragged_tick(void *ws) { return static_cast<uint32_t *>(ws); }
inline uint32_t *ragged_first(void *ws) {
  return reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(ws) + kRaggedCounterBytes);
}

// The kernels of a ragged call (choose_*_ragged: by n_validators alone, the
// contract makes every item's alignment the same)
enum class RaggedKernel {
  encode_k256w_ragged,
  encode_g_ragged,
  reconstruct_n1024x_ragged,
  reconstruct_g_ragged,
  systematic_w_ragged,
  systematic_g_ragged,
};
const char *ragged_kernel_name(RaggedKernel k);
RaggedKernel choose_encode_ragged(const CodeParams &p);
RaggedKernel choose_reconstruct_ragged(const CodeParams &p);
RaggedKernel choose_systematic_ragged(const CodeParams &p);  // systematic_w_ragged from k = 16 on
uint32_t ragged_encode_tile(const CodeParams &p);       // pieces per tile of that kernel
uint32_t ragged_reconstruct_tile(const CodeParams &p);  // columns per tile
uint32_t ragged_systematic_tile(const CodeParams &p);   // columns per (column) tile

size_t ragged_encode_workspace_bytes(const CodeParams &p, size_t batch, size_t max_plen);
size_t ragged_reconstruct_workspace_bytes(const CodeParams &p, size_t batch, size_t max_slen);
size_t ragged_systematic_workspace_bytes(const CodeParams &p, size_t batch);  // the plan alone

// host copy of the items -> status {items that break the contract, lowest such index}
void ragged_check_host(const CodeParams &p, const RaggedItem *items, size_t batch, uint64_t max_len,
                       bool reconstruct, uint32_t status[2]);

// the plan kernel, in stream order before the call's kernel, for tiles of
// `tile` pieces / columns (c.in / c.out go into the RaggedHdr)
hipError_t launch_ragged_plan(const CodeParams &p, const RaggedCall &c, bool reconstruct, uint32_t tile, void *ws,
                              hipStream_t s);

// A ragged call: the plan kernel, then the kernel choose_*_ragged names.  `ws`:
// the whole workspace (ragged_*_workspace_bytes).  The systematic recovery
// reads every item's rows y < k (items in the reconstruct's meaning:
// payload_off in c.out).
hipError_t launch_encode_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                hipStream_t s);
hipError_t launch_reconstruct_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                     hipStream_t s);
hipError_t launch_systematic_ragged(const CodeParams &p, const RaggedCall &c, void *ws, hipStream_t s);
// the kernels' own launchers (enc_k256w_ragged.hip, dec_n1024x_ragged.hip,
// sys_w.hip, ec_kernels.hip), after the plan on the same stream; the persistent
// kernels take the buffers and the items from the plan's header
hipError_t launch_encode_k256w_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                      hipStream_t s);
hipError_t launch_reconstruct_n1024x_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                            hipStream_t s);
hipError_t launch_encode_g_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                  hipStream_t s);
hipError_t launch_reconstruct_g_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                       hipStream_t s);
hipError_t launch_systematic_w_ragged(const CodeParams &p, const RaggedCall &c, void *ws, hipStream_t s);
hipError_t launch_systematic_g_ragged(const CodeParams &p, const RaggedCall &c, void *ws, hipStream_t s);

#if defined(__HIPCC__)
// A global-memory address that travelled through LDS as two words, back as a
// pointer the compiler knows to be global (a plain integer cast gives a generic
// pointer: flat loads and stores, which also count on lgkmcnt).
template <typename T>
__device__ __forceinline__ T *ragged_global_ptr(uint64_t a) {
  return (T *)reinterpret_cast<__attribute__((address_space(1))) T *>(uintptr_t(a));
}

// The item of tile ticket t < tile_first[batch]: the largest i with
// tile_first[i] <= t (items without tiles repeat their successor's entry and
// are never the answer).  Called by one whole wave (all 64 lanes, uniform
// arguments); a 64-ary search, one coalesced probe per lane and round: one
// round up to 64 items, two up to 4096, three up to 2^18.  The result is
// wave-uniform.
__device__ __forceinline__ uint32_t ragged_find_item(const uint32_t *__restrict__ tile_first, uint32_t batch,
                                                     uint32_t t, uint32_t lane) {
  uint32_t lo = 1, n = batch;  // the count of j in [1, batch] with tile_first[j] <= t
  while (n > 0) {
    const uint32_t step = (n + 63) / 64, end = lo + n;
    const uint64_t p = uint64_t(lo) + uint64_t(lane + 1) * step - 1;  // the last entry of the lane's chunk
    const bool below = p < end && tile_first[p] <= t;
    const uint32_t c = uint32_t(__builtin_popcountll(__ballot(below)));  // whole chunks <= t
    lo += c * step;
    n = lo >= end ? 0 : (step - 1 < end - lo ? step - 1 : end - lo);
  }
  return uint32_t(__builtin_amdgcn_readfirstlane(int(lo - 1)));
}
#endif

}  // namespace ecamd
