// sys_w.hip — systematic_w / systematic_w_ragged: the systematic recovery
// (reed-solomon.hpp:143-179), out[2(i*k + y) ..] = row_y[2i ..] for rows y < k
// and columns i < shard_len / 2, as a tiled transpose through LDS for k >= 16
// and 16-B aligned bases and pitches (choose_systematic, ec_kernels.hip).
//
// Tile: 16,384 symbols (32 KB), R = min(k, 256) rows x C = 16384 / R columns;
// for k > 256 a column tile is walked in k / 256 row blocks, one ticket each
// (row block fastest: consecutive tickets write neighbouring output).  Every
// k reads row segments of >= 128 B and writes runs of >= 512 B; the body, the
// LDS layout and its swizzle are in sys_w_body.inc, the account in DESIGN.md
// §5.10.  A workgroup is 4 waves on one tile; four workgroups per CU (128 KB of
// LDS, 4 waves per SIMD) keep 4 x 32 KB of loads in flight per CU.
//
// Tickets: a workgroup's first tile is its index, every further one
// gridDim.x + the counter `tick` (zeroed by a kernel before the launch), or
// the static stride gridDim.x without a counter (no workspace, or a launch
// with no more tiles than workgroups).  Offsets are 64-bit.
#include <hip/hip_runtime.h>

#include "ec_device.hpp"
#include "ec_kernels.hpp"
#include "ragged.hpp"

namespace ecamd {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr int kSysThreads = 256, kSysTileSyms = 16384, kSysPerCu = 4;

// a resolved ticket (every member wave-uniform)
struct SysTile {
  const uint8_t *SH;  // row 0 of the tile's row block
  uint8_t *O;         // the item's output at the row block's first symbol
  uint64_t slen, pitch;
  uint64_t i0;        // the tile's first column
};

__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
  return uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(x))))) |
         (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(x >> 32))))) << 32);
}

// the uniform batch: item b at b * n_validators rows, every item as long
struct UniformSysW {
  const uint8_t *shards;
  uint8_t *out;
  uint64_t slen, sstride, item_pitch, ostride;
  uint64_t tiles_per_item, tiles;
  __device__ __forceinline__ uint64_t total(int) const { return tiles; }
  __device__ __forceinline__ SysTile resolve(uint64_t t, uint32_t, int logR, int lognrb) const {
    const uint64_t b = t / tiles_per_item, r = t - b * tiles_per_item;
    const uint64_t rb = r & ((uint64_t(1) << lognrb) - 1);
    return {shards + b * item_pitch + (rb << logR) * sstride, out + b * ostride + (rb << (logR + 1)), slen, sstride,
            (r >> lognrb) << (14 - logR)};
  }
};

// the ragged batch: column tile ct = t >> lognrb belongs to the item i with
// tile_first[i] <= ct < tile_first[i + 1] (the plan kernel's prefix over
// column tiles, ragged.hip); every wave looks its ticket up itself
struct RaggedSysW {
  const RaggedHdr *hdr;
  __device__ __forceinline__ uint64_t total(int lognrb) const { return uint64_t(hdr->total) << lognrb; }
  __device__ __forceinline__ SysTile resolve(uint64_t t, uint32_t lane, int logR, int lognrb) const {
    const RaggedHdr h = *hdr;
    const uint32_t ct = uint32_t(t >> lognrb);
    const uint64_t rb = t & ((uint64_t(1) << lognrb) - 1);
    // (pointers from the header are global memory: ragged_global_ptr)
    const uint32_t *first = ragged_global_ptr<const uint32_t>(reinterpret_cast<uintptr_t>(h.tile_first));
    const uint32_t i = ragged_find_item(first, h.batch, ct, lane);
    const RaggedItem it = ragged_global_ptr<const RaggedItem>(reinterpret_cast<uintptr_t>(h.items))[i];
    const uint8_t *in = ragged_global_ptr<const uint8_t>(reinterpret_cast<uintptr_t>(h.in));
    uint8_t *o = ragged_global_ptr<uint8_t>(reinterpret_cast<uintptr_t>(h.out));
    // the record was loaded per lane: back into scalars
    const uint64_t soff = uniform64(it.shard_off), ooff = uniform64(it.payload_off);
    const uint64_t slen = uniform64(it.shard_len), pitch = uniform64(it.shard_stride);
    const uint32_t tile = uint32_t(__builtin_amdgcn_readfirstlane(int(ct - first[i])));
    return {in + soff + (rb << logR) * pitch, o + ooff + (rb << (logR + 1)), slen, pitch,
            uint64_t(tile) << (14 - logR)};
  }
};

}  // namespace

__global__ void __launch_bounds__(kSysThreads, 4) systematic_w(const uint8_t *__restrict__ shards, uint64_t slen,
                                                               uint64_t sstride, uint64_t item_pitch, int logk,
                                                               uint8_t *__restrict__ out, uint64_t ostride,
                                                               uint64_t tiles_per_item, uint64_t tiles,
                                                               uint32_t *tick) {
  const UniformSysW geo{shards, out, slen, sstride, item_pitch, ostride, tiles_per_item, tiles};
#include "sys_w_body.inc"
}

__global__ void __launch_bounds__(kSysThreads, 4) systematic_w_ragged(const RaggedHdr *__restrict__ hdr, int logk,
                                                                      uint32_t *tick) {
  const RaggedSysW geo{hdr};
#include "sys_w_body.inc"
}

namespace {
int ilog2(uint32_t v) { return 31 - __builtin_clz(v); }
}  // namespace

uint32_t systematic_w_cols(const CodeParams &p) { return uint32_t(kSysTileSyms) / (p.k < 256 ? p.k : 256u); }
uint32_t systematic_w_row_blocks(const CodeParams &p) { return p.k <= 256 ? 1u : p.k / 256; }

hipError_t launch_systematic_w(const CodeParams &p, const SysCall &c, void *scratch, hipStream_t s) {
  int cus = 0;
  if (const hipError_t e = prepare_kernel(reinterpret_cast<const void *>(&systematic_w), 0, &cus); e != hipSuccess)
    return e;
  const size_t cols = systematic_w_cols(p);
  const size_t per_item = (c.slen / 2 + cols - 1) / cols * systematic_w_row_blocks(p);
  const size_t tiles = per_item * c.batch;
  const size_t slots = size_t(kSysPerCu) * cus;
  const unsigned grid = unsigned(tiles < slots ? tiles : slots);
  // 32-bit tickets from the counter; a launch past them keeps the static
  // stride, and one whose workgroups have a single tile each needs neither
  // (small calls stay one launch)
  uint32_t *tick = tiles > slots && tiles + slots < (size_t(1) << 32) ? static_cast<uint32_t *>(scratch) : nullptr;
  if (tick)
    if (const hipError_t e = launch_zero_counters(tick, sizeof(uint32_t), s); e != hipSuccess) return e;
  hipLaunchKernelGGL(systematic_w, dim3(grid), dim3(kSysThreads), 0, s, c.shards, uint64_t(c.slen),
                     uint64_t(c.sstride), uint64_t(p.nv) * c.sstride, ilog2(p.k), c.out, uint64_t(c.ostride),
                     uint64_t(per_item), uint64_t(tiles), tick);
  return hipGetLastError();
}

// `ws` planned by launch_ragged_plan (tile = systematic_w_cols) in stream order
// before this; the plan zeroes the counter.  The grid is sized from the most
// tiles the call can have: workgroups past the real count leave at once.
hipError_t launch_systematic_w_ragged(const CodeParams &p, const RaggedCall &c, void *ws, hipStream_t s) {
  int cus = 0;
  if (!ws) return hipErrorInvalidValue;
  if (const hipError_t e = prepare_kernel(reinterpret_cast<const void *>(&systematic_w_ragged), 0, &cus);
      e != hipSuccess)
    return e;
  const size_t cols = systematic_w_cols(p);
  const size_t most = (c.max_len / 2 + cols - 1) / cols * systematic_w_row_blocks(p) * c.batch;
  if (most + 4096 >= (size_t(1) << 32)) return hipErrorInvalidValue;  // 32-bit tile tickets
  const size_t slots = size_t(kSysPerCu) * cus;
  const unsigned grid = unsigned(most < slots ? most : slots);
  hipLaunchKernelGGL(systematic_w_ragged, dim3(grid), dim3(kSysThreads), 0, s, ragged_hdr(ws), ilog2(p.k),
                     ragged_tick(ws));
  return hipGetLastError();
}

}  // namespace ecamd
