// ragged.hip — the plan kernel and the dispatch of the ragged device-batch
// calls (ragged.hpp, ec_amd.h ECCR_AMD_*_ragged).
#include <hip/hip_runtime.h>

#include "ragged.hpp"

namespace ecamd {
namespace {

constexpr int kPlanThreads = 1024;

// One workgroup: per item its validation and tile count (ragged_shard_len /
// ragged_tiles, the functions ECCR_AMD_ragged_check runs on the host), the
// exclusive prefix of the counts in chunks of kPlanThreads items with a
// running carry (one chunk up to 1024 items; a million items are ~1000 chunk
// steps of a few hundred ns each), the zeroed tile counter, the header the
// persistent kernels resolve tickets from (RaggedHdr) and the status words.
// Reads 40 B and writes 4 B per item.  Everything the following kernel reads
// from the workspace is written here on every call, so a captured call
// replays with the item array's current contents.
__global__ void __launch_bounds__(kPlanThreads) ragged_plan(const RaggedItem *__restrict__ items, uint32_t batch,
                                                            uint64_t max_len, int reconstruct, uint32_t logk,
                                                            uint32_t tile, const uint8_t *in, uint8_t *out,
                                                            uint32_t *__restrict__ tile_first,
                                                            uint32_t *__restrict__ tick, RaggedHdr *__restrict__ hdr,
                                                            uint32_t *__restrict__ status) {
  __shared__ uint32_t wsum[kPlanThreads / 64];
  __shared__ uint32_t carry, bad_count, bad_first;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    carry = 0;
    bad_count = 0;
    bad_first = 0xFFFFFFFFu;
    tick[0] = 0;
  }
  __syncthreads();
  uint32_t my_bad = 0, my_first = 0xFFFFFFFFu;
  for (uint32_t base = 0; base < batch; base += kPlanThreads) {
    const uint32_t i = base + tid;
    uint32_t cnt = 0;
    if (i < batch) {
      const uint64_t sl = ragged_shard_len(items[i], max_len, reconstruct != 0, logk);
      cnt = ragged_tiles(sl, tile);
      if (sl == 0) {
        ++my_bad;
        if (i < my_first) my_first = i;
      }
    }
    uint32_t incl = cnt;  // inclusive scan over the wave, then over the waves' sums
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = uint32_t(__shfl_up(int(incl), o));
      if (lane >= uint32_t(o)) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
    if (i < batch) tile_first[i] = before + incl - cnt;
    __syncthreads();  // carry and wsum read by everyone
    if (tid == kPlanThreads - 1) carry = before + incl;
    __syncthreads();
  }
  if (my_bad) {
    atomicAdd(&bad_count, my_bad);
    atomicMin(&bad_first, my_first);
  }
  __syncthreads();
  if (tid == 0) {
    tile_first[batch] = carry;
    *hdr = RaggedHdr{in, out, items, tile_first, batch, carry};
    if (status) {
      status[0] = bad_count;
      status[1] = bad_count ? bad_first : 0u;
    }
  }
}

int ilog2(uint32_t v) { return 31 - __builtin_clz(v); }

}  // namespace

void ragged_check_host(const CodeParams &p, const RaggedItem *items, size_t batch, uint64_t max_len,
                       bool reconstruct, uint32_t status[2]) {
  status[0] = status[1] = 0;
  for (size_t i = batch; i-- > 0;)
    if (ragged_shard_len(items[i], max_len, reconstruct, uint32_t(ilog2(p.k))) == 0) {
      ++status[0];
      status[1] = uint32_t(i);
    }
}

hipError_t launch_ragged_plan(const CodeParams &p, const RaggedCall &c, bool reconstruct, uint32_t tile, void *ws,
                              hipStream_t s) {
  hipLaunchKernelGGL(ragged_plan, dim3(1), dim3(kPlanThreads), 0, s, c.items, uint32_t(c.batch),
                     uint64_t(c.max_len), reconstruct ? 1 : 0, uint32_t(ilog2(p.k)), tile, c.in, c.out,
                     ragged_first(ws), ragged_tick(ws), ragged_hdr(ws), c.status);
  return hipGetLastError();
}

const char *ragged_kernel_name(RaggedKernel k) {
  switch (k) {
    case RaggedKernel::encode_k256w_ragged: return "encode_k256w_ragged";
    case RaggedKernel::encode_g_ragged: return "encode_g_ragged";
    case RaggedKernel::reconstruct_n1024x_ragged: return "reconstruct_n1024x_ragged";
    case RaggedKernel::reconstruct_g_ragged: return "reconstruct_g_ragged";
    case RaggedKernel::systematic_w_ragged: return "systematic_w_ragged";
    case RaggedKernel::systematic_g_ragged: return "systematic_g_ragged";
  }
  return nullptr;
}

// k = 256, n = 1024 with the third coset in use (n_validators 766 .. 1024):
// the shapes encode_k256w / reconstruct_n1024x take in the uniform calls
RaggedKernel choose_encode_ragged(const CodeParams &p) {
  return k256_applicable(p) && p.n == 1024 ? RaggedKernel::encode_k256w_ragged : RaggedKernel::encode_g_ragged;
}
RaggedKernel choose_reconstruct_ragged(const CodeParams &p) {
  return n1024_applicable(p) ? RaggedKernel::reconstruct_n1024x_ragged : RaggedKernel::reconstruct_g_ragged;
}

// (the contract puts every item's offsets and pitch on 16 B: k alone decides)
RaggedKernel choose_systematic_ragged(const CodeParams &p) {
  return p.k >= 16 ? RaggedKernel::systematic_w_ragged : RaggedKernel::systematic_g_ragged;
}

size_t ragged_systematic_workspace_bytes(const CodeParams &, size_t batch) { return ragged_scratch_offset(batch); }

size_t ragged_encode_workspace_bytes(const CodeParams &p, size_t batch, size_t max_plen) {
  const size_t own = choose_encode_ragged(p) == RaggedKernel::encode_g_ragged
                         ? generic_scratch_bytes(p.k, shard_len(p.k, max_plen) / 2, batch)
                         : 0;
  return ragged_scratch_offset(batch) + (own + 255) / 256 * 256;
}

size_t ragged_reconstruct_workspace_bytes(const CodeParams &p, size_t batch, size_t max_slen) {
  const size_t own = choose_reconstruct_ragged(p) == RaggedKernel::reconstruct_g_ragged
                         ? generic_scratch_bytes(p.n, max_slen / 2, batch)
                         : gather_order_bytes(p, batch);
  return ragged_scratch_offset(batch) + (own + 255) / 256 * 256;
}

hipError_t launch_encode_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                hipStream_t s) {
  if (const hipError_t e = launch_ragged_plan(p, c, false, ragged_encode_tile(p), ws, s); e != hipSuccess) return e;
  return choose_encode_ragged(p) == RaggedKernel::encode_k256w_ragged ? launch_encode_k256w_ragged(p, t, c, ws, s)
                                                                       : launch_encode_g_ragged(p, t, c, ws, s);
}

hipError_t launch_reconstruct_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                     hipStream_t s) {
  if (const hipError_t e = launch_ragged_plan(p, c, true, ragged_reconstruct_tile(p), ws, s); e != hipSuccess)
    return e;
  return choose_reconstruct_ragged(p) == RaggedKernel::reconstruct_n1024x_ragged
             ? launch_reconstruct_n1024x_ragged(p, t, c, ws, s)
             : launch_reconstruct_g_ragged(p, t, c, ws, s);
}

hipError_t launch_systematic_ragged(const CodeParams &p, const RaggedCall &c, void *ws, hipStream_t s) {
  if (const hipError_t e = launch_ragged_plan(p, c, true, ragged_systematic_tile(p), ws, s); e != hipSuccess)
    return e;
  return choose_systematic_ragged(p) == RaggedKernel::systematic_w_ragged ? launch_systematic_w_ragged(p, c, ws, s)
                                                                           : launch_systematic_g_ragged(p, c, ws, s);
}

}  // namespace ecamd
