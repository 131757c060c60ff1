// ec_kernels.hip — HIP kernels for gfx950: NPB Reed-Solomon encode, erasure
// locator, reconstruct, systematic reconstruct.
//
// Generic path ("g" kernels): one workgroup owns G byte-planar groups (4 pieces
// or 4 shard positions each) and runs the additive FFT stage by stage on a
// [position][group] uint2 array in LDS (or global scratch for FFTs above
// 4096 points).  Butterflies follow additive_fft.hpp:99-141 exactly; the
// multiply is the v_perm lookup of ec_device.hpp.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "ec_device.hpp"
#include "ec_kernels.hpp"
#include "ragged.hpp"

namespace ecamd {
namespace {

constexpr int kBlock = 256;
constexpr int kLdsSlots = 4096;  // uint2 slots per buffer in LDS (32 KiB)

__device__ __forceinline__ void ld(uint2 *p, uint32_t &l, uint32_t &h) {
  const uint2 v = *p;
  l = v.x;
  h = v.y;
}

// inverse_afft (additive_fft.hpp:99-119) on S[pos * G + g], pos < 2^logsz.
// Small transforms (<= 3 stages, at most one butterfly per thread and stage:
// the per-call sizes of tiny codes, e.g. n_validators 6) request every
// stage's table up front, so the stages wait on one table latency instead of
// one each (the per-call C ABI's kernel time).
constexpr int kPreStages = 3;
__device__ void ifft_g(uint2 *S, int logG, int logsz, uint32_t index, const DevTables t) {
  const int G = 1 << logG;
  const int half = (1 << logsz) >> 1;
  if (logsz <= kPreStages && half * G <= int(blockDim.x)) {
    const int b = threadIdx.x, g = b & (G - 1), pi = b >> logG;
    const bool on = b < half * G;
    Tab T[kPreStages];
#pragma unroll
    for (int m = 0; m < kPreStages; ++m) {
      const int d = 1 << m, i = ((pi >> m) << (m + 1)) | (pi & (d - 1)), j = (i & ~(2 * d - 1)) | d;
      if (on && m < logsz) load_tab(t.mslot, j - 1 + index, T[m]);
    }
#pragma unroll
    for (int m = 0; m < kPreStages; ++m) {
      if (m >= logsz) break;
      const int d = 1 << m, i = ((pi >> m) << (m + 1)) | (pi & (d - 1));
      if (on) {
        uint32_t al, ah, bl, bh;
        ld(S + i * G + g, al, ah);
        ld(S + (i + d) * G + g, bl, bh);
        bl ^= al;
        bh ^= ah;
        mul_acc(bl, bh, T[m], al, ah);
        S[i * G + g] = make_uint2(al, ah);
        S[(i + d) * G + g] = make_uint2(bl, bh);
      }
      __syncthreads();
    }
    return;
  }
  for (int m = 0; m < logsz; ++m) {
    const int d = 1 << m;
    for (int b = threadIdx.x; b < half * G; b += blockDim.x) {
      const int g = b & (G - 1), pi = b >> logG;
      const int i = ((pi >> m) << (m + 1)) | (pi & (d - 1));
      const int j = (i & ~(2 * d - 1)) | d;
      Tab T;
      load_tab(t.mslot, j - 1 + index, T);  // (mtab[skews[..]]: no dependent load)
      uint32_t al, ah, bl, bh;
      ld(S + i * G + g, al, ah);
      ld(S + (i + d) * G + g, bl, bh);
      bl ^= al;
      bh ^= ah;
      mul_acc(bl, bh, T, al, ah);
      S[i * G + g] = make_uint2(al, ah);
      S[(i + d) * G + g] = make_uint2(bl, bh);
    }
    __syncthreads();
  }
}

// afft (additive_fft.hpp:121-141); small transforms as in ifft_g
__device__ void fft_g(uint2 *S, int logG, int logsz, uint32_t index, const DevTables t) {
  const int G = 1 << logG;
  const int half = (1 << logsz) >> 1;
  if (logsz <= kPreStages && half * G <= int(blockDim.x)) {
    const int b = threadIdx.x, g = b & (G - 1), pi = b >> logG;
    const bool on = b < half * G;
    Tab T[kPreStages];
#pragma unroll
    for (int m = 0; m < kPreStages; ++m) {
      const int d = 1 << m, i = ((pi >> m) << (m + 1)) | (pi & (d - 1)), j = (i & ~(2 * d - 1)) | d;
      if (on && m < logsz) load_tab(t.mslot, j - 1 + index, T[m]);
    }
#pragma unroll
    for (int m = kPreStages - 1; m >= 0; --m) {
      if (m >= logsz) continue;
      const int d = 1 << m, i = ((pi >> m) << (m + 1)) | (pi & (d - 1));
      if (on) {
        uint32_t al, ah, bl, bh;
        ld(S + i * G + g, al, ah);
        ld(S + (i + d) * G + g, bl, bh);
        mul_acc(bl, bh, T[m], al, ah);
        bl ^= al;
        bh ^= ah;
        S[i * G + g] = make_uint2(al, ah);
        S[(i + d) * G + g] = make_uint2(bl, bh);
      }
      __syncthreads();
    }
    return;
  }
  for (int m = logsz - 1; m >= 0; --m) {
    const int d = 1 << m;
    for (int b = threadIdx.x; b < half * G; b += blockDim.x) {
      const int g = b & (G - 1), pi = b >> logG;
      const int i = ((pi >> m) << (m + 1)) | (pi & (d - 1));
      const int j = (i & ~(2 * d - 1)) | d;
      Tab T;
      load_tab(t.mslot, j - 1 + index, T);
      uint32_t al, ah, bl, bh;
      ld(S + i * G + g, al, ah);
      ld(S + (i + d) * G + g, bl, bh);
      mul_acc(bl, bh, T, al, ah);
      bl ^= al;
      bh ^= ah;
      S[i * G + g] = make_uint2(al, ah);
      S[(i + d) * G + g] = make_uint2(bl, bh);
    }
    __syncthreads();
  }
}

// the fused completion signal (HostSig): every thread's output is made
// visible at system scope, then one lane stores v
__device__ __forceinline__ void signal_end(uint32_t *flag, uint32_t v) {
  if (!flag) return;
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- geometry policies of the generic kernels: where item b's payload,
// shard rows and output are and how long they are, for the block's tile
// blockIdx.x (4 G pieces / positions).  `on` false: the block has nothing to
// do for that item (block-uniform; tested before any barrier of the iteration).
// The reconstruct's policies answer field by field (on, rows, outp, npos,
// pitch), in the order the kernel body asks.
struct EncItemG {
  const uint8_t *P;
  uint8_t *SH;
  uint64_t plen, npieces, sstride;
  bool on;
};
// the uniform batch: item b at b * pitch, every item as long as the others
struct UniformEncG {
  uint64_t plen, pstride, slen, sstride;
  static constexpr bool MASKED = false;
  struct Pre {
    uint64_t npieces;  // per launch: pieces per payload
  };
  __device__ __forceinline__ Pre prepare() const { return {slen / 2}; }
  __device__ __forceinline__ EncItemG item(const Pre &p, const uint8_t *payloads, uint8_t *shards, uint32_t b,
                                           int nv) const {
    return {payloads + uint64_t(b) * pstride, shards + uint64_t(b) * nv * sstride, plen, p.npieces, sstride, true};
  }
};
// the masked encode (encode_g_missing): the uniform batch, and payload b's
// present row (n bytes a row; row pattern[b] with a pattern array)
struct MissingEncG {
  UniformEncG u;
  const uint8_t *present;
  const uint32_t *pattern;
  uint32_t n;
  static constexpr bool MASKED = true;
  using Pre = UniformEncG::Pre;
  __device__ __forceinline__ Pre prepare() const { return u.prepare(); }
  __device__ __forceinline__ EncItemG item(const Pre &p, const uint8_t *payloads, uint8_t *shards, uint32_t b,
                                           int nv) const {
    return u.item(p, payloads, shards, b, nv);
  }
  __device__ __forceinline__ const uint8_t *present_row(uint32_t b) const {
    return present + uint64_t(pattern ? pattern[b] : b) * n;
  }
};
// a MASKED policy's present row of payload b (a form that compiles for every
// policy: the body is a fragment inside non-template kernels)
template <typename Geo>
__device__ __forceinline__ const uint8_t *enc_g_present(const Geo &geo, uint32_t b) {
  if constexpr (Geo::MASKED)
    return geo.present_row(b);
  else
    return nullptr;
}
struct UniformRecG {
  uint64_t slen, sstride, ostride;
  struct Pre {
    uint64_t npos;  // per launch: positions per shard
  };
  __device__ __forceinline__ Pre prepare() const { return {slen / 2}; }
  __device__ __forceinline__ bool on(uint32_t) const { return true; }
  __device__ __forceinline__ const uint8_t *rows(const uint8_t *shards, uint32_t b, int nv) const {
    return shards + uint64_t(b) * nv * sstride;
  }
  __device__ __forceinline__ uint8_t *outp(uint8_t *out, uint32_t b) const { return out + uint64_t(b) * ostride; }
  __device__ __forceinline__ uint64_t npos(const Pre &p, uint32_t) const { return p.npos; }
  __device__ __forceinline__ uint64_t pitch(uint32_t) const { return sstride; }
};
struct NoPre {};
// the ragged batch (ragged.hpp): item b's record, and its tile count from the
// plan kernel's prefix; a block whose tile is past the item's last (or an item
// without tiles: one that broke the contract) skips it without reading its record
struct RaggedEncG {
  const RaggedItem *items;
  const uint32_t *tile_first;
  int logk;
  static constexpr bool MASKED = false;
  __device__ __forceinline__ NoPre prepare() const { return {}; }
  __device__ __forceinline__ EncItemG item(NoPre, const uint8_t *payloads, uint8_t *shards, uint32_t b, int) const {
    if (blockIdx.x >= tile_first[b + 1] - tile_first[b]) return {nullptr, nullptr, 0, 0, 0, false};
    const RaggedItem it = items[b];
    const uint64_t syms = it.payload_len / 2 + (it.payload_len & 1);
    return {payloads + it.payload_off, shards + it.shard_off, it.payload_len,
            (syms + (uint64_t(1) << logk) - 1) >> logk, it.shard_stride, true};
  }
};
struct RaggedRecG {
  const RaggedItem *items;
  const uint32_t *tile_first;
  __device__ __forceinline__ NoPre prepare() const { return {}; }
  __device__ __forceinline__ bool on(uint32_t b) const { return blockIdx.x < tile_first[b + 1] - tile_first[b]; }
  __device__ __forceinline__ const uint8_t *rows(const uint8_t *shards, uint32_t b, int) const {
    return shards + items[b].shard_off;
  }
  __device__ __forceinline__ uint8_t *outp(uint8_t *out, uint32_t b) const { return out + items[b].payload_off; }
  __device__ __forceinline__ uint64_t npos(NoPre, uint32_t b) const { return items[b].shard_len / 2; }
  __device__ __forceinline__ uint64_t pitch(uint32_t b) const { return items[b].shard_stride; }
};

// reed-solomon.hpp:47-81 + poly_encoder.hpp:31-86,217-240 for 4*G pieces: the
// body is enc_g_body.inc (one copy, shared with the ragged form)
__global__ void __launch_bounds__(kBlock) encode_g(const uint8_t *__restrict__ payloads,
                                                   uint64_t plen, uint64_t pstride,
                                                   uint8_t *__restrict__ shards, uint64_t slen,
                                                   uint64_t sstride, int nv, int logn, int logk,
                                                   int logG, uint32_t batch, DevTables t,
                                                   uint2 *scratch, uint32_t *sig_flag, uint32_t sig_v) {
  const UniformEncG geo{plen, pstride, slen, sstride};
#include "enc_g_body.inc"
}

// the ragged form: grid.x from the longest item the call allows, the
// blockIdx.y loop over the items
__global__ void __launch_bounds__(kBlock) encode_g_ragged(const uint8_t *__restrict__ payloads,
                                                          const RaggedItem *__restrict__ items,
                                                          const uint32_t *__restrict__ tile_first,
                                                          uint8_t *__restrict__ shards, int nv, int logn,
                                                          int logk, int logG, uint32_t batch, DevTables t,
                                                          uint2 *scratch) {
  const RaggedEncG geo{items, tile_first, logk};
  uint32_t *const sig_flag = nullptr;  // (no fused completion signal: never a per-call launch)
  const uint32_t sig_v = 0;
#include "enc_g_body.inc"
}

// the masked form (ec_amd.h ECCR_AMD_encode_missing_batch): only the rows a
// payload's present row marks missing are written
__global__ void __launch_bounds__(kBlock) encode_g_missing(const uint8_t *__restrict__ payloads,
                                                           uint64_t plen, uint64_t pstride,
                                                           uint8_t *__restrict__ shards, uint64_t slen,
                                                           uint64_t sstride, int nv, int logn, int logk,
                                                           int logG, uint32_t batch, DevTables t,
                                                           uint2 *scratch,
                                                           const uint8_t *__restrict__ present,
                                                           const uint32_t *__restrict__ pattern) {
  const MissingEncG geo{{plen, pstride, slen, sstride}, present, pattern, 1u << logn};
  uint32_t *const sig_flag = nullptr;  // (no fused completion signal: never a per-call launch)
  const uint32_t sig_v = 0;
#include "enc_g_body.inc"
}

// poly_encoder.hpp:90-116 in the folded n-point form: one
// workgroup per erasure pattern.  W lives in LDS (n <= 65536 -> 128 KiB) or
// in global scratch.
__global__ void __launch_bounds__(kBlock) error_locator_g(const uint8_t *__restrict__ present,
                                                          int nv, int logn,
                                                          const uint16_t *__restrict__ fold,
                                                          const uint32_t *__restrict__ pattern,
                                                          uint16_t *__restrict__ elog,
                                                          uint16_t *scratch) {
  extern __shared__ __attribute__((aligned(16))) uint16_t w16[];
  const int n = 1 << logn;
  if (pattern && pattern[blockIdx.x] != blockIdx.x) return;  // computed by its pattern's leader
  const uint8_t *pr = present + uint64_t(blockIdx.x) * n;
  uint16_t *W = scratch ? scratch + uint64_t(blockIdx.x) * n : w16;
  for (int i = threadIdx.x; i < n; i += blockDim.x) W[i] = (i < nv && pr[i]) ? 0 : 1;
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    for (int h = 1; h < n; h <<= 1) {  // walsh.hpp:15-39
      for (int b = threadIdx.x; b < n / 2; b += blockDim.x) {
        const int i = (b / h) * 2 * h + (b % h);
        const uint32_t x = W[i], y = W[i + h];
        const uint32_t s = x + y, u = x + 65535u - y;
        W[i] = uint16_t((s & 0xffff) + (s >> 16));
        W[i + h] = uint16_t((u & 0xffff) + (u >> 16));
      }
      __syncthreads();
    }
    if (pass == 0) {
      for (int i = threadIdx.x; i < n; i += blockDim.x)
        W[i] = uint16_t((uint32_t(W[i]) * fold[i]) % 65535u);
      __syncthreads();
    }
  }
  uint16_t *E = elog + uint64_t(blockIdx.x) * n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const bool erased = !(i < nv && pr[i]);
    E[i] = erased ? uint16_t(65535u - W[i]) : W[i];
  }
}

// The same folded locator with one WAVE per erasure pattern, for 64 <= n <= 4096
// (round 3): V = n / 64 positions per lane (position lane * V + r), the Walsh
// stages over register bits in registers and over the six lane bits by
// __shfl_xor; no LDS, no barrier, four patterns per 256-thread workgroup.  The
// workgroup form above spends ~20 barriers per pattern; at 4096 distinct
// patterns (n = 1024) it took 43 us, this form ~5 us, which also makes the
// pattern dedup (~35 us of hash / insert / resolve / broadcast kernels) cost
// more than it can save for n <= 4096: ECCR_AMD_error_locator computes every
// row directly there.  Results are congruent mod 65535 to the reference's
// (the workgroup form's arithmetic, term for term).
__device__ __forceinline__ uint32_t fold16(uint32_t s) { return (s & 0xffffu) + (s >> 16); }

template <int V>
__device__ __forceinline__ void walsh_wave(uint32_t (&w)[V], uint32_t lane) {
#pragma unroll
  for (int h = 1; h < V; h <<= 1)  // register bits
#pragma unroll
    for (int r = 0; r < V; ++r)
      if (!(r & h)) {
        const uint32_t x = w[r], y = w[r + h];
        w[r] = fold16(x + y);
        w[r + h] = fold16(x + 65535u - y);
      }
#pragma unroll
  for (int m = 0; m < 6; ++m) {  // lane bits: the partner is lane ^ 2^m
    const bool upper = (lane >> m) & 1;
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const uint32_t o = uint32_t(__shfl_xor(int(w[r]), 1 << m));
      w[r] = upper ? fold16(o + 65535u - w[r]) : fold16(w[r] + o);
    }
  }
}

template <int V>
__global__ void __launch_bounds__(256) error_locator_w(const uint8_t *__restrict__ present, int nv,
                                                       uint32_t rows,
                                                       const uint16_t *__restrict__ fold,
                                                       const uint32_t *__restrict__ pattern,
                                                       uint16_t *__restrict__ elog) {
  constexpr uint32_t n = 64 * V;
  const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= rows) return;                             // whole waves
  if (pattern && pattern[b] != b) return;            // computed by its pattern's leader
  const uint8_t *pr = present + uint64_t(b) * n + lane * V;
  const uint16_t *F = fold + lane * V;
  uint32_t w[V];
  uint64_t erased = 0;
#pragma unroll
  for (int r = 0; r < V; ++r) {
    const bool e = !(int(lane * V + r) < nv && pr[r]);
    erased |= uint64_t(e) << r;
    w[r] = e;
  }
  walsh_wave<V>(w, lane);
#pragma unroll
  for (int r = 0; r < V; ++r) w[r] = fold16(fold16(w[r] * uint32_t(F[r])));  // W * F mod 65535
  walsh_wave<V>(w, lane);
  uint16_t *E = elog + uint64_t(b) * n + lane * V;
#pragma unroll
  for (int r = 0; r < V; ++r) E[r] = uint16_t(((erased >> r) & 1) ? 65535u - w[r] : w[r]);
}

// ---- erasure-pattern dedup: payloads whose erasure
// patterns are equal share one locator.  The locator depends only on the
// flags (present[i] != 0) of positions i < nv, and so do the hash and the
// equality test below.
__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// block per row: H = sum over present positions i of mix64(i) (order-free, so
// a block-wide sum); never 0 (0 marks an empty hash slot)
__global__ void __launch_bounds__(kBlock) pattern_hash(const uint8_t *__restrict__ present, int nv,
                                                       int n, uint64_t *__restrict__ hash) {
  __shared__ uint64_t part[kBlock / 64];
  const uint8_t *pr = present + uint64_t(blockIdx.x) * n;
  uint64_t h = 0;
  for (int i = threadIdx.x; i < nv; i += kBlock)
    if (pr[i]) h += mix64(uint64_t(i));
  for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = h;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (int w = 0; w < kBlock / 64; ++w) t += part[w];
    hash[blockIdx.x] = t ? t : 1;
  }
}

// thread per row: open-addressing insert, each slot keeps the smallest row
// index with its hash
__global__ void __launch_bounds__(kBlock) pattern_insert(const uint64_t *__restrict__ hash,
                                                         uint32_t batch, unsigned long long *keys,
                                                         uint32_t *vals, uint32_t cap) {
  const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= batch) return;
  const uint64_t h = hash[b];
  for (uint32_t slot = uint32_t(h % cap), probe = 0; probe < cap; ++probe, slot = (slot + 1) % cap) {
    const unsigned long long prev = atomicCAS(&keys[slot], 0ull, (unsigned long long)h);
    if (prev == 0ull || prev == h) {
      atomicMin(&vals[slot], b);
      return;
    }
  }
}

// block per row: pattern[b] = the leader (smallest index) of b's hash if its
// flags are identical to b's, else b itself (a hash collision: b keeps its own)
__global__ void __launch_bounds__(kBlock) pattern_resolve(const uint8_t *__restrict__ present, int nv,
                                                          int n, const uint64_t *__restrict__ hash,
                                                          const unsigned long long *__restrict__ keys,
                                                          const uint32_t *__restrict__ vals,
                                                          uint32_t cap, uint32_t *__restrict__ pattern) {
  __shared__ uint32_t leader;
  __shared__ int differ;
  const uint32_t b = blockIdx.x;
  if (threadIdx.x == 0) {
    const uint64_t h = hash[b];
    uint32_t slot = uint32_t(h % cap);
    for (uint32_t probe = 0; probe < cap && keys[slot] != h; ++probe) slot = (slot + 1) % cap;
    leader = keys[slot] == h ? vals[slot] : b;
    differ = 0;
  }
  __syncthreads();
  const uint32_t l = leader;
  if (l != b) {
    const uint8_t *pb = present + uint64_t(b) * n, *pl = present + uint64_t(l) * n;
    for (int i = threadIdx.x; i < nv; i += kBlock)
      if ((pb[i] != 0) != (pl[i] != 0)) differ = 1;
    __syncthreads();
  }
  if (threadIdx.x == 0) pattern[b] = (l != b && !differ) ? l : b;
}

// block per row: a follower's locator row = its leader's
__global__ void __launch_bounds__(kBlock) pattern_broadcast(const uint32_t *__restrict__ pattern, int n,
                                                            uint16_t *__restrict__ elog) {
  const uint32_t b = blockIdx.x, l = pattern[b];
  if (l == b) return;
  const uint16_t *src = elog + uint64_t(l) * n;
  uint16_t *dst = elog + uint64_t(b) * n;
  for (int i = threadIdx.x; i < n; i += kBlock) dst[i] = src[i];
}

// reed-solomon.hpp:83-134 + poly_encoder.hpp:118-215 for 4*G shard positions
__global__ void __launch_bounds__(kBlock) reconstruct_g(
    const uint8_t *__restrict__ shards, uint64_t slen, uint64_t sstride,
    const uint8_t *__restrict__ present, const uint16_t *__restrict__ elog,
    uint8_t *__restrict__ out, uint64_t ostride, int nv, int logn, int logk, int logG,
    uint32_t batch, const uint32_t *__restrict__ pattern, DevTables t, uint2 *scratch) {
  const UniformRecG geo{slen, sstride, ostride};
#include "dec_g_body.inc"
}

__global__ void __launch_bounds__(kBlock) reconstruct_g_ragged(
    const uint8_t *__restrict__ shards, const RaggedItem *__restrict__ items,
    const uint32_t *__restrict__ tile_first, const uint8_t *__restrict__ present,
    const uint16_t *__restrict__ elog, uint8_t *__restrict__ out, int nv, int logn, int logk, int logG,
    uint32_t batch, const uint32_t *__restrict__ pattern, DevTables t, uint2 *scratch) {
  const RaggedRecG geo{items, tile_first};
#include "dec_g_body.inc"
}

// reed-solomon.hpp:143-179: out[2(i*k + y) ..] = shard_y[2i ..]
__global__ void __launch_bounds__(kBlock) systematic_g(const uint8_t *__restrict__ shards,
                                                       uint64_t slen, uint64_t sstride, int nv,
                                                       int logk, uint8_t *__restrict__ out,
                                                       uint64_t ostride, uint32_t batch,
                                                       uint32_t *sig_flag, uint32_t sig_v) {
  const int k = 1 << logk;
  const uint64_t npos = slen / 2;
  const uint64_t total = npos * k;
  for (uint32_t b = blockIdx.y; b < batch; b += gridDim.y) {
    const uint8_t *SH = shards + uint64_t(b) * nv * sstride;
    uint8_t *O = out + uint64_t(b) * ostride;
    for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total;
         e += uint64_t(gridDim.x) * blockDim.x) {
      const uint64_t i = e >> logk;
      const int y = int(e & (k - 1));
      O[2 * e] = SH[uint64_t(y) * sstride + 2 * i];
      O[2 * e + 1] = SH[uint64_t(y) * sstride + 2 * i + 1];
    }
  }
  signal_end(sig_flag, sig_v);  // (single-workgroup launches only)
}

// the ragged form (k < 16): blockIdx.y over the items, an item without tiles in
// the plan's prefix (one that broke the contract) skipped whole
__global__ void __launch_bounds__(kBlock) systematic_g_ragged(const uint8_t *__restrict__ shards,
                                                              const RaggedItem *__restrict__ items,
                                                              const uint32_t *__restrict__ tile_first, int logk,
                                                              uint8_t *__restrict__ out, uint32_t batch) {
  const int k = 1 << logk;
  for (uint32_t b = blockIdx.y; b < batch; b += gridDim.y) {
    if (tile_first[b + 1] == tile_first[b]) continue;
    const RaggedItem it = items[b];
    const uint8_t *SH = shards + it.shard_off;
    uint8_t *O = out + it.payload_off;
    const uint64_t total = it.shard_len / 2 * k;
    for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total;
         e += uint64_t(gridDim.x) * blockDim.x) {
      const uint64_t i = e >> logk;
      const int y = int(e & (k - 1));
      O[2 * e] = SH[uint64_t(y) * it.shard_stride + 2 * i];
      O[2 * e + 1] = SH[uint64_t(y) * it.shard_stride + 2 * i + 1];
    }
  }
}

// completion signal of a per-call C-ABI call: after the call's work on the
// stream, one lane stores `v` to a pinned host word at system scope; the host
// spins on it (a host spin on a kernel-written flag is ~5 us faster per round
// trip than hipStreamSynchronize: scripts/micro/launch_lat.hip)
__global__ void signal_host(uint32_t *flag, uint32_t v) {
  __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int ilog2(uint32_t v) { return 31 - __builtin_clz(v); }

// payload slots in gridDim.y (hardware limit 65535); the kernels loop over the rest
size_t grid_y(size_t batch) { return batch < 65535 ? batch : 65535; }

int groups_for(uint32_t size) {  // byte-planar groups per workgroup
  if (size >= kLdsSlots) return 1;
  uint32_t g = kLdsSlots / size;
  return int(g > 64 ? 64 : g);
}

// Launch geometry of the generic kernels (uniform and ragged, encode and
// reconstruct) for a transform of `size` points over `positions` pieces /
// shard positions per payload: G groups per workgroup, a tile of 4 G
// positions per block of grid.x, the two transform buffers in LDS (shm bytes)
// or, above kLdsSlots points, in global scratch.
struct GenericGeo {
  int G;
  size_t tiles;
  bool lds;
  size_t shm;
};
GenericGeo generic_geo(uint32_t size, size_t positions) {
  const int G = groups_for(size);
  const bool lds = size <= uint32_t(kLdsSlots);
  return {G, (positions + 4 * G - 1) / (4 * G), lds, lds ? 2 * size_t(size) * G * sizeof(uint2) : 0};
}

// blocks of systematic_g / systematic_g_ragged over the columns of the
// (longest) item: grid-stride loops beyond 4096 blocks
unsigned systematic_g_blocks(const CodeParams &p, size_t slen) {
  const size_t blocks = (slen / 2 * p.k + kBlock - 1) / kBlock;
  return unsigned(blocks > 4096 ? 4096 : blocks);
}

}  // namespace

// The generic kernels' scratch: one pair of transform buffers per block of the
// launch.  Needed only where size > kLdsSlots, and there groups_for is 1, so
// the launch's tiles, (positions + 4 G - 1) / (4 G), are the (positions + 3) / 4
// a size query has always answered with.
size_t generic_scratch_bytes(uint32_t size, size_t positions, size_t batch) {
  const GenericGeo g = generic_geo(size, positions);
  return g.lds ? 0 : g.tiles * grid_y(batch) * 2 * size_t(size) * sizeof(uint2);
}

bool locator_wave_applicable(uint32_t n) { return n >= 64 && n <= 4096; }

// zeroes a dynamic schedule's tile counters in stream order.  A kernel, not
// hipMemsetAsync: a memset captured into a hipGraph did not re-zero the
// counters on replay here (the reconstruct of the second replay found its
// queue drained: tests/test_gpu_parity.py test_graph_capture_ws at nv 4096)
__global__ void zero_words(uint32_t *p, uint32_t n) {
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0;
}

hipError_t launch_zero_counters(uint32_t *p, size_t bytes, hipStream_t s) {
  hipLaunchKernelGGL(zero_words, dim3(1), dim3(64), 0, s, p, uint32_t(bytes / 4));
  return hipGetLastError();
}

hipError_t launch_signal_host(uint32_t *h_flag, uint32_t v, hipStream_t s) {
  hipLaunchKernelGGL(signal_host, dim3(1), dim3(1), 0, s, h_flag, v);
  return hipGetLastError();
}

// Encode scratch that is only a tile counter (the k = 16 .. 1024 fast
// kernels): optional, the kernels fall back to a static schedule without it.
bool encode_scratch_optional(const CodeParams &p) {
  return k1024_applicable(p) || k256_applicable(p) || k512w_applicable(p) || kw_applicable(p);
}

size_t encode_scratch_bytes(const CodeParams &p, size_t plen, size_t batch) {
  return encode_scratch_optional(p) ? kTileCounterBytes : generic_scratch_bytes(p.k, shard_len(p.k, plen) / 2, batch);
}

const char *kernel_name(Kernel k) {
  switch (k) {
#define ECAMD_NAME(X) \
  case Kernel::X: return #X;
    ECAMD_NAME(encode_k256w) ECAMD_NAME(encode_k256_packed) ECAMD_NAME(encode_kw)
    ECAMD_NAME(encode_k512w) ECAMD_NAME(encode_k1024) ECAMD_NAME(encode_g)
    ECAMD_NAME(encode_k256w_missing) ECAMD_NAME(encode_g_missing)
    ECAMD_NAME(reconstruct_n1024x) ECAMD_NAME(reconstruct_n1024) ECAMD_NAME(reconstruct_n1024_packed)
    ECAMD_NAME(reconstruct_n4096) ECAMD_NAME(reconstruct_gen) ECAMD_NAME(reconstruct_g)
    ECAMD_NAME(systematic_w) ECAMD_NAME(systematic_g)
#undef ECAMD_NAME
    case Kernel::invalid: break;
  }
  return nullptr;
}

// The fast kernels read payload rows with 16-B loads and write shard rows with
// 8-B stores (a single payload's pitch is never applied).  k = 256 has a
// packed form for what they cannot take: payloads under one tile of pieces,
// any payload base and pitch, any even shard base and pitch, while its
// flattened piece space (pieces rounded up to 8, per payload) stays below
// 2^32; past that, or with an odd shard base or pitch, the shape goes on to
// the kernels below.
Kernel choose_encode(const CodeParams &p, const EncodeCall &c) {
  if (c.batch == 0 || c.plen == 0) return Kernel::invalid;
  const bool aligned = addr(c.payloads) % 16 == 0 && addr(c.shards) % 8 == 0 &&
                       (c.batch == 1 || c.pstride % 16 == 0) && c.sstride % 8 == 0;
  if (k256_applicable(p)) {
    const size_t npp = (c.plen + 2 * 256 - 1) / (2 * 256);  // pieces per payload
    if (aligned && npp >= kK256Tile) return p.n == 1024 ? Kernel::encode_k256w : Kernel::encode_kw;
    const size_t npp8 = (npp + 7) / 8 * 8;  // (>= npp: also bounds the exactly flattened space of PK = 2)
    if (addr(c.shards) % 2 == 0 && c.sstride % 2 == 0 && npp8 * c.batch + kK256Tile < (size_t(1) << 32))
      return Kernel::encode_k256_packed;
  }
  if (aligned && k512w_applicable(p)) return Kernel::encode_k512w;
  if (aligned && kw_applicable(p)) return Kernel::encode_kw;
  if (aligned && k1024_applicable(p)) return Kernel::encode_k1024;
  return Kernel::encode_g;
}

hipError_t launch_encode(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                         hipStream_t s, HostSig *sig) {
  switch (choose_encode(p, c)) {
    case Kernel::encode_k256w: return launch_encode_k256w(p, t, c, scratch, s);
    case Kernel::encode_k256_packed: return launch_encode_k256(p, t, c, scratch, s);
    case Kernel::encode_kw: return launch_encode_kw(p, t, c, scratch, s);
    case Kernel::encode_k512w: return launch_encode_k512w(p, t, c, scratch, s);
    case Kernel::encode_k1024: return launch_encode_k1024(p, t, c, scratch, s);
    case Kernel::encode_g: break;
    default: return hipSuccess;  // an empty call
  }
  const size_t sl = shard_len(p.k, c.plen);
  const GenericGeo g = generic_geo(p.k, sl / 2);
  dim3 grid((unsigned)g.tiles, (unsigned)grid_y(c.batch));
  const bool fuse = sig && sig->flag && grid.x * grid.y == 1;
  if (fuse) sig->fused = true;
  hipLaunchKernelGGL(encode_g, grid, dim3(kBlock), g.shm, s, c.payloads, uint64_t(c.plen),
                     uint64_t(c.pstride), c.shards, uint64_t(sl), uint64_t(c.sstride), int(p.nv),
                     ilog2(p.n), ilog2(p.k), ilog2(uint32_t(g.G)), uint32_t(c.batch), t,
                     g.lds ? nullptr : static_cast<uint2 *>(scratch), fuse ? sig->flag : nullptr,
                     fuse ? sig->v : 0u);
  return hipGetLastError();
}

// The masked encode's kernel follows the plain encode's choice for the same
// buffers: the masked two-workgroup kernel where that is encode_k256w, the
// masked generic kernel (any base, any pitch) everywhere else.
Kernel choose_encode_missing(const CodeParams &p, const MissingCall &c) {
  switch (choose_encode(p, c.enc)) {
    case Kernel::invalid: return Kernel::invalid;
    case Kernel::encode_k256w: return Kernel::encode_k256w_missing;
    default: return Kernel::encode_g_missing;
  }
}

size_t encode_missing_scratch_bytes(const CodeParams &p, size_t plen, size_t batch) {
  const size_t plan = k256_applicable(p) && p.n == 1024 ? row_mask_plan_bytes(batch) : 0;
  const size_t g = generic_scratch_bytes(p.k, shard_len(p.k, plen) / 2, batch);
  return kTileCounterBytes + (plan > g ? plan : g);
}

hipError_t launch_encode_missing(const CodeParams &p, const DevTables &t, const MissingCall &c, void *scratch,
                                 hipStream_t s) {
  switch (choose_encode_missing(p, c)) {
    case Kernel::encode_k256w_missing: return launch_encode_k256w_missing(p, t, c, scratch, s);
    case Kernel::encode_g_missing: break;
    default: return hipSuccess;  // an empty call
  }
  if (!scratch || !c.present) return hipErrorInvalidValue;
  const EncodeCall &ec = c.enc;
  const size_t sl = shard_len(p.k, ec.plen);
  const GenericGeo g = generic_geo(p.k, sl / 2);
  uint2 *bufs = reinterpret_cast<uint2 *>(static_cast<uint8_t *>(scratch) + kTileCounterBytes);
  hipLaunchKernelGGL(encode_g_missing, dim3((unsigned)g.tiles, (unsigned)grid_y(ec.batch)), dim3(kBlock), g.shm, s,
                     ec.payloads, uint64_t(ec.plen), uint64_t(ec.pstride), ec.shards, uint64_t(sl),
                     uint64_t(ec.sstride), int(p.nv), ilog2(p.n), ilog2(p.k), ilog2(uint32_t(g.G)),
                     uint32_t(ec.batch), t, g.lds ? nullptr : bufs, c.present, c.pattern);
  return hipGetLastError();
}

namespace {
size_t dedup_cap(size_t batch) {  // hash slots: a power of two >= 2 * batch (batch < 2^31)
  size_t c = 64;
  while (c < 2 * batch) c <<= 1;
  return c;
}
}  // namespace

size_t dedup_scratch_bytes(size_t batch) {
  const size_t cap = dedup_cap(batch);
  return batch * 8 + cap * 8 + cap * 4;  // hashes, keys, values
}

hipError_t launch_dedup_patterns(const CodeParams &p, const uint8_t *d_present, size_t batch,
                                 uint32_t *d_pattern, void *scratch, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (!scratch || batch >= (size_t(1) << 31)) return hipErrorInvalidValue;
  const uint32_t cap = uint32_t(dedup_cap(batch));
  uint64_t *hash = static_cast<uint64_t *>(scratch);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(hash + batch);
  uint32_t *vals = reinterpret_cast<uint32_t *>(keys + cap);
  if (const hipError_t e = hipMemsetAsync(keys, 0, size_t(cap) * 8, s); e != hipSuccess) return e;
  if (const hipError_t e = hipMemsetAsync(vals, 0xff, size_t(cap) * 4, s); e != hipSuccess) return e;
  hipLaunchKernelGGL(pattern_hash, dim3(unsigned(batch)), dim3(kBlock), 0, s, d_present, int(p.nv),
                     int(p.n), hash);
  hipLaunchKernelGGL(pattern_insert, dim3(unsigned((batch + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     hash, uint32_t(batch), keys, vals, cap);
  hipLaunchKernelGGL(pattern_resolve, dim3(unsigned(batch)), dim3(kBlock), 0, s, d_present,
                     int(p.nv), int(p.n), hash, keys, vals, cap, d_pattern);
  return hipGetLastError();
}

hipError_t launch_error_locator(const CodeParams &p, const uint8_t *d_present, size_t batch,
                                const uint16_t *d_fold, const uint32_t *d_pattern,
                                uint16_t *d_err_log, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (locator_wave_applicable(p.n)) {
    const dim3 grid(unsigned((batch + 3) / 4));
#define ECAMD_LOC_W(VV)                                                                          \
  case VV:                                                                                       \
    hipLaunchKernelGGL(error_locator_w<VV>, grid, dim3(256), 0, s, d_present, int(p.nv),         \
                       uint32_t(batch), d_fold, d_pattern, d_err_log);                           \
    break;
    switch (p.n / 64) {
      ECAMD_LOC_W(1) ECAMD_LOC_W(2) ECAMD_LOC_W(4) ECAMD_LOC_W(8) ECAMD_LOC_W(16) ECAMD_LOC_W(32)
      ECAMD_LOC_W(64)
      default: return hipErrorInvalidValue;
    }
#undef ECAMD_LOC_W
    return hipGetLastError();
  }
  const size_t shm = size_t(p.n) * sizeof(uint16_t);
  int cus = 0;
  if (const hipError_t e = prepare_kernel(reinterpret_cast<const void *>(&error_locator_g), 65536 * 2, &cus);
      e != hipSuccess)
    return e;
  hipLaunchKernelGGL(error_locator_g, dim3(unsigned(batch)), dim3(kBlock), shm, s, d_present,
                     int(p.nv), ilog2(p.n), d_fold, d_pattern, d_err_log,
                     static_cast<uint16_t *>(nullptr));
  return hipGetLastError();
}

hipError_t launch_broadcast_locators(const CodeParams &p, const uint32_t *d_pattern, size_t batch,
                                     uint16_t *d_err_log, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  hipLaunchKernelGGL(pattern_broadcast, dim3(unsigned(batch)), dim3(kBlock), 0, s, d_pattern,
                     int(p.n), d_err_log);
  return hipGetLastError();
}

size_t reconstruct_scratch_bytes(const CodeParams &p, size_t slen, size_t batch) {
  if (n4096_applicable(p)) return n4096_scratch_bytes(p, batch);
  if (n1024_applicable(p)) return n1024_scratch_bytes(p, batch);
  if (decgen_applicable(p)) return gather_order_bytes(p, batch);
  return generic_scratch_bytes(p.n, slen / 2, batch);
}

const ReconOverrides &recon_overrides() {
  static const ReconOverrides o = [] {
    const char *w = std::getenv("ECCR_AMD_RECON_WAVES"), *k = std::getenv("ECCR_AMD_RECON_PACKED");
    ReconOverrides r;
    r.waves8 = w && w[0] == '8';
    r.waves12 = w && w[0] == '1' && w[1] == '2';
    r.force_packed = k && k[0] == '1';
    return r;
  }();
  return o;
}

// The fast kernels read shard rows with 16-B loads.  The n = 1024 kernels
// write out rows with 8-B stores and read a pattern's flag and locator rows
// with vector loads (out8); reconstruct_n4096 and reconstruct_gen write with
// 16-B stores (out16) and read those rows element-wise.  n = 1024 has a packed
// form for payloads under one tile of columns and for any even shard base and
// pitch, while its flattened column space (columns rounded up to 4, per
// payload) stays below 2^32: past that it launches nothing.
Kernel choose_reconstruct(const CodeParams &p, const ReconCall &c, const ReconOverrides &o) {
  const size_t slen = c.slen, sstride = c.sstride, batch = c.batch, ostride = c.ostride;
  const uintptr_t shards = addr(c.shards), present = addr(c.present), err_log = addr(c.err_log), out = addr(c.out);
  if (batch == 0 || slen < 2) return Kernel::invalid;
  const bool aligned = shards % 16 == 0 && out % 8 == 0 && sstride % 16 == 0 &&
                       (batch == 1 || ostride % 8 == 0);
  const bool out8 = out % 8 == 0 && (batch == 1 || ostride % 8 == 0) && present % 16 == 0 &&
                    err_log % 16 == 0;
  const bool out16 = out % 16 == 0 && (batch == 1 || ostride % 16 == 0);
  const size_t ncols = slen / 2;
  if (n1024_applicable(p)) {
    const bool packed = ncols < kN1024Cols || shards % 16 != 0 || sstride % 16 != 0;
    if (!packed && aligned && out8 && !o.waves8 && ncols >= kN1024xMinCols) return Kernel::reconstruct_n1024x;
    if (packed ? out8 && shards % 2 == 0 && sstride % 2 == 0 : aligned && out8) {
      if (!packed && !o.force_packed) return Kernel::reconstruct_n1024;
      const size_t ncols4 = (ncols + 3) / 4 * 4;
      return ncols4 * batch + kN1024Cols < (size_t(1) << 32) ? Kernel::reconstruct_n1024_packed
                                                             : Kernel::invalid;
    }
  }
  if (aligned && out16 && n4096_applicable(p)) return Kernel::reconstruct_n4096;
  if (aligned && out16 && decgen_applicable(p)) return Kernel::reconstruct_gen;
  return Kernel::reconstruct_g;
}

hipError_t launch_reconstruct(const CodeParams &p, const DevTables &t, const ReconCall &c, void *scratch,
                              hipStream_t s) {
  const Kernel kern = choose_reconstruct(p, c, recon_overrides());
  switch (kern) {
    case Kernel::reconstruct_n1024x: return launch_reconstruct_n1024x(p, t, c, scratch, s);
    case Kernel::reconstruct_n1024:
    case Kernel::reconstruct_n1024_packed:
      return launch_reconstruct_n1024(p, t, kern == Kernel::reconstruct_n1024_packed, c, scratch, s);
    case Kernel::reconstruct_n4096: return launch_reconstruct_n4096(p, t, c, scratch, s);
    case Kernel::reconstruct_gen: return launch_reconstruct_gen(p, t, c, scratch, s);
    case Kernel::reconstruct_g: break;
    default:  // an empty call, or the packed form past its 2^32 flattened columns
      return c.batch == 0 || c.slen < 2 ? hipSuccess : hipErrorInvalidValue;
  }
  const GenericGeo g = generic_geo(p.n, c.slen / 2);
  dim3 grid((unsigned)g.tiles, (unsigned)grid_y(c.batch));
  hipLaunchKernelGGL(reconstruct_g, grid, dim3(kBlock), g.shm, s, c.shards, uint64_t(c.slen),
                     uint64_t(c.sstride), c.present, c.err_log, c.out, uint64_t(c.ostride), int(p.nv),
                     ilog2(p.n), ilog2(p.k), ilog2(uint32_t(g.G)), uint32_t(c.batch), c.pattern, t,
                     g.lds ? nullptr : static_cast<uint2 *>(scratch));
  return hipGetLastError();
}

// systematic_w reads rows with 16-B loads and writes the output with 16-B
// stores (a single payload's out pitch is never applied); k < 16 has output
// runs under 32 B per column, which stay with the element-wise kernel.  A
// per-call launch small enough for ONE systematic_g workgroup keeps it: that
// workgroup stores the completion signal itself (HostSig), which a separate
// signal kernel after systematic_w would not match in latency.
Kernel choose_systematic(const CodeParams &p, const SysCall &c, bool host_signal) {
  if (c.batch == 0 || c.slen < 2) return Kernel::invalid;
  if (host_signal && c.batch == 1 && c.slen / 2 * p.k <= size_t(kBlock)) return Kernel::systematic_g;
  const bool aligned = addr(c.shards) % 16 == 0 && c.sstride % 16 == 0 && addr(c.out) % 16 == 0 &&
                       (c.batch == 1 || c.ostride % 16 == 0);
  return p.k >= 16 && aligned ? Kernel::systematic_w : Kernel::systematic_g;
}

size_t systematic_scratch_bytes(const CodeParams &p) { return p.k >= 16 ? kTileCounterBytes : 0; }

hipError_t launch_systematic(const CodeParams &p, const SysCall &c, void *scratch, hipStream_t s, HostSig *sig) {
  switch (choose_systematic(p, c, sig && sig->flag)) {
    case Kernel::systematic_w: return launch_systematic_w(p, c, scratch, s);
    case Kernel::systematic_g: break;
    default: return hipSuccess;  // an empty call
  }
  const unsigned blocks = systematic_g_blocks(p, c.slen);
  const bool fuse = sig && sig->flag && blocks * grid_y(c.batch) == 1;
  if (fuse) sig->fused = true;
  hipLaunchKernelGGL(systematic_g, dim3(blocks, unsigned(grid_y(c.batch))), dim3(kBlock), 0, s, c.shards,
                     uint64_t(c.slen), uint64_t(c.sstride), int(p.nv), ilog2(p.k), c.out, uint64_t(c.ostride),
                     uint32_t(c.batch), fuse ? sig->flag : nullptr, fuse ? sig->v : 0u);
  return hipGetLastError();
}

// ---- ragged forms of the generic kernels (ragged.hpp): the correctness path
// of the ragged calls for every n_validators without a specialised ragged
// kernel.  Tile = the block's 4 G pieces / positions; grid.x = the tiles of
// the longest item the call allows; scratch (FFTs that do not fit LDS) one
// buffer per block as in the uniform launch, sized from that maximum.
uint32_t ragged_encode_tile(const CodeParams &p) {
  return choose_encode_ragged(p) == RaggedKernel::encode_k256w_ragged ? 64u : 4u * uint32_t(groups_for(p.k));
}
uint32_t ragged_reconstruct_tile(const CodeParams &p) {
  return choose_reconstruct_ragged(p) == RaggedKernel::reconstruct_n1024x_ragged ? 64u
                                                                                 : 4u * uint32_t(groups_for(p.n));
}

// columns per plan tile of the systematic ragged kernels: systematic_w's
// tile; below k = 16 (systematic_g_ragged only asks whether an item has tiles)
// the 4096 columns of one sweep of its grid
uint32_t ragged_systematic_tile(const CodeParams &p) {
  return choose_systematic_ragged(p) == RaggedKernel::systematic_w_ragged ? systematic_w_cols(p) : 4096u;
}

hipError_t launch_systematic_g_ragged(const CodeParams &p, const RaggedCall &c, void *ws, hipStream_t s) {
  hipLaunchKernelGGL(systematic_g_ragged, dim3(systematic_g_blocks(p, c.max_len), unsigned(grid_y(c.batch))),
                     dim3(kBlock), 0, s, c.in, c.items, ragged_first(ws), ilog2(p.k), c.out, uint32_t(c.batch));
  return hipGetLastError();
}

namespace {
uint2 *ragged_g_scratch(const GenericGeo &g, size_t batch, void *ws) {
  return g.lds ? nullptr : reinterpret_cast<uint2 *>(static_cast<uint8_t *>(ws) + ragged_scratch_offset(batch));
}
}  // namespace

hipError_t launch_encode_g_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                  hipStream_t s) {
  const GenericGeo g = generic_geo(p.k, shard_len(p.k, c.max_len) / 2);
  hipLaunchKernelGGL(encode_g_ragged, dim3(unsigned(g.tiles), unsigned(grid_y(c.batch))), dim3(kBlock), g.shm, s,
                     c.in, c.items, ragged_first(ws), c.out, int(p.nv), ilog2(p.n), ilog2(p.k),
                     ilog2(uint32_t(g.G)), uint32_t(c.batch), t, ragged_g_scratch(g, c.batch, ws));
  return hipGetLastError();
}

hipError_t launch_reconstruct_g_ragged(const CodeParams &p, const DevTables &t, const RaggedCall &c, void *ws,
                                       hipStream_t s) {
  const GenericGeo g = generic_geo(p.n, c.max_len / 2);
  hipLaunchKernelGGL(reconstruct_g_ragged, dim3(unsigned(g.tiles), unsigned(grid_y(c.batch))), dim3(kBlock), g.shm, s,
                     c.in, c.items, ragged_first(ws), c.present, c.err_log, c.out, int(p.nv), ilog2(p.n),
                     ilog2(p.k), ilog2(uint32_t(g.G)), uint32_t(c.batch), c.pattern, t,
                     ragged_g_scratch(g, c.batch, ws));
  return hipGetLastError();
}

}  // namespace ecamd
