// enc_k256_common.hpp — pieces shared by the k = 256 encode kernels
// (enc_k256.hip: the packed kernel, n = 1024 and n = 2048) and, through
// enc_w_common.hpp, by the two-workgroups-per-CU kernels, whose layouts are
// the k = 256 ones (enc_k256w.hip, enc_kw.hip, enc_k512w.hip).  One
// byte-planar group of 4 pieces per instance (lanes 0-31 / 32-63), 8 positions
// of the 256-point transforms per lane in registers, wave-private LDS
// exchanges between the radix-8 passes.
#pragma once

#include <hip/hip_runtime.h>

#include "ec_device.hpp"

namespace ecamd {
namespace {

struct State {
  uint32_t l[8], h[8];  // [register]: low / high byte planes
};

__device__ __forceinline__ void mul_any(uint32_t xl, uint32_t xh, const Tab &T, uint32_t &yl, uint32_t &yh) {
  mul_acc(xl, xh, T, yl, yh);
}
__device__ __forceinline__ void mul_any(uint32_t xl, uint32_t xh, const SubTab &T, uint32_t &yl,
                                        uint32_t &yh) {
  mul_acc_sub(xl, xh, T, yl, yh);
}
__device__ __forceinline__ void mul_any(uint32_t xl, uint32_t xh, const F9Tab &T, uint32_t &yl,
                                        uint32_t &yh) {
  mul_acc_f9(xl, xh, T, yl, yh);
}

template <typename T>
__device__ __forceinline__ void ibfly(State &s, int ra, int rb, const T &Tb) {
  s.l[rb] ^= s.l[ra];
  s.h[rb] ^= s.h[ra];
  mul_any(s.l[rb], s.h[rb], Tb, s.l[ra], s.h[ra]);
}

template <typename T>
__device__ __forceinline__ void fbfly(State &s, int ra, int rb, const T &Tb) {
  mul_any(s.l[rb], s.h[rb], Tb, s.l[ra], s.h[ra]);
  s.l[rb] ^= s.l[ra];
  s.h[rb] ^= s.h[ra];
}

__device__ __forceinline__ void bxor(State &s, int ra, int rb) {  // b ^= a (no multiply)
  s.l[rb] ^= s.l[ra];
  s.h[rb] ^= s.h[ra];
}

// stage-7 butterfly reading the IFFT coefficients c and writing s (stage 7
// touches every register, so the coset needs no copy of c)
template <typename T>
__device__ __forceinline__ void fbfly_from(State &s, const State &c, int ra, int rb, const T &Tb) {
  s.l[ra] = c.l[ra];
  s.h[ra] = c.h[ra];
  mul_any(c.l[rb], c.h[rb], Tb, s.l[ra], s.h[ra]);
  s.l[rb] = c.l[rb] ^ s.l[ra];
  s.h[rb] = c.h[rb] ^ s.h[ra];
}

// position held in register r by lane q (0..31) in each layout
__device__ __forceinline__ uint32_t posA(uint32_t q, int r) { return (q << 3) | uint32_t(r); }
__device__ __forceinline__ uint32_t posB(uint32_t q, int r) {
  return ((q >> 3) << 6) | (uint32_t(r) << 3) | (q & 7);
}
// ---- wave-private exchange -------------------------------------------------
// 8-byte cell u = pos*2 + inst mapped by a GF(2)-linear bijection M
// (found by search, scripts/search_swizzle.py) under which every layout's
// reads (32-lane groups) and writes (16-lane groups) are bank-conflict free.
// u = lane part XOR register part, so addr = M(lane part) ^ M(r part).
constexpr uint32_t kM[9] = {0b110011100, 0b1001101, 0b111110100, 0b110001111, 0b11110011,
                            0b101101010, 0b110000111, 0b111011000, 0b111100000};
__host__ __device__ constexpr uint32_t mswz(uint32_t u) {
  uint32_t a = 0;
  for (int i = 0; i < 9; ++i) a |= uint32_t(__builtin_popcount(kM[i] & u) & 1) << i;
  return a << 3;
}
// lane part / register part of u for each layout
__device__ __forceinline__ uint32_t ulaneA(uint32_t q, uint32_t inst) { return (q << 4) | inst; }
__device__ __forceinline__ uint32_t ulaneB(uint32_t q, uint32_t inst) {
  return ((q >> 3) << 7) | ((q & 7) << 1) | inst;
}
__device__ __forceinline__ uint32_t ulaneC(uint32_t q, uint32_t inst) { return (q << 1) | inst; }
__host__ __device__ constexpr uint32_t uregA(int r) { return uint32_t(r) << 1; }
__host__ __device__ constexpr uint32_t uregB(int r) { return uint32_t(r) << 4; }
__host__ __device__ constexpr uint32_t uregC(int r) {
  return (uint32_t(r & 3) << 7) | (uint32_t(r >> 2) << 6);
}

enum Layout { LA, LB, LC };

struct XBase {  // per-lane exchange base addresses
  uint32_t a, b, c;
};

template <Layout L>
__device__ __forceinline__ uint32_t xcell(const XBase &xb, int r) {
  if constexpr (L == LA) return xb.a ^ mswz(uregA(r));
  else if constexpr (L == LB) return xb.b ^ mswz(uregB(r));
  else return xb.c ^ mswz(uregC(r));
}

template <Layout FROM, Layout TO>
__device__ __forceinline__ void exchange(State &s, uint8_t *xch, const XBase &xb) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
    *reinterpret_cast<uint2 *>(xch + xcell<FROM>(xb, r)) = make_uint2(s.l[r], s.h[r]);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint2 v = *reinterpret_cast<const uint2 *>(xch + xcell<TO>(xb, r));
    s.l[r] = v.x;
    s.h[r] = v.y;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// 16 payload bytes at any address, zero past `avail` (bytes valid from p):
// aligned dwords that each hold at least one wanted byte (so nothing outside
// the payload's allocation is touched), funnel-shifted by v_alignbyte
__device__ __forceinline__ uint4 load16_any(const uint8_t *p, uint64_t avail) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (avail >= 16 && (a & 15) == 0) return *reinterpret_cast<const uint4 *>(p);
  if (avail == 0) return make_uint4(0, 0, 0, 0);
  const uint32_t sh = uint32_t(a & 3), nb = avail < 16 ? uint32_t(avail) : 16u;
  const uint32_t *q = reinterpret_cast<const uint32_t *>(a & ~uintptr_t(3));
  uint32_t d[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) d[i] = uint32_t(4 * i) < sh + nb ? q[i] : 0u;
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
    const uint32_t have = nb > uint32_t(4 * j) ? nb - uint32_t(4 * j) : 0u;  // valid bytes of word j
    if (have < 4) w[j] &= (1u << (8 * have)) - 1u;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace
}  // namespace ecamd
