// dec_n1024_common.hpp — the n = 1024, k = 256 reconstruct's shared pieces.
// Users: dec_n1024.hip (reconstruct_n1024: the 8-wave kernel and its packed
// form) and, through dec_n1024x_body.hpp, dec_n1024x.hip (reconstruct_n1024x:
// the 12- and 16-wave kernels) and dec_n1024x_ragged.hip (its ragged form).
// The transform primitives (positions, the region swizzle, linear table
// addressing, butterflies, cross-lane helpers) are tf1024.hpp's, taken by
// name; what is declared here is the n = 1024 kernels' own: table addressing
// by skew slot at LDS address 0, the unaligned row load, the issue-priority
// turns.
#pragma once

#include <hip/hip_runtime.h>

#include "ec_device.hpp"
#include "ec_kernels.hpp"
#include "tf1024.hpp"

namespace ecamd {
namespace n1024 {

constexpr int N = 1024;
constexpr int K = 256;
using tf::bx;
using tf::from_upper;
using tf::ib;
using tf::ipass4;
using tf::raddr;
using tf::REG_BYTES;
using tf::S16;
using tf::skew_idx;
using tf::swap_bit;
using tf::Tabs;
using tf::tlin;

// skew index at stage 2 whose element equals the skew element of position
// pos_a at stage m (2 (pos_a >> (m + 1)), additive_fft.hpp:47-97 with the Cantor
// relabelling: skews[i] = log(((i + 1) >> ctz(i + 1)) - 1)): that element is
// < 256 iff the result is < 1024, and its image slot holds a subfield table
__device__ __forceinline__ uint32_t sub_alias(uint32_t pos_a, int m) {
  return ((pos_a >> (m + 1)) << 3) | 3u;
}

// The tables are the first thing in the kernel's LDS: a table is read at an
// absolute address (lds_tab_abs), not through a pointer.  Lds0 is what these
// kernels pass where tf1024.hpp's passes take the table image.
struct Lds0 {};
__device__ __forceinline__ void tab_at(Lds0, uint32_t lin, Tab &T) { lds_tab_abs<Tabs::kPlane>(lin, T); }
// the data runs in tower coordinates and the tables are tower
// image 0: stages >= tower_sub_min(0) = 2 hold subfield tables
__device__ __forceinline__ void tab_at(Lds0, uint32_t lin, SubTab &T) { lds_subtab_abs<Tabs::kPlane>(lin, T); }
constexpr int SUB = tower_sub_min(0);
// IFFT stage 1 with F9 tables (F9 image kind 0)
__device__ __forceinline__ void tab_at(Lds0, uint32_t lin, F9Tab &T) { lds_f9tab_abs<Tabs::kPlane>(lin, T); }

// 8 shard bytes at any even address, zero past `avail` (1..8 bytes valid
// from p): three dword loads, each clamped to the dword that holds the last
// wanted byte (so nothing past the row is touched), funnel-shifted by
// v_alignbyte; no branches
__device__ __forceinline__ uint2 load8_any(const uint8_t *p, uint32_t avail) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), a0 = a & ~uintptr_t(3);
  const uintptr_t last = (a + avail - 1) & ~uintptr_t(3);
  const uint32_t sh = uint32_t(a & 3);
  const uint32_t d0 = *reinterpret_cast<const uint32_t *>(a0);
  const uint32_t d1 = *reinterpret_cast<const uint32_t *>(a0 + 4 < last ? a0 + 4 : last);
  const uint32_t d2 = *reinterpret_cast<const uint32_t *>(a0 + 8 < last ? a0 + 8 : last);
  const uint64_t keep = avail >= 8 ? ~0ull : (1ull << (8 * avail)) - 1;
  return make_uint2(__builtin_amdgcn_alignbyte(d1, d0, sh) & uint32_t(keep),
                    __builtin_amdgcn_alignbyte(d2, d1, sh) & uint32_t(keep >> 32));
}

// The two waves of a SIMD (w, w + 4) take turns at the higher issue priority
// (pass A: w + 4, pass B: w, pass C to the FFT: w + 4, output and gather:
// equal), so
// neither runs far ahead and then idles at the tile barrier while the other
// finishes alone (the arbiter otherwise favours the older wave throughout).
// A/B at B = 2048: 7.06 -> 7.01 ms; one fixed priority for the whole
// transform 7.08, four turns 7.09.
__device__ __forceinline__ void prio_lead(bool lead) {
  if (lead) __builtin_amdgcn_s_setprio(2);
  else __builtin_amdgcn_s_setprio(0);
}

}  // namespace n1024
}  // namespace ecamd
