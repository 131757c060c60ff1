// enc_k512w.hip — encode for k = 512, n = 2048 / 4096 (n_validators 1534..3069:
// the shapes just above a power of two), two 8-wave workgroups per CU.
//
// encode_k256w's model (enc_k256w.hip; shared code and tile schedule: enc_w_common.hpp;
// DESIGN.md §5.1, §5.7) at k = 512: per piece (1024 payload bytes = 512
// symbols) IFFT_512 at index 0, then FFT_512 at each coset 512 j below
// n_validators (encodeLow, poly_encoder.hpp:217-240), radix-8 register passes
// in tower coordinates, wave-private LDS exchanges.  What differs:
//  * one byte-planar group of 4 pieces per wave, its 512 positions over the
//    64 lanes x 8 registers; the position bit 8 is lane bit 5 (encode_k256w's
//    instance bit), so layouts A / B / C and their exchanges are encode_k256w's.
//    Stages 6-8 run in layout C' = C with register bit 2 (p5) and lane bit 5
//    (p8) swapped by v_permlane32_swap, where all three are register bits and
//    every element is wave-uniform;
//  * multiply tables: the compact image's subfield and F9 entries (elements
//    x < 256, 12 KB, resident) and, per coset, an extension image of the
//    general tables its stages 0..2 need (x >= 256: 20-35 KB, ec_kernels.hpp
//    kEImg512*), brought in by LDS-DMA while the previous coset's rows are
//    stored (its stage-0 tables alone are 256 distinct elements per coset:
//    all cosets' would not fit beside the regions, twice per CU);
//  * the tile is 32 pieces (8 waves x 4), each shard row a 64-B segment,
//    stored as 16 B per lane from two adjacent waves' regions.
//
// LDS per workgroup (80 KB, two per CU): extension stage 0 [0, 20480), the
// compact image's F9 and subfield areas at their own offsets [20480, 32768)
// (cimg.hpp ctab reads them unchanged), extension stages 1, 2 [32768, 48128),
// the tile slot, 8 wave regions of 4 KB [49152, 81920).
#include "enc_w_common.hpp"

namespace ecamd {
namespace {

constexpr int K = 512;
constexpr int TILE = 4 * WAVES;                          // pieces per tile
constexpr uint32_t BASE_LO = kCImgF9;                    // compact image bytes [20480, 32768)
constexpr uint32_t EXT[3] = {0, kCImgBytes, kCImgBytes + 5 * 2048};  // extension stages 0, 1, 2
constexpr uint32_t SLOT = EXT[2] + 5 * 1024;             // the next tile's index
constexpr uint32_t XCH0 = 49152;                         // the wave regions (4 KB aligned: XOR addressing)
constexpr int LDS_BYTES = int(XCH0 + WAVES * XCH_BYTES);
static_assert(SLOT + 16 <= XCH0 && XCH0 % (2 * XCH_BYTES) == 0, "LDS map: region pairs XOR-addressed");
static_assert(EXT[0] + 5 * 4096 == BASE_LO && kEImg512Stage[1] == 20480 && kEImg512Stage[2] == 30720,
              "extension stage 0 ends where the compact image's F9 area starts");
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");

// extension image chunks (1 KB, one LDS-DMA wave-instruction each) coset j needs
__host__ __device__ constexpr uint32_t ext_chunks(uint32_t j) { return j == 1 ? 20 : j <= 3 ? 30 : 35; }

// Table kinds of a stage (enc_w_common.hpp ftab): the compact image's subfield
// / F9 entries (SubTab, F9Tab) or a general table of extension stage M (EG<M>)
template <int M>
struct EG : ExtKind {
  static constexpr uint32_t BASE = EXT[M], PLANE = 4096u >> M;
};

// IFFT stage-0 table of element x = 4 lane + rr < 256 (lane part lt =
// cimg_lin(4 lane)): subfield for lanes 0-31 (p8 = 0), F9 for lanes 32-63,
// both read as an F9 table (gf_field.cpp f9_tab: a subfield c0 is (c0, 0, c0,
// mask 0)); the subfield area's plane-1 slots hold (w4, 0, 0, 0)
__device__ __forceinline__ void mixtab(uint32_t lt, uint32_t r, bool hi, F9Tab &T) {
  const uint32_t a = lt ^ r ^ (hi ? cimg_lin(128) : 0u);  // entry 4 (lane & 31) + rr of either area
  const uint32_t p0 = a + (hi ? kCImgF9 : kCImgSub0), p1 = a + (hi ? kCImgF9 + kCImgF9Plane : kCImgSub1);
  const v4u v3 = lds_r128(a + kCImgF9 + 3 * kCImgF9Plane), v2 = lds_r128(a + kCImgF9 + 2 * kCImgF9Plane);
  const v4u v1 = lds_r128(p1), v0 = lds_r128(p0);
  T.t[0] = v0.x;
  T.t[1] = v0.y;
  T.t[2] = v0.z;
  T.t[3] = v0.w;
  T.t[4] = v1.x;
  T.t[5] = v1.y;
  T.t[6] = v1.z;
  T.t[7] = v1.w;
  T.t[8] = hi ? v2.x : 0u;
  T.t[9] = hi ? v2.y : 0u;
  T.t[10] = hi ? v2.z : v0.x;
  T.t[11] = hi ? v2.w : v0.y;
  T.t[12] = hi ? v3.x : v0.z;
  T.t[13] = hi ? v3.y : v0.w;
  T.t[14] = hi ? v3.z : v1.x;
  T.t[15] = hi ? v3.w : 0u;
}

// IFFT pass A (stages 0-2, index 0), base = 8 lane
__device__ __forceinline__ void ipassA(State &s, uint32_t base, bool hi) {
  const XLanes x = xlanes<0>(base);
  F9Tab Ta0, Tb0;
  SubTab Ta1, Tb1, Ta2;
  mixtab(x.l0, cimg_lin(0), hi, Ta0);
  mixtab(x.l0, cimg_lin(1), hi, Tb0);
  ibfly(s, 0, 1, Ta0);
  mixtab(x.l0, cimg_lin(2), hi, Ta0);
  ibfly(s, 2, 3, Tb0);
  mixtab(x.l0, cimg_lin(3), hi, Tb0);
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

// layout C' (register bit 0 = p6, bit 1 = p7, bit 2 = p8): IFFT stages 6-8 at
// index 0, elements x = pos >> (m + 1) uniform: stage 6 block rr (p7 + 2 p8)
// x = rr, stage 7 block p8 x = p8, stage 8 x = 0; x = 0 is b ^= a only (the
// skew 0xFFFF of additive_fft.hpp:110-112)
__device__ __forceinline__ void ipassC9(State &s) {
  SubTab T1, T2;
  ctab(0u, cimg_lin(1), T1);
  ctab(0u, cimg_lin(2), T2);
  bxor(s, 0, 1);
  ibfly(s, 2, 3, T1);
  ibfly(s, 4, 5, T2);
  ctab(0u, cimg_lin(3), T2);
  ibfly(s, 6, 7, T2);
  bxor(s, 0, 2);
  bxor(s, 1, 3);
  ibfly(s, 4, 6, T1);
  ibfly(s, 5, 7, T1);
#pragma unroll
  for (int r = 0; r < 4; ++r) bxor(s, r, r + 4);
}

// FFT stages 8, 7, 6 at index off (layout C'), reading the IFFT coefficients
// c and writing s: stage 8 x = off >> 9, stage 7 x = off >> 8 | p8, stage 6
// x = off >> 7 | (p7 + 2 p8); all subfield (x < 32)
__device__ __forceinline__ void fpassC9(State &s, const State &c, uint32_t off) {
  const uint32_t u0 = cimg_lin(off >> 7), u1 = cimg_lin(off >> 8), u2 = cimg_lin(off >> 9);
  SubTab Ta2, Ta1, Tb1, Ta0, Tb0;
  ctab(0u, u2, Ta2);
  ctab(0u, u1, Tb1);
#pragma unroll
  for (int r = 0; r < 4; ++r) fbfly_from(s, c, r, r + 4, Ta2);
  ctab(0u, u1 ^ cimg_lin(1), Ta1);
  fbfly(s, 0, 2, Tb1);
  fbfly(s, 1, 3, Tb1);
  ctab(0u, u0, Tb0);
  fbfly(s, 4, 6, Ta1);
  fbfly(s, 5, 7, Ta1);
  ctab(0u, u0 ^ cimg_lin(1), Ta0);
  fbfly(s, 0, 1, Tb0);
  ctab(0u, u0 ^ cimg_lin(2), Tb0);
  fbfly(s, 2, 3, Ta0);
  ctab(0u, u0 ^ cimg_lin(3), Ta0);
  fbfly(s, 4, 5, Tb0);
  fbfly(s, 6, 7, Ta0);
}

// C <-> C': register bit 2 and lane bit 5 swapped (registers r, r + 4)
__device__ __forceinline__ void swap_c(State &s) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    auto l = __builtin_amdgcn_permlane32_swap(s.l[r], s.l[r + 4], false, false);
    auto h = __builtin_amdgcn_permlane32_swap(s.h[r], s.h[r + 4], false, false);
    s.l[r] = l[0];
    s.l[r + 4] = l[1];
    s.h[r] = h[0];
    s.h[r + 4] = h[1];
  }
}

// ---- own-region staging: wave w stages its 4 pieces x 512 rows in its own
// 4 KB region, 8 B per row: row v at ((v >> 5) << 8) | 8 ((v ^ (v >> 5) ^
// 8 (w >> 1)) & 31).  Layout-A writes (rows 8 lane + r) and the store reads
// (8 rows x the 4 chunk pairs of regions (2c, 2c + 1) per 32 lanes) touch 32
// distinct 8-B slots of one 256-B block.
__host__ __device__ constexpr uint32_t soff(uint32_t v, uint32_t w) {
  return ((v >> 5) << 8) | ((((v ^ (v >> 5)) ^ ((w >> 1) << 3)) & 31) << 3);
}

__device__ __forceinline__ void stage_own(const State &s, uint32_t lane, uint32_t wave) {
  const uint32_t a = XCH0 + wave * XCH_BYTES + soff(8 * lane, wave);
#pragma unroll
  for (int r = 0; r < 8; ++r) lds_st2(a ^ soff(uint32_t(r), 0), to_be(s.l[r], s.h[r]));
}

// the row stores' geometry (enc_w_common.hpp store_own): lane = (row in 16,
// chunk c = pieces 8c..8c+7 = regions 2c, 2c + 1); row v = it * 128 + wave *
// 16 + lane / 4; a row's 16 bytes are 8 from each of the two regions
struct Rows {
  static constexpr int TILE = ecamd::TILE, K = ecamd::K;
  static constexpr uint32_t VSTEP = 16 * WAVES;
  __device__ static __forceinline__ RowLane lane_role(uint32_t wave, uint32_t lane) {
    const uint32_t c = lane & 3;
    const uint32_t v0 = wave * 16 + (lane >> 2);
    return {v0, c, XCH0 + 2 * c * XCH_BYTES + soff(v0, 2 * c)};  // soff(v, 2c) == soff(v, 2c + 1)
  }
  struct Halves {  // a row's two 8-byte reads, put together where they are stored
    uint2 x, y;
    __device__ __forceinline__ operator v4u() const { return v4u{x.x, x.y, y.x, y.y}; }
  };
  __device__ static __forceinline__ Halves read(uint32_t a, int it) {
    const uint32_t o = soff(uint32_t(it) * VSTEP, 0);
    return {lds_ld2(a ^ o), lds_ld2((a + XCH_BYTES) ^ o)};
  }
};

// coset j's extension image -> LDS by LDS-DMA, chunk i (1 KB) by wave i % 8:
// chunks 0..19 = stage 0, 20..34 = stages 1, 2 (table_images.hpp kEImg512Stage)
__device__ __forceinline__ void dma_ext(const uint8_t *eimg, uint32_t j, uint32_t wave, uint32_t lane) {
  const uint8_t *src = eimg + (j - 1) * kEImg512Bytes + 16 * lane;
  const uint32_t n = ext_chunks(j);
  for (uint32_t i = wave; i < n; i += WAVES)
    lds_dma16(i < 20 ? EXT[0] + 1024 * i : EXT[1] + 1024 * (i - 20), src + 1024 * i);
}

}  // namespace

__global__ void __launch_bounds__(THREADS, 4) encode_k512w(const uint8_t *__restrict__ payloads,
                                                           uint64_t plen, uint64_t pstride,
                                                           uint8_t *__restrict__ shards, uint64_t slen,
                                                           uint64_t sstride, int nv, uint32_t batch,
                                                           const uint8_t *__restrict__ cimg,
                                                           const uint8_t *__restrict__ eimg,
                                                           uint32_t *__restrict__ tick) {
  // the tile schedule: the uniform batch's geometry policy (enc_w_common.hpp)
  const UniformGeo<TILE> geo{payloads, plen, pstride, shards, slen, sstride, nv, batch, tick};
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t tid0 = threadIdx.x;
  auto *slot = reinterpret_cast<LdsWord *>(uintptr_t(SLOT));
  if (geo.publishes(tid0)) geo.first(slot, tid0);  // this workgroup's first tile
  {  // the compact image's F9 + subfield areas (12 KB, 768 chunks of 16 B)
    constexpr uint32_t c0 = BASE_LO / 16, n = (kCImgBytes - BASE_LO) / 16;
    const v4u a = reinterpret_cast<const v4u *>(cimg)[c0 + tid0];
    v4u b = v4u{0, 0, 0, 0};
    if (tid0 + THREADS < n) b = reinterpret_cast<const v4u *>(cimg)[c0 + THREADS + tid0];
    reinterpret_cast<v4u *>(lds)[c0 + tid0] = a;
    if (tid0 + THREADS < n) reinterpret_cast<v4u *>(lds)[c0 + THREADS + tid0] = b;
  }
  __syncthreads();

  const auto pre = geo.prepare();
  const uint32_t total = pre.total;
  const uint32_t wave_s = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  // cosets 512 j, j = 1..J, below n_validators (nv <= n: launch_encode_k512w)
  const uint32_t J = uint32_t(nv - 1) / K;
  // (the ticket protocol -- taken, published, read, rewritten: enc_w_common.hpp)
  uint32_t cur = geo.read(slot).t;

  // This lane's 4 x 16 payload bytes of a tile: pieces piece0 + 4 wave
  // + u, bytes 16 lane .. 16 lane + 15 of each, zero past plen; issued in the
  // previous tile's last coset, turned into the next State after its stores.
  v4u d[4];
  State nxt;
  const auto fetch = [&](const UniformGeo<TILE>::Loc fl) __attribute__((always_inline)) {
    uint32_t flane = tid0;
    asm volatile("" : "+v"(flane));
    flane &= 63;
    const Fetch f = geo.fetch(pre, fl);
    fetch_pieces<K>(f.P, f.plen, f.npieces, f.piece0 + 4 * wave_s, 4, 0, flane, d);
  };
  if (geo.ticket(cur) < total) {
    fetch(geo.loc(pre, cur));
    to_state(d, nxt);
  }

  while (geo.ticket(cur) < total) {
    uint32_t tid = tid0;
    asm volatile("" : "+v"(tid));
    const uint32_t lane = tid & 63, wave = tid >> 6;
    const uint32_t inst = lane >> 5, q = lane & 31;
    const bool hi = inst != 0;  // p8 in layouts A, B, C
    const uint32_t reg0 = XCH0 + wave * XCH_BYTES;  // this wave's region (bits >= 12)
    XBase xb;
    xb.a = reg0 | mswz(ulaneA(q, inst));
    xb.b = reg0 | mswz(ulaneB(q, inst));
    xb.c = reg0 | mswz(ulaneC(q, inst));
    const auto at = geo.at(pre, cur);
    const uint64_t piece0 = geo.piece0(at), npieces = geo.npieces(pre, cur), sstride = geo.sstride(cur);
    uint32_t taken = 0;  // thread 0: the tile taken for after this one
    if (tid0 == 0) taken = geo.next_ticket(cur);
    uint32_t next = 0;   // every wave: that tile, read from the slot
    uint8_t *SH = geo.rows(at);
    // every store phase of this tile takes the fast path (4 stores per lane)
    // or none does (rows 512 j < n_validators for j <= J)
    const bool fast = store_fast<Rows>(SH, sstride, 0, nv, piece0, npieces);
    const auto fetch_next = [&]() __attribute__((always_inline)) {
      next = geo.read(slot).t;
      fetch(geo.loc_or_none(pre, next));
    };
    const auto rsync = [&]() __attribute__((always_inline)) { lds_barrier(); };
    // coset j's extension image landed in every wave, then a barrier.  Coset
    // 1's was issued after the systematic stores (nothing after it), coset
    // j's after the barrier that precedes coset j - 1's store phase (4 stores
    // per lane after it on the fast path)
    const auto ext_ready = [&](uint32_t j) __attribute__((always_inline)) {
      if (j > 1 && fast) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      rsync();
    };
    const auto store = [&](uint32_t s0, bool last) __attribute__((always_inline)) {
      if (last)
        store_rows<Rows>(SH, sstride, s0, nv, piece0, npieces, wave_s, lane,
                         [&]() __attribute__((always_inline)) { to_state(d, nxt); });
      else
        store_rows<Rows>(SH, sstride, s0, nv, piece0, npieces, wave_s, lane, [] {});
    };
    // the systematic rows' store phase, then the ticket thread 0 took is published
    const auto store_sys = [&]() __attribute__((always_inline)) {
      store_rows<Rows>(SH, sstride, 0, nv, piece0, npieces, wave_s, lane, [&]() __attribute__((always_inline)) {
        if (geo.publishes(tid0)) geo.publish(slot, taken, tid0);
      });
    };
    // coset 1's extension image, after the systematic stores (their tile-slot
    // write waits for thread 0's ticket: a DMA issued before them would be
    // waited for with it): the last tile's last coset is past its tables
    // (every wave passed that coset's rows-staged barrier)
    const auto store_sys_dma = [&]() __attribute__((always_inline)) {
      store_sys();
      dma_ext(eimg, 1, wave_s, lane);
    };

    // ---- the tile: its barriers, LDS-DMA issues, counted waits and store phases,
    // written once.  A wave with pieces (LIVE) also stages and transforms; one
    // with none (the payload's last, partial tile) runs the same sequence bare.
    const uint32_t baseA = 8 * lane, baseB = (inst << 8) | posB(q, 0);  // lane parts of the positions
    const auto run = [&](auto live) __attribute__((always_inline)) {
      constexpr bool LIVE = decltype(live)::value;
      [[maybe_unused]] State s, coef;
      if constexpr (LIVE) s = nxt;
      // ---- systematic shards 0..511 = the data symbols (poly_encoder.hpp:239)
      rsync();  // tile start: the other waves are done reading the regions (last tile)
      if constexpr (LIVE) stage_own(s, lane, wave);
      rsync();  // systematic rows staged
      store_sys_dma();
      if constexpr (LIVE) {
        __builtin_amdgcn_sched_barrier(0);
        {  // into tower coordinates
          const TowerK tk = tower_k();
#pragma unroll
          for (int r = 0; r < 8; ++r) s.l[r] = tower_lo(s.l[r], s.h[r], tk);
        }
        // ---- IFFT_512 (index 0): passes A (bits 0-2), B (3-5), C' (6-8)
        ipassA(s, baseA, hi);
      }
      rsync();  // after IFFT pass A: systematic rows read out of the regions
      if constexpr (LIVE) {
        xchg<LA, LB>(s, xb);
        ipass<3>(s, baseB);
        xchg<LB, LC>(s, xb);
        swap_c(s);
        ipassC9(s);
        coef = s;
      }

      // ---- FFT_512 at each coset 512 j (encodeLow, poly_encoder.hpp:229-237).
      // Kinds by coset (x = (pos + off) >> (m + 1), ec_kernels.hpp): stage 3
      // subfield for j <= 3, F9 above; stage 2 subfield (j = 1), F9 (2, 3),
      // extension (4..7); stage 1 F9 (j = 1), extension above; stage 0
      // extension; stages 4-8 subfield.
      [[maybe_unused]] const auto coset = [&](auto k3, auto k2, auto k1, const uint32_t j)
                                              __attribute__((always_inline)) {
        using K3 = decltype(k3);
        using K2 = decltype(k2);
        using K1 = decltype(k1);
        const uint32_t off = K * j;
        // lane bases laundered per coset: the table addresses derived from them
        // are formed in the passes, not hoisted out of the coset loop (spilled)
        uint32_t bA = baseA, bB = baseB;
        asm volatile("" : "+v"(bA), "+v"(bB));
#pragma unroll
        for (int r = 0; r < 8; ++r) asm volatile("" : "+v"(coef.l[r]), "+v"(coef.h[r]));
        fpassC9(s, coef, off);
        swap_c(s);
        ext_ready(j);  // + the previous coset's rows read out of the regions
        xchg<LC, LB>(s, xb);
        fpass<3, SubTab, SubTab, K3>(s, bB, off);
        xchg<LB, LA>(s, xb);
        fpass<0, K2, K1, EG<0>>(s, bA, off);
        {  // back to symbol coordinates
          const TowerK tk = tower_k();
#pragma unroll
          for (int r = 0; r < 8; ++r) s.l[r] = tower_lo(s.l[r], s.h[r], tk);
        }
        stage_own(s, lane, wave);
      };
      // the cosets in a loop (three bodies, by table kinds); the last one leaves
      // it, so the next tile's payload (d, nxt) is live in that one only
      for (uint32_t j = 1;; ++j) {
        if constexpr (LIVE) {
          if (j == 1) coset(SubTab(), SubTab(), F9Tab(), j);
          else if (j <= 3) coset(SubTab(), F9Tab(), EG<1>(), j);
          else coset(F9Tab(), EG<2>(), EG<1>(), j);
        } else {
          ext_ready(j);  // the coset body's wait and barrier
        }
        if (j == J) {
          fetch_next();  // coef and s are dead here
          rsync();       // rows staged
          store(K * j, true);
          break;
        }
        rsync();  // rows staged; every wave is past this coset's tables
        dma_ext(eimg, j + 1, wave_s, lane);
        store(K * j, false);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if (piece0 + 4 * wave_s >= npieces) run(std::false_type());  // (wave-uniform)
    else run(std::true_type());
    cur = next;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA outlives the workgroup
}

bool k512w_applicable(const CodeParams &p) { return p.k == 512 && (p.n == 2048 || p.n == 4096); }

hipError_t launch_encode_k512w(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                               hipStream_t s) {
  if (!t.cimg || !t.eimg512) return hipErrorInvalidValue;
  if (!k512w_applicable(p) || p.nv <= uint32_t(K) || p.nv > p.n) return hipErrorInvalidValue;
  return launch_w(encode_k512w, LDS_BYTES, TILE, p, c, scratch, s, t.cimg, t.eimg512);
}

}  // namespace ecamd
