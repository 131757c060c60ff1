// enc_kw.hip — encode for k = 2^M = 16, 32, 64, 128 (n <= 8 k: n_validators
// 46..765, the Polkadot validator counts of today among them) and k = 256 at
// n = 2048 (n_validators 1025..1533), two 8-wave workgroups per CU.
//
// encode_k256w's model (enc_k256w.hip; shared code and tile schedule: enc_w_common.hpp;
// DESIGN.md §5.1, §5.7): per piece (2 k payload bytes = k symbols) IFFT_k at index 0, then FFT_k at each coset k j
// below n_validators (encodeLow, poly_encoder.hpp:217-240), radix-8 register
// passes in tower coordinates, wave-private LDS exchanges.  A wave holds NG =
// 512 / k byte-planar groups of 4 pieces; a group's k positions lie over k / 8
// lanes x 8 registers, the group index in the lane bits above.  Read as
// position bits M..7 and encode_k256w's instance bit, the group bits make
// every layout and exchange encode_k256w's:
//  * layout A: registers p0..p2 (lane part 8 q, q = lane & (k/8 - 1));
//  * layout B: registers p3..p5 as far as they are positions (M = 4: p3 only,
//    M = 5: p3, p4), lanes p0..p2 and p6; for M <= 6 its elements are
//    wave-uniform;
//  * M = 7: stage 6 in layout C's register bit 0; M = 8: stages 6, 7 in
//    layout C (encode_k256w's pass C);
//  * every element of k <= 128 is x < 2^(M+2) <= 512: the 32 KB compact image
//    holds all tables (LDS 64 KB per workgroup); at k = 256, n = 2048 the
//    stage-0 elements of cosets 4..7 (512..1023) come from a 10 KB per-coset
//    extension image brought in by LDS-DMA, as in enc_k512w.hip (74 KB);
//  * tiles of 8 NG pieces per wave (32 KB of payload), shard-row segments of
//    64 NG bytes stored as 16 B per lane (two groups of one wave).
#include "enc_w_common.hpp"

namespace ecamd {
namespace {

constexpr uint32_t XCH0 = kCImgBytes;        // the wave regions follow the tables
constexpr uint32_t SLOT = XCH0 + WAVES * XCH_BYTES;  // the next tile's index
// k = 256 (n = 2048 only): the extension tables of cosets 4..7 (stage 0,
// elements 512..1023: table_images.hpp kEImg256*) after the slot
constexpr uint32_t EXT8 = SLOT + 1024;
template <int M>
constexpr int lds_bytes() { return int(M == 8 ? EXT8 + kEImg256Bytes : SLOT + 16); }
static_assert(2 * lds_bytes<8>() <= 160 * 1024, "two workgroups per CU");
static_assert(XCH0 % (2 * XCH_BYTES) == 0, "XOR-addressed regions");

template <int M>
struct Geo {
  static constexpr uint32_t K = 1u << M;
  static constexpr int NG = 512 >> M;          // byte-planar groups per wave
  static constexpr int WP = 4 * NG;            // pieces per wave
  static constexpr int TILE = WP * WAVES;      // pieces per tile (32 KB of payload)
  static constexpr int RC = 4 * NG;            // 16-B chunks per shard-row segment
  static constexpr int RPI = 512 / RC;         // rows per store iteration (all waves), 0 if < 1
  static constexpr uint32_t QM = (1u << (M - 3)) - 1;  // lane mask of the layout-A position part
  static_assert(M >= 4 && M <= 8, "k = 16 .. 256");
};

// Stage 0 of cosets 4..7 at k = 256, n = 2048: a general table of the coset's
// extension image in LDS (enc_w_common.hpp ftab)
struct Ext0 : ExtKind {
  static constexpr uint32_t BASE = EXT8, PLANE = kEImg256Bytes / 5;
};

// ---- layout B for M <= 6: registers p3, p4, p5 as far as they are positions
// (the others group bits), no lane part: every element is x = (register
// position bits above m) | (off >> (m + 1)), wave-uniform.  Stage 3 pairs
// registers (2 rr, 2 rr + 1), rr = (p4, p5); stage 4 (r, r + 2), block p5;
// stage 5 (r, r + 4).
template <int M>
constexpr uint32_t bmask3() { return (M > 4 ? 1u : 0u) | (M > 5 ? 2u : 0u); }
template <int M>
constexpr uint32_t bmask4() { return M > 5 ? 1u : 0u; }

// IFFT stages 3 .. M - 1 at index 0 (x = 0: b ^= a only, additive_fft.hpp:110-112)
template <int M>
__device__ __forceinline__ void ipassB_u(State &s) {
  SubTab T1, T2, T3;
  ctab(0u, cimg_lin(1), T1);
  if constexpr (M > 5) {
    ctab(0u, cimg_lin(2), T2);
    ctab(0u, cimg_lin(3), T3);
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const uint32_t x = uint32_t(rr) & bmask3<M>();
    if (x == 0) bxor(s, 2 * rr, 2 * rr + 1);
    else if (x == 1) ibfly(s, 2 * rr, 2 * rr + 1, T1);
    else if (x == 2) ibfly(s, 2 * rr, 2 * rr + 1, T2);
    else ibfly(s, 2 * rr, 2 * rr + 1, T3);
  }
  if constexpr (M > 4) {
#pragma unroll
    for (int r : {0, 1, 4, 5}) {
      if (((uint32_t(r) >> 2) & bmask4<M>()) == 0) bxor(s, r, r + 2);
      else ibfly(s, r, r + 2, T1);
    }
  }
  if constexpr (M > 5) {
#pragma unroll
    for (int r = 0; r < 4; ++r) bxor(s, r, r + 4);
  }
}

// FFT stages M - 1 .. 3 at index off, the first one reading the IFFT
// coefficients c
template <int M>
__device__ __forceinline__ void fpassB_u(State &s, const State &c, uint32_t off) {
  if constexpr (M > 5) {  // stage 5, x = off >> 6
    SubTab T;
    ctab(0u, cimg_lin(off >> 6), T);
#pragma unroll
    for (int r = 0; r < 4; ++r) fbfly_from(s, c, r, r + 4, T);
  }
  if constexpr (M > 4) {  // stage 4, x = off >> 5 | p5
    SubTab Ta, Tb;
    ctab(0u, cimg_lin(off >> 5), Ta);
    ctab(0u, cimg_lin(off >> 5) ^ cimg_lin(bmask4<M>()), Tb);
#pragma unroll
    for (int r : {0, 1, 4, 5}) {
      const SubTab &T = (uint32_t(r) >> 2) & bmask4<M>() ? Tb : Ta;
      if constexpr (M == 5) fbfly_from(s, c, r, r + 2, T);
      else fbfly(s, r, r + 2, T);
    }
  }
  {  // stage 3, x = off >> 4 | (p4, p5)
    SubTab T[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) ctab(0u, cimg_lin(off >> 4) ^ cimg_lin(uint32_t(rr) & bmask3<M>()), T[rr]);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      if constexpr (M == 4) fbfly_from(s, c, 2 * rr, 2 * rr + 1, T[rr]);
      else fbfly(s, 2 * rr, 2 * rr + 1, T[rr]);
    }
  }
}

// ---- own-region staging: wave w stages its NG groups x k rows in its own
// 4 KB region, 8 B per (row v, group g) at slot (v NG + g) ^ (v >> 3) << (8 -
// M) ^ ((w << (9 - M)) & 31).  Layout-A writes (rows 8 q + r; 32 lanes = the
// q and the low group bits) and the store reads (16 lanes x 16 B = group pairs
// (2h, 2h + 1) of one row across waves) hit distinct banks.
// k = 256 (NG = 2): bit 0 stays the group (a store read takes groups 0 and 1
// of a row as one 16-B pair), the row's bits 3-6 go to bits 1-4 (16-lane
// write groups distinct) and the wave to bits 2-4 (the two rows of a 16-lane
// store read, which differ in bit 1, keep their 8 chunks apart).
template <int M>
__host__ __device__ constexpr uint32_t soff(uint32_t v, uint32_t g, uint32_t w) {
  if constexpr (M == 8)
    return (((v << 1) | g) ^ (((v >> 3) & 15u) << 1) ^ ((w << 2) & 31u)) << 3;
  else
    return (((v << (9 - M)) | g) ^ ((v >> 3) << (8 - M)) ^ ((w << (9 - M)) & 31u)) << 3;
}

template <int M>
__device__ __forceinline__ void stage_own(const State &s, uint32_t q, uint32_t g, uint32_t wave) {
  const uint32_t a = XCH0 + wave * XCH_BYTES + soff<M>(8 * q, g, wave);
#pragma unroll
  for (int r = 0; r < 8; ++r) lds_st2(a ^ soff<M>(uint32_t(r), 0, 0), to_be(s.l[r], s.h[r]));
}

// the row stores' geometry (enc_w_common.hpp store_own): chunk it * 512 +
// thread: row v = chunk / RC, chunk c = chunk % RC (16 B = pieces 8c..8c+7 =
// groups 2h, 2h + 1 of wave c / (NG / 2))
template <int M>
struct Rows {
  using G = Geo<M>;
  static constexpr int TILE = G::TILE, K = G::K;
  static constexpr uint32_t VSTEP = 512 / G::RC;
  __device__ static __forceinline__ RowLane lane_role(uint32_t wave, uint32_t lane) {
    const uint32_t t = wave * 64 + lane;
    const uint32_t v0 = t / G::RC, c = t % G::RC;
    const uint32_t cw = c / (G::NG / 2), h = c % (G::NG / 2);
    return {v0, c, XCH0 + cw * XCH_BYTES + soff<M>(v0, 2 * h, cw)};  // 16-B aligned: groups 2h, 2h + 1
  }
  __device__ static __forceinline__ v4u read(uint32_t a, int it) { return lds_r128(a ^ soff<M>(uint32_t(it) * VSTEP, 0, 0)); }
};

}  // namespace

template <int M>
__global__ void __launch_bounds__(THREADS, 4) encode_kw(const uint8_t *__restrict__ payloads,
                                                        uint64_t plen, uint64_t pstride,
                                                        uint8_t *__restrict__ shards, uint64_t slen,
                                                        uint64_t sstride, int nv, uint32_t batch,
                                                        const uint8_t *__restrict__ cimg,
                                                        const uint8_t *__restrict__ eimg,
                                                        uint32_t *__restrict__ tick) {
  using G = Geo<M>;
  constexpr uint32_t K = G::K;
  // the tile schedule: the uniform batch's geometry policy (enc_w_common.hpp)
  using UGeo = UniformGeo<G::TILE>;
  const UGeo geo{payloads, plen, pstride, shards, slen, sstride, nv, batch, tick};
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t tid0 = threadIdx.x;
  auto *slot = reinterpret_cast<LdsWord *>(uintptr_t(SLOT));
  if (geo.publishes(tid0)) geo.first(slot, tid0);  // this workgroup's first tile
  copy_cimg(lds, cimg, tid0);
  __syncthreads();

  const auto pre = geo.prepare();
  const uint32_t total = pre.total;
  const uint32_t wave_s = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  const uint32_t J = uint32_t(nv - 1) / K;  // cosets k j, j = 1..J <= 7 (nv <= n <= 8 k)
  // (the ticket protocol -- taken, published, read, rewritten: enc_w_common.hpp)
  uint32_t cur = geo.read(slot).t;

  // This lane's 4 x 16 payload bytes of a tile: pieces piece0 + WP wave
  // + 4 g + u (g = lane >> (M - 3)), bytes 16 q .. 16 q + 15 of each (q = lane
  // & QM), zero past plen; issued in the previous tile's last coset.
  v4u d[4];
  State nxt;
  const auto fetch = [&](const typename UGeo::Loc fl) __attribute__((always_inline)) {
    uint32_t ftid = tid0;
    asm volatile("" : "+v"(ftid));
    const uint32_t lane = ftid & 63, g = lane >> (M - 3), q = lane & G::QM;
    const Fetch f = geo.fetch(pre, fl);
    fetch_pieces<K>(f.P, f.plen, f.npieces, f.piece0 + G::WP * wave_s, G::WP, g, q, d);
  };
  if (geo.ticket(cur) < total) {
    fetch(geo.loc(pre, cur));
    to_state(d, nxt);
  }

  while (geo.ticket(cur) < total) {
    uint32_t tid = tid0;
    asm volatile("" : "+v"(tid));
    const uint32_t lane = tid & 63, wave = tid >> 6;
    // encode_k256w's lane roles: q5 = position bits 3..7 in layout A (the
    // group bits above p(M-1) read as positions), inst = lane bit 5
    const uint32_t q5 = lane & 31, i0 = lane >> 5;
    const uint32_t reg0 = XCH0 + wave * XCH_BYTES;
    XBase xb;
    xb.a = reg0 | mswz(ulaneA(q5, i0));
    xb.b = reg0 | mswz(ulaneB(q5, i0));
    xb.c = reg0 | mswz(ulaneC(q5, i0));
    const auto at = geo.at(pre, cur);
    const uint64_t piece0 = geo.piece0(at), npieces = geo.npieces(pre, cur), sstride = geo.sstride(cur);
    uint32_t taken = 0;  // thread 0: the tile taken for after this one
    if (tid0 == 0) taken = geo.next_ticket(cur);
    uint32_t next = 0;   // every wave: that tile, read from the slot
    uint8_t *SH = geo.rows(at);
    // every store phase of this tile but possibly the last coset's takes the
    // fast path (4 stores per lane), or none does
    [[maybe_unused]] const bool fast = store_fast<Rows<M>>(SH, sstride, 0, nv, piece0, npieces);
    // k = 256, n = 2048: coset j's extension image (10 x 1 KB) -> LDS, chunk i by
    // wave i % 8, issued after the previous coset's rows-staged barrier
    [[maybe_unused]] const auto dma_ext = [&](uint32_t j) __attribute__((always_inline)) {
      const uint8_t *src = eimg + (j - 4) * kEImg256Bytes + 16 * lane;
      for (uint32_t i = wave_s; i < kEImg256Bytes / 1024; i += WAVES)
        lds_dma16(EXT8 + 1024 * i, src + 1024 * i);
    };
    const auto fetch_next = [&]() __attribute__((always_inline)) {
      next = geo.read(slot).t;
      fetch(geo.loc_or_none(pre, next));
    };
    const auto rsync = [&]() __attribute__((always_inline)) { lds_barrier(); };
    const auto store = [&](uint32_t s0, bool last) __attribute__((always_inline)) {
      if (last)
        store_rows<Rows<M>>(SH, sstride, s0, nv, piece0, npieces, wave_s, lane,
                            [&]() __attribute__((always_inline)) { to_state(d, nxt); });
      else
        store_rows<Rows<M>>(SH, sstride, s0, nv, piece0, npieces, wave_s, lane, [] {});
    };
    // the systematic rows' store phase, then the ticket thread 0 took is published
    const auto store_sys = [&]() __attribute__((always_inline)) {
      store_rows<Rows<M>>(SH, sstride, 0, nv, piece0, npieces, wave_s, lane, [&]() __attribute__((always_inline)) {
        if (geo.publishes(tid0)) geo.publish(slot, taken, tid0);
      });
    };

    // a wave none of whose pieces exist (the payload's last, partial tile)
    // takes part only in the barriers and the row stores (uniform)
    if (piece0 + G::WP * wave_s >= npieces) {
      rsync();  // tile start
      rsync();  // systematic rows staged
      store_sys();
      rsync();  // after IFFT pass A
      for (uint32_t j = 1;; ++j) {
        if constexpr (M == 8) {
          if (j >= 4 && fast) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
          else if (j >= 4) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        rsync();  // previous rows read out
        if (j == J) {
          fetch_next();
          rsync();  // rows staged
          store(K * j, true);
          break;
        }
        rsync();  // rows staged
        if constexpr (M == 8)
          if (j >= 3) dma_ext(j + 1);
        store(K * j, false);
        __builtin_amdgcn_sched_barrier(0);
      }
      cur = next;
      continue;
    }

    State s = nxt;
    const uint32_t q = lane & G::QM, g = lane >> (M - 3);
    // ---- systematic shards 0..k-1 = the data symbols (poly_encoder.hpp:239)
    rsync();  // the other waves are done reading the regions (last tile)
    stage_own<M>(s, q, g, wave);
    rsync();
    store_sys();
    __builtin_amdgcn_sched_barrier(0);
    {  // into tower coordinates
      const TowerK tk = tower_k();
#pragma unroll
      for (int r = 0; r < 8; ++r) s.l[r] = tower_lo(s.l[r], s.h[r], tk);
    }

    // ---- IFFT_k (index 0): pass A (bits 0-2), then pass B (bits 3..M-1;
    // M = 7: 3-5, then stage 6 in layout C).  Lane parts of the positions
    // (group bits excluded): A 8 q, B (M = 7) posB(q5, 0) & 127
    const uint32_t baseA = 8 * q, baseB = posB(q5, 0) & (K - 1);
    ipass<0>(s, baseA);
    rsync();  // systematic rows read out of the regions
    xchg<LA, LB>(s, xb);
    if constexpr (M == 8) {
      ipass<3>(s, baseB);
      xchg<LB, LC>(s, xb);
      ipassC(s);
    } else if constexpr (M == 7) {
      ipass<3>(s, baseB);
      xchg<LB, LC>(s, xb);
#pragma unroll
      for (int r = 0; r < 8; r += 2) bxor(s, r, r + 1);  // stage 6, x = 0 (additive_fft.hpp:110-112)
    } else {
      ipassB_u<M>(s);
    }
    State coef = s;

    // ---- FFT_k at each coset k j (encodeLow, poly_encoder.hpp:229-237).
    // Kinds (x = (pos + off) >> (m + 1)): M = 7: stage 0 subfield (j = 1), F9
    // (2, 3), general (4..7), stage 1 subfield (j <= 3), F9 above; M = 6:
    // stage 0 subfield (j <= 3), F9 above; everything else subfield.
    const auto coset = [&](auto t2, auto t1, auto t0, const uint32_t j) __attribute__((always_inline)) {
      using T2 = decltype(t2);
      using T1 = decltype(t1);
      using T0 = decltype(t0);
      const uint32_t off = K * j;
      uint32_t bA = baseA, bB = baseB;
      asm volatile("" : "+v"(bA), "+v"(bB));  // table addresses formed per coset, not hoisted
#pragma unroll
      for (int r = 0; r < 8; ++r) asm volatile("" : "+v"(coef.l[r]), "+v"(coef.h[r]));
      if constexpr (M == 8) {
        fpassC(s, coef, off);
        // previous coset's rows read out; from coset 4 on, also this coset's
        // extension image landed in every wave (issued before the previous
        // coset's store phase: 4 stores per lane after it on the fast path)
        if (j >= 4 && fast) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (j >= 4) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        rsync();
        xchg<LC, LB>(s, xb);
        fpass<3, SubTab, SubTab, SubTab>(s, bB, off);
      } else if constexpr (M == 7) {
        {  // stage 6, x = off >> 7, from the coefficients
          SubTab T6;
          ctab(0u, cimg_lin(off >> 7), T6);
#pragma unroll
          for (int r = 0; r < 8; r += 2) fbfly_from(s, coef, r, r + 1, T6);
        }
        rsync();  // previous coset's rows read out
        xchg<LC, LB>(s, xb);
        fpass<3, SubTab, SubTab, SubTab>(s, bB, off);
      } else {
        fpassB_u<M>(s, coef, off);
        rsync();  // previous coset's rows read out
      }
      xchg<LB, LA>(s, xb);
      fpass<0, T2, T1, T0>(s, bA, off);
      {  // back to symbol coordinates
        const TowerK tk = tower_k();
#pragma unroll
        for (int r = 0; r < 8; ++r) s.l[r] = tower_lo(s.l[r], s.h[r], tk);
      }
      stage_own<M>(s, q, g, wave);
    };
    // the cosets in a loop (a body per table-kind class); the last one leaves
    // it, so the next tile's payload (d, nxt) is live in that one only
    for (uint32_t j = 1;; ++j) {
      if constexpr (M == 8) {  // n = 2048: stage 0 of cosets 4..7 from the extension image
        if (j == 1) coset(SubTab(), SubTab(), F9Tab(), j);
        else if (j <= 3) coset(SubTab(), F9Tab(), Tab(), j);
        else coset(F9Tab(), Tab(), Ext0(), j);
      } else if constexpr (M == 7) {
        if (j == 1) coset(SubTab(), SubTab(), SubTab(), j);
        else if (j <= 3) coset(SubTab(), SubTab(), F9Tab(), j);
        else coset(SubTab(), F9Tab(), Tab(), j);
      } else if constexpr (M == 6) {
        if (j <= 3) coset(SubTab(), SubTab(), SubTab(), j);
        else coset(SubTab(), SubTab(), F9Tab(), j);
      } else {
        coset(SubTab(), SubTab(), SubTab(), j);
      }
      if (j == J) {
        fetch_next();  // coef and s are dead here
        rsync();       // rows staged
        store(K * j, true);
        break;
      }
      rsync();  // rows staged; every wave is past this coset's tables
      if constexpr (M == 8)
        if (j >= 3) dma_ext(j + 1);
      store(K * j, false);
      __builtin_amdgcn_sched_barrier(0);
    }
    cur = next;
  }
  if constexpr (M == 8) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA outlives the workgroup
}

bool kw_applicable(const CodeParams &p) {
  return (p.k >= 16 && p.k <= 128 && (p.k & (p.k - 1)) == 0 && p.n > p.k && p.n <= 8 * p.k) ||
         (p.k == 256 && p.n == 2048);
}

template <int M>
static hipError_t launch_m(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                           hipStream_t s) {
  return launch_w(encode_kw<M>, lds_bytes<M>(), Geo<M>::TILE, p, c, scratch, s, t.cimg, t.eimg256);
}

hipError_t launch_encode_kw(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                            hipStream_t s) {
  if (!t.cimg || !kw_applicable(p) || p.nv <= p.k || p.nv > p.n) return hipErrorInvalidValue;
  if (p.k == 256 && (!t.eimg256 || p.nv <= 4 * p.k)) return hipErrorInvalidValue;  // cosets 4.. exist (n = 2048)
  switch (p.k) {
    case 16: return launch_m<4>(p, t, c, scratch, s);
    case 32: return launch_m<5>(p, t, c, scratch, s);
    case 64: return launch_m<6>(p, t, c, scratch, s);
    case 128: return launch_m<7>(p, t, c, scratch, s);
    default: return launch_m<8>(p, t, c, scratch, s);
  }
}

}  // namespace ecamd
