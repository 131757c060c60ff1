// enc_k256w.hip — encode for k = 256, n = 1024 (n_validators 766..1024, the
// BASELINE headline), two 8-wave workgroups per CU.
//
// The transforms are those of encode_k256 (enc_k256.hip):
// per piece IFFT_256 at index 0, then FFT_256 at the cosets 256, 512, 768
// (encodeLow, poly_encoder.hpp:217-240), radix-8 register passes with
// wave-private LDS exchanges, tower coordinates with subfield / F9 / general
// multiplies.  What differs:
//  * the multiply tables are the 32 KB element-indexed compact image
//    (ec_kernels.hpp kCImg*, DevTables::cimg) instead of the 80 KB skew-slot
//    image, so a workgroup needs 64 KB of LDS and TWO are resident per CU.
//    Each workgroup still synchronises its waves at every staging step, but
//    while one waits at a barrier, for its payload loads or for its row
//    stores to issue, the other one's waves compute on the same SIMDs
//    (phase stamps of the 16-wave form: 30% of wave time at barriers, 9% in
//    the payload loads, 9% in the stores);
//  * the tile is 64 pieces (8 waves x 8), each shard row a 128-B segment.
// The passes, the payload fetch, the row stores and the launch tail are shared
// with enc_kw.hip and enc_k512w.hip: enc_w_common.hpp.
#include "enc_w_common.hpp"

namespace ecamd {
namespace {

constexpr int K = 256;
constexpr int TILE = 8 * WAVES;  // pieces per tile
constexpr uint32_t XCH0 = kCImgBytes;      // the waves' regions follow the tables
constexpr uint32_t SLOT = XCH0 + WAVES * XCH_BYTES;  // the next tile's index (dynamic schedule)
constexpr int LDS_BYTES = int(SLOT + 16);
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");

// ---- own-region staging: wave w stages its 8 pieces x 256 rows in its own
// 4 KB region, 16 B per row (half = instance); row v in 256-B block v >> 4 at
// 16-B slot (v ^ (v >> 4) ^ 2w) & 15.  The row reads (lane = row-in-8 << 3 |
// source wave c) hit 16 distinct slots in every ds_read_b128 lane group; the
// layout-A writes are 2-way (the minimum for 8-B writes of one instance).
__host__ __device__ constexpr uint32_t soff8(uint32_t v, uint32_t w) {
  return ((v >> 4) << 8) | (((v ^ (v >> 4) ^ (w << 1)) & 15) << 4);
}

__device__ __forceinline__ void stage_own8(const State &s, uint8_t *xch, uint32_t q, uint32_t inst,
                                           uint32_t wave) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
    *reinterpret_cast<uint2 *>(xch + soff8(posA(q, r), wave) + 8 * inst) = to_be(s.l[0][r], s.h[0][r]);
}

// the row stores' geometry (enc_w_common.hpp store_own): lane = (row in 8,
// source wave c = 16-B chunk of pieces [8c, 8c + 8)); row v = it * 64 + wave *
// 8 + lane / 8, 8 lanes per 128-B row segment
struct Rows {
  static constexpr int TILE = ecamd::TILE, K = ecamd::K;
  static constexpr uint32_t VSTEP = 8 * WAVES;
  __device__ static __forceinline__ RowLane lane_role(uint32_t wave, uint32_t lane) {
    const uint32_t c = lane & 7;
    const uint32_t v0 = wave * 8 + (lane >> 3);
    return {v0, c, XCH0 + c * XCH_BYTES + soff8(v0, c)};
  }
  __device__ static __forceinline__ v4u read(uint32_t a, int it) { return lds_r128(a ^ soff8(uint32_t(it) * VSTEP, 0)); }
};

}  // namespace

__global__ void __launch_bounds__(THREADS, 4) encode_k256w(const uint8_t *__restrict__ payloads,
                                                           uint64_t plen, uint64_t pstride,
                                                           uint8_t *__restrict__ shards, uint64_t slen,
                                                           uint64_t sstride, int nv, uint32_t batch,
                                                           const uint8_t *__restrict__ cimg,
                                                           uint32_t *__restrict__ tick) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t tid0 = threadIdx.x;
  auto *slot = reinterpret_cast<__attribute__((address_space(3))) volatile uint32_t *>(uintptr_t(SLOT));
  // this workgroup's first tile; without a counter (no scratch) a static
  // grid stride (slower: the two workgroups of a CU drift apart, below)
  if (tid0 == 0) *slot = tick ? atomicAdd(tick, 1u) : blockIdx.x;
  copy_cimg(lds, cimg, tid0);
  __syncthreads();

  const uint64_t npieces = slen / 2;
  const uint32_t tiles_pp = uint32_t((npieces + TILE - 1) / TILE);
  const uint32_t total = tiles_pp * batch;  // < 2^32 (launch_encode_k256w)
  const uint32_t wave_s = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  // Dynamic schedule: tiles are taken from the launch's counter (`tick`,
  // zeroed before the launch) one tile ahead, so the two workgroups of a CU,
  // which the issue arbiter serves at unequal rates (the older one's waves win
  // ties), finish together.  With a static grid-stride split the faster one
  // ended up to 2.8 ms before the slower one of a 7 ms launch, which then ran
  // alone (scripts/variants/clk_run.py).
  // Thread 0 takes tile t + 1 at the start of tile t and publishes it in the
  // LDS slot after the tile's systematic stores; every wave reads it after the
  // barrier that follows IFFT pass A; the slot is rewritten only after the
  // next tile-start barrier, by which every wave has read it.
  uint32_t cur = __builtin_amdgcn_readfirstlane(*slot);

  // This lane's 4 x 16 payload bytes of tile (b, i): pieces i * TILE + 8 wave +
  // 4 inst + u, bytes 16 q .. 16 q + 15 of each, zero past plen.  A tile's loads
  // are issued at the end of the previous tile, before its last row stores, and
  // turned into the next State right after those stores (store_own's `then`).
  // vmcnt counts loads and stores together in issue order: loads issued after
  // a store phase (the tile start) wait for those stores to complete.
  v4u d[4];
  State nxt;  // the next tile's data, byte-planar, symbol coordinates
  const auto fetch = [&](uint64_t fb, uint64_t fi) __attribute__((always_inline)) {
    uint32_t ftid = tid0;
    asm volatile("" : "+v"(ftid));  // per-lane addresses recomputed here, not hoisted and spilled
    const uint32_t lane = ftid & 63, inst = lane >> 5, q = lane & 31;
    fetch_pieces<K>(payloads + fb * pstride, plen, npieces, fi * TILE + 8 * wave_s, 8, inst, q, d);
  };
  if (cur < total) {
    fetch(cur / tiles_pp, cur % tiles_pp);
    to_state(d, nxt);
  }

  while (cur < total) {
    // lane ids made opaque per tile: per-lane LDS addresses are recomputed in
    // the loop instead of being hoisted out of it and spilled
    uint32_t tid = tid0;
    asm volatile("" : "+v"(tid));
    const uint32_t lane = tid & 63, wave = tid >> 6;
    const uint32_t inst = lane >> 5, q = lane & 31;
    uint8_t *xch = lds + XCH0 + wave * XCH_BYTES;
    XBase xb;
    xb.a = mswz(ulaneA(q, inst));
    xb.b = mswz(ulaneB(q, inst));
    xb.c = mswz(ulaneC(q, inst));
    const uint64_t b = cur / tiles_pp, piece0 = uint64_t(cur % tiles_pp) * TILE;
    uint32_t taken = 0;  // thread 0: the tile taken for after this one
    if (tid0 == 0) taken = tick ? atomicAdd(tick, 1u) : cur + gridDim.x;
    uint32_t next = 0;   // every wave: that tile, read from the slot
    uint8_t *SH = shards + b * uint64_t(nv) * sstride;
    // the last coset of this n_validators (uniform), after whose staging the
    // next tile's payload is fetched
    const uint32_t last_sh = nv > 768 ? 768u : 512u;  // nv > 512 (launch_encode_k256w)
    const auto fetch_next = [&]() __attribute__((always_inline)) {
      next = __builtin_amdgcn_readfirstlane(*slot);
      // past the end: the zero path, no loads
      fetch(next < total ? next / tiles_pp : 0, next < total ? next % tiles_pp : tiles_pp);
    };
    const auto rsync = [&]() __attribute__((always_inline)) { lds_barrier(); };
    const auto store = [&](uint32_t s0) __attribute__((always_inline)) {
      // the row stores (LDS reads + global stores) at raised issue priority
      __builtin_amdgcn_s_setprio(1);
      store_own<Rows>(SH, sstride, s0, nv, piece0, npieces, wave_s, lane, [] {});
      __builtin_amdgcn_s_setprio(0);
    };
    // the systematic rows' store phase; thread 0 then publishes the tile it
    // took (the wait for the atomic's return then counts only the stores
    // issued after it on the fast path, store_own)
    const auto store_sys = [&]() __attribute__((always_inline)) {
      __builtin_amdgcn_s_setprio(1);
      store_own<Rows>(SH, sstride, 0, nv, piece0, npieces, wave_s, lane, [&]() __attribute__((always_inline)) {
        if (tid0 == 0) *slot = taken;
      });
      __builtin_amdgcn_s_setprio(0);
    };
    // the last store phase of the tile, then the next tile's State
    const auto store_last = [&](uint32_t s0) __attribute__((always_inline)) {
      __builtin_amdgcn_s_setprio(1);
      store_own<Rows>(SH, sstride, s0, nv, piece0, npieces, wave_s, lane,
                 [&]() __attribute__((always_inline)) { to_state(d, nxt); });
      __builtin_amdgcn_s_setprio(0);
    };

    // A wave none of whose 8 pieces exist (the last, partial tile of a payload:
    // 1 MB is 1954 pieces, its 31st tile has 34) skips the transforms and only
    // takes part in the barriers and the row stores of the others, in the same
    // order as below (wave-uniform branch)
    if (piece0 + 8 * wave_s >= npieces) {
      rsync();  // tile start
      rsync();  // systematic rows staged
      store(0);
      rsync();  // after IFFT pass A
      for (uint32_t sh = K; sh < 1024u && int(sh) < nv; sh += K) {
        rsync();  // after pass C
        rsync();  // rows staged
        if (sh == last_sh) {
          fetch_next();
          store_last(sh);
        } else {
          store(sh);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      cur = next;
      continue;
    }

    // ---- 8 pieces x 16 bytes (positions 8q..8q+7), fetched by the previous tile
    State s = nxt;

    // ---- systematic shards 0..255 = the data symbols (poly_encoder.hpp:239)
    rsync();  // the other waves are done reading this region (last tile)
    stage_own8(s, xch, q, inst, wave);
    rsync();
    store_sys();
    __builtin_amdgcn_sched_barrier(0);
    {  // into tower coordinates
      const TowerK tk = tower_k();
#pragma unroll
      for (int r = 0; r < 8; ++r) s.l[0][r] = tower_lo(s.l[0][r], s.h[0][r], tk);
    }

    // ---- IFFT_256 (index 0): passes A (bits 0-2), B (3-5), C (6-7)
    ipass<0>(s, posA(q, 0));
    rsync();  // systematic rows read out of the regions
    exchange<LA, LB>(s, xch, xb);
    ipass<3>(s, posB(q, 0));
    exchange<LB, LC>(s, xch, xb);
    ipassC(s);
    State coef = s;

    // ---- FFT_256 at each coset shift (encodeLow, poly_encoder.hpp:229-237).
    // Kinds of pass A's stages 2 / 1 / 0 by coset: 256: sub / sub / F9;
    // 512, 768: sub / F9 / general (x = (pos + off) >> (m + 1), ec_kernels.hpp)
    const auto coset = [&](auto t1, auto t0, const uint32_t off, auto last) __attribute__((always_inline)) {
      using T1 = decltype(t1);
      using T0 = decltype(t0);
      // coef made opaque in place (no copy): keeps the compiler from hoisting
      // the first stage's selector masks out of the coset loop
#pragma unroll
      for (int r = 0; r < 8; ++r) asm volatile("" : "+v"(coef.l[0][r]), "+v"(coef.h[0][r]));
      fpassC(s, coef, off);
      rsync();  // previous coset's rows read out
      exchange<LC, LB>(s, xch, xb);
      fpass<3, SubTab, SubTab, SubTab>(s, posB(q, 0), off);
      exchange<LB, LA>(s, xch, xb);
      fpass<0, SubTab, T1, T0>(s, posA(q, 0), off);
      {  // back to symbol coordinates
        const TowerK tk = tower_k();
#pragma unroll
        for (int r = 0; r < 8; ++r) s.l[0][r] = tower_lo(s.l[0][r], s.h[0][r], tk);
      }
      stage_own8(s, xch, q, inst, wave);
      if constexpr (decltype(last)::value) fetch_next();  // coef and s are dead here
      rsync();
      if constexpr (decltype(last)::value)
        store_last(off);
      else
        store(off);
      __builtin_amdgcn_sched_barrier(0);
    };
    // n_validators 766..1024 (k = 256, n = 1024): cosets 256, 512 and, above
    // 768, 768; the last one has its own body (it fetches the next tile)
    coset(SubTab(), F9Tab(), K, std::false_type());
    if (last_sh == 3 * K) coset(F9Tab(), Tab(), 2 * K, std::false_type());
    coset(F9Tab(), Tab(), last_sh, std::true_type());
    cur = next;
  }
}

hipError_t launch_encode_k256w(const CodeParams &p, const DevTables &t, const uint8_t *d_payloads,
                               size_t plen, size_t pstride, size_t batch, uint8_t *d_shards,
                               size_t sstride, void *scratch, hipStream_t s) {
  if (!t.cimg) return hipErrorInvalidValue;
  if (p.nv <= 2 * K || p.nv > 1024) return hipErrorInvalidValue;  // cosets 256, 512 (, 768)
  return launch_w(encode_k256w, LDS_BYTES, TILE, p, d_payloads, plen, pstride, batch, d_shards, sstride, scratch,
                  s, t.cimg);
}

}  // namespace ecamd
