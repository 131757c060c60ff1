// dec_n1024x_tile.inc — the one copy of reconstruct_n1024x's kernel body: a
// fragment, included inside the kernel function itself by dec_n1024x.hip (the
// uniform batch) and dec_n1024x_ragged.hip (ragged batches), after
// dec_n1024x_body.hpp at namespace scope.  It is a textual fragment and not a
// function template on purpose: called as an (always-inlined) function the
// same statements compile to a different instruction stream -- table fetches
// merged across phases, and the 16-wave form, which sits at 128 VGPRs, spills.
// Included in the kernel, the uniform kernels' code is what it was before the
// body was shared.
//
// In scope at the point of inclusion:
//   WAVES                         12 or 16 (a constant expression)
//   geo                           the geometry policy object (dec_n1024x_body.hpp)
//   present, elog, pattern, order, t
//                                 as reconstruct_n1024x's parameters of these
//                                 names (rows indexed by item / pattern)
// and no other declaration of the names this fragment declares.
{
  using F = Form<WAVES>;
  using Tile = typename std::decay_t<decltype(geo)>::Tile;
  constexpr int THREADS = F::THREADS, COLS = F::COLS, ROW_WORDS = F::ROW_WORDS;
  constexpr uint32_t SLOT = F::SLOT;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint8_t *regions = lds + TAB_REGION;
  // Tiles are handed out dynamically: a workgroup's first tile is blockIdx.x,
  // every later one gridDim.x + a ticket from the counter *tick (zeroed by
  // the launcher).  The ticket for the tile after next is taken by thread 0
  // during a tile and published in the LDS word SLOT at its end (one tile of
  // notice: the next tile's metadata is loaded a tile ahead).  A static
  // grid stride left the workgroups' end times ~3.5% of the launch apart.
  volatile uint32_t *slot = reinterpret_cast<volatile uint32_t *>(lds + SLOT);
  const uint32_t tid0 = threadIdx.x, wave = tid0 >> 6;
  uint32_t taken = 0;
  if (tid0 == 0) taken = geo.first_ticket();
  uint8_t *my = regions + wave * REG_BYTES;

  // the 32 KB compact image (DevTables::cimg), every load issued before the first store
  {
    constexpr int kPer = (TAB_REGION / 16 + THREADS - 1) / THREADS;
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    v4u v[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const uint32_t i = tid0 + k * THREADS;
      if (i < uint32_t(TAB_REGION / 16)) v[k] = reinterpret_cast<const v4u *>(t.cimg)[i];
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const uint32_t i = tid0 + k * THREADS;
      if (i < uint32_t(TAB_REGION / 16)) reinterpret_cast<v4u *>(lds)[i] = v[k];
    }
  }
  __syncthreads();
  geo.settle_first(slot, taken, tid0);
  taken = geo.second_ticket(taken, tid0);
  if (geo.publishes(tid0)) geo.publish(slot, taken, tid0);  // read after the first tile's region barrier

  const auto pre = geo.prepare();
  const uint64_t total = pre.total;
  const uint32_t wave_s = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  // m[0], m[1]: this thread's gather slots (gather_order: present rows first;
  // slot tid and, with 12 waves, 768 + tid, the latter only below 1024): row << 16 |
  // mul_index(E[row]), low half 0xFFFF = absent.  m[2], m[3]: the output rows
  // y = 4 lane + q of phase 5, 16 bits each: 0xFFFF = present, else
  // mul_index(E[y]).  Loaded one tile ahead.
  const auto load_meta = [&](uint64_t bw, uint32_t tid, uint32_t (&m)[4]) {
    const uint64_t pt = pattern ? pattern[bw] : bw;
    m[0] = order[bw * N + tid];
    if constexpr (F::SLOTS == 2) m[1] = tid + THREADS < uint32_t(N) ? order[bw * N + THREADS + tid] : 0xFFFFu;
    const uint32_t y0 = 4 * (tid & 63);
    const uint32_t p4 = *reinterpret_cast<const uint32_t *>(present + pt * N + y0);
    const uint2 e4 = *reinterpret_cast<const uint2 *>(elog + pt * N + y0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t e = ((q < 2 ? e4.x : e4.y) >> (16 * (q & 1))) & 0xFFFFu;
      const uint32_t f = ((p4 >> (8 * q)) & 0xFFu) ? 0xFFFFu : mul_index(e);
      if (q & 1) m[2 + (q >> 1)] |= f << 16;
      else m[2 + (q >> 1)] = f;
    }
  };
  uint32_t meta[4] = {0, 0, 0, 0}, meta_next[4] = {0, 0, 0, 0};
  Tile cur = geo.first_tile(slot);  // (total < 2^32: launchers)
  if (cur.ticket < total) load_meta(geo.item(pre, cur), tid0, meta);
  while (cur.ticket < total) {
    // lane-derived addresses recomputed per tile (not hoisted and spilled)
    uint32_t tid = tid0;
    asm volatile("" : "+v"(tid));
    const uint32_t lane = tid & 63;
    const Where wh = geo.where(pre, cur);
    const uint64_t col0 = wh.col0, slen = wh.slen, ncols = wh.ncols, sstride = wh.sstride;
    const uint8_t *SH = wh.SH;
    uint8_t *O = wh.O;

    Tile nxt;  // the next tile (SLOT)
    // ---- phase 1: gather + scale this thread's slots' rows (decode_main:
    // 174-177), 12 groups of 4 columns each into the groups' regions; absent
    // rows as 0 (16 waves: one slot, 16 groups).  The first slot's row and
    // E[v] table are requested before the tile barrier.
    {
      uint32_t w[ROW_WORDS] = {};  // (defined on every path: not carried across tiles)
      Tab RT = {};
      const uint64_t avail = slen - 2 * col0;  // bytes of a row inside the tile
      const auto load_row = [&](int half) __attribute__((always_inline)) {
        const uint8_t *row = SH + uint64_t(meta[half] >> 16) * sstride + 2 * col0;
        if (avail >= 2 * COLS) {
#pragma unroll
          for (int q = 0; q < ROW_WORDS / 4; ++q) {
            const uint4 d = reinterpret_cast<const uint4 *>(row)[q];
            w[4 * q] = d.x;
            w[4 * q + 1] = d.y;
            w[4 * q + 2] = d.z;
            w[4 * q + 3] = d.w;
          }
        } else {  // the payload's last tile
          load_row_tail<ROW_WORDS>(row, uint32_t(avail), w);
        }
        load_tab(t.mtab_tin, meta[half] & 0xffffu, RT);  // scaled into tower coordinates
      };
      if ((meta[0] & 0xffffu) != 0xffffu) load_row(0);
      lds_barrier();  // the previous tile's readers of the regions are done
      nxt = geo.read(slot);
      if (tid0 == 0) taken = geo.next_ticket();  // the tile after nxt
#pragma unroll
      for (int half = 0; half < F::SLOTS; ++half) {
        if (half == 1 && tid >= uint32_t(N - THREADS)) break;  // (uniform per wave)
        const uint32_t v = meta[half] >> 16;
        const bool on = (meta[half] & 0xffffu) != 0xffffu;
        if (half == 1 && on) load_row(1);
        uint32_t l[WAVES], h[WAVES];
#pragma unroll
        for (int g = 0; g < WAVES; ++g) l[g] = h[g] = 0;
        if (on) {  // one divergent branch for the tile's groups
          if constexpr (F::STAGED) {
            if (v < uint32_t(K)) {  // phase 5's copy of a received data row
#pragma unroll
              for (int j = 0; j < ROW_WORDS / 4; ++j)
                *reinterpret_cast<__attribute__((address_space(3))) v4u *>(uintptr_t(stg_row<WAVES>(v) + 16 * j)) =
                    v4u{w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]};
            }
          }
#pragma unroll
          for (int g = 0; g < WAVES; ++g) {  // columns 4g..4g+3: words (h0 l0 h1 l1)(h2 l2 h3 l3)
            const uint32_t a = w[2 * g], c = w[2 * g + 1];
            const uint32_t xh = vperm(c, a, 0x06040200u), xl = vperm(c, a, 0x07050301u);
            mul_acc(xl, xh, RT, l[g], h[g]);
          }
        }
#pragma unroll
        for (int g = 0; g < WAVES; ++g)
          *reinterpret_cast<uint2 *>(regions + g * REG_BYTES + rz(v)) = make_uint2(l[g], h[g]);
      }
    }
    if (nxt.ticket < total) load_meta(geo.item(pre, nxt), tid, meta_next);
    __syncthreads();  // (every wave has read SLOT)
    const uint64_t cbase = col0 + 4 * uint64_t(wave_s);  // wave-uniform
    // a group past the payload's last column (the last, partial tile: 1 MB is
    // 1954 columns, the 41st tile has 34): phases 2-5 are this wave's alone
    if (cbase >= ncols) {
#pragma unroll
      for (int i = 0; i < 4; ++i) meta[i] = meta_next[i];
      cur = nxt;
      continue;
    }

    S16 s;
    // ---- phase 2: IFFT_1024 on this wave's group: layouts A', B', C (above)
    {
      const uint32_t la = lds_addr(my) | rz(lane << 2);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint2 x = lds_ld2(la ^ rz(posA2_reg(r)));
        s.l[r] = x.x;
        s.h[r] = x.y;
      }
      ipassA2(s, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) lds_st2(la ^ rz(posA2_reg(r)), make_uint2(s.l[r], s.h[r]));
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    {
      const uint32_t lb = lds_addr(my) | rz(posB2_lane(lane));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint2 x = lds_ld2(lb ^ rz(uint32_t(r) << 2));
        s.l[r] = x.x;
        s.h[r] = x.y;
      }
      ipassB2(s, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) lds_st2(lb ^ rz(uint32_t(r) << 2), make_uint2(s.l[r], s.h[r]));
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    // layout C: r bit0 = p8, bit1 = p9, bit2 = p6, bit3 = p7; lane = p0..p5
    const uint32_t lc = lds_addr(my) | rz(lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint2 x = lds_ld2(lc ^ rz(posC_reg(r)));
      s.l[r] = x.x;
      s.h[r] = x.y;
    }
    ipassC2(s);

    // phase-5 operands requested now, consumed after the derivative and the
    // FFT.  16 waves: the received rows y = 4 lane + q < 256 themselves, this
    // wave's 4 columns: an aligned 8-B word whose first two bytes are inside
    // the row (cbase < ncols), so it stays on the row's page and, a data row
    // never being the buffer's last, inside the buffer.  Absent rows are not
    // read.  (Requested before the tables: after them, or one by one between
    // them, the compiler spills 46 dwords.)
    uint2 RV[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t m = (meta[2 + (q >> 1)] >> (16 * (q & 1))) & 0xFFFFu;
      RV[q] = make_uint2(0, 0);
      if constexpr (!F::STAGED) {
        if (m == 0xFFFFu)
          RV[q] = *reinterpret_cast<const uint2 *>(SH + uint64_t(4 * lane + uint32_t(q)) * sstride + 2 * cbase);
      }
    }
    // E[y] of this lane's erased output rows y = 4 lane + q (and the received
    // ones)
    Tab T5[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t m = (meta[2 + (q >> 1)] >> (16 * (q & 1))) & 0xFFFFu;
      // defined on every path (a table read only where used would be carried
      // across the tile loop, and spilled, by the compiler)
      load_tab(t.mtab_tout, m != 0xFFFFu ? m : 0u, T5[q]);  // tower in, symbols out
    }

    // ---- phases 3 + 4: the closed-form derivative at y < 256 and the FFT
    // restricted to y < 256, dec_n1024_dfft.inc (one copy, shared with
    // reconstruct_n1024); the table of its step i is at L(i)
    const uint32_t hi67 = ((lane >> 4) & 3) << 6, lo = lane & 15;
    const uint32_t hi47 = ((lane >> 2) & 15) << 4, lo01 = lane & 3;
    const uint32_t hi27 = lane << 2;
    // the restricted FFT's elements x = pos >> (m + 1) (compact image entries)
    auto L = [&](int i) -> uint32_t {
      switch (i) {
        case 2: return cimg_lin(1);                         // stage 6, p7 = 1
        case 3: return cimg_lin((hi67 | lo) >> 6);          // stage 5
        case 4: return cimg_lin((hi67 | lo) >> 5);          // stage 4
        case 5: return cimg_lin((hi67 | 32u | lo) >> 5);
        case 6: return cimg_lin((hi47 | lo01) >> 4);        // stage 3
        case 7: return cimg_lin((hi47 | lo01) >> 3);        // stage 2
        case 8: return cimg_lin((hi47 | 8u | lo01) >> 3);
        case 9: return cimg_lin(hi27 >> 2);                 // stage 1
        case 10: return cimg_lin(hi27 >> 1);                // stage 0
        default: return cimg_lin((hi27 | 2u) >> 1);
      }
    };
#define DFFT_TAB(i, T) ctab(0u, L(i), T)
#include "dec_n1024_dfft.inc"
#undef DFFT_TAB

    // ---- phase 5: y = 4*lane + q; columns cbase + c (decode_main:185-188,
    // reconstructSub:138-149)
    {
      uint32_t ol[4], oh[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t m = (meta[2 + (q >> 1)] >> (16 * (q & 1))) & 0xFFFFu;
        ol[q] = oh[q] = 0;
        if (m != 0xFFFFu) {
          mul_acc(ql[q], qh[q], T5[q], ol[q], oh[q]);
        } else {
          uint2 rv = RV[q];
          if constexpr (F::STAGED) rv = lds_ld2(stg_row<WAVES>(4 * lane + uint32_t(q)) + 8 * wave_s);
          oh[q] = vperm(rv.y, rv.x, 0x06040200u);
          ol[q] = vperm(rv.y, rv.x, 0x07050301u);
        }
      }
#include "dec_n1024_store.inc"
    }
    // the tile after next is published (wave 0 never idles: its columns start
    // the tile, so thread 0 and its wave get here); the atomic returned during
    // the transform
    if (geo.publishes(tid0)) geo.publish(slot, taken, tid0);
#pragma unroll
    for (int i = 0; i < 4; ++i) meta[i] = meta_next[i];
    cur = nxt;
  }
}
