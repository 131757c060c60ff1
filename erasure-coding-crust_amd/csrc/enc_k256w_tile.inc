// enc_k256w_tile.inc — the one copy of the k = 256, n = 1024 encode's kernel
// body (DESIGN.md §5.1): a fragment, included inside the kernel function itself
// by enc_k256w.hip (the uniform batch) and enc_k256w_ragged.hip (ragged
// batches), after enc_k256w_body.hpp at namespace scope.  A textual fragment
// and not a function template on purpose: called as an (always-inlined)
// function the same statements compile to a different instruction stream for
// the uniform kernel (block layout, scheduling, register allocation); included
// in the kernel, encode_k256w's code is what it was before the body was shared.
//
// In scope at the point of inclusion:
//   geo        the geometry policy object (contract: enc_w_common.hpp)
//   nv, cimg   as encode_k256w's parameters of these names
// and no other declaration of the names this fragment declares.
//
// A policy with MASKED (enc_k256w_missing.hip, which states the schedule) skips
// the phases its tile's flags leave out and stores under the tile's row mask:
// every `if constexpr (M)` below.  For the other policies these are discarded
// and `!M || ...` is true: their code is what it was without them.
{
  using namespace k256w;
  using Geo = std::decay_t<decltype(geo)>;
  using Tile = typename Geo::Tile;
  constexpr bool M = Geo::MASKED;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t tid0 = threadIdx.x;
  auto *slot = reinterpret_cast<LdsWord *>(uintptr_t(SLOT));
  if (geo.publishes(tid0)) geo.first(slot, tid0);  // this workgroup's first tile
  copy_cimg(lds, cimg, tid0);
  __syncthreads();

  const auto pre = geo.prepare();
  const uint32_t total = pre.total;
  const uint32_t wave_s = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  // (the ticket protocol -- taken, published, read, rewritten: enc_w_common.hpp)
  Tile cur = geo.read(slot).t;

  // This lane's 4 x 16 payload bytes of a tile: pieces piece0 + 8 wave +
  // 4 inst + u, bytes 16 q .. 16 q + 15 of each, zero past plen.  A tile's loads
  // are issued at the end of the previous tile, before its last row stores, and
  // turned into the next State right after those stores (store_own's `then`).
  // vmcnt counts loads and stores together in issue order: loads issued after
  // a store phase (the tile start) wait for those stores to complete.
  // The 16-B loads need 16-B aligned pieces: a 16-B aligned payload (the
  // uniform dispatch; the ragged contract's payload_off), pieces of 512 bytes.
  v4u d[4];
  State nxt;  // the next tile's data, byte-planar, symbol coordinates
  const auto fetch = [&](const typename Geo::Loc fl) __attribute__((always_inline)) {
    uint32_t ftid = tid0;
    asm volatile("" : "+v"(ftid));  // per-lane addresses recomputed here, not hoisted and spilled
    const uint32_t lane = ftid & 63, inst = lane >> 5, q = lane & 31;
    const Fetch f = geo.fetch(pre, fl);
    fetch_pieces<K>(f.P, f.plen, f.npieces, f.piece0 + 8 * wave_s, 8, inst, q, d);
  };
  if (geo.ticket(cur) < total) {
    fetch(geo.loc(pre, cur));
    to_state(d, nxt);
  }

  while (geo.ticket(cur) < total) {
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
    const auto at = geo.at(pre, cur);
    const uint64_t piece0 = geo.piece0(at), npieces = geo.npieces(pre, cur), sstride = geo.sstride(cur);
    uint32_t taken = 0;  // thread 0: the tile taken for after this one
    if (tid0 == 0) taken = geo.next_ticket(cur);
    Tile next = {};    // every wave: that tile, read from the slot
    uint8_t *SH = geo.rows(at);
    // the last coset of this n_validators (uniform), after whose staging the
    // next tile's payload is fetched
    const uint32_t last_sh = nv > 768 ? 768u : 512u;  // nv > 512 (the launchers)
    const auto fetch_next = [&]() __attribute__((always_inline)) {
      next = geo.read(slot).t;
      fetch(geo.loc_or_none(pre, next));
    };
    const auto rsync = [&]() __attribute__((always_inline)) { lds_barrier(); };
    // M: the tile's phases F (bit 0: systematic rows, bits 1..3: cosets 256,
    // 512, 768; uniform) and a store phase of theirs.  The ticket is published
    // behind the systematic stores, as in the uniform kernel, when they and a
    // coset run; in every other tile right after the tile-start barrier
    // (`early`: the taken ticket is not kept in a register across a transform).
    // Coset 768, when it runs, is the last phase whatever else ran: it ends the
    // tile as the uniform kernel's last coset does (fetch_next in front of its
    // staging barrier, store_last).  A tile without it ends with tile_end: the
    // next ticket's read, the next tile's fetch and its State.
    [[maybe_unused]] const uint32_t F = tile_phases(geo, cur);
    [[maybe_unused]] const bool early = !(F & 1u) || F == 1u;
    [[maybe_unused]] const auto store_m = [&](uint32_t s0) __attribute__((always_inline)) {
      const bool first = !early && s0 == 0;
      store_rows<Rows>(
          SH, sstride, s0, nv, piece0, npieces, wave_s, lane,
          [&]() __attribute__((always_inline)) {
            if (first && geo.publishes(tid0)) geo.publish(slot, taken, tid0);
          },
          tile_mask(geo, cur));
    };
    [[maybe_unused]] const auto tile_end = [&]() __attribute__((always_inline)) {
      if (F == 0) rsync();  // no phase: the barrier between the publication and the read
      fetch_next();
      to_state(d, nxt);
    };
    // store_own's fast path needs 16-B aligned row slices (SH and sstride
    // multiples of 16: the uniform dispatch's alignment test, the ragged
    // contract's shard_off / shard_stride on a 16-B aligned base)
    const auto store = [&](uint32_t s0) __attribute__((always_inline)) {
      if constexpr (M)
        store_m(s0);
      else
        store_rows<Rows>(SH, sstride, s0, nv, piece0, npieces, wave_s, lane, [] {});
    };
    // the systematic rows' store phase; the ticket thread 0 took is then
    // published (the wait for the atomic's return then counts only the stores
    // issued after it on the fast path, store_own)
    const auto store_sys = [&]() __attribute__((always_inline)) {
      store_rows<Rows>(SH, sstride, 0, nv, piece0, npieces, wave_s, lane, [&]() __attribute__((always_inline)) {
        if (geo.publishes(tid0)) geo.publish(slot, taken, tid0);
      });
    };
    // the last store phase of the tile, then the next tile's State
    const auto store_last = [&](uint32_t s0) __attribute__((always_inline)) {
      if constexpr (M)
        store_rows<Rows>(
            SH, sstride, s0, nv, piece0, npieces, wave_s, lane,
            [&]() __attribute__((always_inline)) { to_state(d, nxt); }, tile_mask(geo, cur));
      else
        store_rows<Rows>(SH, sstride, s0, nv, piece0, npieces, wave_s, lane,
                         [&]() __attribute__((always_inline)) { to_state(d, nxt); });
    };

    // A wave none of whose 8 pieces exist (the last, partial tile of a payload:
    // 1 MB is 1954 pieces, its 31st tile has 34; most waves of a tiny ragged
    // item) skips the transforms and only takes part in the barriers and the
    // row stores of the others, in the same order as below (wave-uniform
    // branch).  Wave 0 never idles: a tile's first piece exists.
    if (piece0 + 8 * wave_s >= npieces) {
      rsync();  // tile start
      if (!M || (F & 1u)) {
        rsync();  // systematic rows staged
        store(0);
      }
      if (!M || (F & 0xEu)) rsync();  // after IFFT pass A
      for (uint32_t sh = K; sh < 1024u && int(sh) < nv; sh += K) {
        if constexpr (M) {
          if (!(F & (1u << (sh >> 8)))) continue;
        }
        rsync();  // after pass C
        rsync();  // rows staged
        if (M ? sh == 3 * K : sh == last_sh) {
          fetch_next();
          store_last(sh);
        } else {
          store(sh);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (M) {
        if (!(F & 8u)) tile_end();
      }
      cur = next;
      continue;
    }

    // ---- 8 pieces x 16 bytes (positions 8q..8q+7), fetched by the previous tile
    State s = nxt;

    // ---- systematic shards 0..255 = the data symbols (poly_encoder.hpp:239)
    rsync();  // the other waves are done reading this region (last tile)
    if constexpr (M) {
      if (early && geo.publishes(tid0)) geo.publish(slot, taken, tid0);
    }
    if (!M || (F & 1u)) {
      stage_own8(s, xch, q, inst, wave);
      rsync();
      if constexpr (M)
        store(0);
      else
        store_sys();
      __builtin_amdgcn_sched_barrier(0);
    }
    State coef;
    if (!M || (F & 0xEu)) {
      {  // into tower coordinates
        const TowerK tk = tower_k();
#pragma unroll
        for (int r = 0; r < 8; ++r) s.l[r] = tower_lo(s.l[r], s.h[r], tk);
      }

      // ---- IFFT_256 (index 0): passes A (bits 0-2), B (3-5), C (6-7)
      ipass<0>(s, posA(q, 0));
      rsync();  // systematic rows read out of the regions
      exchange<LA, LB>(s, xch, xb);
      ipass<3>(s, posB(q, 0));
      exchange<LB, LC>(s, xch, xb);
      ipassC(s);
      coef = s;
    }

    // ---- FFT_256 at each coset shift (encodeLow, poly_encoder.hpp:229-237).
    // Kinds of pass A's stages 2 / 1 / 0 by coset: 256: sub / sub / F9;
    // 512, 768: sub / F9 / general (x = (pos + off) >> (m + 1), ec_kernels.hpp)
    const auto coset = [&](auto t1, auto t0, const uint32_t off, auto last) __attribute__((always_inline)) {
      using T1 = decltype(t1);
      using T0 = decltype(t0);
      // coef made opaque in place (no copy): keeps the compiler from hoisting
      // the first stage's selector masks out of the coset loop
#pragma unroll
      for (int r = 0; r < 8; ++r) asm volatile("" : "+v"(coef.l[r]), "+v"(coef.h[r]));
      fpassC(s, coef, off);
      rsync();  // previous coset's rows read out
      exchange<LC, LB>(s, xch, xb);
      fpass<3, SubTab, SubTab, SubTab>(s, posB(q, 0), off);
      exchange<LB, LA>(s, xch, xb);
      fpass<0, SubTab, T1, T0>(s, posA(q, 0), off);
      {  // back to symbol coordinates
        const TowerK tk = tower_k();
#pragma unroll
        for (int r = 0; r < 8; ++r) s.l[r] = tower_lo(s.l[r], s.h[r], tk);
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
    if constexpr (M) {
      // the wanted cosets (the plan sets no bit of a coset at or above nv)
      if (F & 2u) coset(SubTab(), F9Tab(), K, std::false_type());
      if (F & 4u) coset(F9Tab(), Tab(), 2 * K, std::false_type());
      if (F & 8u)
        coset(F9Tab(), Tab(), 3 * K, std::true_type());
      else
        tile_end();
    } else {
      // n_validators 766..1024 (k = 256, n = 1024): cosets 256, 512 and, above
      // 768, 768; the last one has its own body (it fetches the next tile)
      coset(SubTab(), F9Tab(), K, std::false_type());
      if (last_sh == 3 * K) coset(F9Tab(), Tab(), 2 * K, std::false_type());
      coset(F9Tab(), Tab(), last_sh, std::true_type());
    }
    cur = next;
  }
}
