// sys_w_body.inc — the body of systematic_w and systematic_w_ragged (sys_w.hip),
// one copy, written against a geometry policy `geo`:
//   geo.total(lognrb)                     tickets of the launch (64-bit)
//   geo.resolve(t, lane, logR, lognrb)    ticket -> SysTile; called by every wave
//                                         with all lanes active and a wave-uniform t
// In scope besides geo: logk (k = 2^logk, 16 <= k) and tick (nullable).
//
// One ticket is one LDS tile: R = min(k, 256) rows x C = 16384 / R columns.
// Load side: lane (jl, pl) = (lane & 7, lane >> 3) of a wave takes, in each of
// its four 64-column x 16-row blocks, rows 2p and 2p + 1 at the 8 columns of
// chunk j (one 16-B load each: 8 lanes cover 128 B of a row), pairs the two
// rows' symbols column by column into dwords (v_perm) and stores them with
// ds_write_b32 into the tile kept in OUTPUT order: 16-B group G = c * R/8 + g
// holds column c, rows 8g .. 8g + 7.  Store side: lane reads group G = 256 it
// + tid with one ds_read_b128 and writes it with one 16-B streaming store, a
// wave 1 KB of contiguous output (two 512-B runs for k > 256).
//
// Swizzle: group G sits at G ^ ((G >> logR) & 7), i.e. XORed with the low
// three bits of its column chunk j.  ds_write_b32 (groups of 32 lanes = 8
// chunks x 4 row pairs of one g): the 8 chunks land in 8 different groups
// mod 8, the 4 pairs in that group's 4 dwords: 32 banks.  ds_read_b128
// (groups of 16 lanes made of 4-aligned lane quads that cover every residue
// mod 16 of G): the XOR moves bits 0-1 inside a quad's own residues and bit 2
// for the whole wave alike (G bit logR + 2 >= 6), so the 16 residues stay
// distinct: 64 banks.
  __shared__ __attribute__((aligned(16))) uint32_t tile[kSysTileSyms / 2];
  __shared__ uint32_t next_ticket[2];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(tid >> 6)));
  const int logR = logk < 8 ? logk : 8;
  const int logGs = logR - 3;   // 16-B groups (8 rows) per column
  const int logCb = 8 - logR;   // 64-column blocks per tile row of blocks
  const int lognrb = logk - logR;
  const uint32_t jl = lane & 7, pl = lane >> 3;
  const uint64_t total = geo.total(lognrb);
  uint64_t t = blockIdx.x;
  if (t >= total) return;  // (the ragged grid is sized from the longest item allowed)

  v4u v[8];
  // Loads run to the 16-B boundary after a row's last byte: the row's base and
  // pitch are multiples of 16 and the pitch is at least the shard length, so
  // that boundary lies inside the row's own pitch; and a data row (y < k <
  // n_validators) is never the buffer's last row, so the pitch is there.
  // block blk = 4 it + wave of the tile's 16: 64 columns x 16 rows; the lane's
  // place in a block is the same in every block (lane_off), the block's a scalar
  const auto load = [&](const SysTile &c) {
    const uint64_t lane_off = uint64_t(2 * pl) * c.pitch + 16 * jl;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const uint32_t blk = uint32_t(it) * 4 + wave;
      const uint32_t jb = blk & ((1u << logCb) - 1), pb = blk >> logCb;
      const uint64_t col = 2 * c.i0 + 128 * uint64_t(jb);  // the block's first byte in the row
      const uint8_t *src = c.SH + uint64_t(16 * pb) * c.pitch + col + lane_off;
      const bool on = col + 16 * jl < c.slen;
      v[2 * it] = on ? *reinterpret_cast<const v4u *>(src) : v4u{0, 0, 0, 0};
      v[2 * it + 1] = on ? *reinterpret_cast<const v4u *>(src + c.pitch) : v4u{0, 0, 0, 0};
    }
  };
  const auto to_lds = [&]() {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const uint32_t blk = uint32_t(it) * 4 + wave;
      const uint32_t j = ((blk & ((1u << logCb) - 1)) << 3) | jl, p = ((blk >> logCb) << 3) | pl;
      const uint32_t base = (j << (3 + logGs)) | (p >> 2);
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) {
        const uint32_t a = v[2 * it][cc >> 1], b = v[2 * it + 1][cc >> 1];
        const uint32_t dw = (cc & 1) ? vperm(b, a, 0x07060302u) : vperm(b, a, 0x05040100u);
        tile[((((base + (uint32_t(cc) << logGs)) ^ jl)) << 2) | (p & 3)] = dw;
      }
    }
  };
  // a column is stored whole or not at all: 16 B are 8 rows of ONE column, so
  // nothing is written outside shard_len * k bytes of the item's output
  // (256 threads are a whole number of columns: the lane keeps its rows 8g ..
  // and steps 256 >> logGs columns per iteration; a tile's output spans at
  // most 2 MB, so the lane's offset from the tile's first byte has 32 bits)
  const auto store = [&](const SysTile &c) {
    uint8_t *const O = c.O + ((c.i0 << logk) << 1);
    const uint32_t c0 = tid >> logGs, cstep = uint32_t(kSysThreads) >> logGs;
    const uint32_t off = ((c0 << logk) << 1) + 16 * (tid & ((1u << logGs) - 1)), ostep = (cstep << logk) << 1;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const uint32_t G = uint32_t(it) * kSysThreads + tid;
      const v4u val = reinterpret_cast<const v4u *>(tile)[G ^ ((G >> logR) & 7)];
      if (2 * (c.i0 + c0 + uint32_t(it) * cstep) < c.slen)
        __builtin_nontemporal_store(val, reinterpret_cast<v4u *>(O + (off + uint32_t(it) * ostep)));
    }
  };

  SysTile cur = geo.resolve(t, lane, logR, lognrb);
  load(cur);
  for (;;) {
    if (tid == 0) {  // the next ticket, read by everyone behind the barrier below
      const uint64_t nx = tick ? uint64_t(gridDim.x) + atomicAdd(tick, 1u) : t + gridDim.x;
      next_ticket[0] = uint32_t(nx);
      next_ticket[1] = uint32_t(nx >> 32);
    }
    to_lds();
    lds_barrier();  // (LDS only: the stores of the tile before stay in flight)
    const uint64_t tn = uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(next_ticket[0])))) |
                        (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(next_ticket[1])))) << 32);
    const bool more = tn < total;
    SysTile nxt = cur;
    if (more) {  // the next tile's loads fly while this one is stored
      nxt = geo.resolve(tn, lane, logR, lognrb);
      load(nxt);
    }
    store(cur);
    if (!more) break;
    lds_barrier();  // the tile and the ticket words are free again; the loads above stay in flight
    cur = nxt;
    t = tn;
  }
