// dec_n1024x.hip — reconstruct for n = 1024, k = 256 (n_validators 766..1024,
// the BASELINE headline) with 12 or 16 waves per CU: three or four per SIMD
// instead of the two of reconstruct_n1024 (dec_n1024.hip), for the latency
// the 2-wave form leaves exposed (31% of wave time waiting
// to issue, the VALU ~57% busy at 2 waves per SIMD).  One kernel template,
// reconstruct_n1024x<WAVES>; the 12-wave form first, what the 16-wave form
// changes at the end of this comment.
//
// The per-wave work is reconstruct_n1024's (one byte-planar group of 4 shard
// columns per wave; gather + E[v] scaling, IFFT_1024 in radix-16 register
// passes with wave-private LDS exchanges, the closed-form derivative and the
// FFT restricted to the k outputs, phase 5: erased outputs times E[y]).  What
// it takes to fit 12 waves in one CU:
//  * LDS = the 32 KB element-indexed compact image (DevTables::cimg, the
//    headline encode's; since round 6: layouts whose element kinds are
//    register-indexed, below) + 12 x 8 KB exchange regions = 128 KB.  Until
//    round 6 a 64 KB reduced skew-slot image (every stage-0 table in the
//    general form, because the kinds varied across the lanes).
//  * phase 5's received data rows y < k: the gather copies each present
//    row's raw 96-B segment into LDS beside the regions (24 KB of the 32 KB
//    the compact image freed; until round 6 they were re-read from the
//    shards into registers held across the IFFT: 10.58 -> 10.54 ms at
//    nv = 1024, 10.23 -> 10.12 at nv = 800, profiles/r06/ab/rec_stage/).
//  * <= 168 VGPRs: the output tables E[y] are requested after IFFT pass C,
//    not before the transform.
// Tile = 48 shard columns (12 waves x 4); 1 MB at n_validators 1024 is 1954
// columns, 41 tiles per payload.
//
// 16 waves (shards of kN1024x16MinCols columns and more; n1024x_waves):
//  * LDS = the 32 KB image + 16 x 8 KB regions = 160 KB, all a workgroup may
//    take: no staging area.  Phase 5's received rows are read from the shards
//    again (L2: the gather read the same lines earlier in the tile), 8 B per
//    lane and row, requested beside the E[y] tables after IFFT pass C.  The
//    schedule word sits in dword 1 of the image's first kCImgSub1 entry, which
//    no table fetch reads (ctab: dword 0 of those entries only).
//  * <= 128 VGPRs (launch bounds 1024).
//  * Tile = 64 columns: a row segment is 128 B, one gather slot per thread
//    (1024 threads, 1024 slots); 1 MB at n_validators 1024 is 31 tiles.
#include "dec_n1024x_body.hpp"

namespace ecamd {

// the kernel body: dec_n1024x_tile.inc (one copy, shared with the ragged
// form); this kernel runs it on the uniform batch's geometry
template <int WAVES>
__global__ void __launch_bounds__(64 * WAVES) reconstruct_n1024x(
    const uint8_t *__restrict__ shards, uint64_t slen, uint64_t sstride,
    const uint8_t *__restrict__ present, const uint16_t *__restrict__ elog,
    const uint32_t *__restrict__ pattern, const uint32_t *__restrict__ order,
    uint8_t *__restrict__ out, uint64_t ostride, int nv, uint32_t batch, uint32_t *tick, DevTables t) {
  const UniformGeo<WAVES> geo{shards, slen, sstride, out, ostride, nv, batch, tick};
#include "dec_n1024x_tile.inc"
}

// scratch of the n = 1024 reconstructs: the gather order, then the tile
// counter of reconstruct_n1024x (256 B apart)
size_t n1024_tick_offset(const CodeParams &p, size_t batch) { return (gather_order_bytes(p, batch) + 255) / 256 * 256; }
size_t n1024_scratch_bytes(const CodeParams &p, size_t batch) { return n1024_tick_offset(p, batch) + kTileCounterBytes; }

static_assert(size_t(Form<12>::COLS) == kN1024xMinCols, "choose_reconstruct: at least one whole tile");
static_assert(size_t(Form<16>::COLS) <= kN1024x16MinCols, "n1024x_waves: at least one whole tile");

// the form launch_reconstruct_n1024x runs: 16 waves from kN1024x16MinCols
// columns, 12 below and where ECCR_AMD_RECON_WAVES=12 is set
int n1024x_waves(size_t slen) {
  return !recon_overrides().waves12 && slen / 2 >= kN1024x16MinCols ? 16 : 12;
}

namespace {
template <int WAVES>
hipError_t launch_form(const CodeParams &p, const DevTables &t, const ReconCall &c, void *scratch, hipStream_t s) {
  using F = Form<WAVES>;
  int cus = 0;
  if (!t.cimg || !scratch || c.slen / 2 < size_t(F::COLS)) return hipErrorInvalidValue;
  if (const hipError_t e = prepare_kernel(reinterpret_cast<const void *>(&reconstruct_n1024x<WAVES>), F::LDS_BYTES, &cus);
      e != hipSuccess)
    return e;
  const size_t tiles = (c.slen / 2 + F::COLS - 1) / F::COLS * c.batch;
  if (tiles + 4096 >= (size_t(1) << 32)) return hipErrorInvalidValue;  // 32-bit tile tickets
  uint32_t *order = static_cast<uint32_t *>(scratch);  // n1024_scratch_bytes(p, batch)
  uint32_t *tick = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(scratch) + n1024_tick_offset(p, c.batch));
  if (const hipError_t e = launch_gather_order(p, c.present, c.err_log, c.pattern, c.batch, order, s);
      e != hipSuccess)
    return e;
  if (const hipError_t e = launch_zero_counters(tick, sizeof(uint32_t), s); e != hipSuccess) return e;
  const unsigned grid = unsigned(tiles < size_t(cus) ? tiles : size_t(cus));
  hipLaunchKernelGGL(reconstruct_n1024x<WAVES>, dim3(grid), dim3(F::THREADS), F::LDS_BYTES, s, c.shards,
                     uint64_t(c.slen), uint64_t(c.sstride), c.present, c.err_log, c.pattern, order, c.out,
                     uint64_t(c.ostride), int(p.nv), uint32_t(c.batch), tick, t);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_reconstruct_n1024x(const CodeParams &p, const DevTables &t, const ReconCall &c, void *scratch,
                                     hipStream_t s) {
  return n1024x_waves(c.slen) == 16 ? launch_form<16>(p, t, c, scratch, s) : launch_form<12>(p, t, c, scratch, s);
}

}  // namespace ecamd
