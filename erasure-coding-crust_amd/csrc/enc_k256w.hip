// enc_k256w.hip — encode for k = 256, n = 1024 (n_validators 766..1024, the
// BASELINE headline), two 8-wave workgroups per CU.
//
// The transforms are those of encode_k256 (enc_k256.hip):
// per piece IFFT_256 at index 0, then FFT_256 at the cosets 256, 512, 768
// (encodeLow, poly_encoder.hpp:217-240), radix-8 register passes with
// wave-private LDS exchanges, tower coordinates with subfield / F9 / general
// multiplies.  What differs:
//  * the multiply tables are the 32 KB element-indexed compact image
//    (table_images.hpp kCImg*, DevTables::cimg) instead of the 80 KB skew-slot
//    image, so a workgroup needs 64 KB of LDS and TWO are resident per CU.
//    Each workgroup still synchronises its waves at every staging step, but
//    while one waits at a barrier, for its payload loads or for its row
//    stores to issue, the other one's waves compute on the same SIMDs
//    (phase stamps of the 16-wave form: 30% of wave time at barriers, 9% in
//    the payload loads, 9% in the stores);
//  * the tile is 64 pieces (8 waves x 8), each shard row a 128-B segment.
// The passes, the payload fetch, the row stores, the tile schedule and the launch
// tail are shared with enc_kw.hip and enc_k512w.hip: enc_w_common.hpp.  The tile body itself
// is in enc_k256w_body.hpp, shared with encode_k256w_ragged.
#include "enc_k256w_body.hpp"

namespace ecamd {

// the kernel body: enc_k256w_tile.inc (one copy, shared with the ragged form);
// this kernel runs it on the uniform batch's geometry
__global__ void __launch_bounds__(THREADS, 4) encode_k256w(const uint8_t *__restrict__ payloads,
                                                           uint64_t plen, uint64_t pstride,
                                                           uint8_t *__restrict__ shards, uint64_t slen,
                                                           uint64_t sstride, int nv, uint32_t batch,
                                                           const uint8_t *__restrict__ cimg,
                                                           uint32_t *__restrict__ tick) {
  const UniformGeo<k256w::TILE> geo{payloads, plen, pstride, shards, slen, sstride, nv, batch, tick};
#include "enc_k256w_tile.inc"
}

hipError_t launch_encode_k256w(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                               hipStream_t s) {
  if (!t.cimg) return hipErrorInvalidValue;
  if (p.nv <= 2 * k256w::K || p.nv > 1024) return hipErrorInvalidValue;  // cosets 256, 512 (, 768)
  return launch_w(encode_k256w, k256w::lds_bytes<UniformGeo<k256w::TILE>>(), k256w::TILE, p, c, scratch, s, t.cimg);
}

}  // namespace ecamd
