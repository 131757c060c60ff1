// dec_g_body.inc — the one copy of the generic reconstruct's kernel body
// (reed-solomon.hpp:83-134 + poly_encoder.hpp:118-215 for 4*G shard positions):
// a fragment included inside reconstruct_g and reconstruct_g_ragged
// (ec_kernels.hip); textual for the reason given in enc_g_body.inc.
//
// In scope at the point of inclusion: geo (a geometry policy of
// ec_kernels.hip: prepare(), on(b), rows(shards, b, nv), outp(out, b), npos(pre, b),
// pitch(b)), shards, present, elog,
// out, nv, logn, logk, logG, batch, pattern, t, scratch as reconstruct_g's
// parameters of these names.
{
  extern __shared__ __attribute__((aligned(16))) uint2 smem[];
  const int n = 1 << logn, k = 1 << logk, G = 1 << logG;
  const auto pre = geo.prepare();
  const uint64_t pos0 = uint64_t(blockIdx.x) * 4 * G;
  uint2 *S = smem, *D = smem + size_t(n) * G;
  if (scratch) {  // one buffer per block, reused by its payloads in turn
    S = scratch + (uint64_t(blockIdx.y) * gridDim.x + blockIdx.x) * 2 * uint64_t(n) * G;
    D = S + size_t(n) * G;
  }
  for (uint32_t b = blockIdx.y; b < batch; b += gridDim.y) {  // batch may exceed gridDim.y's limit
  if (!geo.on(b)) continue;  // (block-uniform, before the iteration's first barrier)
  const uint64_t pt = pattern ? pattern[b] : b;  // erasure pattern of payload b
  const uint8_t *SH = geo.rows(shards, b, nv);
  const uint8_t *pr = present + pt * n;
  const uint16_t *E = elog + pt * n;
  uint8_t *O = geo.outp(out, b);
  const uint64_t npos = geo.npos(pre, b), sstride = geo.pitch(b);
  __syncthreads();  // the previous payload's readers of S / D are done
  // gather the column, multiply present symbols by the locator (decode_main:174-177)
  for (int e = threadIdx.x; e < n * G; e += blockDim.x) {
    const int g = e & (G - 1), v = e >> logG;
    uint32_t yl = 0, yh = 0;
    if (v < nv && pr[v]) {
      uint32_t xl = 0, xh = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint64_t pos = pos0 + 4 * g + q;
        if (pos < npos) {
          xh |= uint32_t(SH[uint64_t(v) * sstride + 2 * pos]) << (8 * q);
          xl |= uint32_t(SH[uint64_t(v) * sstride + 2 * pos + 1]) << (8 * q);
        }
      }
      Tab T;
      load_tab(t.mtab, mul_index(E[v]), T);
      mul_acc(xl, xh, T, yl, yh);
    }
    S[e] = make_uint2(yl, yh);
  }
  __syncthreads();
  ifft_g(S, logG, logn, 0, t);
  // formal derivative (poly_encoder.hpp:195-215), closed form:
  //   c'[j] = c[j] ^ XOR_{b : bit b of j is 0} c[j | 2^b]
  for (int e = threadIdx.x; e < n * G; e += blockDim.x) {
    const int g = e & (G - 1), j = e >> logG;
    uint2 acc = S[e];
    for (int b = 0; b < logn; ++b)
      if (!(j & (1 << b))) {
        const uint2 o = S[(j | (1 << b)) * G + g];
        acc.x ^= o.x;
        acc.y ^= o.y;
      }
    D[e] = acc;
  }
  __syncthreads();
  fft_g(D, logG, logn, 0, t);
  // erased systematic positions: * locator (decode_main:185-188); present: as received
  for (int e = threadIdx.x; e < k * G; e += blockDim.x) {
    const int g = e & (G - 1), y = e >> logG;
    const bool have = y < nv && pr[y];
    uint32_t xl = 0, xh = 0;
    if (have) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint64_t pos = pos0 + 4 * g + q;
        if (pos < npos) {
          xh |= uint32_t(SH[uint64_t(y) * sstride + 2 * pos]) << (8 * q);
          xl |= uint32_t(SH[uint64_t(y) * sstride + 2 * pos + 1]) << (8 * q);
        }
      }
    } else {
      Tab T;
      load_tab(t.mtab, mul_index(E[y]), T);
      const uint2 r = D[e];
      mul_acc(r.x, r.y, T, xl, xh);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t pos = pos0 + 4 * g + q;
      if (pos < npos) {
        O[(pos * k + y) * 2] = uint8_t(xh >> (8 * q));
        O[(pos * k + y) * 2 + 1] = uint8_t(xl >> (8 * q));
      }
    }
  }
  }
}
