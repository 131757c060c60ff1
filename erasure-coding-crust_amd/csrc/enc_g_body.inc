// enc_g_body.inc — the one copy of the generic encode's kernel body
// (reed-solomon.hpp:47-81 + poly_encoder.hpp:31-86,217-240 for 4*G pieces): a
// fragment included inside encode_g and encode_g_ragged (ec_kernels.hip).  A
// textual fragment and not a function template: as a called function the same
// statements compile to a different instruction stream for the uniform kernel.
//
// In scope at the point of inclusion: geo (a geometry policy of
// ec_kernels.hip: prepare(), item(pre, payloads, shards, b, nv) -> EncItemG), payloads, shards,
// nv, logn, logk, logG, batch, t, scratch, sig_flag, sig_v as encode_g's
// parameters of these names.
//
// A policy with MASKED (encode_g_missing) writes only the rows whose byte in
// the payload's present row (enc_g_present) is 0, and skips the FFT of a coset
// none of whose rows is wanted: every `if constexpr (MG)` below, discarded for
// the other policies.
{
  constexpr bool MG = std::decay_t<decltype(geo)>::MASKED;
  extern __shared__ __attribute__((aligned(16))) uint2 smem[];
  const int k = 1 << logk, n = 1 << logn, G = 1 << logG;
  const auto pre = geo.prepare();
  const uint64_t piece0 = uint64_t(blockIdx.x) * 4 * G;
  uint2 *S = smem, *Cf = smem + size_t(k) * G;
  if (scratch) {  // one buffer per block, reused by its payloads in turn
    S = scratch + (uint64_t(blockIdx.y) * gridDim.x + blockIdx.x) * 2 * uint64_t(k) * G;
    Cf = S + size_t(k) * G;
  }
  for (uint32_t b = blockIdx.y; b < batch; b += gridDim.y) {  // batch may exceed gridDim.y's limit
  const EncItemG it = geo.item(pre, payloads, shards, b, nv);
  if (!it.on) continue;  // (block-uniform, before the iteration's first barrier)
  const uint8_t *P = it.P;
  uint8_t *SH = it.SH;
  const uint64_t plen = it.plen, npieces = it.npieces, sstride = it.sstride;
  [[maybe_unused]] const uint8_t *const pr = enc_g_present(geo, b);  // MG: the payload's present row
  // BE-unpack 4 pieces per group, zero-padded (poly_encoder.hpp:53-76); the
  // systematic shards are the data symbols themselves (poly_encoder.hpp:239)
  for (int e = threadIdx.x; e < k * G; e += blockDim.x) {
    const int g = e & (G - 1), i = e >> logG;
    uint32_t xl = 0, xh = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t p = piece0 + 4 * g + q;
      const uint64_t off = p * 2 * uint64_t(k) + 2 * uint64_t(i);
      const uint32_t hi = off < plen ? P[off] : 0;
      const uint32_t lo = off + 1 < plen ? P[off + 1] : 0;
      xl |= lo << (8 * q);
      xh |= hi << (8 * q);
      if (p < npieces) {
        if constexpr (MG) {
          if (i >= nv || pr[i]) continue;
        }
        SH[uint64_t(i) * sstride + 2 * p] = uint8_t(hi);
        SH[uint64_t(i) * sstride + 2 * p + 1] = uint8_t(lo);
      }
    }
    S[e] = make_uint2(xl, xh);
  }
  __syncthreads();
  ifft_g(S, logG, logk, 0, t);
  for (int e = threadIdx.x; e < k * G; e += blockDim.x) Cf[e] = S[e];
  __syncthreads();
  for (int s = k; s < n && s < nv; s += k) {
    if constexpr (MG) {  // block-uniform, before the iteration's barriers
      bool any = false;
      for (int v = s + int(threadIdx.x); v < s + k && v < nv; v += blockDim.x) any |= pr[v] == 0;
      if (!__syncthreads_or(any)) continue;
    }
    if (s > k) {
      for (int e = threadIdx.x; e < k * G; e += blockDim.x) S[e] = Cf[e];
      __syncthreads();
    }
    fft_g(S, logG, logk, uint32_t(s), t);
    for (int e = threadIdx.x; e < k * G; e += blockDim.x) {
      const int g = e & (G - 1), v = s + (e >> logG);
      if (v >= nv) continue;
      if constexpr (MG) {
        if (pr[v]) continue;
      }
      const uint2 x = S[e];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint64_t p = piece0 + 4 * g + q;
        if (p < npieces) {
          SH[uint64_t(v) * sstride + 2 * p] = uint8_t(x.y >> (8 * q));
          SH[uint64_t(v) * sstride + 2 * p + 1] = uint8_t(x.x >> (8 * q));
        }
      }
    }
    __syncthreads();
  }
  }
  signal_end(sig_flag, sig_v);  // (single-workgroup launches only)
}
