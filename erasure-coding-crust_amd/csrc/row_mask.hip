// row_mask.hip — the row-mask plan of the masked encode (enc_k256w_missing.hip,
// DESIGN.md §5.11): one record of kRowMaskWords words per payload, from the
// payload's row of d_present (row b, or row d_pattern[b]: the only rows that
// are read, so a shared-pattern buffer may hold fewer rows than the batch;
// n = 1024 bytes a row): words 0..31 a mask with bit y set iff row y is to be
// written -- y < n_validators and present[y] == 0 -- and word 32 the phase
// flags: bit 0 a row below k = 256 is wanted, bits 1..3 a row of coset 256,
// 512, 768.  Rows at or above n_validators are never wanted, whatever their
// present bytes.  Runs once per call in stream order before the encode and
// writes every word of the plan, so a captured call is replayed with the
// present bytes of that moment.
#include <hip/hip_runtime.h>

#include "ec_kernels.hpp"

namespace ecamd {

// one workgroup of 1024 threads per payload: thread y tests byte y of the
// payload's row, a wave's ballot is two mask words, its flag bit is y >> 8
__global__ void __launch_bounds__(1024) row_mask_plan(const uint8_t *__restrict__ present,
                                                      const uint32_t *__restrict__ pattern, int nv,
                                                      uint32_t *__restrict__ plan) {
  __shared__ uint32_t flags;
  const uint32_t y = threadIdx.x;
  const uint64_t r = blockIdx.x;  // the payload, and its record
  const uint64_t row = pattern ? pattern[r] : r;
  if (y == 0) flags = 0;
  __syncthreads();
  const bool want = int(y) < nv && present[row * 1024 + y] == 0;
  const uint64_t m = __ballot(want);
  if ((y & 63) == 0) {
    plan[r * kRowMaskWords + (y >> 5)] = uint32_t(m);
    plan[r * kRowMaskWords + (y >> 5) + 1] = uint32_t(m >> 32);
    if (m) atomicOr(&flags, 1u << (y >> 8));
  }
  __syncthreads();
  if (y == 0) plan[r * kRowMaskWords + 32] = flags;
}

size_t row_mask_plan_bytes(size_t batch) { return (batch * kRowMaskWords * sizeof(uint32_t) + 255) / 256 * 256; }

hipError_t launch_row_mask_plan(const CodeParams &p, const uint8_t *d_present, const uint32_t *d_pattern,
                                size_t batch, uint32_t *plan, hipStream_t s) {
  if (p.n != 1024 || batch == 0 || batch >= (size_t(1) << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(row_mask_plan, dim3(unsigned(batch)), dim3(1024), 0, s, d_present, d_pattern, int(p.nv),
                     plan);
  return hipGetLastError();
}

}  // namespace ecamd
