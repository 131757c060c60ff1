// ec_kernels.hpp — launch interface of the HIP kernels (internal, C++).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "gf_field.hpp"
#include "table_images.hpp"  // the image layouts DevTables points to

namespace ecamd {

struct DevTables {
  const uint16_t *skews = nullptr;     // 65535; no kernel reads it (they use mslot)
  const MulTab *mtab = nullptr;        // 65536
  const MulTab *mtab_tin = nullptr;    // 65536, symbols in, tower out
  const MulTab *mtab_tout = nullptr;   // 65536, tower in, symbols out
  const uint8_t *timg_t = nullptr;     // kTabImages x kTabImageBytes, tower images
  const uint8_t *timg_f9 = nullptr;    // kF9Images x kTabImageBytes, F9 variants of tower image 0
  const uint8_t *cimg = nullptr;       // kCImgBytes, the element-indexed compact image
  const MulTab *mslot = nullptr;       // 65535, mslot[i] = mtab[skews[i]]: by skew slot, one load
  const uint8_t *eimg512 = nullptr;    // kEImg512Cosets x kEImg512Bytes, the k = 512 encode's coset images
  const uint8_t *eimg256 = nullptr;    // kEImg256Cosets x kEImg256Bytes, the k = 256 / n = 2048 encode's
};

// Completion signal of a per-call C-ABI call fused into its last kernel: when
// the launcher's kernel runs as a single workgroup it stores v to *flag at
// system scope after its own output (fused = true); otherwise the caller
// launches the separate signal kernel (finish_call).
struct HostSig {
  uint32_t *flag = nullptr;
  uint32_t v = 0;
  bool fused = false;
};

// Per (device, kernel), once and thread-safe: raise `fn`'s dynamic-LDS limit
// to `lds_bytes` (if above the 64 KB default) and return the current device's
// CU count in *cus.  The count is handed out only after the attribute call
// succeeded, so no thread launches a kernel whose limit is not set yet; a
// failed call is retried on the next launch (ec_runtime.cpp).
hipError_t prepare_kernel(const void *fn, int lds_bytes, int *cus);

// One batch call's buffers, lengths and pitches: built once where the call
// enters the library and handed down by const reference to the chooser, the
// launcher and the kernel's own launcher.  Plain data; device or (per-call
// paths) pinned host pointers.
struct EncodeCall {
  const uint8_t *payloads;
  size_t plen, pstride, batch;
  uint8_t *shards;
  size_t sstride;
};
// pattern (nullable): payload b's erasure pattern is row pattern[b] of
// present / err_log (NULL: row b)
struct ReconCall {
  const uint8_t *shards;
  size_t slen, sstride;
  const uint8_t *present;
  const uint16_t *err_log;
  const uint32_t *pattern;
  size_t batch;
  uint8_t *out;
  size_t ostride;
};
// A masked encode (ECCR_AMD_encode_missing_batch, the second stage of a
// repair): the encode's record plus the rows to write: payload b writes the
// rows y < n_validators whose byte in row b of present (row pattern[b]) is 0
struct MissingCall {
  EncodeCall enc;
  const uint8_t *present;
  const uint32_t *pattern;
};
struct SysCall {
  const uint8_t *shards;
  size_t slen, sstride, batch;
  uint8_t *out;
  size_t ostride;
};
// a pointer as the choosers look at it: an address, never dereferenced
inline uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

// A dynamic schedule's tile counter: one word on a 256-B block of its own.  The
// whole scratch of the k = 16 .. 1024 fast encodes and of systematic_w
// (optional: a kernel without it runs the static schedule), and the last
// block of the n = 1024 reconstructs' scratch.
constexpr size_t kTileCounterBytes = 256;

// Scratch (global memory) needed by each launch: the tile counter, the
// reconstructs' gather orders, and the generic kernels' transform buffers for
// FFT sizes whose working set does not fit LDS (generic_scratch_bytes: a
// transform of `size` points over `positions` pieces / shard positions per
// payload; 0 for the common sizes).
size_t encode_scratch_bytes(const CodeParams &p, size_t payload_len, size_t batch);
bool encode_scratch_optional(const CodeParams &p);  // only a tile counter: static schedule without it
size_t reconstruct_scratch_bytes(const CodeParams &p, size_t shard_len, size_t batch);
size_t generic_scratch_bytes(uint32_t size, size_t positions, size_t batch);

// The kernel a batch call runs: decided by the code, the lengths, the batch
// and the alignment of every base and pitch, in choose_encode /
// choose_reconstruct / choose_systematic and nowhere else (launch_encode /
// launch_reconstruct / launch_systematic switch on the result).  `invalid`: nothing is launched (an empty call, or a
// packed form whose flattened space passes 2^32: hipErrorInvalidValue).
enum class Kernel {
  invalid,
  encode_k256w,
  encode_k256_packed,  // encode_k256<1024, 2> / encode_k256<2048, 1>
  encode_kw,
  encode_k512w,
  encode_k1024,
  encode_g,
  encode_k256w_missing,
  encode_g_missing,
  reconstruct_n1024x,
  reconstruct_n1024,         // reconstruct_n1024<false>
  reconstruct_n1024_packed,  // reconstruct_n1024<true>
  reconstruct_n4096,
  reconstruct_gen,
  reconstruct_g,
  systematic_w,
  systematic_g,
};
const char *kernel_name(Kernel k);  // the enumerator's name; nullptr for invalid

// Pure host functions: the pointers are only looked at as addresses, no device
// is needed.  recon_overrides(): the experiment switches ECCR_AMD_RECON_WAVES=8
// (waves8: the 8-wave kernel where reconstruct_n1024x applies), =12 (waves12:
// reconstruct_n1024x in its 12-wave form at every size, n1024x_waves) and
// ECCR_AMD_RECON_PACKED=1 (force_packed: reconstruct_n1024 packed at every
// size), read from the environment once per process.
Kernel choose_encode(const CodeParams &p, const EncodeCall &c);
struct ReconOverrides {
  bool waves8 = false, waves12 = false, force_packed = false;
};
const ReconOverrides &recon_overrides();
Kernel choose_reconstruct(const CodeParams &p, const ReconCall &c, const ReconOverrides &o);

hipError_t launch_encode(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                         hipStream_t s, HostSig *sig = nullptr);

// The masked encode.  choose_encode_missing: a pure host
// function like choose_encode: encode_k256w_missing exactly where choose_encode
// picks encode_k256w for the same buffers, encode_g_missing everywhere else
// (invalid where that is invalid).  Scratch, required (no static schedule):
// the tile counter's block, then encode_k256w_missing's row-mask plan
// (n = 1024) or encode_g_missing's transform buffers (generic_scratch_bytes);
// never 0.  The query cannot see the alignments, so it covers both kernels.
Kernel choose_encode_missing(const CodeParams &p, const MissingCall &c);
size_t encode_missing_scratch_bytes(const CodeParams &p, size_t payload_len, size_t batch);
hipError_t launch_encode_missing(const CodeParams &p, const DevTables &t, const MissingCall &c, void *scratch,
                                 hipStream_t s);
hipError_t launch_encode_k256w_missing(const CodeParams &p, const DevTables &t, const MissingCall &c,
                                       void *scratch, hipStream_t s);
// the row-mask plan (row_mask.hip): kRowMaskWords words per payload (n =
// 1024): a 1024-bit mask of the rows to write and a word of phase flags, from
// the payload's row of d_present (row b, or row d_pattern[b]: no other row is read)
constexpr uint32_t kRowMaskWords = 33;
size_t row_mask_plan_bytes(size_t batch);  // a multiple of 256
hipError_t launch_row_mask_plan(const CodeParams &p, const uint8_t *d_present, const uint32_t *d_pattern,
                                size_t batch, uint32_t *plan, hipStream_t s);

// Erasure locators (poly_encoder.hpp:90-116, folded form), one workgroup per
// row of d_present.  d_pattern (nullable): rows b with d_pattern[b] != b are
// skipped (their pattern's leader row holds the locator).
hipError_t launch_error_locator(const CodeParams &p, const uint8_t *d_present, size_t batch,
                                const uint16_t *d_fold, const uint32_t *d_pattern,
                                uint16_t *d_err_log, hipStream_t s);
// Pattern dedup: d_pattern[b] = a row whose erasure
// pattern equals payload b's and which is its own leader, or b itself (a hash
// collision with a different pattern only costs the sharing; ec_amd.h).
// Needs dedup_scratch_bytes(batch); batch < 2^31.
// true if launch_error_locator runs the wave-per-pattern form (64 <= n <= 4096),
// cheap enough that a batch computes every row instead of deduplicating
bool locator_wave_applicable(uint32_t n);
// one-lane kernel storing v to a pinned host word (system scope, release)
hipError_t launch_signal_host(uint32_t *h_flag, uint32_t v, hipStream_t s);
// zeroes `bytes` (a multiple of 4) of tile counters at p in stream order
hipError_t launch_zero_counters(uint32_t *p, size_t bytes, hipStream_t s);
size_t dedup_scratch_bytes(size_t batch);
hipError_t launch_dedup_patterns(const CodeParams &p, const uint8_t *d_present, size_t batch,
                                 uint32_t *d_pattern, void *scratch, hipStream_t s);
// follower rows of d_err_log <- their leader's row
hipError_t launch_broadcast_locators(const CodeParams &p, const uint32_t *d_pattern, size_t batch,
                                     uint16_t *d_err_log, hipStream_t s);

hipError_t launch_reconstruct(const CodeParams &p, const DevTables &t, const ReconCall &c, void *scratch,
                              hipStream_t s);

// The systematic recovery's kernel (a pure host function, like the two above):
// systematic_w (sys_w.hip) for k >= 16 with the shard base and pitch, the out
// base and (batch > 1) the out pitch on 16 B; systematic_g otherwise, and for
// a per-call launch whose single workgroup stores the completion signal itself
// (host_signal: the caller passes a HostSig).
Kernel choose_systematic(const CodeParams &p, const SysCall &c, bool host_signal);
// scratch (nullable: static tile schedule): systematic_w's tile counter,
// systematic_scratch_bytes (kTileCounterBytes from k = 16 on)
size_t systematic_scratch_bytes(const CodeParams &p);
hipError_t launch_systematic(const CodeParams &p, const SysCall &c, void *scratch, hipStream_t s,
                             HostSig *sig = nullptr);
// systematic_w's tile: columns per tile (16384 / min(k, 256)) and the row
// blocks a column tile is walked in (k / 256 above k = 256)
uint32_t systematic_w_cols(const CodeParams &p);
uint32_t systematic_w_row_blocks(const CodeParams &p);
hipError_t launch_systematic_w(const CodeParams &p, const SysCall &c, void *scratch, hipStream_t s);

// the per-call encode of tiny codes (enc_tiny.hip): n <= kTinyMaxN, payload
// <= kTinyBytes and the code's tables carried in the kernel arguments, one workgroup, output rows
// (pitch ostride) written where `out` points (pinned host memory), the
// completion flag stored by the kernel (sig->fused)
constexpr int kTinyMaxN = 16;
constexpr size_t kTinyBytes = 2048;
bool tiny_applicable(const CodeParams &p, size_t plen, size_t ostride);
hipError_t launch_encode_tiny(const CodeParams &p, const DevTables &t, const uint8_t *h_payload, size_t plen,
                              uint8_t *out, size_t ostride, hipStream_t s, HostSig *sig);
// the per-call decode from all k systematic shards of a tiny call (k * slen <=
// kTinyBytes, shards at h_shards with pitch sstride, read on the host into the
// kernel arguments): out = the interleaved payload (pinned), flag by the kernel
bool systematic_tiny_applicable(const CodeParams &p, size_t slen);
hipError_t launch_systematic_tiny(const CodeParams &p, const uint8_t *h_shards, size_t slen, size_t sstride,
                                  uint8_t *out, hipStream_t s, HostSig *sig);
hipError_t warm_encode_tiny(hipStream_t s);  // device set-up: the first launches of the tiny kernels

// k = 256, n = 1024 / 2048 (enc_k256.hip, enc_k256w.hip, enc_kw.hip)
bool k256_applicable(const CodeParams &p);
// tile sizes the choosers test (static_asserts beside the kernels): the
// fewest pieces per payload from which k = 256 runs unpacked (encode_k256w /
// encode_kw<8>), which is also the packed kernel's tile; columns per tile of
// reconstruct_n1024<false>, the fewest columns reconstruct_n1024x takes, and
// the fewest from which it runs its 16-wave form (n1024x_waves: measured; at
// 96 and 144 columns, two and three whole 12-wave tiles, the 12-wave form is
// still the faster one, from 145 on the 16-wave form at every count measured,
// profiles/n1024x16/)
constexpr size_t kK256Tile = 128, kN1024Cols = 32, kN1024xMinCols = 48, kN1024x16MinCols = 145;
// encode_k256_packed (choose_encode): the packed (flattened-piece,
// any-alignment) kernel for small payloads or pitches the unpacked kernels
// cannot take; no scratch (the argument is not looked at)
hipError_t launch_encode_k256(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                              hipStream_t s);
// encode_k256w (n = 1024, unpacked): two 8-wave workgroups per
// CU on the compact image, tiles scheduled dynamically from the tile counter
// in `scratch` (enc_k256w.hip; nullable: static tile schedule)
hipError_t launch_encode_k256w(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                               hipStream_t s);

// specialised kernels (enc_k1024.hip): k = 1024, n = 4096; scratch (nullable)
// the tile counter
bool k1024_applicable(const CodeParams &p);
hipError_t launch_encode_k1024(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                               hipStream_t s);

// k = 512, n = 2048 / 4096 (enc_k512w.hip): two 8-wave workgroups per CU on
// the compact image and the per-coset extension images; scratch (nullable:
// static tile schedule) the tile counter
bool k512w_applicable(const CodeParams &p);
hipError_t launch_encode_k512w(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                               hipStream_t s);

// k = 16 .. 128, n <= 8 k, and k = 256 at n = 2048 (enc_kw.hip): the same
// model on the compact image (+ coset extension tables at k = 256); scratch
// (nullable) the tile counter
bool kw_applicable(const CodeParams &p);
hipError_t launch_encode_kw(const CodeParams &p, const DevTables &t, const EncodeCall &c, void *scratch,
                            hipStream_t s);

// Per-payload gather order of the received rows, present rows first, per
// 1024-row quarter (or the n < 1024 rows; dec_n1024.hip): the scratch of
// reconstruct_n1024, _n4096 and _gen, gather_order_bytes(p, batch)
size_t gather_order_bytes(const CodeParams &p, size_t batch);
hipError_t launch_gather_order(const CodeParams &p, const uint8_t *d_present,
                               const uint16_t *d_err_log, const uint32_t *d_pattern, size_t batch,
                               uint32_t *order, hipStream_t s);

// specialised kernels (dec_n1024.hip); scratch: n1024_scratch_bytes(p, batch)
bool n1024_applicable(const CodeParams &p);
// packed (choose_reconstruct): flattened columns, any even shard pitch and base
hipError_t launch_reconstruct_n1024(const CodeParams &p, const DevTables &t, bool packed, const ReconCall &c,
                                    void *scratch, hipStream_t s);
// reconstruct_n1024x (dec_n1024x.hip) for the unpacked case, in its 12- or
// 16-wave form: n1024x_waves(shard_len), a pure host function.  Every n = 1024
// form takes n1024_scratch_bytes (the gather order + n1024x's tile counter,
// kTileCounterBytes)
int n1024x_waves(size_t slen);
size_t n1024_scratch_bytes(const CodeParams &p, size_t batch);
size_t n1024_tick_offset(const CodeParams &p, size_t batch);
hipError_t launch_reconstruct_n1024x(const CodeParams &p, const DevTables &t, const ReconCall &c, void *scratch,
                                     hipStream_t s);

// specialised kernels (dec_n4096.hip); scratch: n4096_scratch_bytes(p, batch)
bool n4096_applicable(const CodeParams &p);
size_t n4096_scratch_bytes(const CodeParams &p, size_t batch);
hipError_t launch_reconstruct_n4096(const CodeParams &p, const DevTables &t, const ReconCall &c, void *scratch,
                                    hipStream_t s);

// register-blocked reconstruct for 64 <= n <= 1024, 16 <= k <= 512 (dec_gen.hip);
// scratch: gather_order_bytes(p, batch)
bool decgen_applicable(const CodeParams &p);
hipError_t launch_reconstruct_gen(const CodeParams &p, const DevTables &t, const ReconCall &c, void *scratch,
                                  hipStream_t s);

}  // namespace ecamd
