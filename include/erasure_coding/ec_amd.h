/*
 * ec_amd.h — MI355X device-resident batch extension of the erasure_coding.h
 * C ABI.  These are NEW symbols (the nine ECCR_* entry points are unchanged).
 *
 * All pointers named d_* are device pointers on the codec's device; `stream`
 * is a hipStream_t (NULL = the legacy default stream).  Calls are asynchronous
 * on `stream` and the caller owns every buffer it passes.  Shapes that need
 * device scratch (k = 1024 encodes, the fast reconstructs' per-payload gather
 * order (4 n bytes per payload; n = 2048 / 4096 add an 80 KB output-table
 * image per payload), n > 4096 generic kernels,
 * ECCR_AMD_error_locator / ECCR_AMD_dedup_patterns with batch > 1) use, in the
 * plain calls, a scratch buffer private to (device, stream): the first call of
 * a larger shape on a stream allocates it (hipMalloc, after synchronising that
 * stream if a smaller one is replaced); afterwards the plain calls allocate,
 * record and wait on nothing, and calls on different streams never wait on
 * each other.  Host threads may issue plain calls on the same stream
 * concurrently: each call holds that stream's scratch until it has enqueued
 * all its kernels, so the calls run one after the other on the stream.  A
 * stream keeps its largest scratch until ECCR_AMD_release_stream_scratch or
 * until more than 64 streams of the device have one: then the least recently
 * used is evicted, and evicted buffers are freed 16 at a time, after a
 * device-wide synchronisation (which waits for work on every stream of the
 * device), at the start of a plain call on a stream that is not being
 * captured.  That synchronisation invalidates a hipGraph capture another
 * thread has open in global mode (hipStreamCaptureModeGlobal) at that moment:
 * programs that capture in global mode while more than 64 streams use the
 * plain calls should release retired streams' scratch with
 * ECCR_AMD_release_stream_scratch (outside any capture), use the *_ws calls,
 * or capture in thread-local / relaxed mode.  The *_ws variants take caller-owned scratch instead (size from
 * the matching *_workspace_bytes query) and never allocate.  Either form can
 * be captured into a hipGraph and replayed once the shape has run once on the
 * stream outside capture (the first call per (device, kernel) also sets a
 * kernel attribute and uploads the tables).  Results are bit-exact with ec-cpp:
 *   encode      == ReedSolomon::encode      (include/ec-cpp/reed-solomon.hpp:47-81)
 *   reconstruct == ReedSolomon::reconstruct (include/ec-cpp/reed-solomon.hpp:83-134)
 *   systematic  == ReedSolomon::reconstruct_from_systematic (:143-179)
 *
 * Layouts (one batch = `batch` independent payloads of the same length; for
 * payloads of unequal length see "ragged batches" below):
 *   payloads   : [batch][payload_stride] bytes, payload_len used
 *   shards     : [batch][n_validators][shard_stride] bytes, shard_len used
 *   present    : [batch][n] bytes, any non-zero byte = shard present, 0 =
 *                erased (indices >= n_validators are always treated as
 *                erased, whatever their bytes)
 *   err_log    : [batch][n] uint16 log-domain erasure-locator multipliers
 *                (poly_encoder.hpp:90-116), produced by ECCR_AMD_error_locator.
 *                The values are logs mod 65535: 0 and 65535 both mean
 *                "multiply by one", a row produced by the locator may hold
 *                either, and the reconstruct calls take both.  Only the
 *                entries of present rows and of erased rows below k enter the
 *                result (decode_main, poly_encoder.hpp:174-188): entries at
 *                erased rows >= k and at rows >= n_validators may hold
 *                anything
 *   out        : [batch][out_stride] bytes, shard_len * k used (zero-padded
 *                past payload_len, as the reference)
 * (tests/test_locator_contract.py pins the present / err_log rules on every
 * reconstruct kernel.)
 */
#ifndef ERASURE_CODING_EC_AMD_H_
#define ERASURE_CODING_EC_AMD_H_

#include "erasure_coding.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Code parameters for n_validators (ec-cpp.cpp:15-37): n = po2 >= nv,
 * k = po2 <= threshold.  Host-only. */
struct NPRSResult ECCR_AMD_code_params(unsigned long n_validators, unsigned long *n,
                                       unsigned long *k, unsigned long *threshold);

/* shard_len(payload_len) = ceil(ceil(len/2)/k)*2 (reed-solomon.hpp:191-196). */
unsigned long ECCR_AMD_shard_len(unsigned long n_validators, unsigned long payload_len);

/* Number of visible HIP devices (0 if none / runtime unusable). */
int ECCR_AMD_device_count(void);

/* Upload field tables and skews to the current device (idempotent). */
struct NPRSResult ECCR_AMD_init_device(void);

/* Device-resident batch encode. */
struct NPRSResult ECCR_AMD_encode_batch(unsigned long n_validators, const uint8_t *d_payloads,
                                        unsigned long payload_len, unsigned long payload_stride,
                                        unsigned long batch, uint8_t *d_shards,
                                        unsigned long shard_stride, void *stream);

/* Erasure-locator multipliers for a batch of erasure patterns, one row of
 * d_err_log per row of d_present.  With batch > 1, equal patterns are found on
 * the device (ECCR_AMD_dedup_patterns) and each distinct one is computed once,
 * then copied to the payloads that share it. */
struct NPRSResult ECCR_AMD_error_locator(unsigned long n_validators, const uint8_t *d_present,
                                         unsigned long batch, uint16_t *d_err_log,
                                         void *stream);

/* Device-resident batch reconstruct (needs ECCR_AMD_error_locator output).
 * The device path does not count shards: a payload with fewer than k present
 * shards yields unspecified bytes (never an out-of-bounds access).  The host
 * entry points (ECCR_reconstruct, ECCR_AMD_reconstruct_host_batch) check the
 * count and return NOT_ENOUGH_CHUNKS.  Missing shards' bytes are never read. */
struct NPRSResult ECCR_AMD_reconstruct_batch(unsigned long n_validators, const uint8_t *d_shards,
                                             unsigned long shard_len, unsigned long shard_stride,
                                             const uint8_t *d_present, const uint16_t *d_err_log,
                                             unsigned long batch, uint8_t *d_out,
                                             unsigned long out_stride, void *stream);

/* ---- caller-owned scratch (graph capture) ---------------------------------
 * Bytes of device scratch the batch calls above need for a shape (0 = none;
 * also 0 for invalid parameters, which the calls themselves report), and the
 * same calls with that scratch passed in: d_workspace 256-B aligned, at least
 * the queried size (else UNKNOWN_* and nothing is launched).  A workspace may
 * be shared by calls that are ordered on one stream.  Encode shapes with
 * k = 16 .. 1024 and n <= 4096 (n_validators 46 .. 4096) query 256 bytes
 * since round 5: a tile counter for their dynamic schedule.  A smaller (or NULL) workspace is accepted for those
 * shapes and runs them on a static schedule (a few percent slower), so a size
 * of 0 cached from an earlier release still works. */
unsigned long ECCR_AMD_encode_workspace_bytes(unsigned long n_validators,
                                              unsigned long payload_len, unsigned long batch);
unsigned long ECCR_AMD_error_locator_workspace_bytes(unsigned long n_validators,
                                                     unsigned long batch);
unsigned long ECCR_AMD_reconstruct_workspace_bytes(unsigned long n_validators,
                                                   unsigned long shard_len, unsigned long batch);
struct NPRSResult ECCR_AMD_encode_batch_ws(unsigned long n_validators, const uint8_t *d_payloads,
                                           unsigned long payload_len, unsigned long payload_stride,
                                           unsigned long batch, uint8_t *d_shards,
                                           unsigned long shard_stride, void *d_workspace,
                                           unsigned long workspace_bytes, void *stream);
struct NPRSResult ECCR_AMD_error_locator_ws(unsigned long n_validators, const uint8_t *d_present,
                                            unsigned long batch, uint16_t *d_err_log,
                                            void *d_workspace, unsigned long workspace_bytes,
                                            void *stream);
/* d_pattern as in ECCR_AMD_reconstruct_batch_patterns (NULL = row b). */
struct NPRSResult ECCR_AMD_reconstruct_batch_ws(
    unsigned long n_validators, const uint8_t *d_shards, unsigned long shard_len,
    unsigned long shard_stride, const uint8_t *d_present, const uint16_t *d_err_log,
    const uint32_t *d_pattern, unsigned long batch, uint8_t *d_out, unsigned long out_stride,
    void *d_workspace, unsigned long workspace_bytes, void *stream);

/* ---- shared erasure patterns ------------------------
 * d_pattern [batch] (uint32): payload b's erasure pattern is row d_pattern[b]
 * of d_present / d_err_log (rows may be shared by any number of payloads;
 * NULL = row b).  The usual case: the same validators missing for every block,
 * i.e. ONE present row and ONE locator for the whole batch. */

/* d_pattern[b] = a row whose pattern (present flags of positions < n_validators)
 * equals payload b's and which is its own leader (d_pattern[l] == l), or b
 * itself; normally the smallest such index (a 64-bit hash collision between
 * different patterns only costs the sharing: each row then leads itself).
 * batch < 2^31 (else BAD_PAYLOAD, nothing launched). */
struct NPRSResult ECCR_AMD_dedup_patterns(unsigned long n_validators, const uint8_t *d_present,
                                          unsigned long batch, uint32_t *d_pattern, void *stream);

/* Locators of the rows b with d_pattern[b] == b only (the other rows of
 * d_err_log are left untouched; d_pattern NULL: every row). */
struct NPRSResult ECCR_AMD_error_locator_patterns(unsigned long n_validators,
                                                  const uint8_t *d_present,
                                                  const uint32_t *d_pattern, unsigned long batch,
                                                  uint16_t *d_err_log, void *stream);

/* ECCR_AMD_reconstruct_batch with payload b's pattern = row d_pattern[b]. */
struct NPRSResult ECCR_AMD_reconstruct_batch_patterns(
    unsigned long n_validators, const uint8_t *d_shards, unsigned long shard_len,
    unsigned long shard_stride, const uint8_t *d_present, const uint16_t *d_err_log,
    const uint32_t *d_pattern, unsigned long batch, uint8_t *d_out, unsigned long out_stride,
    void *stream);

/* ---- ragged batches: payloads of unequal length in one call -----------------
 * The batch calls above take `batch` payloads of one length.  The ragged calls
 * take a device-resident array of `batch` items, one per payload, each with
 * its own length and its own place in the buffers, and run them in one launch
 * whose work queue spans every item: a 15-byte item and a 10 MB item share the
 * launch and finish together.  Results are bit-exact with the uniform calls
 * (and ec-cpp) item by item.
 *
 * Contract, the same for every n_validators: payload_off, shard_off and
 * shard_stride are multiples of 16, the buffers they refer to (d_payloads,
 * d_shards, d_out; for the reconstruct also d_present and d_err_log) are 16-B
 * aligned, d_items is 8-B aligned, and the items' regions do not overlap (not
 * checked).  Lengths are stated per item; the call states their maximum.
 *
 * Validation.  What the host can see is checked on the host before anything is
 * launched, with the usual tags and an ECCR_AMD_last_error text: n_validators;
 * a NULL or misaligned buffer, batch == 0 or >= 2^31, a work-queue size
 * batch x tiles(maximum) that reaches 2^32 (BAD_PAYLOAD; a tile is 64 shard
 * columns of 2 bytes for n_validators 766 .. 1024); a maximum of 0 (BAD_PAYLOAD
 * for the encode, NON_UNIFORM_CHUNKS for the reconstruct).  The items live on
 * the device, so they are checked on the device: an item that breaks the
 * contract -- length 0 or above the stated maximum, odd shard_len,
 * shard_stride below the item's shard length, a field that is no multiple of
 * 16 -- is skipped as a whole: nothing of it is read or written, the other
 * items are unaffected.  d_status (device, uint32_t[2], nullable) receives
 * {number of such items, lowest such index} on every call, {0, 0} when there
 * are none.  ECCR_AMD_ragged_check runs the same test on a host copy.
 *
 * Workspace.  Unlike the uniform encode, a ragged call always needs device
 * scratch (the plan of the call lives in it: 4 bytes per item, plus what the
 * kernel needs).  The plain calls take it from the scratch private to
 * (device, stream), as every plain call does; the _ws calls take the caller's:
 * 256-B aligned, at least ECCR_AMD_*_ragged_workspace_bytes for the same
 * n_validators, batch and maximum, else UNKNOWN_CODE_PARAM (encode) /
 * UNKNOWN_RECONSTRUCTION with nothing launched.  Both forms are asynchronous
 * on `stream`; the _ws forms allocate nothing and, after one warm call, can be
 * captured into a hipGraph: every word of the plan is rebuilt by a kernel on
 * each replay from the item array's contents at that time, so the items may
 * change between replays (same batch and maxima).
 *
 * n_validators 766 .. 1024 run kernels of their own (the uniform calls' fast
 * kernels on the ragged work queue); every other n_validators runs the
 * generic kernels.  Work is handed out in tiles of 64 pieces / columns there,
 * so a batch made of tiny payloads only is better served by the uniform
 * calls, which pick packed kernels for it. */
typedef struct ECCR_AMD_RaggedItem { /* 40 bytes */
  uint64_t payload_off;  /* encode: offset of the payload in d_payloads;
                            reconstruct: offset in d_out where shard_len * k
                            bytes are written (zero-padded, as the reference) */
  uint64_t payload_len;  /* encode: > 0, <= max_payload_len.  reconstruct: ignored */
  uint64_t shard_off;    /* offset in d_shards of this item's
                            [n_validators][shard_stride] rows */
  uint64_t shard_len;    /* reconstruct: even, > 0, <= max_shard_len.  encode:
                            ignored (ECCR_AMD_shard_len(n_validators, payload_len)) */
  uint64_t shard_stride; /* >= the item's shard length */
} ECCR_AMD_RaggedItem;

/* payloads -> shard rows, item by item.  d_status nullable. */
struct NPRSResult ECCR_AMD_encode_ragged(unsigned long n_validators, const uint8_t *d_payloads,
                                         const ECCR_AMD_RaggedItem *d_items, unsigned long batch,
                                         unsigned long max_payload_len, uint8_t *d_shards,
                                         uint32_t *d_status, void *stream);
struct NPRSResult ECCR_AMD_encode_ragged_ws(unsigned long n_validators, const uint8_t *d_payloads,
                                            const ECCR_AMD_RaggedItem *d_items, unsigned long batch,
                                            unsigned long max_payload_len, uint8_t *d_shards,
                                            uint32_t *d_status, void *d_workspace,
                                            unsigned long workspace_bytes, void *stream);

/* shard rows -> shard_len * k output bytes, item by item.  d_present /
 * d_err_log / d_pattern exactly as in ECCR_AMD_reconstruct_batch_ws: row b (or
 * row d_pattern[b]) is item b's erasure pattern and locator, the locator
 * calls above are used as they are.  As there, an item with fewer than k
 * present shards yields unspecified bytes, and missing shards are never read. */
struct NPRSResult ECCR_AMD_reconstruct_ragged(unsigned long n_validators, const uint8_t *d_shards,
                                              const ECCR_AMD_RaggedItem *d_items,
                                              const uint8_t *d_present, const uint16_t *d_err_log,
                                              const uint32_t *d_pattern, unsigned long batch,
                                              unsigned long max_shard_len, uint8_t *d_out,
                                              uint32_t *d_status, void *stream);
struct NPRSResult ECCR_AMD_reconstruct_ragged_ws(unsigned long n_validators, const uint8_t *d_shards,
                                                 const ECCR_AMD_RaggedItem *d_items,
                                                 const uint8_t *d_present, const uint16_t *d_err_log,
                                                 const uint32_t *d_pattern, unsigned long batch,
                                                 unsigned long max_shard_len, uint8_t *d_out,
                                                 uint32_t *d_status, void *d_workspace,
                                                 unsigned long workspace_bytes, void *stream);

/* Workspace of a ragged call in bytes: never 0 for valid parameters, monotone
 * in batch and in the maximum; 0 for invalid ones (n_validators, batch == 0
 * or >= 2^31, a maximum of 0), which the calls themselves report. */
unsigned long ECCR_AMD_encode_ragged_workspace_bytes(unsigned long n_validators, unsigned long batch,
                                                     unsigned long max_payload_len);
unsigned long ECCR_AMD_reconstruct_ragged_workspace_bytes(unsigned long n_validators,
                                                          unsigned long batch,
                                                          unsigned long max_shard_len);

/* The device-side item validation on a host copy of the items (host-only, no
 * device needed): status = {items that break the contract, lowest such index},
 * {0, 0} when there are none.  max_len: max_payload_len (reconstruct == 0) or
 * max_shard_len (reconstruct != 0).  Buffer alignment and overlaps are not its
 * business.  BAD_PAYLOAD for a NULL argument or batch == 0 / >= 2^31. */
struct NPRSResult ECCR_AMD_ragged_check(unsigned long n_validators, const ECCR_AMD_RaggedItem *h_items,
                                        unsigned long batch, unsigned long max_len, int reconstruct,
                                        uint32_t status[2]);

/* The kernel a ragged call launches after its plan kernel (ragged_plan): it
 * depends on n_validators only.  A static string, one of encode_k256w_ragged,
 * encode_g_ragged, reconstruct_n1024x_ragged, reconstruct_g_ragged, or NULL for
 * an invalid n_validators.  Host-only; as ECCR_AMD_encode_kernel below, for
 * tests and triage, not a stable part of the interface. */
const char *ECCR_AMD_encode_ragged_kernel(unsigned long n_validators);
const char *ECCR_AMD_reconstruct_ragged_kernel(unsigned long n_validators);

/* ---- diagnostics ---------------------------------------------------------
 * The name of the kernel ECCR_AMD_encode_batch / ECCR_AMD_reconstruct_batch
 * (and their _ws / _patterns forms) would launch in this process for exactly
 * these arguments: the choice depends on the code, the lengths, the batch and
 * on the alignment of every base and pitch.  A static string, one of
 *   encode_k256w, encode_k256_packed, encode_kw, encode_k512w, encode_k1024,
 *   encode_g, reconstruct_n1024x, reconstruct_n1024, reconstruct_n1024_packed,
 *   reconstruct_n4096, reconstruct_gen, reconstruct_g,
 * or NULL where the call would launch nothing (invalid parameters, an empty
 * batch).  Host-only: no pointer is dereferenced and no device is needed, so
 * made-up addresses may be passed.  For tests and performance triage (a
 * misaligned buffer silently costs a slower kernel); not a stable part of the
 * interface: the names follow the kernels. */
const char *ECCR_AMD_encode_kernel(unsigned long n_validators, const uint8_t *d_payloads,
                                   unsigned long payload_len, unsigned long payload_stride,
                                   unsigned long batch, const uint8_t *d_shards,
                                   unsigned long shard_stride);
const char *ECCR_AMD_reconstruct_kernel(unsigned long n_validators, const uint8_t *d_shards,
                                        unsigned long shard_len, unsigned long shard_stride,
                                        const uint8_t *d_present, const uint16_t *d_err_log,
                                        unsigned long batch, const uint8_t *d_out,
                                        unsigned long out_stride);
/* Waves per workgroup (12 or 16) of reconstruct_n1024x for shards of shard_len
 * bytes, where ECCR_AMD_reconstruct_kernel names that kernel: 16 from 145
 * shard columns (290 bytes) upward, 12 below, and 12 everywhere in a process
 * started with ECCR_AMD_RECON_WAVES=12.  Host-only. */
int ECCR_AMD_reconstruct_n1024x_waves(unsigned long shard_len);

/* Hits / misses of the per-device locator cache of ECCR_reconstruct (the
 * locator of a pattern is computed once and reused while it is among the 64
 * most recent patterns). */
struct NPRSResult ECCR_AMD_locator_cache_stats(unsigned long *hits, unsigned long *misses);

/* Device-resident batch reconstruct_from_systematic (shards 0..k-1 of each
 * payload, same [batch][n_validators][shard_stride] layout): writes
 * shard_len / 2 * 2 * k bytes per payload at d_out + b * out_stride and never
 * a byte outside them.  Rows y >= k are not read.  With k >= 16 and d_shards,
 * shard_stride, d_out and (batch > 1) out_stride on 16 B the call runs the
 * tiled transpose systematic_w, otherwise the element-wise systematic_g
 * (ECCR_AMD_systematic_kernel names the choice); the bytes are the same.
 *
 * Workspace: systematic_w hands out its tiles from a counter.  The plain call
 * keeps it in the scratch private to (device, stream); the _ws form takes the
 * caller's (256-B aligned, ECCR_AMD_systematic_workspace_bytes), allocates
 * nothing and can be captured into a hipGraph.  A NULL, short or misaligned
 * workspace is not an error: the kernel then runs a static tile schedule, as
 * the encode does.  ECCR_AMD_systematic_workspace_bytes is 0 for an invalid
 * n_validators, shard_len < 2 or batch == 0. */
struct NPRSResult ECCR_AMD_systematic_batch(unsigned long n_validators, const uint8_t *d_shards,
                                            unsigned long shard_len, unsigned long shard_stride,
                                            unsigned long batch, uint8_t *d_out,
                                            unsigned long out_stride, void *stream);
unsigned long ECCR_AMD_systematic_workspace_bytes(unsigned long n_validators, unsigned long shard_len,
                                                  unsigned long batch);
struct NPRSResult ECCR_AMD_systematic_batch_ws(unsigned long n_validators, const uint8_t *d_shards,
                                               unsigned long shard_len, unsigned long shard_stride,
                                               unsigned long batch, uint8_t *d_out,
                                               unsigned long out_stride, void *d_workspace,
                                               unsigned long workspace_bytes, void *stream);
/* The kernel ECCR_AMD_systematic_batch (and _ws) would launch for exactly
 * these arguments: systematic_w or systematic_g, NULL where nothing would be
 * launched (invalid parameters, shard_len < 2, an empty batch).  Host-only, as
 * ECCR_AMD_encode_kernel. */
const char *ECCR_AMD_systematic_kernel(unsigned long n_validators, const uint8_t *d_shards,
                                       unsigned long shard_len, unsigned long shard_stride,
                                       unsigned long batch, const uint8_t *d_out,
                                       unsigned long out_stride);

/* The ragged form (see "ragged batches" above): item b's rows y < k at
 * d_shards + shard_off (pitch shard_stride) -> shard_len * k bytes at d_out +
 * payload_off.  The items have the reconstruct's meaning, and so have the
 * contract, the host validation and its tags (NON_UNIFORM_CHUNKS for a maximum
 * of 0, UNKNOWN_RECONSTRUCTION for a bad _ws workspace), d_status and the
 * graph-capture rules; ECCR_AMD_ragged_check(reconstruct = 1) is the item test.
 * An item that breaks the contract is skipped whole.  The work-queue bound of
 * the host validation counts systematic_w's tiles: 16384 / min(k, 256) columns
 * by k / 256 row blocks above k = 256.  k >= 16 runs systematic_w_ragged,
 * smaller k systematic_g_ragged (ECCR_AMD_systematic_ragged_kernel, by
 * n_validators alone; NULL for an invalid n_validators). */
struct NPRSResult ECCR_AMD_systematic_ragged(unsigned long n_validators, const uint8_t *d_shards,
                                             const ECCR_AMD_RaggedItem *d_items, unsigned long batch,
                                             unsigned long max_shard_len, uint8_t *d_out,
                                             uint32_t *d_status, void *stream);
struct NPRSResult ECCR_AMD_systematic_ragged_ws(unsigned long n_validators, const uint8_t *d_shards,
                                                const ECCR_AMD_RaggedItem *d_items, unsigned long batch,
                                                unsigned long max_shard_len, uint8_t *d_out,
                                                uint32_t *d_status, void *d_workspace,
                                                unsigned long workspace_bytes, void *stream);
unsigned long ECCR_AMD_systematic_ragged_workspace_bytes(unsigned long n_validators, unsigned long batch,
                                                         unsigned long max_shard_len);
const char *ECCR_AMD_systematic_ragged_kernel(unsigned long n_validators);

/* ---- repair: regenerate only the missing rows -------------------------------
 * The other half of the codec: from any k present rows the reconstruct gives
 * the payload back; these calls give the missing ROWS back, and only those.
 *
 * ECCR_AMD_encode_missing_batch is the encode under a row mask: it writes the
 * rows y < n_validators of payload b whose byte in its present row (row b of
 * d_present, or row d_pattern[b]; layouts as in ECCR_AMD_reconstruct_batch_ws)
 * is 0.  As there, only the rows the payloads name are read: with d_pattern,
 * d_present (and a repair's d_err_log) may hold fewer rows than the batch, for
 * instance ONE row for every payload.  No other byte of d_shards is written: not a present row, not the
 * bytes between shard_len and shard_stride, not a row at or above
 * n_validators whatever its present byte.  d_shards is never read.  A caller
 * that wants one validator's chunk marks every other row present.
 *
 * ECCR_AMD_repair_batch works in place on a damaged set: it reconstructs the
 * payloads into d_out exactly as ECCR_AMD_reconstruct_batch_ws does (d_err_log
 * from ECCR_AMD_error_locator), then writes the missing rows of d_shards from
 * them (the masked encode with payload_len = shard_len * k and pitch
 * out_stride).  Present rows are read and never written.  d_out is required:
 * the payload is a product of the call.  It must not overlap d_shards (not
 * checked).  With fewer than k present rows the bytes of d_out and of the
 * missing rows are unspecified, and nothing outside them is touched; the
 * device path does not count, as the reconstruct's.
 *
 * Validation.  A NULL buffer (d_pattern excepted) is BAD_PAYLOAD with an
 * ECCR_AMD_last_error text; then the encode's tests (BAD_PAYLOAD) for the
 * masked encode, the reconstruct's (UNEVEN_LENGTH, NON_UNIFORM_CHUNKS; a
 * shard_len of 0: BAD_PAYLOAD) for the repair.  An empty batch is OK and does
 * nothing.
 *
 * Workspace.  Both calls always need device scratch: the tile counter, the
 * masked encode's row-mask plan (132 bytes per payload at
 * n_validators 766 .. 1024) or the generic kernel's transform buffers, and
 * for the repair the reconstruct's.  The plain calls take it from the scratch
 * private to (device, stream), as every plain call does.  The _ws forms take
 * the caller's: 256-B aligned, at least the queried size; a NULL, short or
 * misaligned workspace is UNKNOWN_CODE_PARAM (masked encode) /
 * UNKNOWN_RECONSTRUCTION (repair) with nothing launched and the device not
 * touched: there is no static-schedule fallback.  The two stages of a repair
 * run one after the other on the stream and SHARE the workspace:
 * ECCR_AMD_repair_workspace_bytes is the larger of the two stages' needs, not
 * their sum.  The queries are never 0 for valid parameters, monotone in
 * batch, and 0 for invalid ones (n_validators, an empty batch, a payload_len
 * of 0; for the repair an odd or zero shard_len).  After one warm call the
 * _ws forms can be captured into a hipGraph: every word of the plan is
 * rebuilt and the tile counter zeroed by kernels on each replay, so
 * d_present and d_err_log may change between replays.
 *
 * Kernels.  Where ECCR_AMD_encode_kernel names encode_k256w for the same
 * buffers (n_validators 766 .. 1024, at least 128 pieces of 512 bytes per
 * payload, the alignments of the fast encode), the masked encode runs
 * encode_k256w_missing, which skips the transforms of a coset none of whose
 * rows is wanted; everywhere else it runs encode_g_missing, the generic
 * kernel under the same mask: correct, and slow.
 * ECCR_AMD_encode_missing_kernel names the choice (host-only, as
 * ECCR_AMD_encode_kernel; NULL where nothing would be launched). */
struct NPRSResult ECCR_AMD_encode_missing_batch(unsigned long n_validators, const uint8_t *d_payloads,
                                                unsigned long payload_len, unsigned long payload_stride,
                                                unsigned long batch, uint8_t *d_shards,
                                                unsigned long shard_stride, const uint8_t *d_present,
                                                const uint32_t *d_pattern, void *stream);
struct NPRSResult ECCR_AMD_encode_missing_batch_ws(unsigned long n_validators, const uint8_t *d_payloads,
                                                   unsigned long payload_len, unsigned long payload_stride,
                                                   unsigned long batch, uint8_t *d_shards,
                                                   unsigned long shard_stride, const uint8_t *d_present,
                                                   const uint32_t *d_pattern, void *d_workspace,
                                                   unsigned long workspace_bytes, void *stream);
unsigned long ECCR_AMD_encode_missing_workspace_bytes(unsigned long n_validators, unsigned long payload_len,
                                                      unsigned long batch);
const char *ECCR_AMD_encode_missing_kernel(unsigned long n_validators, const uint8_t *d_payloads,
                                           unsigned long payload_len, unsigned long payload_stride,
                                           unsigned long batch, const uint8_t *d_shards,
                                           unsigned long shard_stride);
struct NPRSResult ECCR_AMD_repair_batch(unsigned long n_validators, uint8_t *d_shards, unsigned long shard_len,
                                        unsigned long shard_stride, const uint8_t *d_present,
                                        const uint16_t *d_err_log, const uint32_t *d_pattern,
                                        unsigned long batch, uint8_t *d_out, unsigned long out_stride,
                                        void *stream);
struct NPRSResult ECCR_AMD_repair_batch_ws(unsigned long n_validators, uint8_t *d_shards,
                                           unsigned long shard_len, unsigned long shard_stride,
                                           const uint8_t *d_present, const uint16_t *d_err_log,
                                           const uint32_t *d_pattern, unsigned long batch, uint8_t *d_out,
                                           unsigned long out_stride, void *d_workspace,
                                           unsigned long workspace_bytes, void *stream);
unsigned long ECCR_AMD_repair_workspace_bytes(unsigned long n_validators, unsigned long shard_len,
                                              unsigned long batch);

/* ---- host-resident batches --------------------------
 * Stream a host batch through the device in chunks of `chunk` payloads (0 =
 * automatic: ~16 MB over the link per chunk), three chunks in flight (H2D /
 * kernels / D2H overlap).  Synchronous:
 * returns when the output is in host memory.  Host buffers should come from
 * ECCR_AMD_host_alloc (pinned) for full PCIe rate. */
void *ECCR_AMD_host_alloc(unsigned long bytes);
void ECCR_AMD_host_free(void *ptr);

/* payloads [batch][payload_stride] -> shards [batch][n_validators][shard_stride] */
struct NPRSResult ECCR_AMD_encode_host_batch(unsigned long n_validators, const uint8_t *h_payloads,
                                             unsigned long payload_len,
                                             unsigned long payload_stride, unsigned long batch,
                                             uint8_t *h_shards, unsigned long shard_stride,
                                             unsigned long chunk);

/* `count` present shards per payload, compacted: h_shards [batch][count][shard_stride]
 * with their validator indices h_index [batch][count] (a repeated index counts
 * once and must carry identical bytes) -> h_out [batch][out_stride >= shard_len*k].
 * Payloads with the same set of indices share one erasure locator per chunk.
 * Errors as ECCR_reconstruct: CHUNK_INDEX_OUT_OF_BOUNDS, NOT_ENOUGH_CHUNKS (< k
 * distinct), UNEVEN_LENGTH. */
struct NPRSResult ECCR_AMD_reconstruct_host_batch(unsigned long n_validators,
                                                  const uint8_t *h_shards, unsigned long shard_len,
                                                  unsigned long shard_stride,
                                                  const uint16_t *h_index, unsigned long count,
                                                  unsigned long batch, uint8_t *h_out,
                                                  unsigned long out_stride, unsigned long chunk);

/* Cap on one scratch allocation in bytes (per device or per stream; 0 = no
 * cap, the default).  A call whose shape needs more fails with UNKNOWN_CODE_PARAM
 * (encode) / UNKNOWN_RECONSTRUCTION (reconstruct) exactly as when hipMalloc
 * runs out of memory; nothing is launched.  Applies to the per-call C ABI
 * and the device-batch calls; the host-batch pipeline's slots own their
 * (chunk-sized) scratch and are not capped.  For memory-constrained
 * deployments and the failure-path tests. */
void ECCR_AMD_set_scratch_limit(unsigned long bytes);

/* Frees the device scratch the plain batch calls keep for `stream` on the
 * current device (after synchronising `stream`); call it before destroying a
 * stream that issued batch calls.  Returns 1 if a buffer was kept, else 0. */
int ECCR_AMD_release_stream_scratch(void *stream);

/* Last error message of the calling thread ("" if none). */
const char *ECCR_AMD_last_error(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* ERASURE_CODING_EC_AMD_H_ */
