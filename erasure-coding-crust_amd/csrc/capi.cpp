// capi.cpp — the erasure_coding.h C ABI (src/erasure_coding.rs of the
// reference) plus the ec_amd.h device-batch extension, on the HIP path.
//
// Validation order and error mapping follow src/erasure_coding.rs; the codec
// results follow ec-cpp (include/ec-cpp/reed-solomon.hpp).  Deliberate
// divergence: where the Rust layer panics (null/empty payload, null out
// pointers) we return NPRS_RESULT_BAD_PAYLOAD / abort with a message.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <optional>
#include <string>
#include <vector>

#include "../../include/erasure_coding/ec_amd.h"
#include "../../include/erasure_coding/erasure_coding.h"
#include "ec_kernels.hpp"
#include "ec_runtime.hpp"
#include "gf_field.hpp"
#include "ragged.hpp"

using namespace ecamd;

namespace {

struct Workspace {  // caller-owned device scratch (the *_ws batch entry points)
  void *ptr;
  size_t bytes;
};

[[noreturn]] void contract_violation(const char *what) {  // Rust assert! == abort
  std::fprintf(stderr, "erasure_coding_crust(amd): contract violation: %s\n", what);
  std::abort();
}

// src/erasure_coding.rs:70-98 (recovery_threshold + code_params)
NPRSResult params_or_error(unsigned long nv, CodeParams *p) {
  switch (code_params(nv, p)) {
    case ParamError::kTooManyValidators: return result(NPRS_RESULT_TOO_MANY_VALIDATORS);
    case ParamError::kNotEnoughValidators: return result(NPRS_RESULT_NOT_ENOUGH_VALIDATORS);
    default: return result(NPRS_RESULT_OK);
  }
}

// Calls whose input and output together stay below this run the kernel on
// the pinned staging buffers themselves (device-mapped host memory, read and
// written over PCIe): no copy commands, so a small call costs one launch and
// one synchronisation instead of three commands.  Kernel launches acquire
// and release at system scope, so the host's staging writes are seen by the
// kernel and its results by the host after the synchronisation.
constexpr size_t kDirectBytes = size_t(64) << 10;

// host -> device -> host encode of one payload into pinned h_out [nv][dev_pitch(sl)]
bool encode_host(const CodeParams &p, const uint8_t *payload, size_t len, HostCtx *c,
                 size_t *sl_out) {
  DeviceState *d = device_state();
  if (!d) return false;
  const size_t sl = shard_len(p.k, len);
  const size_t dstride = dev_pitch(sl);
  const size_t out_bytes = size_t(p.nv) * dstride;
  if (tiny_applicable(p, len, dstride) && out_bytes <= kDirectBytes) {
    // tiny codes and payloads (enc_tiny.hip): the payload rides in the kernel
    // arguments, the rows go straight to the pinned output
    if (!c->h_out.grow(out_bytes)) return false;
    HostSig sig = call_signal(c);
    if (!hip_check(launch_encode_tiny(p, device_tables(d), payload, len, c->h_out.get(), dstride, c->stream,
                                      &sig),
                   "encode launch") ||
        !finish_call(c, "encode", &sig))
      return false;
    *sl_out = sl;
    return true;
  }
  if (len + out_bytes <= kDirectBytes) {
    if (!c->h_in.grow(len) || !c->h_out.grow(out_bytes))
      return false;
    ScratchLease lease(d, encode_scratch_bytes(p, len, 1), c->stream);
    if (!lease.ok()) return false;
    std::memcpy(c->h_in.get(), payload, len);
    HostSig sig = call_signal(c);  // stored by the encode kernel itself when it can (HostSig)
    const EncodeCall call{c->h_in.get(), len, len, 1, c->h_out.get(), dstride};
    if (!hip_check(launch_encode(p, device_tables(d), call, lease.ptr(), c->stream, &sig), "encode launch") ||
        !finish_call(c, "encode", &sig))
      return false;
    *sl_out = sl;
    return true;
  }
  if (!c->h_in.grow(len) || !c->d_in.grow(len) || !c->h_out.grow(out_bytes) || !c->d_out.grow(out_bytes))
    return false;
  ScratchLease lease(d, encode_scratch_bytes(p, len, 1), c->stream);
  if (!lease.ok()) return false;
  std::memcpy(c->h_in.get(), payload, len);
  const EncodeCall call{c->d_in.get(), len, len, 1, c->d_out.get(), dstride};
  if (!hip_check(hipMemcpyAsync(c->d_in.get(), c->h_in.get(), len, hipMemcpyHostToDevice, c->stream), "H2D") ||
      !hip_check(launch_encode(p, device_tables(d), call, lease.ptr(), c->stream), "encode launch") ||
      !hip_check(hipMemcpyAsync(c->h_out.get(), c->d_out.get(), out_bytes, hipMemcpyDeviceToHost, c->stream),
                 "D2H") ||
      !hip_check(hipStreamSynchronize(c->stream), "encode"))
    return false;
  *sl_out = sl;
  return true;
}

// reconstruct from shards staged in c->h_in ([nv][dev_pitch(sl)], present[] flags) into c->h_out
bool reconstruct_host(const CodeParams &p, const std::vector<uint8_t> &present, size_t sl,
                      HostCtx *c) {
  DeviceState *d = device_state();
  if (!d) return false;
  const size_t out_bytes = sl * p.k, dstride = dev_pitch(sl);
  if (!c->d_in.grow(size_t(p.nv) * dstride) || !c->d_out.grow(out_bytes) || !c->h_out.grow(out_bytes))
    return false;
  bool all_systematic = true;
  for (uint32_t y = 0; y < p.k; ++y) all_systematic &= present[y] != 0;
  // small calls: the kernels read the staged shards and write the payload
  // in pinned host memory (kDirectBytes)
  const bool direct = size_t(p.nv) * dstride + out_bytes <= kDirectBytes;
  const uint8_t *src = direct ? c->h_in.get() : c->d_in.get();
  uint8_t *dst = direct ? c->h_out.get() : c->d_out.get();
  if (!direct && !hip_check(hipMemcpyAsync(c->d_in.get(), c->h_in.get(), size_t(p.nv) * dstride,
                                           hipMemcpyHostToDevice, c->stream),
                            "H2D"))
    return false;
  HostSig sig = direct ? call_signal(c) : HostSig();
  // the tail of every branch: the payload copied back unless direct, then the
  // wait.  Kernels only (direct): the signal-kernel wait; after a D2H copy the
  // copy-to-kernel hand-off makes that slower than waiting on the stream
  // 
  const auto finish = [&](bool launched) {
    return launched &&
           (direct ||
            hip_check(hipMemcpyAsync(c->h_out.get(), c->d_out.get(), out_bytes, hipMemcpyDeviceToHost, c->stream),
                      "D2H")) &&
           (direct ? finish_call(c, "reconstruct", &sig) : hip_check(hipStreamSynchronize(c->stream), "reconstruct"));
  };
  if (all_systematic && direct && systematic_tiny_applicable(p, sl))
    // tiny calls: the k systematic shards ride in the kernel arguments (enc_tiny.hip)
    return finish(
        hip_check(launch_systematic_tiny(p, c->h_in.get(), sl, dstride, dst, c->stream, &sig), "systematic launch"));
  if (all_systematic) {
    // every systematic shard is present: decode == interleave (exact)
    // (one payload: no tile counter, systematic_w's static schedule)
    const SysCall call{src, sl, dstride, 1, dst, out_bytes};
    return finish(hip_check(launch_systematic(p, call, nullptr, c->stream, &sig), "systematic launch"));
  }
  // the pattern's locator: computed once per device, then reused (§8f row 3)
  std::shared_ptr<const Locator> loc = cached_locator(d, p, present, c->stream);
  if (!loc) return false;
  // on every path below `loc` is dropped only after the stream finished (the
  // cache recycles entries nobody holds, and uses an entry's event only
  // while it is not done: ec_runtime.hpp)
  const auto release = [&](bool ok) {
    // a failed synchronisation may mean the locator kernel itself faulted:
    // the entry leaves the cache instead of being marked done, so no later
    // hit skips the event wait and reads d_elog that was never written
    if (!ok && hipStreamSynchronize(c->stream) != hipSuccess) locator_drop(d, *loc);
    else locator_done(d, *loc);
    return ok;
  };
  ScratchLease lease(d, reconstruct_scratch_bytes(p, sl, 1), c->stream);
  if (!lease.ok()) return release(false);
  const ReconCall call{src, sl, dstride, loc->d_present, loc->d_elog, nullptr, 1, dst, out_bytes};
  return release(finish(
      hip_check(launch_reconstruct(p, device_tables(d), call, lease.ptr(), c->stream), "reconstruct launch")));
}

bool take_output(HostCtx *c, size_t bytes, DataBlock *out) {
  uint8_t *buf = static_cast<uint8_t *>(std::malloc(bytes ? bytes : 1));
  if (!buf) return false;
  std::memcpy(buf, c->h_out.get(), bytes);
  out->array = buf;
  out->length = bytes;
  return true;
}

}  // namespace

extern "C" {

NPRSResult ECCR_get_recovery_threshold(unsigned long nv, unsigned long *threshold_out) {
  if (!threshold_out) contract_violation("threshold_out is null");
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag == NPRS_RESULT_OK) *threshold_out = p.threshold;
  return r;
}

void ECCR_deallocate_data_block(DataBlock *data) {
  if (!data || !data->array) contract_violation("deallocate_data_block: null");
  std::free(data->array);
  data->array = nullptr;
  data->length = 0;
}

void ECCR_deallocate_chunk(Chunk *data) {
  if (!data) contract_violation("deallocate_chunk: null");
  ECCR_deallocate_data_block(&data->data);
}

void ECCR_deallocate_chunk_list(ChunksList *list) {
  if (!list || !list->data) contract_violation("deallocate_chunk_list: null");
  for (unsigned long i = 0; i < list->count; ++i) ECCR_deallocate_chunk(&list->data[i]);
  std::free(list->data);
  list->data = nullptr;
  list->count = 0;
}

NPRSResult ECCR_AFFT_Table(uint16_t (*output)[65535]) {
  if (!output) contract_violation("AFFT_Table: null");
  std::memcpy(*output, field().skews.data(), 65535 * sizeof(uint16_t));
  return result(NPRS_RESULT_OK);
}

NPRSResult ECCR_obtain_chunks(unsigned long nv, const DataBlock *message, ChunksList *output) {
  if (!message || !output) contract_violation("obtain_chunks: null argument");
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  if (!message->array || message->length == 0) return result(NPRS_RESULT_BAD_PAYLOAD);
  HostCtx *c = host_ctx();
  size_t sl = 0;
  if (!c || !encode_host(p, message->array, message->length, c, &sl))
    return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
  Chunk *chunks = static_cast<Chunk *>(std::malloc(sizeof(Chunk) * nv));
  if (!chunks) return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
  for (unsigned long v = 0; v < nv; ++v) {
    uint8_t *b = static_cast<uint8_t *>(std::malloc(sl));
    std::memcpy(b, c->h_out.get() + v * dev_pitch(sl), sl);
    chunks[v].data.array = b;
    chunks[v].data.length = sl;
    chunks[v].index = v;
  }
  output->data = chunks;
  output->count = nv;
  return result(NPRS_RESULT_OK);
}

NPRSResult ECCR_reconstruct(unsigned long nv, const ChunksList *input, DataBlock *outdata) {
  if (!outdata || !input || !input->data) contract_violation("reconstruct: null argument");
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  // src/erasure_coding.rs:363-387: first n_validators entries, positional
  std::vector<const Chunk *> slot(nv, nullptr);
  unsigned long sl = 0;
  bool have_len = false;
  const unsigned long take = input->count < nv ? input->count : nv;
  for (unsigned long i = 0; i < take; ++i) {
    const Chunk &ch = input->data[i];
    if (ch.index >= nv) {
      NPRSResult e = result(NPRS_RESULT_CHUNK_INDEX_OUT_OF_BOUNDS);
      e.chunk_index_out_of_bounds.chunk_index = ch.index;
      e.chunk_index_out_of_bounds.n_validators = nv;
      return e;
    }
    if (!ch.data.array || ch.data.length == 0) continue;
    if (!have_len) {
      sl = ch.data.length;
      have_len = true;
    }
    if (sl % 2 != 0) return result(NPRS_RESULT_UNEVEN_LENGTH);
    if (sl != ch.data.length) return result(NPRS_RESULT_NON_UNIFORM_CHUNKS);
    slot[ch.index] = &ch;
  }
  std::vector<uint8_t> present(p.n, 0);
  uint32_t count = 0;
  for (unsigned long v = 0; v < nv; ++v)
    if (slot[v]) {
      present[v] = 1;
      ++count;
    }
  if (count < p.k) return result(NPRS_RESULT_NOT_ENOUGH_CHUNKS);  // reed-solomon.hpp:99-100
  HostCtx *c = host_ctx();
  if (!c || !c->h_in.grow(size_t(nv) * dev_pitch(sl)))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  for (unsigned long v = 0; v < nv; ++v)
    if (slot[v]) std::memcpy(c->h_in.get() + v * dev_pitch(sl), slot[v]->data.array, sl);
  if (!reconstruct_host(p, present, sl, c) || !take_output(c, sl * p.k, outdata))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  return result(NPRS_RESULT_OK);
}

NPRSResult ECCR_reconstruct_from_systematic(unsigned long nv, const ChunksList *input,
                                            DataBlock *outdata) {
  if (!outdata || !input || !input->data) contract_violation("systematic: null argument");
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  // src/erasure_coding.rs:291-312: chunks with index < k, all k required
  std::vector<const Chunk *> slot(p.k, nullptr);
  for (unsigned long i = 0; i < input->count; ++i) {
    const Chunk &ch = input->data[i];
    if (ch.index < p.k) slot[ch.index] = &ch;
  }
  for (uint32_t y = 0; y < p.k; ++y)
    if (!slot[y]) return result(NPRS_RESULT_NOT_ENOUGH_CHUNKS);
  // reed-solomon.hpp:155-165: first shard sets the length; empty -> error
  const unsigned long sl = slot[0]->data.array ? slot[0]->data.length : 0;
  if (sl / 2 == 0) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);  // kEmptyShard
  for (uint32_t y = 0; y < p.k; ++y) {
    const unsigned long l = slot[y]->data.array ? slot[y]->data.length : 0;
    if (l / 2 != sl / 2) return result(NPRS_RESULT_NON_UNIFORM_CHUNKS);
  }
  const size_t used = sl / 2 * 2;
  HostCtx *c = host_ctx();
  DeviceState *d = c ? device_state() : nullptr;
  // rows staged at a 16-B pitch, like every other staged layout (systematic_w's loads)
  const size_t pitch = dev_pitch(used);
  const size_t in_bytes = size_t(p.k) * pitch, out_bytes = used * p.k;
  if (!c || !d || !c->h_in.grow(in_bytes) || !c->h_out.grow(out_bytes) || !c->d_in.grow(in_bytes) ||
      !c->d_out.grow(out_bytes))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  for (uint32_t y = 0; y < p.k; ++y) std::memcpy(c->h_in.get() + y * pitch, slot[y]->data.array, used);
  CodeParams pk = p;
  pk.nv = p.k;  // staged layout holds only the k systematic shards
  if (!hip_check(hipMemcpyAsync(c->d_in.get(), c->h_in.get(), in_bytes, hipMemcpyHostToDevice, c->stream),
                 "H2D") ||
      !hip_check(launch_systematic(pk, SysCall{c->d_in.get(), used, pitch, 1, c->d_out.get(), out_bytes}, nullptr,
                                   c->stream),
                 "systematic launch") ||
      !hip_check(hipMemcpyAsync(c->h_out.get(), c->d_out.get(), out_bytes, hipMemcpyDeviceToHost, c->stream),
                 "D2H") ||
      !hip_check(hipStreamSynchronize(c->stream), "systematic") ||
      !take_output(c, out_bytes, outdata))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  return result(NPRS_RESULT_OK);
}

NPRSResult ECCR_Test_MeasurePerformance(const DataBlock *message, unsigned long nv,
                                        unsigned long *us_enc, unsigned long *us_dec) {
  if (!message) return result(NPRS_RESULT_BAD_PAYLOAD);
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  if (!message->array || message->length == 0) return result(NPRS_RESULT_BAD_PAYLOAD);
  HostCtx *c = host_ctx();
  if (!c) return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
  using clk = std::chrono::steady_clock;
  size_t sl = 0;
  {  // this thread's pinned staging and completion word for the call's size,
     // allocated before the clock starts (a first call otherwise timed the
     // hipHostMalloc), as the reference builds its encoders outside its timed
     // regions (src/erasure_coding.rs:190-207)
    const size_t pitch_bytes = size_t(nv) * dev_pitch(shard_len(p.k, message->length));
    if (!c->h_out.grow(pitch_bytes) || !c->h_in.grow(std::max(pitch_bytes, size_t(message->length))))
      return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
    (void)call_signal(c);
  }
  const auto t0 = clk::now();
  if (!encode_host(p, message->array, message->length, c, &sl))
    return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
  const auto t1 = clk::now();
  // reconstruct from all shards (src/erasure_coding.rs:200-211)
  if (!c->h_in.grow(size_t(nv) * dev_pitch(sl)))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  std::memcpy(c->h_in.get(), c->h_out.get(), size_t(nv) * dev_pitch(sl));
  std::vector<uint8_t> present(p.n, 0);
  for (unsigned long v = 0; v < nv; ++v) present[v] = 1;
  const auto t2 = clk::now();
  if (!reconstruct_host(p, present, sl, c)) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  const auto t3 = clk::now();
  if (us_enc)
    *us_enc = (unsigned long)std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
  if (us_dec)
    *us_dec = (unsigned long)std::chrono::duration_cast<std::chrono::microseconds>(t3 - t2).count();
  return result(NPRS_RESULT_OK);
}

// ------------------------------------------------------------- ec_amd.h --

NPRSResult ECCR_AMD_code_params(unsigned long nv, unsigned long *n, unsigned long *k,
                                unsigned long *thr) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  if (n) *n = p.n;
  if (k) *k = p.k;
  if (thr) *thr = p.threshold;
  return r;
}

unsigned long ECCR_AMD_shard_len(unsigned long nv, unsigned long plen) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk) return 0;
  return shard_len(p.k, plen);
}

int ECCR_AMD_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

NPRSResult ECCR_AMD_init_device(void) {
  return device_state() ? result(NPRS_RESULT_OK) : result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
}

}  // extern "C"

namespace {
// The one test of a caller's workspace: there, large enough, and (align = 256)
// on the alignment every kernel's scratch layout assumes.  What follows from a
// workspace that does not fit differs by call, on purpose:
//
// | call                                | short or NULL workspace  | large enough, not 256-B aligned |
// |-------------------------------------|--------------------------|---------------------------------|
// | encode_batch_ws, optional-counter   | static schedule, OK      | error UNKNOWN_CODE_PARAM (the   |
// |   shapes (encode_scratch_optional)  |                          |   alignment is not part of      |
// |                                     |                          |   "optional": align = 1 there)  |
// | encode_batch_ws, other shapes       | error                    | error                           |
// | reconstruct_batch_ws, and           | error                    | error                           |
// |   error_locator_ws with need > 0    |                          |                                 |
// | systematic_batch_ws                 | static schedule, OK      | static schedule, OK             |
// | ragged *_ws                         | error, before the device | the same                        |
// |                                     |   is touched             |                                 |
bool workspace_fits(const Workspace &ws, size_t need, size_t align = 256) {
  return ws.ptr && ws.bytes >= need && reinterpret_cast<uintptr_t>(ws.ptr) % align == 0;
}

void workspace_error(const Workspace &ws, size_t need, const char *needs) {
  set_error("erasure_coding_crust(amd): workspace of " + std::to_string(ws.bytes) +
            " bytes (256-B aligned required) is below the " + std::to_string(need) + " bytes this " + needs);
}

// Device scratch of one batch call: the caller's workspace (the *_ws entry
// points) or else the scratch private to the call's stream (stream_scratch).
// Either way, once the shape has run once on the stream, the call allocates,
// records and waits on nothing (capturable into a hipGraph), and calls on
// different streams never wait on each other.  `ok` false = too small /
// misaligned workspace or a failed allocation: nothing may be launched.
// Without a workspace the stream's scratch lease is held for the object's
// lifetime, i.e. until the call has enqueued all its kernels (ec_runtime.hpp).
struct BatchScratch {
  void *p = nullptr;
  bool ok = false;
  std::optional<StreamScratch> lease;
  BatchScratch(DeviceState *d, size_t need, hipStream_t s, const Workspace *ws) {
    if (need == 0) {
      ok = true;
    } else if (!ws) {
      lease.emplace(d, s, need);
      p = lease->ptr();
      ok = lease->ok();
    } else if (!workspace_fits(*ws, need)) {
      workspace_error(*ws, need, "shape needs (ECCR_AMD_*_workspace_bytes)");
    } else {
      ok = true;
      p = ws->ptr;
    }
  }
};

// batch > 1 deduplicates patterns only where a locator is expensive (n > 4096:
// the workgroup form); below, every row is computed by the wave form (ec_kernels)
size_t locator_scratch_bytes(const CodeParams &p, size_t batch) {
  return batch <= 1 || locator_wave_applicable(p.n) ? 0
                                                     : (batch * 4 + 255) / 256 * 256 + dedup_scratch_bytes(batch);
}

// What a batch call is refused for before anything else is looked at, one
// predicate per kind: the batch function and the ECCR_AMD_*_kernel diagnostic
// of the kind share it.  NPRS_RESULT_OK: the call is well formed.
NPRSResult_Tag encode_call_tag(const CodeParams &p, const EncodeCall &c) {
  return c.plen == 0 || c.sstride < shard_len(p.k, c.plen) || c.pstride < c.plen ? NPRS_RESULT_BAD_PAYLOAD
                                                                                 : NPRS_RESULT_OK;
}
NPRSResult_Tag recon_call_tag(const CodeParams &p, const ReconCall &c) {
  if (c.slen % 2 != 0) return NPRS_RESULT_UNEVEN_LENGTH;
  return c.sstride < c.slen || c.ostride < c.slen * p.k ? NPRS_RESULT_NON_UNIFORM_CHUNKS : NPRS_RESULT_OK;
}
// (the recovery moves whole symbols: once the pitches are checked against the
// stated length, the call goes on with an odd trailing byte dropped)
NPRSResult_Tag sys_call_tag(const CodeParams &p, SysCall *c) {
  if (c->sstride < c->slen || c->ostride < c->slen / 2 * 2 * p.k) return NPRS_RESULT_NON_UNIFORM_CHUNKS;
  c->slen = c->slen / 2 * 2;
  return NPRS_RESULT_OK;
}

NPRSResult encode_batch(unsigned long nv, const EncodeCall &c, hipStream_t s, const Workspace *ws) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  if (const NPRSResult_Tag t = encode_call_tag(p, c); t != NPRS_RESULT_OK) return result(t);
  DeviceState *d = device_state();
  if (!d) return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
  // a workspace below the queried size (e.g. a size of 0 cached from an older
  // release) runs the shapes whose scratch is only a tile counter on the
  // static schedule: slower, not an error
  const size_t need = encode_scratch_bytes(p, c.plen, c.batch);
  const bool optional = ws && encode_scratch_optional(p) && !workspace_fits(*ws, need, 1);
  BatchScratch sc(d, optional ? 0 : need, s, ws);
  if (!sc.ok) return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
  if (!hip_check(launch_encode(p, device_tables(d), c, sc.p, s), "encode launch"))
    return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
  return result(NPRS_RESULT_OK);
}

NPRSResult error_locator(unsigned long nv, const uint8_t *d_present, unsigned long batch,
                         uint16_t *d_err_log, hipStream_t s, const Workspace *ws) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  DeviceState *d = device_state();
  const uint16_t *fold = d ? device_fold(d, p.n) : nullptr;
  if (!fold) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  if (batch <= 1 || locator_wave_applicable(p.n)) {
    if (!hip_check(launch_error_locator(p, d_present, batch, fold, nullptr, d_err_log, s),
                   "error locator launch"))
      return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
    return result(NPRS_RESULT_OK);
  }
  // one locator per distinct pattern (§8f row 3), then copied to its followers
  if (batch >= (1ul << 31)) return result(NPRS_RESULT_BAD_PAYLOAD);  // uint32 pattern indices
  const size_t pat_bytes = (batch * 4 + 255) / 256 * 256;
  BatchScratch sc(d, locator_scratch_bytes(p, batch), s, ws);
  if (!sc.ok) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  uint32_t *pat = static_cast<uint32_t *>(sc.p);
  void *work = static_cast<uint8_t *>(sc.p) + pat_bytes;
  if (!hip_check(launch_dedup_patterns(p, d_present, batch, pat, work, s), "pattern dedup") ||
      !hip_check(launch_error_locator(p, d_present, batch, fold, pat, d_err_log, s),
                 "error locator launch") ||
      !hip_check(launch_broadcast_locators(p, pat, batch, d_err_log, s), "locator broadcast"))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  return result(NPRS_RESULT_OK);
}

NPRSResult reconstruct_batch(unsigned long nv, const ReconCall &c, hipStream_t s, const Workspace *ws) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  if (const NPRSResult_Tag t = recon_call_tag(p, c); t != NPRS_RESULT_OK) return result(t);
  DeviceState *d = device_state();
  if (!d) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  BatchScratch sc(d, reconstruct_scratch_bytes(p, c.slen, c.batch), s, ws);
  if (!sc.ok) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  if (!hip_check(launch_reconstruct(p, device_tables(d), c, sc.p, s), "reconstruct launch"))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  return result(NPRS_RESULT_OK);
}

// ---- the masked encode and the repair (ec_amd.h "repair").  Like the ragged
// calls they always need scratch and check what the host can see -- NULL
// buffers, the encode's / reconstruct's own predicate, the caller's workspace
// -- before the device is touched: nothing is launched on a refusal.
bool refuse_null(const char *what, std::initializer_list<const void *> bufs) {
  for (const void *b : bufs)
    if (!b) {
      set_error(std::string("erasure_coding_crust(amd): ") + what + ": a NULL buffer");
      return true;
    }
  return false;
}

NPRSResult encode_missing_batch(unsigned long nv, const MissingCall &c, hipStream_t s, const Workspace *ws) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  if (refuse_null("encode_missing_batch", {c.enc.payloads, c.enc.shards, c.present}))
    return result(NPRS_RESULT_BAD_PAYLOAD);
  if (const NPRSResult_Tag t = encode_call_tag(p, c.enc); t != NPRS_RESULT_OK) return result(t);
  if (c.enc.batch == 0) return result(NPRS_RESULT_OK);  // an empty call, as the encode's
  const size_t need = encode_missing_scratch_bytes(p, c.enc.plen, c.enc.batch);
  if (ws && !workspace_fits(*ws, need)) {
    workspace_error(*ws, need, "masked encode needs (ECCR_AMD_encode_missing_workspace_bytes)");
    return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
  }
  DeviceState *d = device_state();
  if (!d) return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
  BatchScratch sc(d, need, s, ws);
  if (!sc.ok || !hip_check(launch_encode_missing(p, device_tables(d), c, sc.p, s), "masked encode launch"))
    return result(NPRS_RESULT_UNKNOWN_CODE_PARAM);
  return result(NPRS_RESULT_OK);
}

// the encode stage of a repair: the reconstruct's output is its payloads
// (shard_len * k bytes each, pitch out_stride), its rows the reconstruct's input
MissingCall repair_encode_call(const CodeParams &p, const ReconCall &c) {
  return {{c.out, c.slen * p.k, c.ostride, c.batch, const_cast<uint8_t *>(c.shards), c.sstride}, c.present, c.pattern};
}
// one workspace for both stages: they are ordered on the stream, and the
// reconstruct's scratch is dead when the masked encode's plan is written
size_t repair_scratch_bytes(const CodeParams &p, size_t slen, size_t batch) {
  const size_t need =
      std::max(reconstruct_scratch_bytes(p, slen, batch), encode_missing_scratch_bytes(p, slen * p.k, batch));
  return (need + 255) / 256 * 256;
}

NPRSResult repair_batch(unsigned long nv, const ReconCall &c, hipStream_t s, const Workspace *ws) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  if (refuse_null("repair_batch", {c.shards, c.present, c.err_log, c.out})) return result(NPRS_RESULT_BAD_PAYLOAD);
  if (const NPRSResult_Tag t = recon_call_tag(p, c); t != NPRS_RESULT_OK) return result(t);
  const MissingCall mc = repair_encode_call(p, c);
  if (const NPRSResult_Tag t = encode_call_tag(p, mc.enc); t != NPRS_RESULT_OK) return result(t);  // shard_len 0
  if (c.batch == 0) return result(NPRS_RESULT_OK);
  const size_t need = repair_scratch_bytes(p, c.slen, c.batch);
  if (ws && !workspace_fits(*ws, need)) {
    workspace_error(*ws, need, "repair needs (ECCR_AMD_repair_workspace_bytes)");
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  }
  DeviceState *d = device_state();
  if (!d) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  BatchScratch sc(d, need, s, ws);
  if (!sc.ok || !hip_check(launch_reconstruct(p, device_tables(d), c, sc.p, s), "repair: reconstruct launch") ||
      !hip_check(launch_encode_missing(p, device_tables(d), mc, sc.p, s), "repair: masked encode launch"))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  return result(NPRS_RESULT_OK);
}

// The scratch is systematic_w's tile counter only: a workspace that does not
// fit (NULL, short or misaligned) runs the static schedule.
NPRSResult systematic_batch(unsigned long nv, SysCall c, hipStream_t s, const Workspace *ws) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  if (const NPRSResult_Tag t = sys_call_tag(p, &c); t != NPRS_RESULT_OK) return result(t);
  DeviceState *d = device_state();
  if (!d) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  const size_t need = choose_systematic(p, c, false) == Kernel::systematic_w ? systematic_scratch_bytes(p) : 0;
  const bool skip = ws && !workspace_fits(*ws, need);
  BatchScratch sc(d, skip ? 0 : need, s, ws);
  if (!sc.ok) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  if (!hip_check(launch_systematic(p, c, sc.p, s), "systematic launch"))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  return result(NPRS_RESULT_OK);
}

// ---- ragged device batches (ragged.hpp).  What the host can see is checked
// here, before anything is launched and before the device is touched; the
// items live on the device and are validated there (the plan kernel).
static_assert(sizeof(ECCR_AMD_RaggedItem) == sizeof(RaggedItem) && sizeof(RaggedItem) == 40, "item layout");

// batch and the stated maximum: a count the 32-bit item indices and tile
// tickets can hold.  tiles_of_max: tiles of the longest item the call allows.
NPRSResult ragged_counts(const char *what, unsigned long batch, unsigned long max_len, size_t tiles_of_max,
                         NPRSResult_Tag empty_tag) {
  if (batch == 0 || batch >= (1ul << 31)) {
    set_error(std::string("erasure_coding_crust(amd): ") + what + ": batch " + std::to_string(batch) +
              " is outside 1 .. 2^31 - 1");
    return result(NPRS_RESULT_BAD_PAYLOAD);
  }
  if (max_len == 0) {
    set_error(std::string("erasure_coding_crust(amd): ") + what + ": a maximum length of 0");
    return result(empty_tag);
  }
  // batch * tiles(max) bounds every ticket; the kernels' grids add a few
  // thousand tickets past the end
  if (tiles_of_max >= (size_t(1) << 32) || size_t(batch) * tiles_of_max + 4096 >= (size_t(1) << 32)) {
    set_error(std::string("erasure_coding_crust(amd): ") + what + ": batch x tiles of the maximum length (" +
              std::to_string(batch) + " x " + std::to_string(tiles_of_max) + ") reaches 2^32");
    return result(NPRS_RESULT_BAD_PAYLOAD);
  }
  return result(NPRS_RESULT_OK);
}

// What tells the three ragged calls apart; ragged_call is the rest.
struct RaggedBuffer {
  const void *ptr = nullptr;
  unsigned align = 1;
  bool required = false;  // NULL refused (the others are nullable)
};
struct RaggedKind {
  const char *what;                    // the call's name in messages
  RaggedBuffer bufs[7];                // its buffers with the alignment each needs (unused slots pass)
  const char *alignment;               // the message's words for those
  size_t tiles_of_max;                 // tile tickets of the longest item the call allows
  NPRSResult_Tag empty_tag, fail_tag;  // a maximum of 0 / a workspace, device or launch failure
  size_t need;                         // workspace bytes (a ragged call always has one: the plan lives in it)
  const char *launching;               // hip_check's words for the launch
};

// The sequence of every ragged call, in this order: NULL buffers, the counts,
// the alignments, the caller's workspace (all without a device: nothing is
// launched on failure), then the device, the scratch and the launch.
template <typename Launch>
NPRSResult ragged_call(const RaggedKind &k, const RaggedCall &c, hipStream_t s, const Workspace *ws, Launch launch) {
  const std::string what = std::string("erasure_coding_crust(amd): ") + k.what;
  for (const RaggedBuffer &b : k.bufs)
    if (b.required && !b.ptr) {
      set_error(what + ": a NULL buffer");
      return result(NPRS_RESULT_BAD_PAYLOAD);
    }
  const NPRSResult r = ragged_counts(k.what, c.batch, c.max_len, k.tiles_of_max, k.empty_tag);
  if (r.tag != NPRS_RESULT_OK) return r;
  for (const RaggedBuffer &b : k.bufs)
    if (reinterpret_cast<uintptr_t>(b.ptr) % b.align != 0) {
      set_error(what + ": " + k.alignment);
      return result(NPRS_RESULT_BAD_PAYLOAD);
    }
  if (ws && !workspace_fits(*ws, k.need)) {
    workspace_error(*ws, k.need, "ragged call needs (ECCR_AMD_*_ragged_workspace_bytes)");
    return result(k.fail_tag);
  }
  DeviceState *d = device_state();
  if (!d) return result(k.fail_tag);
  BatchScratch sc(d, k.need, s, ws);
  if (!sc.ok || !hip_check(launch(d, sc.p), k.launching)) return result(k.fail_tag);
  return result(NPRS_RESULT_OK);
}

NPRSResult encode_ragged(unsigned long nv, const RaggedCall &c, hipStream_t s, const Workspace *ws) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  const size_t tile = ragged_encode_tile(p);
  const RaggedKind k{"encode_ragged",
                     {{c.in, 16, true}, {c.items, 8, true}, {c.out, 16, true}, {c.status, 4, false}},
                     "d_payloads and d_shards must be 16-B aligned, d_items 8-B",
                     (shard_len(p.k, c.max_len) / 2 + tile - 1) / tile,
                     NPRS_RESULT_BAD_PAYLOAD,
                     NPRS_RESULT_UNKNOWN_CODE_PARAM,
                     ragged_encode_workspace_bytes(p, c.batch, c.max_len),
                     "ragged encode launch"};
  return ragged_call(k, c, s, ws,
                     [&](DeviceState *d, void *w) { return launch_encode_ragged(p, device_tables(d), c, w, s); });
}

NPRSResult reconstruct_ragged(unsigned long nv, const RaggedCall &c, hipStream_t s, const Workspace *ws) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  const size_t tile = ragged_reconstruct_tile(p);
  // (the n = 1024 kernel reads a pattern's flag and locator rows with vector loads)
  const RaggedKind k{"reconstruct_ragged",
                     {{c.in, 16, true},
                      {c.items, 8, true},
                      {c.present, 16, true},
                      {c.err_log, 16, true},
                      {c.out, 16, true},
                      {c.pattern, 4, false},
                      {c.status, 4, false}},
                     "d_shards, d_out, d_present and d_err_log must be 16-B aligned, d_items 8-B",
                     (c.max_len / 2 + tile - 1) / tile,
                     NPRS_RESULT_NON_UNIFORM_CHUNKS,
                     NPRS_RESULT_UNKNOWN_RECONSTRUCTION,
                     ragged_reconstruct_workspace_bytes(p, c.batch, c.max_len),
                     "ragged reconstruct launch"};
  return ragged_call(k, c, s, ws,
                     [&](DeviceState *d, void *w) { return launch_reconstruct_ragged(p, device_tables(d), c, w, s); });
}

NPRSResult systematic_ragged(unsigned long nv, const RaggedCall &c, hipStream_t s, const Workspace *ws) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  // tickets: column tiles x systematic_w's row blocks
  const size_t tile = ragged_systematic_tile(p);
  const size_t row_blocks =
      choose_systematic_ragged(p) == RaggedKernel::systematic_w_ragged ? systematic_w_row_blocks(p) : 1;
  const RaggedKind k{"systematic_ragged",
                     {{c.in, 16, true}, {c.items, 8, true}, {c.out, 16, true}, {c.status, 4, false}},
                     "d_shards and d_out must be 16-B aligned, d_items 8-B",
                     (c.max_len / 2 + tile - 1) / tile * row_blocks,
                     NPRS_RESULT_NON_UNIFORM_CHUNKS,
                     NPRS_RESULT_UNKNOWN_RECONSTRUCTION,
                     ragged_systematic_workspace_bytes(p, c.batch),
                     "ragged systematic launch"};
  return ragged_call(k, c, s, ws, [&](DeviceState *, void *w) { return launch_systematic_ragged(p, c, w, s); });
}

// the ABI's item pointer as the library's own type (the same 40 bytes)
const RaggedItem *items_of(const ECCR_AMD_RaggedItem *d_items) {
  return reinterpret_cast<const RaggedItem *>(d_items);
}
}  // namespace

extern "C" {

NPRSResult ECCR_AMD_encode_batch(unsigned long nv, const uint8_t *d_payloads, unsigned long plen,
                                 unsigned long pstride, unsigned long batch, uint8_t *d_shards,
                                 unsigned long sstride, void *stream) {
  return encode_batch(nv, {d_payloads, plen, pstride, batch, d_shards, sstride}, static_cast<hipStream_t>(stream),
                      nullptr);
}

unsigned long ECCR_AMD_encode_workspace_bytes(unsigned long nv, unsigned long plen,
                                              unsigned long batch) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk || plen == 0) return 0;
  return encode_scratch_bytes(p, plen, batch);
}

NPRSResult ECCR_AMD_encode_batch_ws(unsigned long nv, const uint8_t *d_payloads,
                                    unsigned long plen, unsigned long pstride, unsigned long batch,
                                    uint8_t *d_shards, unsigned long sstride, void *d_workspace,
                                    unsigned long workspace_bytes, void *stream) {
  const Workspace ws{d_workspace, workspace_bytes};
  return encode_batch(nv, {d_payloads, plen, pstride, batch, d_shards, sstride}, static_cast<hipStream_t>(stream),
                      &ws);
}

NPRSResult ECCR_AMD_error_locator(unsigned long nv, const uint8_t *d_present, unsigned long batch,
                                  uint16_t *d_err_log, void *stream) {
  return error_locator(nv, d_present, batch, d_err_log, static_cast<hipStream_t>(stream), nullptr);
}

unsigned long ECCR_AMD_error_locator_workspace_bytes(unsigned long nv, unsigned long batch) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk) return 0;
  return locator_scratch_bytes(p, batch);
}

NPRSResult ECCR_AMD_error_locator_ws(unsigned long nv, const uint8_t *d_present,
                                     unsigned long batch, uint16_t *d_err_log, void *d_workspace,
                                     unsigned long workspace_bytes, void *stream) {
  const Workspace ws{d_workspace, workspace_bytes};
  return error_locator(nv, d_present, batch, d_err_log, static_cast<hipStream_t>(stream), &ws);
}

NPRSResult ECCR_AMD_dedup_patterns(unsigned long nv, const uint8_t *d_present, unsigned long batch,
                                   uint32_t *d_pattern, void *stream) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  if (batch >= (1ul << 31)) return result(NPRS_RESULT_BAD_PAYLOAD);  // uint32 pattern indices
  DeviceState *d = device_state();
  if (!d) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  BatchScratch sc(d, dedup_scratch_bytes(batch), s, nullptr);
  if (!sc.ok || !hip_check(launch_dedup_patterns(p, d_present, batch, d_pattern, sc.p, s), "pattern dedup"))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  return result(NPRS_RESULT_OK);
}

NPRSResult ECCR_AMD_error_locator_patterns(unsigned long nv, const uint8_t *d_present,
                                           const uint32_t *d_pattern, unsigned long batch,
                                           uint16_t *d_err_log, void *stream) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  DeviceState *d = device_state();
  const uint16_t *fold = d ? device_fold(d, p.n) : nullptr;
  if (!fold) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  if (!hip_check(launch_error_locator(p, d_present, batch, fold, d_pattern, d_err_log,
                                      static_cast<hipStream_t>(stream)),
                 "error locator launch"))
    return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  return result(NPRS_RESULT_OK);
}

NPRSResult ECCR_AMD_reconstruct_batch_patterns(unsigned long nv, const uint8_t *d_shards,
                                               unsigned long slen, unsigned long sstride,
                                               const uint8_t *d_present, const uint16_t *d_err_log,
                                               const uint32_t *d_pattern, unsigned long batch,
                                               uint8_t *d_out, unsigned long ostride, void *stream) {
  return reconstruct_batch(nv, {d_shards, slen, sstride, d_present, d_err_log, d_pattern, batch, d_out, ostride},
                           static_cast<hipStream_t>(stream), nullptr);
}

unsigned long ECCR_AMD_reconstruct_workspace_bytes(unsigned long nv, unsigned long slen,
                                                   unsigned long batch) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk) return 0;
  return reconstruct_scratch_bytes(p, slen, batch);
}

NPRSResult ECCR_AMD_reconstruct_batch_ws(unsigned long nv, const uint8_t *d_shards,
                                         unsigned long slen, unsigned long sstride,
                                         const uint8_t *d_present, const uint16_t *d_err_log,
                                         const uint32_t *d_pattern, unsigned long batch,
                                         uint8_t *d_out, unsigned long ostride, void *d_workspace,
                                         unsigned long workspace_bytes, void *stream) {
  const Workspace ws{d_workspace, workspace_bytes};
  return reconstruct_batch(nv, {d_shards, slen, sstride, d_present, d_err_log, d_pattern, batch, d_out, ostride},
                           static_cast<hipStream_t>(stream), &ws);
}

NPRSResult ECCR_AMD_reconstruct_batch(unsigned long nv, const uint8_t *d_shards,
                                      unsigned long slen, unsigned long sstride,
                                      const uint8_t *d_present, const uint16_t *d_err_log,
                                      unsigned long batch, uint8_t *d_out,
                                      unsigned long ostride, void *stream) {
  return ECCR_AMD_reconstruct_batch_patterns(nv, d_shards, slen, sstride, d_present, d_err_log,
                                             nullptr, batch, d_out, ostride, stream);
}

const char *ECCR_AMD_encode_kernel(unsigned long nv, const uint8_t *d_payloads, unsigned long plen,
                                   unsigned long pstride, unsigned long batch,
                                   const uint8_t *d_shards, unsigned long sstride) {
  CodeParams p;
  const EncodeCall c{d_payloads, plen, pstride, batch, const_cast<uint8_t *>(d_shards), sstride};
  if (code_params(nv, &p) != ParamError::kOk || encode_call_tag(p, c) != NPRS_RESULT_OK) return nullptr;
  return kernel_name(choose_encode(p, c));
}

const char *ECCR_AMD_reconstruct_kernel(unsigned long nv, const uint8_t *d_shards,
                                        unsigned long slen, unsigned long sstride,
                                        const uint8_t *d_present, const uint16_t *d_err_log,
                                        unsigned long batch, const uint8_t *d_out,
                                        unsigned long ostride) {
  CodeParams p;
  const ReconCall c{d_shards, slen, sstride, d_present, d_err_log, nullptr, batch, const_cast<uint8_t *>(d_out),
                    ostride};
  if (code_params(nv, &p) != ParamError::kOk || recon_call_tag(p, c) != NPRS_RESULT_OK) return nullptr;
  return kernel_name(choose_reconstruct(p, c, recon_overrides()));
}

int ECCR_AMD_reconstruct_n1024x_waves(unsigned long slen) { return n1024x_waves(slen); }

NPRSResult ECCR_AMD_encode_missing_batch(unsigned long nv, const uint8_t *d_payloads, unsigned long plen,
                                         unsigned long pstride, unsigned long batch, uint8_t *d_shards,
                                         unsigned long sstride, const uint8_t *d_present,
                                         const uint32_t *d_pattern, void *stream) {
  return encode_missing_batch(nv, {{d_payloads, plen, pstride, batch, d_shards, sstride}, d_present, d_pattern},
                              static_cast<hipStream_t>(stream), nullptr);
}

NPRSResult ECCR_AMD_encode_missing_batch_ws(unsigned long nv, const uint8_t *d_payloads, unsigned long plen,
                                            unsigned long pstride, unsigned long batch, uint8_t *d_shards,
                                            unsigned long sstride, const uint8_t *d_present,
                                            const uint32_t *d_pattern, void *d_workspace,
                                            unsigned long workspace_bytes, void *stream) {
  const Workspace ws{d_workspace, workspace_bytes};
  return encode_missing_batch(nv, {{d_payloads, plen, pstride, batch, d_shards, sstride}, d_present, d_pattern},
                              static_cast<hipStream_t>(stream), &ws);
}

unsigned long ECCR_AMD_encode_missing_workspace_bytes(unsigned long nv, unsigned long plen, unsigned long batch) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk || plen == 0 || batch == 0) return 0;
  return encode_missing_scratch_bytes(p, plen, batch);
}

const char *ECCR_AMD_encode_missing_kernel(unsigned long nv, const uint8_t *d_payloads, unsigned long plen,
                                           unsigned long pstride, unsigned long batch, const uint8_t *d_shards,
                                           unsigned long sstride) {
  CodeParams p;
  const MissingCall c{{d_payloads, plen, pstride, batch, const_cast<uint8_t *>(d_shards), sstride}, nullptr, nullptr};
  if (code_params(nv, &p) != ParamError::kOk || encode_call_tag(p, c.enc) != NPRS_RESULT_OK) return nullptr;
  return kernel_name(choose_encode_missing(p, c));
}

NPRSResult ECCR_AMD_repair_batch(unsigned long nv, uint8_t *d_shards, unsigned long slen, unsigned long sstride,
                                 const uint8_t *d_present, const uint16_t *d_err_log, const uint32_t *d_pattern,
                                 unsigned long batch, uint8_t *d_out, unsigned long ostride, void *stream) {
  return repair_batch(nv, {d_shards, slen, sstride, d_present, d_err_log, d_pattern, batch, d_out, ostride},
                      static_cast<hipStream_t>(stream), nullptr);
}

NPRSResult ECCR_AMD_repair_batch_ws(unsigned long nv, uint8_t *d_shards, unsigned long slen, unsigned long sstride,
                                    const uint8_t *d_present, const uint16_t *d_err_log, const uint32_t *d_pattern,
                                    unsigned long batch, uint8_t *d_out, unsigned long ostride, void *d_workspace,
                                    unsigned long workspace_bytes, void *stream) {
  const Workspace ws{d_workspace, workspace_bytes};
  return repair_batch(nv, {d_shards, slen, sstride, d_present, d_err_log, d_pattern, batch, d_out, ostride},
                      static_cast<hipStream_t>(stream), &ws);
}

unsigned long ECCR_AMD_repair_workspace_bytes(unsigned long nv, unsigned long slen, unsigned long batch) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk || slen == 0 || slen % 2 != 0 || batch == 0) return 0;
  return repair_scratch_bytes(p, slen, batch);
}

NPRSResult ECCR_AMD_locator_cache_stats(unsigned long *hits, unsigned long *misses) {
  DeviceState *d = device_state();
  if (!d) return result(NPRS_RESULT_UNKNOWN_RECONSTRUCTION);
  locator_cache_stats(d, hits, misses);
  return result(NPRS_RESULT_OK);
}

NPRSResult ECCR_AMD_systematic_batch(unsigned long nv, const uint8_t *d_shards, unsigned long slen,
                                     unsigned long sstride, unsigned long batch, uint8_t *d_out,
                                     unsigned long ostride, void *stream) {
  return systematic_batch(nv, {d_shards, slen, sstride, batch, d_out, ostride}, static_cast<hipStream_t>(stream),
                          nullptr);
}

unsigned long ECCR_AMD_systematic_workspace_bytes(unsigned long nv, unsigned long slen, unsigned long batch) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk || slen < 2 || batch == 0) return 0;
  return systematic_scratch_bytes(p);
}

NPRSResult ECCR_AMD_systematic_batch_ws(unsigned long nv, const uint8_t *d_shards, unsigned long slen,
                                        unsigned long sstride, unsigned long batch, uint8_t *d_out,
                                        unsigned long ostride, void *d_workspace, unsigned long workspace_bytes,
                                        void *stream) {
  const Workspace ws{d_workspace, workspace_bytes};
  return systematic_batch(nv, {d_shards, slen, sstride, batch, d_out, ostride}, static_cast<hipStream_t>(stream),
                          &ws);
}

const char *ECCR_AMD_systematic_kernel(unsigned long nv, const uint8_t *d_shards, unsigned long slen,
                                       unsigned long sstride, unsigned long batch, const uint8_t *d_out,
                                       unsigned long ostride) {
  CodeParams p;
  SysCall c{d_shards, slen, sstride, batch, const_cast<uint8_t *>(d_out), ostride};
  if (code_params(nv, &p) != ParamError::kOk || sys_call_tag(p, &c) != NPRS_RESULT_OK) return nullptr;
  return kernel_name(choose_systematic(p, c, false));
}

NPRSResult ECCR_AMD_systematic_ragged(unsigned long nv, const uint8_t *d_shards, const ECCR_AMD_RaggedItem *d_items,
                                      unsigned long batch, unsigned long max_slen, uint8_t *d_out,
                                      uint32_t *d_status, void *stream) {
  return systematic_ragged(nv, {d_shards, items_of(d_items), batch, max_slen, d_out, d_status},
                           static_cast<hipStream_t>(stream), nullptr);
}

NPRSResult ECCR_AMD_systematic_ragged_ws(unsigned long nv, const uint8_t *d_shards,
                                         const ECCR_AMD_RaggedItem *d_items, unsigned long batch,
                                         unsigned long max_slen, uint8_t *d_out, uint32_t *d_status,
                                         void *d_workspace, unsigned long workspace_bytes, void *stream) {
  const Workspace ws{d_workspace, workspace_bytes};
  return systematic_ragged(nv, {d_shards, items_of(d_items), batch, max_slen, d_out, d_status},
                           static_cast<hipStream_t>(stream), &ws);
}

unsigned long ECCR_AMD_systematic_ragged_workspace_bytes(unsigned long nv, unsigned long batch,
                                                         unsigned long max_slen) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk || batch == 0 || batch >= (1ul << 31) || max_slen == 0) return 0;
  return ragged_systematic_workspace_bytes(p, batch);
}

const char *ECCR_AMD_systematic_ragged_kernel(unsigned long nv) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk) return nullptr;
  return ragged_kernel_name(choose_systematic_ragged(p));
}

NPRSResult ECCR_AMD_encode_ragged(unsigned long nv, const uint8_t *d_payloads,
                                  const ECCR_AMD_RaggedItem *d_items, unsigned long batch,
                                  unsigned long max_plen, uint8_t *d_shards, uint32_t *d_status, void *stream) {
  return encode_ragged(nv, {d_payloads, items_of(d_items), batch, max_plen, d_shards, d_status},
                       static_cast<hipStream_t>(stream), nullptr);
}

NPRSResult ECCR_AMD_encode_ragged_ws(unsigned long nv, const uint8_t *d_payloads,
                                     const ECCR_AMD_RaggedItem *d_items, unsigned long batch,
                                     unsigned long max_plen, uint8_t *d_shards, uint32_t *d_status,
                                     void *d_workspace, unsigned long workspace_bytes, void *stream) {
  const Workspace ws{d_workspace, workspace_bytes};
  return encode_ragged(nv, {d_payloads, items_of(d_items), batch, max_plen, d_shards, d_status},
                       static_cast<hipStream_t>(stream), &ws);
}

NPRSResult ECCR_AMD_reconstruct_ragged(unsigned long nv, const uint8_t *d_shards,
                                       const ECCR_AMD_RaggedItem *d_items, const uint8_t *d_present,
                                       const uint16_t *d_err_log, const uint32_t *d_pattern,
                                       unsigned long batch, unsigned long max_slen, uint8_t *d_out,
                                       uint32_t *d_status, void *stream) {
  return reconstruct_ragged(
      nv, {d_shards, items_of(d_items), batch, max_slen, d_out, d_status, d_present, d_err_log, d_pattern},
      static_cast<hipStream_t>(stream), nullptr);
}

NPRSResult ECCR_AMD_reconstruct_ragged_ws(unsigned long nv, const uint8_t *d_shards,
                                          const ECCR_AMD_RaggedItem *d_items, const uint8_t *d_present,
                                          const uint16_t *d_err_log, const uint32_t *d_pattern,
                                          unsigned long batch, unsigned long max_slen, uint8_t *d_out,
                                          uint32_t *d_status, void *d_workspace,
                                          unsigned long workspace_bytes, void *stream) {
  const Workspace ws{d_workspace, workspace_bytes};
  return reconstruct_ragged(
      nv, {d_shards, items_of(d_items), batch, max_slen, d_out, d_status, d_present, d_err_log, d_pattern},
      static_cast<hipStream_t>(stream), &ws);
}

unsigned long ECCR_AMD_encode_ragged_workspace_bytes(unsigned long nv, unsigned long batch,
                                                     unsigned long max_plen) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk || batch == 0 || batch >= (1ul << 31) || max_plen == 0) return 0;
  return ragged_encode_workspace_bytes(p, batch, max_plen);
}

unsigned long ECCR_AMD_reconstruct_ragged_workspace_bytes(unsigned long nv, unsigned long batch,
                                                          unsigned long max_slen) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk || batch == 0 || batch >= (1ul << 31) || max_slen == 0) return 0;
  return ragged_reconstruct_workspace_bytes(p, batch, max_slen);
}

NPRSResult ECCR_AMD_ragged_check(unsigned long nv, const ECCR_AMD_RaggedItem *h_items, unsigned long batch,
                                 unsigned long max_len, int reconstruct, uint32_t status[2]) {
  CodeParams p;
  NPRSResult r = params_or_error(nv, &p);
  if (r.tag != NPRS_RESULT_OK) return r;
  if (!h_items || !status || batch == 0 || batch >= (1ul << 31)) return result(NPRS_RESULT_BAD_PAYLOAD);
  ragged_check_host(p, reinterpret_cast<const RaggedItem *>(h_items), batch, max_len, reconstruct != 0, status);
  return result(NPRS_RESULT_OK);
}

const char *ECCR_AMD_encode_ragged_kernel(unsigned long nv) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk) return nullptr;
  return ragged_kernel_name(choose_encode_ragged(p));
}

const char *ECCR_AMD_reconstruct_ragged_kernel(unsigned long nv) {
  CodeParams p;
  if (code_params(nv, &p) != ParamError::kOk) return nullptr;
  return ragged_kernel_name(choose_reconstruct_ragged(p));
}

void ECCR_AMD_set_scratch_limit(unsigned long bytes) { set_scratch_limit(bytes); }

int ECCR_AMD_release_stream_scratch(void *stream) {
  DeviceState *d = device_state();
  return d && release_stream_scratch(d, static_cast<hipStream_t>(stream)) ? 1 : 0;
}

const char *ECCR_AMD_last_error(void) { return last_error(); }

}  // extern "C"
