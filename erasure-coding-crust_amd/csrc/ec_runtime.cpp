// ec_runtime.cpp — device table residency, scratch, per-thread contexts.
#include "ec_runtime.hpp"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

namespace ecamd {

// Device memory owned by a DeviceState: freed with a state that is destroyed
// (a failed set-up; a published state never is, see g_dev).
struct HipFree {
  void operator()(void *p) const { (void)hipFree(p); }
};
template <typename T>
using DevPtr = std::unique_ptr<T, HipFree>;

struct DeviceState {
  int id = -1;
  DevPtr<uint16_t> skews;
  DevPtr<MulTab> mtab, mtab_t, mslot;  // mtab_t: mtab_tin, then mtab_tout; mslot: mtab by skew slot
  DevPtr<uint8_t> timg_t, timg_f9, cimg, eimg512, eimg256;
  std::mutex mu;
  std::map<uint32_t, DevPtr<uint16_t>> fold;
  std::mutex scratch_mu;  // held by a ScratchLease
  void *scratch = nullptr;
  size_t scratch_cap = 0;
  hipEvent_t scratch_done = nullptr;  // the last lease's work on its stream
  hipStream_t scratch_stream = nullptr;  // that stream (a HostCtx's)
  bool scratch_used = false;
  std::mutex loc_mu;
  std::list<std::shared_ptr<Locator>> loc;  // most recent first
  unsigned long loc_hits = 0, loc_misses = 0;
  std::mutex ss_mu;
  std::list<std::shared_ptr<StreamScratchEntry>> ss;  // per-stream scratch, most recent first
  std::list<std::shared_ptr<StreamScratchEntry>> ss_dead;  // evicted, freed by drain_dead()
};

// One stream's scratch buffer.  `mu` is held by a StreamScratch lease while
// its caller enqueues.  An evicted entry is never freed by a lease's
// destructor (that could be inside another thread's graph capture, ADVICE
// r04): it waits in DeviceState::ss_dead for drain_dead() (see ec_runtime.hpp).
struct StreamScratchEntry {
  hipStream_t s = nullptr;
  void *p = nullptr;
  size_t cap = 0;
  std::mutex mu;
};

namespace {
thread_local std::string t_err;
std::mutex g_mu;
// never destroyed: its entries own HIP objects, and HIP calls from static
// destructors at process exit can crash or hang; process teardown reclaims them
std::vector<std::unique_ptr<DeviceState>> &g_dev = *new std::vector<std::unique_ptr<DeviceState>>();

// `bytes` of device memory for `owner`, filled from `data` (if any); false (error set) on failure
template <typename T>
bool upload(DevPtr<T> &owner, const void *data, size_t bytes, const char *what) {
  void *p = nullptr;
  if (!hip_check(hipMalloc(&p, bytes), (std::string("hipMalloc(") + what + ")").c_str())) return false;
  owner.reset(static_cast<T *>(p));
  return !data ||
         hip_check(hipMemcpy(p, data, bytes, hipMemcpyHostToDevice), (std::string("upload ") + what).c_str());
}
}  // namespace

void set_error(const std::string &msg) {
  t_err = msg;
  std::fprintf(stderr, "%s\n", msg.c_str());
}
const char *last_error() { return t_err.c_str(); }

DeviceState *device_state() {
  int dev = -1, count = 0;
  // this thread's last device, if still current: no device count, no lock
  // (the per-call C ABI asks this two or three times per call)
  thread_local DeviceState *t_last = nullptr;
  if (t_last && hipGetDevice(&dev) == hipSuccess && dev == t_last->id) return t_last;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    set_error("erasure_coding_crust(amd): no HIP device available (the HIP path is required; "
              "there is no CPU fallback)");
    return nullptr;
  }
  if (!hip_check(hipGetDevice(&dev), "hipGetDevice")) return nullptr;
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_dev.size() < size_t(count)) g_dev.resize(count);
  auto &slot = g_dev[dev];
  if (slot) return t_last = slot.get();
  const Field &f = field();
  auto st = std::make_unique<DeviceState>();
  st->id = dev;
  // the LDS and element-indexed table images (table_images.hpp), then the
  // multiply tables by skew slot (the generic kernels: one load per table)
  const std::vector<uint8_t> cimg = compact_image(f), e256 = eimg256_images(f), e512 = eimg512_images(f),
                             f9 = f9_images(f), tower = tower_images(f);
  const std::vector<MulTab> ms = mslot_tables(f);
  if (cimg.empty() || f9.empty()) {
    set_error("erasure_coding_crust(amd): a table image's constant has no F9 table");
    return nullptr;
  }
  const size_t mtab_bytes = f.mtab.size() * sizeof(MulTab);
  // a failure frees what was uploaded before it (st's members) and leaves the slot empty
  if (!upload(st->skews, f.skews.data(), f.skews.size() * 2, "skews") ||
      !upload(st->mtab, f.mtab.data(), mtab_bytes, "mtab") ||
      !upload(st->cimg, cimg.data(), cimg.size(), "compact image") ||
      !upload(st->eimg256, e256.data(), e256.size(), "k256 coset images") ||
      !upload(st->eimg512, e512.data(), e512.size(), "k512 coset images") ||
      !upload(st->timg_f9, f9.data(), f9.size(), "F9 images") ||
      !upload(st->timg_t, tower.data(), tower.size(), "tower images") ||
      !upload(st->mslot, ms.data(), ms.size() * sizeof(MulTab), "mslot") ||
      !upload(st->mtab_t, nullptr, 2 * mtab_bytes, "tower mtab") ||  // one buffer: mtab_tin, then mtab_tout
      !hip_check(hipMemcpy(st->mtab_t.get(), f.mtab_tin.data(), mtab_bytes, hipMemcpyHostToDevice),
                 "upload mtab_tin") ||
      !hip_check(hipMemcpy(st->mtab_t.get() + f.mtab.size(), f.mtab_tout.data(), mtab_bytes,
                           hipMemcpyHostToDevice),
                 "upload mtab_tout"))
    return nullptr;
  // load the library's code object now (the first kernel launch of a process
  // loads it, ~1 ms): one one-lane launch, so no C-ABI call's timed region
  // (ECCR_Test_MeasurePerformance starts its clock after this) pays it
  uint32_t *warm = nullptr;
  if (hipMalloc(&warm, 64) == hipSuccess) {
    if (launch_signal_host(warm, 1, nullptr) == hipSuccess && warm_encode_tiny(nullptr) == hipSuccess)
      (void)hipDeviceSynchronize();
    (void)hipFree(warm);
  }
  slot = std::move(st);
  return t_last = slot.get();
}

DevTables device_tables(DeviceState *d) {
  DevTables t;
  t.skews = d->skews.get();
  t.mtab = d->mtab.get();
  t.mtab_tin = d->mtab_t.get();
  t.mtab_tout = d->mtab_t.get() + kFieldSize;
  t.timg_t = d->timg_t.get();
  t.timg_f9 = d->timg_f9.get();
  t.cimg = d->cimg.get();
  t.mslot = d->mslot.get();
  t.eimg512 = d->eimg512.get();
  t.eimg256 = d->eimg256.get();
  return t;
}

const uint16_t *device_fold(DeviceState *d, uint32_t n) {
  std::lock_guard<std::mutex> lk(d->mu);
  auto it = d->fold.find(n);
  if (it != d->fold.end()) return it->second.get();
  std::vector<uint16_t> F = field().fold_log_walsh(n);
  DevPtr<uint16_t> p;
  if (!upload(p, F.data(), n * 2, "fold")) return nullptr;
  return (d->fold[n] = std::move(p)).get();
}

hipError_t prepare_kernel(const void *fn, int lds_bytes, int *cus) {
  static std::mutex mu;
  static std::map<std::pair<int, const void *>, bool> prepared;
  static std::map<int, int> cu_count;
  int dev = 0;
  if (const hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  auto c = cu_count.find(dev);
  if (c == cu_count.end()) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    c = cu_count.emplace(dev, n).first;
  }
  bool &done = prepared[{dev, fn}];
  if (!done && lds_bytes >= 65536) {
    // these kernels address their multiply tables by absolute LDS address,
    // assuming their dynamic LDS starts at 0, i.e. no static LDS (lds_tab_at)
    hipFuncAttributes attr{};
    if (const hipError_t e = hipFuncGetAttributes(&attr, fn); e != hipSuccess) return e;
    if (attr.sharedSizeBytes != 0) return hipErrorInvalidKernelFile;
    if (lds_bytes > 65536) {
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
      if (e != hipSuccess) return e;
    }
  }
  done = true;
  *cus = c->second;
  return hipSuccess;
}

namespace {
std::atomic<size_t> g_scratch_limit{0};  // 0 = no limit (ECCR_AMD_set_scratch_limit)
}

void set_scratch_limit(size_t bytes) { g_scratch_limit = bytes; }

ScratchLease::ScratchLease(DeviceState *d, size_t bytes, hipStream_t stream)
    : d_(d), s_(stream), want_(bytes) {
  if (!d || bytes == 0) return;
  const size_t limit = g_scratch_limit;
  if (limit && bytes > limit) {  // as if hipMalloc had failed
    set_error("erasure_coding_crust(amd): scratch of " + std::to_string(bytes) +
              " bytes exceeds the limit set by ECCR_AMD_set_scratch_limit");
    return;
  }
  d->scratch_mu.lock();
  held_ = true;
  if (d->scratch_cap < bytes) {
    if (d->scratch) {
      if (d->scratch_used) (void)hipEventSynchronize(d->scratch_done);
      (void)hipFree(d->scratch);
    }
    d->scratch = nullptr;
    d->scratch_cap = 0;
    if (!hip_check(hipMalloc(&d->scratch, bytes), "hipMalloc(scratch)")) return;
    d->scratch_cap = bytes;
  } else if (d->scratch_used) {
    (void)hipStreamWaitEvent(stream, d->scratch_done, 0);
  }
  p_ = d->scratch;
}

ScratchLease::~ScratchLease() {
  if (!held_) return;
  if (!d_->scratch_done) (void)hipEventCreateWithFlags(&d_->scratch_done, hipEventDisableTiming);
  d_->scratch_used = d_->scratch_done && hipEventRecord(d_->scratch_done, s_) == hipSuccess;
  d_->scratch_stream = s_;
  d_->scratch_mu.unlock();
}

namespace {
// A HostCtx's stream, synchronised, is about to be destroyed: the scratch
// event recorded on it is complete and must not be waited on any more (HIP
// would consult the destroyed stream).  Locator events need nothing: their
// creating call marks them done before it returns (locator_done).
void forget_stream(int dev, hipStream_t s) {
  DeviceState *d = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (dev >= 0 && size_t(dev) < g_dev.size()) d = g_dev[dev].get();
  }
  if (!d) return;
  std::lock_guard<std::mutex> lk(d->scratch_mu);
  if (d->scratch_stream == s) {
    d->scratch_used = false;
    d->scratch_stream = nullptr;
  }
}
}  // namespace

Locator::~Locator() {
  // idle: every holder synchronised its stream before dropping it
  if (ready) (void)hipEventDestroy(ready);
  if (d_present) (void)hipFree(d_present);
  if (d_elog) (void)hipFree(d_elog);
}

std::shared_ptr<const Locator> cached_locator(DeviceState *d, const CodeParams &p,
                                              const std::vector<uint8_t> &present,
                                              hipStream_t stream) {
  // declared first, so destroyed last: an evicted entry still held elsewhere
  // is freed by its last holder, never here under loc_mu
  std::shared_ptr<Locator> evicted;
  std::shared_ptr<Locator> L;
  {
    std::lock_guard<std::mutex> lk(d->loc_mu);
    for (auto it = d->loc.begin(); it != d->loc.end(); ++it)
      if ((*it)->nv == p.nv && (*it)->present == present) {
        std::shared_ptr<Locator> hit = *it;
        d->loc.erase(it);
        d->loc.push_front(hit);
        ++d->loc_hits;
        // not done: the creating call is still in flight (it marks the entry
        // under this lock before returning), so `ready`'s stream is alive
        if (!hit->done && !hip_check(hipStreamWaitEvent(stream, hit->ready, 0), "locator wait")) return nullptr;
        return hit;
      }
    ++d->loc_misses;
    if (d->loc.size() >= kLocatorCache) {
      evicted = std::move(d->loc.back());
      d->loc.pop_back();
      // nobody else holds it (no new holder can appear: it left the list under
      // the lock), so only its own locator kernel may still touch the buffers
      if (evicted.use_count() == 1 && evicted->cap_n >= p.n) L = std::move(evicted);
    }
  }
  const uint16_t *fold = device_fold(d, p.n);
  if (!fold) return nullptr;
  if (L) {
    // nobody holds it, so every call that used it has synchronised its stream
    // (its kernel and the H2D of its key are complete); a fresh event, as the
    // old one may belong to a destroyed stream
    (void)hipEventDestroy(L->ready);
    L->ready = nullptr;
    L->done = false;
    if (!hip_check(hipEventCreateWithFlags(&L->ready, hipEventDisableTiming), "hipEventCreate")) return nullptr;
  } else {
    L = std::make_shared<Locator>();
    L->cap_n = p.n;
    if (!hip_check(hipMalloc(&L->d_present, p.n), "hipMalloc(locator)") ||
        !hip_check(hipMalloc(&L->d_elog, size_t(p.n) * 2), "hipMalloc(locator)") ||
        !hip_check(hipEventCreateWithFlags(&L->ready, hipEventDisableTiming), "hipEventCreate"))
      return nullptr;
  }
  L->nv = p.nv;
  L->present = present;
  if (!hip_check(hipMemcpyAsync(L->d_present, L->present.data(), p.n, hipMemcpyHostToDevice, stream),
              "H2D present") ||
      !hip_check(launch_error_locator(p, L->d_present, 1, fold, nullptr, L->d_elog, stream),
              "error locator launch") ||
      !hip_check(hipEventRecord(L->ready, stream), "hipEventRecord")) {
    (void)hipStreamSynchronize(stream);  // nothing issued above may outlive L
    return nullptr;
  }
  std::lock_guard<std::mutex> lk(d->loc_mu);
  d->loc.push_front(L);
  return L;
}

namespace {
// Frees the evicted entries nobody holds any more, after a device
// synchronisation (their streams may be gone, so the whole device is waited
// for).  Called where waiting is allowed: never while `s` is being captured.
// A device-wide synchronisation (and hipFree) made while ANOTHER thread
// captures a stream in global mode invalidates that capture, so the implicit
// drain at the start of a plain call runs only once kDeadDrain evicted buffers
// have gathered (at most one such drain per kDeadDrain evictions, i.e. only
// when more than 64 streams of a device use the plain calls; ec_amd.h); the
// explicit one (ECCR_AMD_release_stream_scratch) always runs.
constexpr size_t kDeadDrain = 16;
void drain_dead(DeviceState *d, hipStream_t s, bool force) {
  std::list<std::shared_ptr<StreamScratchEntry>> dead;
  {
    std::lock_guard<std::mutex> lk(d->ss_mu);
    if (d->ss_dead.empty() || (!force && d->ss_dead.size() < kDeadDrain)) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return;
    for (auto it = d->ss_dead.begin(); it != d->ss_dead.end();)
      if (it->use_count() == 1) {  // no lease holds it
        dead.push_back(std::move(*it));
        it = d->ss_dead.erase(it);
      } else {
        ++it;
      }
  }
  if (dead.empty()) return;
  (void)hipDeviceSynchronize();
  for (auto &e : dead)
    if (e->p) (void)hipFree(e->p);
}
}  // namespace

StreamScratch::StreamScratch(DeviceState *d, hipStream_t s, size_t bytes) : want_(bytes) {
  if (!d || bytes == 0) return;
  drain_dead(d, s, false);
  const size_t limit = g_scratch_limit;
  if (limit && bytes > limit) {  // as if hipMalloc had failed
    set_error("erasure_coding_crust(amd): scratch of " + std::to_string(bytes) +
              " bytes exceeds the limit set by ECCR_AMD_set_scratch_limit");
    return;
  }
  {
    std::lock_guard<std::mutex> lk(d->ss_mu);
    auto it = d->ss.begin();
    while (it != d->ss.end() && (*it)->s != s) ++it;
    if (it != d->ss.end()) {
      d->ss.splice(d->ss.begin(), d->ss, it);  // most recent first
    } else {
      if (d->ss.size() >= kStreamScratch) {
        d->ss_dead.push_back(std::move(d->ss.back()));  // freed by a later drain_dead()
        d->ss.pop_back();
      }
      auto e = std::make_shared<StreamScratchEntry>();
      e->s = s;
      d->ss.push_front(std::move(e));
    }
    e_ = d->ss.front();
  }
  e_->mu.lock();
  locked_ = true;
  if (e_->cap < bytes) {
    // every earlier holder on this stream has finished enqueueing (they held
    // mu), so once the stream drains nothing reads the smaller buffer
    if (e_->p) {
      if (!hip_check(hipStreamSynchronize(s), "scratch grow sync")) return;
      (void)hipFree(e_->p);
    }
    e_->p = nullptr;
    e_->cap = 0;
    if (!hip_check(hipMalloc(&e_->p, bytes), "hipMalloc(stream scratch)")) return;
    e_->cap = bytes;
  }
  p_ = e_->p;
}

StreamScratch::~StreamScratch() {
  if (locked_) e_->mu.unlock();
}

bool release_stream_scratch(DeviceState *d, hipStream_t s) {
  std::shared_ptr<StreamScratchEntry> e;
  {
    std::lock_guard<std::mutex> lk(d->ss_mu);
    for (auto it = d->ss.begin(); it != d->ss.end(); ++it)
      if ((*it)->s == s) {
        e = std::move(*it);
        d->ss.erase(it);
        break;
      }
  }
  if (!e) return false;
  {
    std::lock_guard<std::mutex> lk(e->mu);  // no caller is enqueueing on it
    if (e.use_count() == 1 && e->p) {       // nobody else can reach it any more
      (void)hipStreamSynchronize(s);
      (void)hipFree(e->p);
      e->p = nullptr;
      e->cap = 0;
    }
  }
  if (e->p) {  // a lease still holds it: freed by a later drain
    std::lock_guard<std::mutex> lk(d->ss_mu);
    d->ss_dead.push_back(std::move(e));
  }
  drain_dead(d, s, true);
  return true;
}

void locator_done(DeviceState *d, const Locator &L) {
  std::lock_guard<std::mutex> lk(d->loc_mu);
  L.done = true;
}

void locator_drop(DeviceState *d, const Locator &L) {
  std::shared_ptr<Locator> gone;  // released after the lock (~Locator frees)
  std::lock_guard<std::mutex> lk(d->loc_mu);
  for (auto it = d->loc.begin(); it != d->loc.end(); ++it)
    if (it->get() == &L) {
      gone = std::move(*it);
      d->loc.erase(it);
      break;
    }
}

void locator_cache_stats(DeviceState *d, unsigned long *hits, unsigned long *misses) {
  std::lock_guard<std::mutex> lk(d->loc_mu);
  if (hits) *hits = d->loc_hits;
  if (misses) *misses = d->loc_misses;
}

HostCtx::~HostCtx() {
  // the thread's work is finished (every C-ABI call synchronises its stream);
  // release on the context's own device
  int cur = -1;
  const bool switched = hipGetDevice(&cur) == hipSuccess && cur != device && device >= 0 &&
                        hipSetDevice(device) == hipSuccess;
  if (stream) {
    (void)hipStreamSynchronize(stream);
    forget_stream(device, stream);
    (void)hipStreamDestroy(stream);
  }
  // here, on the context's device, not in the members' destructors after the switch back
  h_in.release(), h_out.release();
  if (h_flag) (void)hipHostFree(h_flag);
  d_in.release(), d_out.release();
  if (switched) (void)hipSetDevice(cur);
}

HostSig call_signal(HostCtx *c) {
  HostSig s;
  if (!c->h_flag) {
    if (hipHostMalloc(reinterpret_cast<void **>(&c->h_flag), 64, hipHostMallocDefault) != hipSuccess) {
      c->h_flag = nullptr;
      return s;
    }
    // a recycled pinned word may hold any stale value: start from a known one
    __atomic_store_n(c->h_flag, 0u, __ATOMIC_RELEASE);
    c->seq = 0;
  }
  uint32_t v = ++c->seq;
  if (v == 0) v = c->seq = 1;  // (wrap) 0 is the initial value
  s.flag = c->h_flag;
  s.v = v;
  return s;
}

bool finish_call(HostCtx *c, const char *what, const HostSig *sig) {
  const auto sync = [&]() { return hip_check(hipStreamSynchronize(c->stream), what); };
  const HostSig s = sig ? *sig : call_signal(c);
  if (!s.flag) return sync();
  const uint32_t v = s.v;
  if (!s.fused && launch_signal_host(s.flag, v, c->stream) != hipSuccess) return sync();
  // now and then ask the stream for an asynchronous error the spin cannot see
  const bool probe = (v & (kFinishProbeEvery - 1)) == 0;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  for (;;) {
    for (int i = 0; i < 64; ++i)
      if (__atomic_load_n(c->h_flag, __ATOMIC_ACQUIRE) == v) {
        if (!probe) return true;
        const hipError_t e = hipStreamQuery(c->stream);
        return e == hipSuccess || e == hipErrorNotReady || hip_check(e, what);
      }
    if (std::chrono::duration<double, std::micro>(clk::now() - t0).count() > kFinishSpinUs)
      return sync();  // long calls block instead of spinning; errors surface here
  }
}

HostCtx *host_ctx() {
  // destroyed (buffers and stream released) at thread exit or when the
  // thread switches devices
  thread_local std::unique_ptr<HostCtx> ctx;
  DeviceState *d = device_state();
  if (!d) return nullptr;
  if (ctx && ctx->device == d->id) return ctx.get();
  ctx = std::make_unique<HostCtx>();
  ctx->device = d->id;
  if (!hip_check(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking), "hipStreamCreate")) {
    ctx.reset();
    return nullptr;
  }
  return ctx.get();
}

}  // namespace ecamd
