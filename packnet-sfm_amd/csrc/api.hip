// api.hip -- error plumbing, build identification and live kernel timing for libpnsfm_hip.so.
#include "pnsfm_common.h"
#include "../../include/pnsfm.h"

#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <cstdlib>
#include <utility>
#include <vector>

namespace pnsfm {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  int e = (int)hipGetLastError();
  if (e != 0) {
    set_error("%s: launch failed: %s", what, hipGetErrorString((hipError_t)e));
    return e;
  }
  return 0;
}

// ---- per-stream scratch ---------------------------------------------------------------------------------------------
// Two-stage reductions (wgrad3's pixel splits, the loss scalars) need a few KB .. tens of MB that live from one kernel to
// the next ON THE SAME STREAM.  The library keeps one grow-only device buffer per (device, stream) -- the null stream's handle is
// the same on every device, so the device is part of the key: stream order already serialises its users, so nothing is
// allocated, freed or synchronised in steady state (hipMallocAsync / hipFreeAsync per call measured -3.3 % on the training
// step: 126.2 -> 121.8 img/s).  This is the ONE place the library owns
// device memory (include/pnsfm.h): a buffer that has to grow is replaced, and the old one -- kernels already enqueued may
// still use it -- is retired behind an event recorded on its stream and freed by a later call once that event has completed
// (growth only happens while the first steps discover the sizes).
struct Scratch { void* p = nullptr; size_t cap = 0; };
struct ScratchKey { int dev; hipStream_t stream; };
static std::mutex g_scratch_mu;
static std::vector<std::pair<ScratchKey, Scratch>> g_scratch;
#ifndef PNSFM_EMU
struct Retired { void* p; hipEvent_t done; int dev; };
static std::vector<Retired> g_retired;
static void scratch_reap(int dev) {      // g_scratch_mu held
  for (size_t i = 0; i < g_retired.size();) {
    if (g_retired[i].dev == dev && hipEventQuery(g_retired[i].done) == hipSuccess) {
      (void)hipEventDestroy(g_retired[i].done);
      (void)hipFree(g_retired[i].p);
      g_retired[i] = g_retired.back();
      g_retired.pop_back();
    } else {
      ++i;
    }
  }
  (void)hipGetLastError();               // hipEventQuery's hipErrorNotReady is not an error of ours
}
#endif

void* scratch_get(hipStream_t stream, size_t bytes) {
  int dev = 0;
#ifndef PNSFM_EMU
  if (hipGetDevice(&dev) != hipSuccess) { set_error("scratch: hipGetDevice failed"); return nullptr; }
  if (stream_capturing(stream)) {
    // Round 4 removed the hipGraph path (whole-step replay measured no faster than eager launches and its capture buffers were the
    // library's only state a graph could dangle on): a two-stage reduction cannot take scratch inside a capture.
    set_error("scratch: the stream is being captured into a hipGraph -- launches that need reduction scratch are not capturable");
    return nullptr;
  }
#endif
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  Scratch* sc = nullptr;
  for (auto& e : g_scratch)
    if (e.first.dev == dev && e.first.stream == stream) { sc = &e.second; break; }
  if (!sc) { g_scratch.emplace_back(ScratchKey{dev, stream}, Scratch()); sc = &g_scratch.back().second; }
  if (bytes > sc->cap) {
    size_t cap = sc->cap ? sc->cap : (size_t)1 << 20;
    while (cap < bytes) cap *= 2;
    void* p = nullptr;
#ifdef PNSFM_EMU
    p = malloc(cap);
    if (p && sc->p) free(sc->p);        // the emulator runs every kernel synchronously: nothing is in flight
#else
    scratch_reap(dev);
    if (hipMalloc(&p, cap) != hipSuccess) p = nullptr;
    if (p && sc->p) {
      Retired r{sc->p, nullptr, dev};
      if (hipEventCreateWithFlags(&r.done, hipEventDisableTiming) == hipSuccess && hipEventRecord(r.done, stream) == hipSuccess)
        g_retired.push_back(r);         // freed by a later scratch_get, once the stream has passed this point
      else
        (void)hipGetLastError();        // cannot track it: keep it alive (a one-off, bounded by the growth steps)
    }
#endif
    if (!p) { set_error("cannot allocate %zu bytes of scratch", cap); return nullptr; }
    sc->p = p;
    sc->cap = cap;
  }
  return sc->p;
}

int block_map_mode() {
  return 2;      // one contiguous range of the operand-sharing logical order per XCD (rounds 2-3's orders 0 / 1 and their A/B switch are gone)
}

int ensure_lds_limit(const void* kernel, unsigned long long* mask, int bytes, const char* what) {
#ifndef PNSFM_EMU
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("%s: hipGetDevice failed", what); return -1; }
  const unsigned long long bit = 1ull << (dev & 63);
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (*mask & bit) return 0;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
    set_error("%s: cannot raise the dynamic LDS limit", what);
    return -1;
  }
  *mask |= bit;
#else
  (void)kernel; (void)mask; (void)bytes; (void)what;
#endif
  return 0;
}

// ---- live timing -------------------------------------------------------------------------------
// bench.py needs the dominant kernel's duration measured "live" with events recorded on the very
// stream the kernel is launched on.  When enabled, each profiled launch records a (start, stop)
// event pair; collect() synchronises on them and adds up hipEventElapsedTime.
#ifndef PNSFM_EMU
struct ProfRec { hipEvent_t a, b; double flops; int meta[9]; };      // meta[8]: which kernel ran (prof_dump's `kernel` column)
static bool g_prof_on = false;
static std::vector<ProfRec> g_recs[2];
static std::vector<hipEvent_t> g_pool;
static std::mutex g_prof_mu;

static hipEvent_t get_event() {
  if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

// true while `stream` is being captured into a hipGraph: nothing that synchronises (autotune timing, profiling events that
// are read back with hipEventElapsedTime) may be enqueued then
bool stream_capturing(hipStream_t stream) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
  return st != hipStreamCaptureStatusNone;
}

void prof_begin(int kind, double flops, hipStream_t stream, const int* meta) {
  if (!g_prof_on || stream_capturing(stream)) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec r;
  r.a = get_event();
  r.b = get_event();
  r.flops = flops;
  for (int i = 0; i < 9; ++i) r.meta[i] = meta ? meta[i] : 0;
  hipEventRecord(r.a, stream);
  g_recs[kind].push_back(r);
}

void prof_end(int kind, hipStream_t stream) {
  if (!g_prof_on || stream_capturing(stream)) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (g_recs[kind].empty()) return;
  hipEventRecord(g_recs[kind].back().b, stream);
}
#else
void prof_begin(int, double, hipStream_t, const int*) {}
void prof_end(int, hipStream_t) {}
bool stream_capturing(hipStream_t) { return false; }
#endif

}  // namespace pnsfm

extern "C" {

int pnsfm_version(void) { return 10; }

const char* pnsfm_last_error(void) { return pnsfm::g_err; }

const char* pnsfm_build_target(void) {
#ifdef PNSFM_EMU
  return "emu";
#else
  return "gfx950";
#endif
}

// Stream fork / join without Python stream objects (round 5): `waiter` will not run anything enqueued after this call before everything
// enqueued on `signaler` so far has finished.  One event record + one stream wait from a per-device ring of timing-less events (an
// event may be re-recorded while an earlier wait on it is still pending: a wait captures the record that precedes it).  The weight
// gradients' side stream forks and joins ~75 times per training step; torch's Stream.wait_stream + the stream context manager cost
// the host ~50 us per fork (profiles/r05_host_profile.txt), this call ~3.
int pnsfm_stream_wait_stream(void* waiter, void* signaler) {
#ifdef PNSFM_EMU
  (void)waiter; (void)signaler;
  return 0;
#else
  if (waiter == signaler) return 0;
  static std::mutex mu;
  static std::vector<std::vector<hipEvent_t>> ring(64);
  static int next[64] = {0};
  // the event must belong to the device that OWNS the streams, which need not be the calling thread's current device (ADVICE r05:
  // FlatAdam or the reducer running under another device guard); a null handle is the legacy default stream of the current device
  // (the device of a stream handle is looked up once and remembered: this call runs ~90 times per training step)
  static std::vector<std::pair<void*, int>> known;
  auto device_of = [&](void* st, int fallback) -> int {
    if (!st) return fallback;
    {
      std::lock_guard<std::mutex> lk(mu);
      for (auto& e : known) if (e.first == st) return e.second;
    }
    int d = -1;
    if (hipStreamGetDevice((hipStream_t)st, &d) != hipSuccess) { (void)hipGetLastError(); return fallback; }
    std::lock_guard<std::mutex> lk(mu);
    if (known.size() >= 64) known.clear();
    known.emplace_back(st, d);
    return d;
  };
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) { pnsfm::set_error("stream_wait_stream: hipGetDevice failed"); return -1; }
  const int dev = device_of(signaler, cur), dw = device_of(waiter, dev);
  if (dev < 0 || dev >= 64) { pnsfm::set_error("stream_wait_stream: bad device %d", dev); return -1; }
  if (dw != dev) { pnsfm::set_error("stream_wait_stream: the two streams live on different devices (%d, %d)", dw, dev); return -1; }
  struct DevGuard { int prev, now; DevGuard(int p, int n) : prev(p), now(n) { if (p != n) (void)hipSetDevice(n); } ~DevGuard() { if (prev != now) (void)hipSetDevice(prev); } } guard(cur, dev);
  hipEvent_t ev;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto& r = ring[dev];
    if (r.size() < 256) {
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { pnsfm::set_error("stream_wait_stream: hipEventCreate failed"); return -1; }
      r.push_back(ev);
    } else {
      ev = r[next[dev]];
      next[dev] = (next[dev] + 1) % 256;
    }
  }
  if (hipEventRecord(ev, (hipStream_t)signaler) != hipSuccess) { pnsfm::set_error("stream_wait_stream: hipEventRecord failed"); return -1; }
  if (hipStreamWaitEvent((hipStream_t)waiter, ev, 0) != hipSuccess) { pnsfm::set_error("stream_wait_stream: hipStreamWaitEvent failed"); return -1; }
  return 0;
#endif
}

int pnsfm_prof_enable(int on) {
#ifndef PNSFM_EMU
  std::lock_guard<std::mutex> lk(pnsfm::g_prof_mu);
  pnsfm::g_prof_on = on != 0;
#else
  (void)on;
#endif
  return 0;
}

int pnsfm_prof_reset(void) {
#ifndef PNSFM_EMU
  std::lock_guard<std::mutex> lk(pnsfm::g_prof_mu);
  for (int k = 0; k < 2; ++k) {
    for (auto& r : pnsfm::g_recs[k]) {
      hipEventSynchronize(r.b);
      pnsfm::g_pool.push_back(r.a);
      pnsfm::g_pool.push_back(r.b);
    }
    pnsfm::g_recs[k].clear();
  }
#endif
  return 0;
}

int pnsfm_prof_collect(int kind, double* total_ms, double* total_flops, long long* launches) {
  if (kind < 0 || kind > 1) { pnsfm::set_error("prof_collect: bad kind %d", kind); return -1; }
  double ms = 0.0, fl = 0.0;
  long long n = 0;
#ifndef PNSFM_EMU
  std::lock_guard<std::mutex> lk(pnsfm::g_prof_mu);
  for (auto& r : pnsfm::g_recs[kind]) {
    hipEventSynchronize(r.b);
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) { ms += t; fl += r.flops; n++; }
  }
#endif
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = fl;
  if (launches) *launches = n;
  return 0;
}

int pnsfm_prof_dump(const char* path) {
#ifndef PNSFM_EMU
  std::lock_guard<std::mutex> lk(pnsfm::g_prof_mu);
  FILE* f = fopen(path, "w");
  if (!f) { pnsfm::set_error("prof_dump: cannot open %s", path); return -1; }
  // kernel: forward / backward-data (kind 0) = the variant of pnsfm_conv2d_last_config (0-2 f32 stagings, 3-6 split-bf16 plans, 7 ping-pong);
  // weight gradient (kind 1) = 0 generic f32, 2 tap-major f32, 3 split-bf16 one kernel row per workgroup, 4 split-bf16 nine taps
  fprintf(f, "kind,B,Cin,Cout,H,W,ks,split,blocks,ms,gflop,tflops,kernel\n");
  for (int k = 0; k < 2; ++k)
    for (auto& r : pnsfm::g_recs[k]) {
      hipEventSynchronize(r.b);
      float t = 0.f;
      if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) continue;
      fprintf(f, "%d,%d,%d,%d,%d,%d,%d,%d,%d,%.4f,%.3f,%.2f,%d\n", k, r.meta[0], r.meta[1], r.meta[2], r.meta[3], r.meta[4],
              r.meta[5], r.meta[6], r.meta[7], t, r.flops * 1e-9, t > 0 ? r.flops / (t * 1e-3) * 1e-12 : 0.0, r.meta[8]);
    }
  fclose(f);
#else
  (void)path;
#endif
  return 0;
}

}  // extern "C"
