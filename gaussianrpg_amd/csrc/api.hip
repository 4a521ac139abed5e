// C ABI of libgrpg_rasterizer.so (include/grpg_rasterizer.h): host orchestration of the HIP
// pipeline.  Mirrors CudaRasterizer::Rasterizer::{forward,backward,markVisible,visible_filter}
// (cuda_rasterizer/rasterizer_impl.cu:197-343, :396-505, :141-153, :345-392).
//
// Forward schedule on the caller's stream:
//   frame init -> preprocess (+ per-workgroup sums of the tile counts) -> count publish (num_rendered
//   and the coarse pair count land in a pinned host word, event) -> depth sort of the (key,id)
//   pairs -> binning (hierarchical: coarse scan / emit / partition / counts / fill; or sort: offsets
//   scan / instance emit / stable tile partition / ranges) -> render (-> semantic render).
// The binning blob is carved for a capacity remembered from earlier frames, every kernel reads the
// instance count from device memory, and the host reads the published count only AFTER the whole
// frame is enqueued (it needs it for the return value): by then the count -- known 70 us into the
// frame -- has arrived, so neither the stream nor the host idles.  First frame of a shape / exact
// mode: read the count first, then carve and enqueue the tail; capacity overflow: redo the tail,
// like the reference's one blocking read (rasterizer_impl.cu:284).
// There is no CPU fallback: without a usable HIP device every entry point fails.
// Only the frame is here.  The entries of the self-contained ops (losses, PSNR, Adam, kNN, sky cube map) sit next to
// their kernels; what they share with this file is declared in abi_util.h and defined below.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <sys/syscall.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <functional>
#include <vector>

#include "../../include/grpg_rasterizer.h"
#include "abi_util.h"
#include "common.h"

using namespace grpg;

// ---- what every entry point shares, the leaf ops' in their own units included (abi_util.h).  Ahead of the unnamed
// namespace, which stays ONE block up to the entries: hipcc numbers the lambdas of namespace-scope initializers per
// block, and the first lambdas of two blocks (g_binning_mode's, g_binning_alg's) would share one name and one body. ----
static thread_local std::string g_last_error;

namespace grpg {

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int ensure_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(GRPG_ERR_NO_DEVICE,
                "no usable HIP device (libgrpg_rasterizer has no CPU fallback by design)");
  return GRPG_OK;
}

int begin_call() {
  g_last_error.clear();
  return ensure_device();
}

int loss_plane_check(const char* what, int height, int width) {
  const bool sides = height > 0 && width > 0;
  if (sides && (long long)height * width <= 0x7FFFFFFFll) return GRPG_OK;
  if (what) g_last_error = std::string(what) + (sides ? ": H*W must be < 2^31" : ": height and width must be positive");
  return GRPG_ERR_INVALID_ARGUMENT;
}

// the one pinned staging ring of optim.hip's and reg_loss.hip's entries (abi_util.h)
constexpr int OPTIM_STAGING_SLOTS = 32;
static thread_local OptimStagingSlot g_optim_staging[OPTIM_STAGING_SLOTS];
static thread_local int g_optim_staging_next = 0;
OptimStagingSlot* optim_staging_acquire(size_t bytes) {
  OptimStagingSlot& b = g_optim_staging[g_optim_staging_next];
  g_optim_staging_next = (g_optim_staging_next + 1) % OPTIM_STAGING_SLOTS;
  if (!b.ev && hipEventCreateWithFlags(&b.ev, hipEventDisableTiming) != hipSuccess) return nullptr;
  if (b.used) (void)hipEventSynchronize(b.ev);
  if (b.bytes < bytes) {
    if (b.host) (void)hipHostFree(b.host);
    b.host = nullptr;
    b.bytes = 0;
    size_t cap = 4096;
    while (cap < bytes) cap *= 2;
    if (hipHostMalloc((void**)&b.host, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
    b.bytes = cap;
  }
  b.used = true;
  return &b;
}

}  // namespace grpg

namespace {

thread_local int g_timing_enabled = 0;   // 0 off, 1 all stages, 2 render stage only

// ---- num_rendered hand-over: pinned, device-mapped host words + one event per (thread, device) ----
struct HostWord {
  int dev = -1;
  uint32_t* host_ptr = nullptr;   // [0] num_rendered, [1] coarse pairs, [3] sticky asynchronous error
  uint32_t* dev_ptr = nullptr;    // the same memory as the device addresses it
  hipEvent_t ev = nullptr;
};
// released when the owning thread exits (as the deferred-frame ring below)
// ... except on the MAIN thread: its thread_local destructors run during process exit, when the HIP
// runtime may already be shutting down (Python finalisation with the torch extension loaded); calling
// into it then is a known source of exit-time errors, and the OS reclaims the memory anyway.
static bool on_main_thread() { return (long)syscall(SYS_gettid) == (long)getpid(); }
struct HostWords : std::vector<HostWord> {
  ~HostWords() {
    if (on_main_thread()) return;
    for (auto& h : *this) {
      if (h.host_ptr) (void)hipHostFree(h.host_ptr);
      if (h.ev) (void)hipEventDestroy(h.ev);
    }
  }
};
thread_local HostWords g_host_words;

HostWord* host_word() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  for (auto& h : g_host_words)
    if (h.dev == dev) return &h;
  HostWord h;
  h.dev = dev;
  if (hipHostMalloc((void**)&h.host_ptr, 64, hipHostMallocMapped) != hipSuccess) return nullptr;
  if (hipHostGetDevicePointer((void**)&h.dev_ptr, h.host_ptr, 0) != hipSuccess ||
      hipEventCreateWithFlags(&h.ev, hipEventDisableTiming) != hipSuccess) {
    (void)hipHostFree(h.host_ptr);
    return nullptr;
  }
  h.host_ptr[0] = 0u; h.host_ptr[1] = 0u; h.host_ptr[2] = 0u; h.host_ptr[3] = 0u;
  g_host_words.push_back(h);
  return &g_host_words.back();
}

// ---- capacity hints: high-water mark of num_rendered per (device, P, W, H), process-wide ----
struct CapKey { int dev, P, W, H; };

// ---- deferred frames (grpg_forward_deferred / grpg_frame_status): the count of a frame lands in
// its own pinned words; nobody waits for it until its status is asked for.  A ring per thread;
// a slot that comes round again while still pending is resolved first. ----
struct DeferSlot {
  int dev = -1;
  uint32_t* host_ptr = nullptr;
  uint32_t* dev_ptr = nullptr;
  hipEvent_t ev = nullptr;
  int state = 0;            // 0 free, 1 pending (count not looked at yet), 2 resolved
  int result = 0;           // resolved: num_rendered or GRPG_ERR_CAPACITY
  uint32_t Rcap = 0, Ccap = 0;
  bool hier = false;
  bool with_pass3 = true;   // the frame was enqueued with the fourth depth-sort pass
  CapKey key{-1, 0, 0, 0};
  int generation = 0;       // ticket = generation * DEFER_SLOTS + slot: a recycled slot's old tickets expire
};
constexpr int DEFER_SLOTS = GRPG_MAX_DEFERRED_FRAMES;
// The ring belongs to the thread that enqueues the frames: tickets are only valid on that thread
// (documented in the header), and the pinned words / events are released when the thread exits.
struct DeferRing {
  DeferSlot slot[DEFER_SLOTS];
  ~DeferRing() {
    if (on_main_thread()) return;   // process exit: see HostWords
    for (auto& d : slot) {
      if (d.host_ptr) (void)hipHostFree(d.host_ptr);
      if (d.ev) (void)hipEventDestroy(d.ev);
      d.host_ptr = nullptr; d.ev = nullptr;
    }
  }
  DeferSlot& operator[](int i) { return slot[i]; }
};
thread_local DeferRing g_defer;
thread_local int g_defer_next = 0;
struct CapHint {
  CapKey key{-1, 0, 0, 0};
  uint32_t high = 0;      // decaying high-water mark of num_rendered
  uint32_t high_c = 0;    // same for the coarse (Gaussian, super-tile) count of the hierarchical binning
  bool far = true;        // a recent frame's depth keys needed the fourth sort pass (sort.hip key_far)
  uint32_t far_hold = 0;  // near frames left before `far` is dropped again (sticky with decay, below)
  uint32_t once = 0, once_c = 0;   // grpg_set_capacity_hint: exact capacities for the next frame only
  bool seen = false;      // a frame of this shape has reported its counts (high / high_c / far are real)
  uint64_t stamp = 0;     // last use (LRU replacement)
  bool valid = false;
};
std::mutex g_hint_mu;
CapHint g_hints[16];
uint64_t g_hint_clock = 0;
std::atomic<int> g_binning_mode{[] {
  const char* e = getenv("GRPG_SYNC_R");
  return (e && atoi(e) != 0) ? GRPG_BINNING_EXACT : GRPG_BINNING_SPECULATIVE;
}()};

bool same_key(const CapKey& a, const CapKey& b) {
  return a.dev == b.dev && a.P == b.P && a.W == b.W && a.H == b.H;
}
// capacity carved for an expected count: +25 % head room, 64 Ki granules (stable blob sizes, so the
// caller's caching allocator hands the same block back every frame)
uint32_t padded_capacity(uint32_t r) {
  const uint64_t c = ((uint64_t)r + r / 4 + 65536 + 65535) / 65536 * 65536;
  return (uint32_t)(c > 0x7FFF0000ull ? 0x7FFF0000ull : c);
}
uint32_t capacity_from_hint(const CapKey& k, uint32_t* coarse_cap, bool* far) {
  *far = true;   // no history: enqueue the (normally idle) fourth depth-sort pass
  std::lock_guard<std::mutex> lk(g_hint_mu);
  for (auto& h : g_hints)
    if (h.valid && same_key(h.key, k)) {
      h.stamp = ++g_hint_clock;
      if (h.once != 0u) {   // grpg_set_capacity_hint: exactly what the caller promised, once
        const uint32_t cap = h.once, cc = h.once_c;
        h.once = 0u; h.once_c = 0u;
        *coarse_cap = cc;
        *far = true;
        return cap;
      }
      if (!h.seen) break;   // only ever seeded: no history yet
      const uint32_t cap = padded_capacity(h.high);
      const uint32_t cc = h.high_c ? padded_capacity(h.high_c) : cap;
      *coarse_cap = cc < cap ? cc : cap;     // a (Gaussian, super-tile) pair holds >= 1 instance
      *far = h.far;
      return cap;
    }
  *coarse_cap = 0u;
  return 0u;
}
// the hint of this key, or a fresh one in a free / the least recently used slot (g_hint_mu held)
CapHint* hint_slot(const CapKey& k) {
  for (auto& h : g_hints)
    if (h.valid && same_key(h.key, k)) return &h;
  CapHint* slot = &g_hints[0];
  for (auto& h : g_hints) {
    if (!h.valid) { slot = &h; break; }
    if (h.stamp < slot->stamp) slot = &h;
  }
  *slot = CapHint{};
  slot->key = k;
  slot->valid = true;
  return slot;
}
void update_hint(const CapKey& k, uint32_t R, uint32_t Rc, bool far) {
  std::lock_guard<std::mutex> lk(g_hint_mu);
  CapHint* slot = hint_slot(k);
  const uint32_t decayed = slot->high - slot->high / 64;   // lets the mark follow a shrinking scene
  slot->high = R > decayed ? R : decayed;
  // decays on sort-binning frames too (Rc == 0 there), so it never outlives `high`
  const uint32_t dc = slot->high_c - slot->high_c / 64;
  slot->high_c = Rc > dc ? Rc : dc;
  if (slot->high_c > slot->high) slot->high_c = slot->high;
  // Sticky with decay: frames alternating between a near and a far depth range under one
  // (device, P, W, H) -- two cameras, two scenes of one size -- would otherwise enqueue every far frame
  // without its fourth pass and render it twice.  An enqueued-but-idle fourth pass costs two launch
  // boundaries (~9 us of a single stream); it is dropped after FAR_HOLD consecutive near frames.
  constexpr uint32_t FAR_HOLD = 32;
  if (far) slot->far_hold = FAR_HOLD;
  else if (slot->far_hold > 0u) slot->far_hold--;
  slot->far = slot->far_hold > 0u;
  slot->seen = true;
  slot->stamp = ++g_hint_clock;
}

// The fat depth sort (sort.hip) sweeps the whole count table in every workgroup: fine up to a few
// hundred chunks, quadratic beyond (P > 4 M: the classic three-kernel passes).
bool depth_sort_is_fat(uint32_t nchunks_ds) { return nchunks_ds <= DS_MAX_CHUNKS; }

// debug=true: synchronise and check after every stage, like CHECK_CUDA (auxiliary.h:166-173).
#define STAGE_CHECK(name)                                                                    \
  do {                                                                                       \
    hipError_t e_ = hipGetLastError();                                                       \
    if (e_ == hipSuccess && debug) e_ = hipStreamSynchronize(stream);                        \
    if (e_ != hipSuccess)                                                                    \
      return fail(GRPG_ERR_HIP, std::string("stage ") + name + ": " + hipGetErrorString(e_)); \
  } while (0)

// Asynchronous device-side failures (today: a producer / consumer hand-over of the render that timed
// out, render_fwd.hip pc_fail) raise a sticky word in pinned host memory.  Like an asynchronous HIP
// error it is reported by the NEXT entry point the thread calls (all forwards, the backwards,
// grpg_frame_status), once; with debug = true the forward that suffered it fails itself.
int check_async_error(HostWord* hw) {
  if (hw && hw->host_ptr[3] != 0u) {
    hw->host_ptr[3] = 0u;
    return fail(GRPG_ERR_HIP, "render: a producer/consumer hand-over timed out in an earlier frame "
                              "of this thread (image blob header pc_timeout): that frame's image is invalid");
  }
  return GRPG_OK;
}

// Tile binning algorithm: "hier" (hier_binning.hip, default) or "sort" (emit + stable partition).
std::atomic<int> g_binning_alg{[] {
  const char* e = getenv("GRPG_BINNING");
  return (e && strcmp(e, "sort") == 0) ? GRPG_BINNING_ALG_SORT : GRPG_BINNING_ALG_HIER;
}()};
bool binning_is_hier() { return g_binning_alg.load() == GRPG_BINNING_ALG_HIER; }
bool alpha_rect_enabled() {
  static const bool on = [] { const char* v = getenv("GRPG_ALPHA_RECT"); return !(v && atoi(v) == 0); }();
  return on;
}

int bits_for(uint32_t T) {  // smallest b with (1 << b) >= T, i.e. tile ids fit in b bits
  int b = 0;
  while ((1ull << b) < (unsigned long long)T) b++;
  return b;
}

// Per-stage device timing with HIP events recorded on the op's stream.  Nothing is synchronised
// while frames are in flight: every grpg_forward appends one record of events to a thread-local
// list; grpg_get_stage_timing() waits for them, sums per stage and clears the list.
struct TimingRecord {
  hipEvent_t ev[GRPG_NUM_STAGES + 1];
  int stage_of[GRPG_NUM_STAGES + 1];
  int n = 0;
};
thread_local std::vector<TimingRecord*> g_pending;
thread_local std::vector<TimingRecord*> g_free;

struct StageTimer {
  hipStream_t s;
  TimingRecord* r = nullptr;
  int mode = 0;
  StageTimer(hipStream_t s_, int mode_) : s(s_), mode(mode_) {
    if (!mode) return;
    if (!g_free.empty()) { r = g_free.back(); g_free.pop_back(); }
    else { r = new TimingRecord(); for (auto& e : r->ev) (void)hipEventCreate(&e); }
    r->n = 0;
  }
  int tail_n = -1;   // record count when the tail of the frame (everything redone on overflow) began
  void begin_tail() { if (r && tail_n < 0) tail_n = r->n; }
  void restart_tail() { if (r && tail_n >= 0) r->n = tail_n; }
  void mark(int next_stage) {
    if (!r || r->n > GRPG_NUM_STAGES) return;
    if (mode == 2 && next_stage != 6 && next_stage != 7) return;   // render start / render end only
    (void)hipEventRecord(r->ev[r->n], s);
    r->stage_of[r->n] = next_stage;
    r->n++;
  }
  void finish() {
    if (r) { g_pending.push_back(r); r = nullptr; }
  }
  ~StageTimer() {
    if (r) g_free.push_back(r);   // call failed before finish(): recycle
  }
};

// Backward: two device times per call (blend backward, preprocess backward), same mechanism -- but
// process-wide: PyTorch runs an op's backward on its autograd thread, not on the thread that
// switched the timing on.
struct BwdTimingRecord { hipEvent_t ev[3]; };
std::atomic<int> g_bwd_timing{0};
std::mutex g_bwd_mu;
std::vector<BwdTimingRecord*> g_bwd_pending;
std::vector<BwdTimingRecord*> g_bwd_free;
BwdTimingRecord* bwd_timing_begin(hipStream_t s) {
  if (!g_bwd_timing.load()) return nullptr;
  BwdTimingRecord* r = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_bwd_mu);
    if (!g_bwd_free.empty()) { r = g_bwd_free.back(); g_bwd_free.pop_back(); }
  }
  if (!r) { r = new BwdTimingRecord(); for (auto& e : r->ev) (void)hipEventCreate(&e); }
  (void)hipEventRecord(r->ev[0], s);
  return r;
}
constexpr size_t BWD_PENDING_CAP = 256;   // a caller that never collects them keeps the newest 256
void bwd_timing_mark(BwdTimingRecord* r, int i, hipStream_t s) {
  if (!r) return;
  (void)hipEventRecord(r->ev[i], s);
  if (i == 2) {
    std::lock_guard<std::mutex> lk(g_bwd_mu);
    if (g_bwd_pending.size() >= BWD_PENDING_CAP) {   // recycle the oldest record (its events are reused)
      g_bwd_free.push_back(g_bwd_pending.front());
      g_bwd_pending.erase(g_bwd_pending.begin());
    }
    g_bwd_pending.push_back(r);
  }
}
// a backward that fails between begin and the last mark hands its record back
struct BwdTimingGuard {
  BwdTimingRecord* r;
  bool done = false;
  explicit BwdTimingGuard(BwdTimingRecord* r_) : r(r_) {}
  ~BwdTimingGuard() {
    if (r && !done) { std::lock_guard<std::mutex> lk(g_bwd_mu); g_bwd_free.push_back(r); }
  }
};

// ---- which geometry blobs were carved WITH the backward's gradient records (a training forward)?
// grpg_backward writes P x 64 bytes behind the rest of the blob; a blob carved by an evaluation
// forward (GRPG_FORWARD_NO_BACKWARD) has no such region.  The last forwards' blob addresses are
// remembered so that the mistake is an error return, not an out-of-bounds device write. ----
struct GeomSeen { const void* ptr = nullptr; int P = 0; bool has_grad = false; uint64_t stamp = 0; };
std::mutex g_geom_mu;
GeomSeen g_geom_seen[64];
uint64_t g_geom_clock = 0;
void remember_geom(const void* ptr, int P, bool has_grad) {
  std::lock_guard<std::mutex> lk(g_geom_mu);
  GeomSeen* slot = &g_geom_seen[0];
  for (auto& g : g_geom_seen) {
    if (g.ptr == ptr) { slot = &g; break; }
    if (g.stamp < slot->stamp) slot = &g;
  }
  slot->ptr = ptr; slot->P = P; slot->has_grad = has_grad; slot->stamp = ++g_geom_clock;
}
// The table is ADVISORY: every forward of this process overwrites the entry of the address it carves
// (an evaluation forward at a recycled address turns a "yes" into a "no"), but a blob the CALLER copies into an
// address a training forward of the same P once carved is invisible to it -- the one case left in which the fast
// path vouches for a buffer it has not seen (validating every call would cost the training loop a host wait per
// backward: the host could no longer run ahead of the device).  Only its "yes, the training forward of this P
// carved that address" answer is taken as is (the training loop's case: no host round trip).  A "no" (possibly stale: a reloaded training blob
// at an address an evaluation forward used) or an unknown address is settled by the geometry header
// itself -- one 4-byte read behind the stream's work, off the hot path.
// returns GRPG_OK, or the error the backward must return
int geom_check_backward(const void* ptr, int P, hipStream_t stream) {
  {
    std::lock_guard<std::mutex> lk(g_geom_mu);
    for (auto& g : g_geom_seen)
      if (g.ptr == ptr && g.P == P && g.has_grad) return GRPG_OK;
  }
  // An address the table does not vouch for: the blob's own header decides.  That is a host read behind the
  // stream's work -- grpg_backward is NOT asynchronous for such a blob (documented in grpg_rasterizer.h), and a
  // stream that is being captured into a graph cannot be waited for at all: refuse instead of breaking the capture.
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
    return fail(GRPG_ERR_BAD_BUFFER, "grpg_backward under stream capture needs the geometry buffer of a training "
                                     "forward made by this process (its address is not on record, and reading the "
                                     "header would synchronize the capturing stream)");
  BlobHeader h;
  hipError_t e = hipMemcpyAsync(&h, ptr, sizeof(BlobHeader), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail(GRPG_ERR_HIP, std::string("reading the geometry header: ") + hipGetErrorString(e));
  if (h.magic != GEOM_MAGIC || h.P != (uint32_t)P)
    return fail(GRPG_ERR_BAD_BUFFER, "the geometry buffer does not hold a forward of this P (magic / P)");
  if (h.has_grad_rec == 0u)
    return fail(GRPG_ERR_BAD_BUFFER, "the geometry buffer was carved by an evaluation forward "
                                     "(GRPG_FORWARD_NO_BACKWARD): it has no room for the backward's gradient records");
  remember_geom(ptr, P, true);
  return GRPG_OK;
}
// what every backward settles about its state before it looks at its other arguments: the geometry blob, then the
// asynchronous failures of the thread's earlier frames
int check_backward_state(const void* geom_buffer, int P, hipStream_t stream) {
  if (int rc = geom_check_backward(geom_buffer, P, stream)) return rc;
  for (auto& hw : g_host_words)
    if (int rc = check_async_error(&hw)) return rc;
  return GRPG_OK;
}

CameraArgs make_camera(const float* view, const float* proj, const float* campos, int W, int H,
                       float tan_fovx, float tan_fovy) {
  CameraArgs c;
  c.view = view; c.proj = proj; c.campos = campos;
  c.W = W; c.H = H;
  c.gx = (W + TILE - 1) / TILE;
  c.gy = (H + TILE - 1) / TILE;
  c.tan_fovx = tan_fovx; c.tan_fovy = tan_fovy;
  c.focal_y = H / (2.0f * tan_fovy);  // rasterizer_impl.cu:225-226
  c.focal_x = W / (2.0f * tan_fovx);
  return c;
}

}  // namespace

extern "C" {

int grpg_abi_version(void) { return GRPG_ABI_VERSION; }
const char* grpg_last_error(void) { return g_last_error.c_str(); }

int grpg_set_stage_timing(int enabled) {
  g_timing_enabled = enabled == 2 ? 2 : (enabled != 0 ? 1 : 0);
  for (auto* r : g_pending) g_free.push_back(r);
  g_pending.clear();
  g_bwd_timing.store(enabled != 0 ? 1 : 0);
  {
    std::lock_guard<std::mutex> lk(g_bwd_mu);
    for (auto* r : g_bwd_pending) g_bwd_free.push_back(r);
    g_bwd_pending.clear();
  }
  return GRPG_OK;
}
int grpg_get_stage_timing(float* stage_ms_sum, int* num_calls) {
  if (!stage_ms_sum || !num_calls) return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL output");
  for (int i = 0; i < GRPG_NUM_STAGES; i++) stage_ms_sum[i] = 0.f;
  *num_calls = 0;
  for (auto* r : g_pending) {
    if (r->n < 2) { g_free.push_back(r); continue; }
    hipError_t e = hipEventSynchronize(r->ev[r->n - 1]);
    if (e != hipSuccess) return fail(GRPG_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
    for (int i = 0; i + 1 < r->n; i++) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, r->ev[i], r->ev[i + 1]);
      if (r->stage_of[i] >= 0 && r->stage_of[i] < GRPG_NUM_STAGES) stage_ms_sum[r->stage_of[i]] += ms;
    }
    (*num_calls)++;
    g_free.push_back(r);
  }
  g_pending.clear();
  return GRPG_OK;
}

int grpg_get_backward_timing(float* blend_ms_sum, float* preprocess_ms_sum, int* num_calls) {
  if (!blend_ms_sum || !preprocess_ms_sum || !num_calls) return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL output");
  *blend_ms_sum = 0.f; *preprocess_ms_sum = 0.f; *num_calls = 0;
  std::lock_guard<std::mutex> lk(g_bwd_mu);
  for (auto* r : g_bwd_pending) {
    hipError_t e = hipEventSynchronize(r->ev[2]);
    if (e != hipSuccess) return fail(GRPG_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
    float a = 0.f, b = 0.f;
    (void)hipEventElapsedTime(&a, r->ev[0], r->ev[1]);
    (void)hipEventElapsedTime(&b, r->ev[1], r->ev[2]);
    *blend_ms_sum += a; *preprocess_ms_sum += b; (*num_calls)++;
    g_bwd_free.push_back(r);
  }
  g_bwd_pending.clear();
  return GRPG_OK;
}

int grpg_set_binning_mode(int mode) {
  if (mode != GRPG_BINNING_SPECULATIVE && mode != GRPG_BINNING_EXACT)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "unknown binning mode");
  g_binning_mode.store(mode);
  return GRPG_OK;
}
int grpg_get_binning_algorithm(void) { return g_binning_alg.load(); }
int grpg_set_binning_algorithm(int alg) {
  if (alg != GRPG_BINNING_ALG_SORT && alg != GRPG_BINNING_ALG_HIER)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "unknown binning algorithm");
  g_binning_alg.store(alg);
  return GRPG_OK;
}
int grpg_reset_capacity_hints(void) {
  std::lock_guard<std::mutex> lk(g_hint_mu);
  for (auto& h : g_hints) h = CapHint{};
  return GRPG_OK;
}
int grpg_set_capacity_hint(int P, int width, int height, unsigned instances, unsigned coarse_pairs) {
  if (int rc = begin_call()) return rc;
  if (P <= 0 || width <= 0 || height <= 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "bad shape");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const CapKey k = {dev, P, width, height};
  std::lock_guard<std::mutex> lk(g_hint_mu);
  CapHint* slot = hint_slot(k);
  slot->once = instances ? instances : 1u;
  slot->once_c = coarse_pairs ? coarse_pairs : 1u;
  slot->stamp = ++g_hint_clock;
  return GRPG_OK;
}

}  // extern "C"

namespace {

// Pinned staging for the composed forward's segment table (thread-local; the frame's one host wait
// guarantees the previous upload has been consumed before the buffer is reused).
thread_local SegmentDev* g_seg_staging = nullptr;
thread_local FeatureSegDev* g_feat_staging = nullptr;   // ... and for its feature table (grpg_forward_composed_features)

// grpg_backward_composed returns without a host wait, so the pinned tables its asynchronous copies
// read must outlive the call: a ring of slots, each guarded by an event recorded behind its copies
// (a slot comes round again 8 backward calls later; its event has long fired by then).
struct BwdStagingSlot {
  SegmentDev* segs = nullptr;
  grpg_model_segment_grad* grads = nullptr;
  FeatureSegDev* feats = nullptr;   // (grpg_backward_composed_features)
  hipEvent_t ev = nullptr;
  bool used = false;
};
constexpr int BWD_STAGING_SLOTS = 8;
thread_local BwdStagingSlot g_bwd_staging[BWD_STAGING_SLOTS];
thread_local int g_bwd_staging_next = 0;
BwdStagingSlot* bwd_staging_acquire() {
  BwdStagingSlot& b = g_bwd_staging[g_bwd_staging_next];
  g_bwd_staging_next = (g_bwd_staging_next + 1) % BWD_STAGING_SLOTS;
  if (!b.segs) {
    if (hipHostMalloc((void**)&b.segs, sizeof(SegmentDev) * MAX_SEGMENTS, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&b.grads, sizeof(grpg_model_segment_grad) * MAX_SEGMENTS, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&b.feats, sizeof(FeatureSegDev) * MAX_SEGMENTS, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&b.ev, hipEventDisableTiming) != hipSuccess)
      return nullptr;
  }
  if (b.used) (void)hipEventSynchronize(b.ev);
  b.used = true;
  return &b;
}

// ---- device poses (grpg_bind_device_poses): a binding waits in g_pose_pending until the next entry point that takes
// a grpg_model_segment* opens its PoseScope, which moves it into g_pose_cur for the length of that call -- through
// nested entries (grpg_forward_composed -> _flags, the backward's shared bodies) and every table the call builds --
// and drops it when the outermost scope closes, whatever the call returns.  Plain arrays: no destructor at thread exit.
struct PoseBinding {
  bool set = false, any = false;   // any: some row >= 0, i.e. the gather kernel has work
  const float* rot = nullptr;
  const float* trans = nullptr;
  int n = 0;
  int row[MAX_SEGMENTS];
  void clear() { set = any = false; rot = trans = nullptr; n = 0; }
};
thread_local PoseBinding g_pose_pending, g_pose_cur;
thread_local int g_pose_depth = 0;
struct PoseScope {
  PoseScope() {
    if (g_pose_depth++ != 0) return;
    g_pose_cur.clear();
    if (g_pose_pending.set) {
      g_pose_cur.set = true; g_pose_cur.any = g_pose_pending.any;
      g_pose_cur.rot = g_pose_pending.rot; g_pose_cur.trans = g_pose_pending.trans; g_pose_cur.n = g_pose_pending.n;
      memcpy(g_pose_cur.row, g_pose_pending.row, sizeof(int) * (size_t)g_pose_pending.n);
    }
    g_pose_pending.clear();
  }
  ~PoseScope() {
    if (--g_pose_depth == 0) g_pose_cur.clear();
  }
};
// ---- frame correction (grpg_bind_frame_correction): the device matrix waits here until the next grpg_forward_frame /
// grpg_forward_composed_frame on this thread, which takes it first thing -- whatever that call returns then.
thread_local const float* g_affine_pending = nullptr;
const float* take_frame_correction() {
  const float* a = g_affine_pending;
  g_affine_pending = nullptr;
  return a;
}
// the epilogue a bound correction runs in (fe: the call's resolved epilogue, or NULL when it has none)
int attach_frame_correction(const float* affine, FrameEpilogue* fe) {
  if (affine == nullptr) return GRPG_OK;
  if (fe == nullptr)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "a frame correction was bound, but the frame has no epilogue to apply it in");
  fe->affine = affine;
  return GRPG_OK;
}

// ---- a baked frame table (grpg_bind_frame_table): one frame's rows of a grpg_frame_tables_bake table wait here until
// the next composed forward on this thread, which takes them first thing -- whatever that call returns then.
struct TableBinding {
  const SegmentDev* rows = nullptr;
  int n = 0, P = 0;
};
thread_local TableBinding g_table_pending;
TableBinding take_frame_table() {
  const TableBinding t = g_table_pending;
  g_table_pending = TableBinding{};
  return t;
}

// behind the asynchronous copy of a table fill_segments built: the bound rows' poses, on the same stream
void gather_device_poses(hipStream_t stream, SegmentDev* seg_dev, int nseg) {
  if (g_pose_cur.set && g_pose_cur.any && g_pose_cur.n == nseg)
    launch_segment_pose_gather(stream, seg_dev, nseg, g_pose_cur.rot, g_pose_cur.trans);
}

// grpg_forward_layers: the class of every Gaussian and the two extra plane pairs
struct LayerArgs {
  const unsigned char* segment_class;   // composed frames: [num_segments] HOST bytes (NULL: the segment's rigid flag)
  const unsigned char* layer_class;
  const float* layer_background;
  float* out_color_bg; float* out_alpha_bg; float* out_color_obj; float* out_alpha_obj;
};

// The device segment table of a composed model: one row per segment, `start` running over the counts.  layers: the
// layered frame whose class bit (pad1: 1 = object layer) the rows carry, NULL: none -- the rows then carry the
// default class, "actors are objects" (only a layered frame's preprocess looks at the bit; grpg_object_alpha_forward
// reads it from a training frame's table).
void fill_segments(SegmentDev* dst, const grpg_model_segment* segs, int nseg, const LayerArgs* layers) {
  uint32_t start = 0;
  for (int i = 0; i < nseg; i++) {
    const grpg_model_segment& g = segs[i];
    SegmentDev& d = dst[i];
    const bool obj = (layers && layers->segment_class) ? layers->segment_class[i] != 0 : g.rigid != 0;
    d.xyz = g.xyz; d.scaling = g.scaling; d.rotation = g.rotation; d.opacity = g.opacity;
    // the symmetry prior mirrors posed actors only (street_gaussian_model.py:332,360 sit inside the per-actor loop):
    // a static segment's mask is ignored, by the forward and by both backwards alike (they all read this table)
    d.fdc = g.features_dc; d.frest = g.features_rest; d.flip = g.rigid ? g.flip : nullptr;
    d.pad1 = (const void*)(uintptr_t)(obj ? 1u : 0u);
    d.start = start; d.count = (uint32_t)g.count;
    d.fourier_dim = g.fourier_dim; d.rigid = g.rigid;
    for (int k = 0; k < 4; k++) d.rot[k] = g.obj_rot[k];
    for (int k = 0; k < 3; k++) d.trans[k] = g.obj_trans[k];
    d.pad0 = 0.f;
    for (int k = 0; k < MAX_FOURIER; k++) d.idft[k] = g.idft[k];
    start += (uint32_t)g.count;
  }
  // device poses: pose_row + 1 travels in the bits of the spare word, to the gather kernel behind the table's copy
  // (gather_device_poses), which puts the word back to 0.f -- the hot kernels load the same 144 bytes as ever
  if (g_pose_cur.set && g_pose_cur.n == nseg)
    for (int i = 0; i < nseg; i++)
      if (g_pose_cur.row[i] >= 0) {
        const int parked = g_pose_cur.row[i] + 1;
        memcpy(&dst[i].pad0, &parked, sizeof(parked));
      }
}

// One forward frame as an entry point hands it to forward_impl.  Every extern "C" forward fills the fields it has;
// the rest stay zero / NULL.  segs == NULL: flat input tensors (grpg_forward); segs: per-model raw parameters
// (grpg_forward_composed), P = sum of their counts, the flat pointers stay NULL.
struct FrameRequest {
  grpg_alloc_fn geometry_alloc = nullptr, binning_alloc = nullptr, image_alloc = nullptr;
  void *geometry_user = nullptr, *binning_user = nullptr, *image_user = nullptr;
  int P = 0, D = 0, M = 0, S = 0, width = 0, height = 0;
  float scale_modifier = 0.f, tan_fovx = 0.f, tan_fovy = 0.f;
  int debug = 0;
  hipStream_t stream = nullptr;
  unsigned flags = 0u;
  const float *means3D = nullptr, *shs = nullptr, *colors_precomp = nullptr, *semantics = nullptr,
              *opacities = nullptr, *scales = nullptr, *rotations = nullptr, *cov3D_precomp = nullptr;
  const float *background = nullptr, *viewmatrix = nullptr, *projmatrix = nullptr, *cam_pos = nullptr;
  float *out_color = nullptr, *out_depth = nullptr, *out_alpha = nullptr, *out_semantic = nullptr;
  int* radii = nullptr;
  const grpg_model_segment* segs = nullptr;
  int nseg = 0;
  // grpg_bind_frame_table: the frame's device rows, baked earlier -- read in place of a table staged from segs
  const SegmentDev* bound_rows = nullptr;
  // grpg_forward_composed_features: the segments' semantic arrays (host array of device pointers, or NULL), the
  // channel split S = 3 * feat_normals + feat_S, and the blob whose head is the [P,S] array `semantics` points at
  const float* const* seg_semantic = nullptr;
  int feat_S = 0, feat_normals = 0;
  char* feat_blob = nullptr;
  DeferSlot* defer = nullptr;           // grpg_forward_deferred: the slot the frame's count is published to
  const LayerArgs* layers = nullptr;    // a layered frame
  const FrameEpilogue* epi = nullptr;   // grpg_forward_frame: sky composite / clamp / bytes behind the blend
  // an evaluation frame (GRPG_FORWARD_NO_BACKWARD: no backward can follow) is not a training frame
  bool training() const { return (flags & GRPG_FORWARD_NO_BACKWARD) == 0u; }
};

// The three groups of fields every entry point fills alike; what is an entry's own (S and the semantic arrays, layers,
// epilogue, deferred slot, feature split) it states itself.
void set_allocators(FrameRequest& q, grpg_alloc_fn geometry_alloc, void* geometry_user, grpg_alloc_fn binning_alloc,
                    void* binning_user, grpg_alloc_fn image_alloc, void* image_user) {
  q.geometry_alloc = geometry_alloc; q.geometry_user = geometry_user; q.binning_alloc = binning_alloc;
  q.binning_user = binning_user; q.image_alloc = image_alloc; q.image_user = image_user;
}
void set_camera(FrameRequest& q, const float* background, int width, int height, float scale_modifier,
                const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                float tan_fovy, float* out_color, float* out_depth, float* out_alpha, int* radii, int debug,
                void* hip_stream, unsigned flags) {
  q.background = background; q.width = width; q.height = height; q.scale_modifier = scale_modifier;
  q.viewmatrix = viewmatrix; q.projmatrix = projmatrix; q.cam_pos = cam_pos; q.tan_fovx = tan_fovx;
  q.tan_fovy = tan_fovy; q.out_color = out_color; q.out_depth = out_depth; q.out_alpha = out_alpha;
  q.radii = radii; q.debug = debug; q.stream = (hipStream_t)hip_stream; q.flags = flags;
}
// the model: flat tensors ...
void set_model(FrameRequest& q, int P, int D, int M, const float* means3D, const float* shs,
               const float* colors_precomp, const float* opacities, const float* scales, const float* rotations,
               const float* cov3D_precomp) {
  q.P = P; q.D = D; q.M = M; q.means3D = means3D; q.shs = shs; q.colors_precomp = colors_precomp;
  q.opacities = opacities; q.scales = scales; q.rotations = rotations; q.cov3D_precomp = cov3D_precomp;
}
// ... or the checked segments of a composition (P: check_composed_model's)
void set_model(FrameRequest& q, const grpg_model_segment* segments, int num_segments, long long P, int D, int M) {
  q.segs = segments; q.nseg = num_segments; q.P = (int)P; q.D = D; q.M = M;
}

// A bound frame table joins the composed evaluation frame it was baked for (q: model, camera and flags set) -- or the
// call is refused: the table holds no gradient bookkeeping's worth of a training frame (its backward rebuilds the
// table from the host segments), feature planes stage a table of their own next to it, and device poses would be
// gathered into the caller's baked rows.
int attach_frame_table(const TableBinding& tb, FrameRequest& q) {
  if (tb.rows == nullptr) return GRPG_OK;
  if (q.training())
    return fail(GRPG_ERR_INVALID_ARGUMENT, "a frame table was bound in front of a training forward");
  if (q.feat_blob != nullptr || q.S != 0)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "a frame table was bound in front of a frame with feature planes");
  if (g_pose_cur.set)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "a frame table and device poses were bound for the same call");
  if (tb.n != q.nseg || tb.P != q.P)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "the bound frame table was baked for another number of segments or Gaussians");
  q.bound_rows = tb.rows;
  return GRPG_OK;
}

// the argument checks of every forward, behind ensure_device
int validate(const FrameRequest& q) {
  if (q.P < 0 || q.width <= 0 || q.height <= 0 || q.S < 0 || q.M < 0)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "negative size");
  if (!q.geometry_alloc || !q.binning_alloc || !q.image_alloc)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "buffer allocators must not be NULL");
  if (!q.background || !q.viewmatrix || !q.projmatrix || !q.cam_pos)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL camera/background/output pointer");
  // the float planes may be left out only when a frame epilogue delivers the bytes instead (grpg_forward_frame)
  if ((!q.out_color || !q.out_depth || !q.out_alpha) && !(q.epi && !q.epi->planes && q.epi->rgb8))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL camera/background/output pointer");
  if (q.epi && (q.training() || q.S != 0))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "a frame epilogue needs an evaluation frame without semantic planes");
  if ((unsigned)q.P > ID_MASK) return fail(GRPG_ERR_INVALID_ARGUMENT, "P must be < 2^28");
  if (q.P > 0 && q.segs == nullptr) {
    if (!q.means3D || !q.opacities) return fail(GRPG_ERR_INVALID_ARGUMENT, "means3D/opacities NULL");
    if (!q.cov3D_precomp && (!q.scales || !q.rotations))
      return fail(GRPG_ERR_INVALID_ARGUMENT, "need scales+rotations or cov3D_precomp");
    if (!q.colors_precomp && (!q.shs || q.M <= 0))
      return fail(GRPG_ERR_INVALID_ARGUMENT, "need shs (M>0) or colors_precomp");
    if (!q.colors_precomp && (q.D < 0 || q.D > 3 || (q.D + 1) * (q.D + 1) > q.M))
      return fail(GRPG_ERR_INVALID_ARGUMENT, "SH degree needs (D+1)^2 <= M, D <= 3");
  }
  // (a composed frame's feature array is the head of its feature blob: grpg_forward_composed_features)
  if (q.P > 0 && q.S > 0 && (!q.semantics || !q.out_semantic))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "semantics/out_semantic NULL with S>0");
  if (q.segs != nullptr && q.S > 0 && (q.layers || q.defer))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "feature planes of a composed frame: not in a layered or deferred frame");
  return GRPG_OK;
}

// One backward as an entry point hands it to its body.  Every extern "C" backward fills the fields it has; the rest
// stay zero / NULL.  All four fill the frame (set_frame).  grpg_backward: P, the flat tensors and its per-Gaussian
// outputs; its semantic channels are the blend's feature channels (F = S, dL_dpix_features / dL_dfeatures =
// dL_dpix_semantic / dL_dsemantic).  grpg_backward_composed: segs / nseg / grads and dL_dposes (set_model; P is the sum
// of the counts, the body's); _features adds the feature planes (set_features), _objects the object-alpha plane.
struct BackwardRequest {
  const float *means3D = nullptr, *shs = nullptr, *colors_precomp = nullptr, *semantics = nullptr, *scales = nullptr,
              *rotations = nullptr, *cov3D_precomp = nullptr;
  const grpg_model_segment* segs = nullptr;
  const grpg_model_segment_grad* grads = nullptr;
  int nseg = 0, P = 0, D = 0, M = 0, R = 0;
  const float *background = nullptr, *viewmatrix = nullptr, *projmatrix = nullptr, *campos = nullptr;
  int width = 0, height = 0;
  float scale_modifier = 0.f, tan_fovx = 0.f, tan_fovy = 0.f;
  const int* radii = nullptr;
  const float* alphas = nullptr;
  char *geom_buffer = nullptr, *binning_buffer = nullptr, *image_buffer = nullptr, *feature_buffer = nullptr,
       *workspace = nullptr;   // (workspace: the object-alpha plane's)
  const float *dL_dpix = nullptr, *dL_dpix_depth = nullptr, *dL_dalphas = nullptr, *dL_dpix_features = nullptr;
  int S = 0, normals = 0, F = 0;   // the blend's feature channels: F = 3 * normals + S composed, F = S flat
  float* const* seg_dL_dsemantic = nullptr;
  float *dL_dfeatures = nullptr, *dL_dmean2D = nullptr, *dL_dposes = nullptr;
  const float *alpha_object = nullptr, *dL_dalpha_object = nullptr;   // alpha_object == NULL: no object-alpha plane
  float *dL_dconic = nullptr, *dL_dopacity = nullptr, *dL_dcolor = nullptr, *dL_ddepth = nullptr,
        *dL_dmean3D = nullptr, *dL_dcov3D = nullptr, *dL_dsh = nullptr, *dL_dscale = nullptr, *dL_drot = nullptr;
  int debug = 0;
  hipStream_t stream = nullptr;
};

// The frame: the camera, what the forward left, and the gradients of its three planes.
void set_frame(BackwardRequest& q, int R, const float* background, int width, int height, float scale_modifier,
               const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
               const int* radii, const float* alphas, char* geom_buffer, char* binning_buffer, char* image_buffer,
               const float* dL_dpix, const float* dL_dpix_depth, const float* dL_dalphas, float* dL_dmean2D, int debug,
               void* hip_stream) {
  q.R = R; q.background = background; q.width = width; q.height = height; q.scale_modifier = scale_modifier;
  q.viewmatrix = viewmatrix; q.projmatrix = projmatrix; q.campos = campos; q.tan_fovx = tan_fovx;
  q.tan_fovy = tan_fovy; q.radii = radii; q.alphas = alphas; q.geom_buffer = geom_buffer;
  q.binning_buffer = binning_buffer; q.image_buffer = image_buffer; q.dL_dpix = dL_dpix;
  q.dL_dpix_depth = dL_dpix_depth; q.dL_dalphas = dL_dalphas; q.dL_dmean2D = dL_dmean2D; q.debug = debug;
  q.stream = (hipStream_t)hip_stream;
}
// The segments of a composition with the tables of their gradients, and its feature planes (F is formed here; the
// body checks the split, check_feature_split, before anything reads it).
void set_model(BackwardRequest& q, const grpg_model_segment* segments, const grpg_model_segment_grad* grads,
               int num_segments, int D, int M, float* dL_dposes) {
  q.segs = segments; q.grads = grads; q.nseg = num_segments; q.D = D; q.M = M; q.dL_dposes = dL_dposes;
}
void set_features(BackwardRequest& q, float* const* seg_dL_dsemantic, int S, int normals, char* feature_buffer,
                  const float* dL_dpix_features, float* dL_dfeatures) {
  q.seg_dL_dsemantic = seg_dL_dsemantic; q.S = S; q.normals = normals; q.F = 3 * normals + S;
  q.feature_buffer = feature_buffer; q.dL_dpix_features = dL_dpix_features; q.dL_dfeatures = dL_dfeatures;
}

// The frame of every backward (grpg_backward, grpg_backward_composed*): the camera and the blob layouts, then -- run()
// -- the blend backward into the cleared gradient records; the caller's preprocess backward takes cam / GL / rec /
// grad_rec from it, and finish() closes the call behind that launch.
struct BlendBackward {
  const BackwardRequest& q;
  const int P;
  const hipStream_t stream;
  const int debug;
  const CameraArgs cam;
  const GeomLayout GL;
  const ImgLayout IL;
  const RecView rec;
  float* const grad_rec;   // per-Gaussian gradient records (one 64-byte line each) in the tail of the geometry blob
  BwdTimingRecord* btr = nullptr;
  BwdTimingGuard btg{nullptr};

  BlendBackward(const BackwardRequest& q_, int P_)
      : q(q_), P(P_), stream(q_.stream), debug(q_.debug),
        cam(make_camera(q_.viewmatrix, q_.projmatrix, q_.campos, q_.width, q_.height, q_.tan_fovx, q_.tan_fovy)),
        GL(geom_layout((size_t)P_)), IL(img_layout((size_t)cam.gx * (size_t)cam.gy, (size_t)q_.width * q_.height)),
        rec{(const float4*)(q_.geom_buffer + GL.rec)}, grad_rec((float*)(q_.geom_buffer + GL.grad_rec)) {}

  // the point list is the first array of the binning blob whatever capacity it was carved for
  const uint32_t* point_list() const { return (const uint32_t*)(q.binning_buffer + bin_layout(0).val_a); }
  const uint2* ranges() const { return (const uint2*)(q.image_buffer + IL.ranges); }

  // features [P,F] / q.dL_dpix_features [F,H,W] / q.dL_dfeatures [P,F] (accumulated into): NULL at F == 0
  int run(const float* features) {
    char* const image_buffer = q.image_buffer;
    HIP_TRY(hipMemsetAsync(grad_rec, 0, (size_t)P * GRAD_STRIDE * sizeof(float), stream));
    btg.r = btr = bwd_timing_begin(stream);
    launch_render_backward(stream, ranges(), point_list(), rec, features, q.F, cam.W, cam.H, cam.gx, cam.gy,
                           q.background, q.alphas, (const uint32_t*)(image_buffer + IL.n_contrib),
                           (const uint32_t*)(image_buffer + IL.work), q.dL_dpix, q.dL_dpix_depth, q.dL_dalphas,
                           q.dL_dpix_features, grad_rec, q.dL_dfeatures, (const BlobHeader*)q.binning_buffer,
                           (const uint32_t*)(image_buffer + IL.ck_count),
                           (const uint32_t*)(image_buffer + IL.bwd_ctl), (uint32_t)q.R);
    STAGE_CHECK("render backward");
    bwd_timing_mark(btr, 1, stream);
    return GRPG_OK;
  }
  // behind the preprocess backward's launch (`stage`: its label)
  int finish(const char* stage) {
    bwd_timing_mark(btr, 2, stream);
    btg.done = true;
    STAGE_CHECK(stage);
    return GRPG_OK;
  }
};

uint32_t num_tiles(const CameraArgs& c) { return (uint32_t)c.gx * (uint32_t)c.gy; }

// What the stages of one forward frame share: the request, the carved geometry / image blobs, the frame's mode
// switches, and the stages themselves in the order forward_impl runs them.  Built once the two blobs are allocated.
struct Frame {
  const FrameRequest& q;
  const CameraArgs cam;
  const GeomLayout GL;
  const ImgLayout IL;
  char* const geom;
  char* const img;
  Frame(const FrameRequest& q_, const CameraArgs& cam_, const GeomLayout& GL_, const ImgLayout& IL_, char* geom_,
        char* img_) : q(q_), cam(cam_), GL(GL_), IL(IL_), geom(geom_), img(img_) { setup_drain(); }
  Frame(const Frame&) = delete;   // (epi may point at epi_drained)

  const int debug = q.debug;            // (STAGE_CHECK)
  const hipStream_t stream = q.stream;
  const bool training = q.training();
  const uint32_t T = num_tiles(cam);
  const size_t N = (size_t)q.width * q.height;

  float4* const rec_w = (float4*)(geom + GL.rec);
  const RecView rec = {rec_w};
  uint32_t* const key_a = (uint32_t*)(geom + GL.key_a);
  uint32_t* const key_b = (uint32_t*)(geom + GL.key_b);
  uint32_t* const val_a = (uint32_t*)(geom + GL.val_a);
  uint32_t* const val_b = (uint32_t*)(geom + GL.val_b);
  uint32_t* const tiles = (uint32_t*)(geom + GL.tiles);
  uint32_t* const offsets = (uint32_t*)(geom + GL.offsets);
  int* const radii_int = q.radii ? q.radii : (int*)(geom + GL.radii);
  uint32_t* const table = (uint32_t*)(geom + GL.table);
  uint32_t* const totals = (uint32_t*)(geom + GL.totals);
  uint32_t* const block_sums = (uint32_t*)(geom + GL.block_sums);
  uint32_t* const ds_table = (uint32_t*)(geom + GL.ds_table);
  uint32_t* const tiles_sorted = (uint32_t*)(geom + GL.tiles_sorted);
  uint32_t* const emit_win = (uint32_t*)(geom + GL.emit_win);
  uint2* const rect_sorted = (uint2*)(geom + GL.rect_sorted);
  uint4* const pre_counts = (uint4*)(geom + GL.pre_counts);
  BlobHeader* const gh = (BlobHeader*)geom;
  uint2* const ranges = (uint2*)(img + IL.ranges);
  uint32_t* const n_contrib = (uint32_t*)(img + IL.n_contrib);
  uint32_t* const work = (uint32_t*)(img + IL.work);

  // Instance capacity of the binning blob.  Speculative mode (default): from the high-water mark
  // of earlier frames of this (device, P, W, H), so the blob is carved and every kernel of the
  // frame is enqueued BEFORE the host learns num_rendered; the kernels read the count from device
  // memory.  Exact mode, or no history yet: wait for the count first, like the reference
  // (rasterizer_impl.cu:284).
  const bool spec_mode = g_binning_mode.load() == GRPG_BINNING_SPECULATIVE;
  const bool fat_sort = depth_sort_is_fat(GL.nchunks_ds);
  // hierarchical binning needs the compacted depth order of the fat sort (its coarse scan gathers
  // the super-tile counts by sorted id); otherwise emit + partition
  const uint32_t NS = super_tiles(cam.gx, cam.gy);
  const bool hier = fat_sort && binning_is_hier() && NS <= 65536u;   // 16 id bits in a coarse key
  // hierarchical binning on a grid of <= 255 x 255 tiles: the tile rectangles ride through the
  // depth sort as a packed payload and arrive in depth order together with the super-tile counts
  // (sort.hip RectPayload); larger grids: the coarse scan gathers them by sorted id instead
  const bool rect_sorted_by_sort = hier && cam.gx <= 255 && cam.gy <= 255;
  uint2* const rects = hier ? (uint2*)(geom + GL.rects) : nullptr;
  // An evaluation frame (no n_contrib, no checkpoints: nothing a backward or the oracle's lists are compared with)
  // bins the 3-sigma rectangle cut to the alpha ellipse's box (preprocess.hip binned_rect): the device's instance
  // total (gh->R) is then BELOW the published num_rendered, which stays the reference's sum -- an upper bound that
  // still sizes every capacity.  GRPG_ALPHA_RECT=0 (experiments): the reference's rectangle.
  const bool binned_rects = hier && !training && alpha_rect_enabled();
  // a training forward leaves blend checkpoints of its long tile lists behind the binning blob
  // (common.h CK_*; the backward starts its segments from them)
  const bool with_ckpt = training && q.S == 0;
  // work-list classes of the frame's render.  A layered frame: the plain frame's classes, plus one flag per tile
  // -- does its list hold an object entry (preprocess sets the flags; they live in the image blob's checkpoint-count
  // area, which only a training forward uses) -- that sends short tiles WITH objects down the quarter-wave path
  const LayerArgs* const layers = q.layers;
  unsigned char* const tile_obj = layers ? (unsigned char*)(img + IL.ck_count) : nullptr;
  const uint32_t tile_obj_words = layers ? (T + 3u) / 4u : 0u;
  const TileClasses frame_classes = layers ? tile_classes_layers(tile_obj, cam.gx)
                                           : (binned_rects ? tile_classes_binned(q.S) : tile_classes(q.S));
  const LayerMarks marks = {layers ? layers->layer_class : nullptr, tile_obj, cam.gx};

  const FrameEpilogue* epi = q.epi;     // the request's, or epi_drained
  FrameEpilogue epi_drained;
  uint32_t drain_cnt_words = 0u;
  StageTimer tm{stream, g_timing_enabled};

  // ---- set by begin() (P > 0) ----
  HostWord* hw = nullptr;
  // where the speculative frame publishes its count: the thread's word, or the deferred frame's own
  uint32_t* pub_ptr = nullptr;          // ... as the device addresses it
  const uint32_t* pub_host = nullptr;   // ... as the host reads it, once pub_ev has fired
  hipEvent_t pub_ev = nullptr;
  CapKey ck{-1, 0, 0, 0};
  bool speculative = false;             // the tail is enqueued for remembered capacities, before the count is known
  // Fourth pass of the depth sort (sort.hip): needed when the visible depth keys span >= 2^27
  // values -- a property of the scene's scale that does not change from frame to frame.  Its two
  // launches are only enqueued when the previous frame of this shape needed them (or nothing is
  // known yet); a frame that turns out to need them without having them is rendered again.
  bool with_pass3 = true;
  // The binning blob and the capacities it is carved for, written by carve_bin() only.  Rcap: instances (point
  // list); Ccap: coarse (Gaussian, super-tile) pairs, <= Rcap.  All zero: not carved yet (no history / exact mode).
  char* bin = nullptr;
  BinLayout BL{};
  uint32_t Rcap = 0u, Ccap = 0u;
  const uint32_t* sorted_gid = nullptr; // ids in depth order, once the depth sort is enqueued

  // A frame whose bytes go to pinned host memory is DRAINED (render_fwd.hip FrameEpi) when its width allows whole
  // 16-byte pieces per tile row (W % 16 == 0; whole 64-byte lines per unit when W % 64 == 0): staging bytes in the n_contrib plane (an evaluation frame tracks no n_contrib: 4 bytes
  // per pixel lie idle), the units' arrival counters behind the layered frame's tile flags in the checkpoint-count
  // area (a training forward's; T / 4 of its 4 T words).  GRPG_DRAIN_WGS (experiments): workgroups that carry the
  // units, 0 = the blending waves store straight into host memory.
  void setup_drain() {
    if (!(epi && epi->rgb8 && epi->rgb8_host && (q.width & 15) == 0 && q.P > 0)) return;
    static const int drain_cfg = [] { const char* v = getenv("GRPG_DRAIN_WGS"); return v ? atoi(v) : FRAME_DRAIN_WGS; }();
    // every unit needs a slot (64 per drain wave, RW_WAVES waves per workgroup), the counters 3 T words at most
    const uint32_t NU = (uint32_t)((q.width + 63) / 64) * (uint32_t)cam.gy;
    uint32_t wgs = (uint32_t)drain_cfg > (NU + 255u) / 256u ? (uint32_t)drain_cfg : (NU + 255u) / 256u;
    if (wgs > 3u * T / 256u) wgs = 3u * T / 256u;
    if (drain_cfg > 0 && wgs > 0u && wgs * 256u >= NU) {
      epi_drained = *epi;
      epi_drained.drain_stage = (unsigned char*)(img + IL.n_contrib);
      epi_drained.drain_cnt = (uint32_t*)(img + IL.ck_count) + T;
      epi_drained.drain_wgs = (int)wgs;
      drain_cnt_words = wgs * 256u;
      epi = &epi_drained;
    }
  }

  // P == 0: the reference launches nothing and its pre-zeroed planes stay zero
  // (rasterize_points.cu:85-86,123); write the zeros explicitly.
  int empty_frame() {
    if (q.out_color) HIP_TRY(hipMemsetAsync(q.out_color, 0, 3 * N * 4, stream));
    if (q.out_depth) HIP_TRY(hipMemsetAsync(q.out_depth, 0, N * 4, stream));
    if (q.out_alpha) HIP_TRY(hipMemsetAsync(q.out_alpha, 0, N * 4, stream));
    if (epi) launch_frame_epilogue_empty(stream, q.width, q.height, *epi, q.out_color);   // sky over nothing, bytes
    if (q.S > 0 && q.out_semantic) HIP_TRY(hipMemsetAsync(q.out_semantic, 0, (size_t)q.S * N * 4, stream));
    HIP_TRY(hipMemsetAsync(n_contrib, 0, N * 4, stream));
    if (layers) {
      // ONE contract for an empty layer: its colour plane is layer_background, its alpha plane zero --
      // what the kernels write for an empty class when P > 0, and what the reference's render_kernel returns for a
      // model set without Gaussians (street_gaussian_renderer.py:131-144: ones on a white background, acc zeros)
      launch_fill_layer_planes(stream, N, layers->layer_background, layers->out_color_bg, layers->out_alpha_bg,
                               layers->out_color_obj, layers->out_alpha_obj);
    }
    char* bin0 = q.binning_alloc(bin_layout(0).total, q.binning_user);
    if (!bin0) return fail(GRPG_ERR_ALLOC, "binning buffer allocation failed");
    launch_frame_init(stream, geom, bin0, img, 0u, 0u, 0u, (uint32_t)q.width, (uint32_t)q.height,
                      (uint32_t)q.S, ranges, T, work, geom + GL.zero_begin, GL.zero_end - GL.zero_begin,
                      training);
    return GRPG_OK;
  }

  // The one place the binning blob and its capacities change: carved for `cap` instances and `ccap` coarse pairs
  // (+ the blend checkpoints of a training forward behind it).
  int carve_bin(uint32_t cap, uint32_t ccap) {
    Rcap = cap;
    Ccap = ccap;
    BL = hier ? bin_layout((size_t)Rcap, T, NS, Ccap) : bin_layout((size_t)Rcap);
    bin = q.binning_alloc(BL.total + (with_ckpt ? ckpt_bytes(ckpt_slots(Rcap)) : 0), q.binning_user);
    if (!bin) return fail(GRPG_ERR_ALLOC, "binning buffer allocation failed");
    return GRPG_OK;
  }

  // P > 0: the thread's pinned words, where the count is published, and whether the frame can be enqueued whole
  // for capacities remembered from earlier frames of its shape (then the blob is carved here)
  int begin(bool force_pass3) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hw = host_word();
    if (!hw) return fail(GRPG_ERR_HIP, "pinned host word / event allocation failed");
    if (int rc = check_async_error(hw)) return rc;
    pub_ptr = q.defer ? q.defer->dev_ptr : hw->dev_ptr;
    pub_host = q.defer ? q.defer->host_ptr : hw->host_ptr;
    pub_ev = q.defer ? q.defer->ev : hw->ev;
    ck = {dev, q.P, q.width, q.height};
    uint32_t ccap = 0u;
    bool hint_far = true;
    const uint32_t cap = spec_mode ? capacity_from_hint(ck, &ccap, &hint_far) : 0u;
    speculative = cap != 0u;
    with_pass3 = force_pass3 || !speculative || hint_far;
    return speculative ? carve_bin(cap, ccap) : GRPG_OK;
  }

  // composed frame -- segment table: host structs -> pinned staging -> the geometry blob (asynchronous copy)
  int stage_segments(SegmentDev* seg_dev) {
    if (!g_seg_staging)
      HIP_TRY(hipHostMalloc((void**)&g_seg_staging, sizeof(SegmentDev) * MAX_SEGMENTS, hipHostMallocDefault));
    fill_segments(g_seg_staging, q.segs, q.nseg, layers);
    HIP_TRY(hipMemcpyAsync(seg_dev, g_seg_staging, sizeof(SegmentDev) * (size_t)q.nseg,
                           hipMemcpyHostToDevice, stream));
    gather_device_poses(stream, seg_dev, q.nseg);
    return GRPG_OK;
  }

  // composed frame with feature planes -- the feature table like the segment table, then the producer kernel
  int stage_features(const SegmentDev* seg_dev) {
    if (!g_feat_staging)
      HIP_TRY(hipHostMalloc((void**)&g_feat_staging, sizeof(FeatureSegDev) * MAX_SEGMENTS, hipHostMallocDefault));
    for (int i = 0; i < q.nseg; i++)
      g_feat_staging[i] = FeatureSegDev{q.seg_semantic ? q.seg_semantic[i] : nullptr, nullptr, nullptr, nullptr};
    const FeatLayout FL = feat_layout((size_t)q.P, (size_t)q.S);
    FeatureSegDev* fdev = (FeatureSegDev*)(q.feat_blob + FL.table);
    HIP_TRY(hipMemcpyAsync(fdev, g_feat_staging, sizeof(FeatureSegDev) * (size_t)q.nseg, hipMemcpyHostToDevice, stream));
    launch_compose_features(stream, q.P, seg_dev, fdev, q.nseg, q.feat_S, q.feat_normals, q.cam_pos,
                            (float*)(q.feat_blob + FL.features));
    return GRPG_OK;
  }

  // Everything that does not depend on the binning capacities: frame init, preprocess, the count's publish, the
  // depth sort.  (A frame without a carved blob -- bin all zero -- initialises the other two blobs only.)
  int enqueue_head() {
    tm.mark(0);
    launch_frame_init(stream, geom, bin, img, (uint32_t)q.P, fat_sort ? 0u : (uint32_t)q.P, Rcap,
                      (uint32_t)q.width, (uint32_t)q.height, (uint32_t)q.S, ranges, T, work,
                      geom + GL.zero_begin, GL.zero_end - GL.zero_begin, training,
                      drain_cnt_words ? (uint32_t*)(img + IL.ck_count) : (uint32_t*)tile_obj,
                      drain_cnt_words ? T + drain_cnt_words : tile_obj_words);   // (drained: flags and counters in one sweep)
    if (q.segs == nullptr) {
      launch_preprocess(stream, q.P, q.D, q.M, q.means3D, q.scales, q.scale_modifier, q.rotations, q.opacities,
                        q.shs, q.cov3D_precomp, q.colors_precomp, cam, radii_int, rec_w, key_a, tiles, rects,
                        fat_sort ? ds_table : nullptr, pre_counts, marks, binned_rects);
    } else {
      // the frame's table: staged into the geometry blob, or the rows baked for it earlier, where they lie
      const SegmentDev* seg_dev = q.bound_rows;
      if (seg_dev == nullptr) {
        SegmentDev* staged = (SegmentDev*)(geom + GL.seg_table);
        if (int rc = stage_segments(staged)) return rc;
        seg_dev = staged;
      }
      launch_preprocess_composed(stream, q.P, q.D, q.M, seg_dev, q.nseg, q.scale_modifier, cam, radii_int, rec_w,
                                 key_a, tiles, rects, fat_sort ? ds_table : nullptr, pre_counts, marks, binned_rects);
      if (q.S > 0) {   // the frame's feature planes: [P,S] from the models' own arrays (features.hip)
        if (int rc = stage_features(seg_dev)) return rc;
      }
    }
    // num_rendered (and the coarse pair count) as sums of the per-Gaussian counts: in the pinned
    // word ~70 us into the frame, with an event behind it.  The host looks at it only after the
    // whole frame is enqueued (speculative mode) -- by then it has long arrived, so grpg_forward
    // returns the exact count without ever idling the stream or itself.
    // With the fat depth sort the sum rides in its first pass (one launch fewer; the count arrives
    // ~35 us later, still long before the host has enqueued the frame); the classic sort of very
    // large P: the separate one-workgroup launch right here.
    const bool fold_publish = fat_sort;
    if (!fold_publish) {
      launch_publish_counts(stream, pre_counts, (uint32_t)((q.P + 255) / 256), pub_ptr, &gh->R_pre);
      HIP_TRY(hipEventRecord(pub_ev, stream));
    }
    STAGE_CHECK("preprocess");
    tm.mark(1);
    // (depth_bits, id) order: stable sort of ids by the 32-bit depth key.
    if (fat_sort) {   // drops the culled Gaussians: V pairs remain
      const uint32_t pnb = (uint32_t)((q.P + 255) / 256);
      uint32_t* key_c = (uint32_t*)(geom + GL.key_c);
      uint32_t* val_c = (uint32_t*)(geom + GL.val_c);
      if (rect_sorted_by_sort)   // scratch: rect_sorted's own first half, the not yet written offsets, aux_c
        depth_sort_fat(stream, (uint32_t)q.P, key_a, val_a, key_b, val_b, key_c, val_c, ds_table,
                       GL.nchunks_ds, &gh->V, &gh->key_base, with_pass3,
                       rects, (uint32_t*)rect_sorted, offsets,
                       (uint32_t*)(geom + GL.aux_c), rect_sorted, tiles_sorted, pre_counts, pnb, fold_publish,
                       pub_ptr, &gh->R_pre, pub_ev);
      else
        depth_sort_fat(stream, (uint32_t)q.P, key_a, val_a, key_b, val_b, key_c, val_c, ds_table,
                       GL.nchunks_ds, &gh->V, &gh->key_base, with_pass3,
                       nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr, pre_counts, pnb, fold_publish, pub_ptr, &gh->R_pre, pub_ev);
      sorted_gid = val_a;
    } else {          // culled keys sort last (tile count 0); V stays P
      const bool in_b = radix_sort_pairs(stream, (uint32_t)q.P, nullptr, key_a, val_a, key_b, val_b, true,
                                         0, 32, table, totals, GL.nchunks_sort, false, tiles,
                                         tiles_sorted);
      sorted_gid = in_b ? val_b : val_a;  // 4 passes -> back in "a"
    }
    STAGE_CHECK("depth sort");
    tm.begin_tail();
    return GRPG_OK;
  }

  // The tail of the frame -- everything that works on the binning blob, and so is enqueued again after a capacity
  // overflow: the binning for the blob as carved, then the render.
  int enqueue_tail() {
    if (hier) return tail_hier();
    // sort path: exclusive offsets of the per-Gaussian tile counts in depth order (the count itself
    // is already on its way to the host, see enqueue_head)
    tm.mark(2);
    launch_offsets_scan(stream, (uint32_t)q.P, &gh->V, tiles_sorted, fat_sort ? sorted_gid : nullptr, tiles,
                        offsets, block_sums, GL.nblocks_scan, &gh->R, nullptr, emit_win,
                        GL.emit_win_cap);
    STAGE_CHECK("offsets scan");
    return tail_sort();
  }

  // sort path: everything behind the offsets scan
  int tail_sort() {
    const BinLayout& L = BL;
    const uint32_t cap = Rcap;
    const int tbits = bits_for(T);
    const int passes = radix_sort_num_passes(0, tbits);
    const int bits0 = radix_sort_first_pass_bits(0, tbits);
    uint32_t* bkey_a = (uint32_t*)(bin + L.key_a);
    uint32_t* bkey_b = (uint32_t*)(bin + L.key_b);
    uint32_t* bval_a = (uint32_t*)(bin + L.val_a);
    uint32_t* bval_b = (uint32_t*)(bin + L.val_b);
    uint32_t* btable = (uint32_t*)(bin + L.table);
    uint32_t* btotals = (uint32_t*)(bin + L.totals);
    tm.mark(3);
    // emit into whichever pair makes the LAST pass land in "a" (point_list lives in val_a)
    const bool start_in_b = (passes & 1) != 0;
    uint32_t *const key0 = start_in_b ? bkey_b : bkey_a, *const val0 = start_in_b ? bval_b : bval_a;
    uint32_t *const key1 = start_in_b ? bkey_a : bkey_b, *const val1 = start_in_b ? bval_a : bval_b;
    launch_emit(stream, &gh->V, &gh->R, cap, sorted_gid, offsets, emit_win, GL.emit_win_cap, rec,
                cam.gx, cam.gy, key0, val0, passes > 0 ? btable : nullptr, (1u << bits0) - 1u, L.nchunks_sort);
    STAGE_CHECK("emit");
    tm.mark(4);
    if (passes > 0 && cap > 0) {
      const bool in_1 = radix_sort_pairs(stream, cap, &gh->R, key0, val0, key1, val1, false, 0, tbits,
                                         btable, btotals, L.nchunks_sort, true);
      if ((in_1 ? key1 : key0) != bkey_a) return fail(GRPG_ERR_HIP, "internal: tile sort landed in the wrong buffer");
    }
    STAGE_CHECK("tile sort");
    tm.mark(5);
    launch_tile_ranges(stream, &gh->R, cap, bkey_a, ranges, T);
    STAGE_CHECK("tile ranges");
    return render_tail(bval_a, false);
  }

  // hierarchical path (hier_binning.hip): everything behind the depth sort.  Stage slots: 2 = scan
  // over the super-tile counts, 3 = coarse emit, 4 = coarse partition + super-tile runs,
  // 5 = segment counts, tile ranges and the point-list fill.
  int tail_hier() {
    const BinLayout& L = BL;
    char* const binp = bin;
    const uint32_t cap = Rcap, ccap = Ccap;
    const int sgx = (cam.gx + STILE - 1) / STILE, sgy = (cam.gy + STILE - 1) / STILE;
    const int cbits = bits_for(NS);
    const int cpasses = radix_sort_num_passes(0, cbits);
    const int cbits0 = radix_sort_first_pass_bits(0, cbits);
    uint32_t* ckey_a = (uint32_t*)(binp + L.key_a);
    uint32_t* ckey_b = (uint32_t*)(binp + L.key_b);
    uint32_t* cval_a = (uint32_t*)(binp + L.val_b);
    uint32_t* cval_b = (uint32_t*)(binp + L.val_c);
    uint32_t* plist = (uint32_t*)(binp + L.val_a);
    uint32_t* btable = (uint32_t*)(binp + L.table);
    uint32_t* btotals = (uint32_t*)(binp + L.totals);
    uint2* cranges = (uint2*)(binp + L.cranges);
    tm.mark(2);
    // counts and rectangles already in depth order (from the sort's last pass): the emit scans the offsets it
    // needs itself from the block sums (binning.hip emit_coarse_fused_kernel); otherwise the two-launch scan
    const bool fused_emit = rect_sorted_by_sort && emit_coarse_fused_ok(GL.nblocks_scan);
    if (fused_emit)
      launch_offsets_reduce(stream, (uint32_t)q.P, &gh->V, tiles_sorted, block_sums, GL.nblocks_scan);
    else if (rect_sorted_by_sort)
      launch_offsets_scan(stream, (uint32_t)q.P, &gh->V, tiles_sorted, nullptr, nullptr, offsets,
                          block_sums, GL.nblocks_scan, &gh->Rc, nullptr, emit_win, GL.emit_win_cap);
    else
      launch_offsets_scan(stream, (uint32_t)q.P, &gh->V, tiles_sorted, sorted_gid, nullptr, offsets,
                          block_sums, GL.nblocks_scan, &gh->Rc, nullptr, emit_win, GL.emit_win_cap, rects,
                          rect_sorted);
    STAGE_CHECK("coarse offsets scan");
    tm.mark(3);
    if (fused_emit)
      launch_emit_coarse_fused(stream, &gh->V, &gh->Rc, ccap, sorted_gid, tiles_sorted, block_sums,
                               GL.nblocks_scan, rect_sorted, sgx, ckey_a, cval_a, cpasses > 0 ? btable : nullptr,
                               (1u << cbits0) - 1u, L.nchunks_coarse, cranges, NS);
    else
      launch_emit_coarse(stream, &gh->V, &gh->Rc, ccap, sorted_gid, rect_sorted, offsets, emit_win,
                         GL.emit_win_cap, sgx, sgy, ckey_a, cval_a, cpasses > 0 ? btable : nullptr,
                         (1u << cbits0) - 1u, L.nchunks_coarse, cranges, NS);
    STAGE_CHECK("coarse emit");
    tm.mark(4);
    bool in_b = false;
    if (cpasses > 0 && ccap > 0)
      in_b = radix_sort_pairs(stream, ccap, &gh->Rc, ckey_a, cval_a, ckey_b, cval_b, false, 0, cbits,
                              btable, btotals, L.nchunks_coarse, true);
    STAGE_CHECK("coarse partition");
    const uint32_t* ckey = in_b ? ckey_b : ckey_a;
    // one pass (<= 256 super-tiles): its digit totals ARE the run lengths; otherwise find the runs
    const bool runs_from_totals = cpasses == 1 && ccap > 0;
    if (!runs_from_totals) launch_tile_ranges(stream, &gh->Rc, ccap, ckey, cranges, NS, 0xFFFFu);
    STAGE_CHECK("super-tile runs");
    tm.mark(5);
    const uint32_t* cval = in_b ? cval_b : cval_a;
    launch_hier_count(stream, cranges, runs_from_totals ? btotals : nullptr, NS, binp + L.seg_desc, (uint2*)(binp + L.st_seg),
                      (uint32_t*)(binp + L.nseg), L.max_seg, ckey, cam.gx, cam.gy,
                      (uint32_t*)(binp + L.seg_table), (uint32_t*)(binp + L.tile_tot),
                      (uint32_t*)(binp + L.tile_start), ranges, &gh->R, nullptr,
                      &gh->Rc, (BlobHeader*)binp, cap, ccap, work, frame_classes);
    STAGE_CHECK("tile counts");
    launch_hier_fill(stream, binp + L.seg_desc, (const uint32_t*)(binp + L.nseg), L.max_seg, ckey, cval, rec,
                     cam.gx, cam.gy, (const uint32_t*)(binp + L.seg_table),
                     (const uint32_t*)(binp + L.tile_start), cap, plist);
    STAGE_CHECK("point list fill");
    return render_tail(plist, true);
  }

  // the render over the finished point list (classified: the binning has already sorted the tiles into work lists)
  int render_tail(const uint32_t* point_list, bool classified) {
    const uint32_t cap = Rcap;
    tm.mark(6);
    const CkptArgs ckpt = {(float*)(bin + BL.total), (uint32_t*)(img + IL.ck_count),
                           (uint32_t*)(img + IL.bwd_ctl), (BlobHeader*)bin,
                           (uint32_t)(BL.total / 256), ckpt_slots(cap)};
    if (layers)
      launch_render_layers(stream, ranges, const_cast<uint32_t*>(point_list), rec, q.width, q.height, cam.gx, cam.gy,
                           q.background, q.out_color, q.out_depth, q.out_alpha, work, frame_classes, cap,
                           classified, layers->layer_background, layers->out_color_bg,
                           layers->out_alpha_bg, layers->out_color_obj, layers->out_alpha_obj,
                           PCErr{&((BlobHeader*)img)->pc_timeout, hw->dev_ptr + 3}, epi);
    else
      launch_render_forward(stream, ranges, point_list, rec, q.width, q.height, cam.gx, cam.gy, q.background,
                            q.out_color, q.out_depth, q.out_alpha, n_contrib, work, frame_classes, cap,
                            training, classified, with_ckpt ? &ckpt : nullptr,
                            PCErr{&((BlobHeader*)img)->pc_timeout, hw->dev_ptr + 3},
                            q.S > 0 ? q.semantics : nullptr, q.S, q.out_semantic, epi);
    STAGE_CHECK("render");
    if (debug)   // the stage check has synchronised: a hand-over timeout of THIS frame is known
      if (int rc = check_async_error(hw)) return rc;
    tm.mark(7);
    if (q.S > RENDER_NSEM) {   // the first RENDER_NSEM planes rode in the render launch
      launch_render_semantic(stream, ranges, point_list, rec, q.semantics, q.S, RENDER_NSEM, q.width, q.height,
                             cam.gx, cam.gy, q.out_semantic);
      STAGE_CHECK("semantic render");
    }
    tm.mark(-1);
    return GRPG_OK;
  }

  // A blob for the counts just read.  First frame of a shape / exact mode: nothing was carved yet.  Capacity
  // overflow: the speculative tail clamped its work to the old capacities and its results are discarded (tile
  // ranges and work lists are cleared again); both counts are exact, so one redo on a larger blob settles it.
  int recarve(uint32_t R, uint32_t Rc) {
    uint32_t cap = Rcap, ccap = Ccap;
    if (!speculative) {
      cap = spec_mode ? padded_capacity(R) : R;
      ccap = hier ? (spec_mode ? padded_capacity(Rc) : Rc) : cap;
    } else {
      if (R > Rcap) cap = padded_capacity(R);
      if (hier && Rc > Ccap) ccap = padded_capacity(Rc);
    }
    if (ccap > cap) ccap = cap;     // a (Gaussian, super-tile) pair holds >= 1 instance
    const bool redo = speculative;
    if (redo) tm.restart_tail();
    if (int rc = carve_bin(cap, ccap)) return rc;
    launch_bin_header(stream, bin, (uint32_t)q.P, Rcap, (uint32_t)q.width, (uint32_t)q.height, (uint32_t)q.S,
                      redo ? ranges : nullptr, T, redo ? work : nullptr);
    return GRPG_OK;
  }
};

// Shared body of every forward entry point.
// Speculative (capacities remembered from earlier frames of this shape): the whole frame is enqueued, then the host
// reads the count (published right behind preprocess: normally there already).  No history / exact
// mode: read the count first, carve the blob for it, then enqueue the tail -- like the
// reference's one blocking read (rasterizer_impl.cu:284), only much earlier in the frame.
int forward_impl(const FrameRequest& q, bool force_pass3 = false) {
  if (int rc = begin_call()) return rc;
  if (int rc = validate(q)) return rc;
  const CameraArgs cam = make_camera(q.viewmatrix, q.projmatrix, q.cam_pos, q.width, q.height, q.tan_fovx, q.tan_fovy);
  // an evaluation frame carves the geometry blob without the gradient records
  const GeomLayout GL = geom_layout((size_t)q.P, q.training());
  const ImgLayout IL = img_layout(num_tiles(cam), (size_t)q.width * q.height);
  char* geom = q.geometry_alloc(GL.total, q.geometry_user);
  char* img = q.image_alloc(IL.total, q.image_user);
  if (!geom || !img) return fail(GRPG_ERR_ALLOC, "geometry/image buffer allocation failed");
  remember_geom(geom, q.P, q.training());
  Frame f(q, cam, GL, IL, geom, img);
  DeferSlot* const defer = q.defer;
  uint32_t R = 0;
  if (q.P == 0) {
    if (int rc = f.empty_frame()) return rc;
  } else {
    if (int rc = f.begin(force_pass3)) return rc;
    if (int rc = f.enqueue_head()) return rc;
    if (f.speculative) {
      if (int rc = f.enqueue_tail()) return rc;
      if (defer) {
        // deferred frame: the count is checked by grpg_frame_status, nothing to wait for here
        defer->state = 1;
        defer->Rcap = f.Rcap; defer->Ccap = f.Ccap; defer->hier = f.hier; defer->key = f.ck;
        defer->with_pass3 = f.with_pass3 || !f.fat_sort;
        f.tm.finish();
        return 0;
      }
    }
    // the counts as published behind preprocess: num_rendered, coarse pairs, did the depth keys need the fourth pass
    HIP_TRY(hipEventSynchronize(f.pub_ev));
    R = f.pub_host[0];
    const uint32_t Rc = f.hier ? f.pub_host[1] : 0u;
    const bool far = f.fat_sort && f.pub_host[2] != 0u;
    if (R > 0x7FFFFFFFu) return fail(GRPG_ERR_INVALID_ARGUMENT, "num_rendered exceeds int32");
    if (far && !f.with_pass3) {
      // the scene's depth range grew beyond what three sort passes order: this frame's lists are in
      // the wrong order.  Remember it and render the frame again, this time with the fourth pass.
      update_hint(f.ck, R, Rc, true);
      return forward_impl(q, true);
    }
    if (!f.speculative || R > f.Rcap || (f.hier && Rc > f.Ccap)) {
      if (int rc = f.recarve(R, Rc)) return rc;
      if (int rc = f.enqueue_tail()) return rc;
    }
    update_hint(f.ck, R, Rc, far);
    f.tm.finish();
    if (defer) { defer->state = 2; defer->result = (int)R; }   // no capacity history: ran synchronously
  }
  if (defer && defer->state == 0) { defer->state = 2; defer->result = (int)R; }
  return (int)R;
}

// ---- deferred frames: slot management ----
int defer_resolve(DeferSlot& d, bool wait) {
  if (d.state == 2) return d.result;
  if (d.state != 1) return fail(GRPG_ERR_INVALID_ARGUMENT, "ticket does not name a frame in flight");
  if (wait) {
    HIP_TRY(hipEventSynchronize(d.ev));
  } else {
    const hipError_t q = hipEventQuery(d.ev);
    if (q == hipErrorNotReady) return GRPG_ERR_NOT_READY;
    if (q != hipSuccess) return fail(GRPG_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
  }
  const uint32_t R = d.host_ptr[0], Rc = d.hier ? d.host_ptr[1] : 0u;
  const bool far = d.host_ptr[2] != 0u;
  // a clamped coarse list undercounts R; either overflow invalidates the frame's outputs -- and so
  // does a depth range that needed the fourth sort pass the frame was enqueued without
  const bool ok = R <= d.Rcap && (!d.hier || Rc <= d.Ccap) && R <= 0x7FFFFFFFu && (!far || d.with_pass3);
  update_hint(d.key, R > Rc ? R : Rc, Rc, far);   // (an undercounted R is at least the coarse count)
  d.state = 2;
  d.result = ok ? (int)R : GRPG_ERR_CAPACITY;
  return d.result;
}

DeferSlot* defer_acquire(int* ticket) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  const int idx = g_defer_next;
  g_defer_next = (g_defer_next + 1) % DEFER_SLOTS;
  DeferSlot& d = g_defer[idx];
  if (d.state == 1) (void)defer_resolve(d, true);   // comes round while pending: look at it now
  if (d.host_ptr && d.dev != dev) {                  // pinned words map into one device's space
    (void)hipHostFree(d.host_ptr);
    (void)hipEventDestroy(d.ev);
    const int gen = d.generation;
    d = DeferSlot{};
    d.generation = gen;
  }
  if (!d.host_ptr) {
    if (hipHostMalloc((void**)&d.host_ptr, 64, hipHostMallocMapped) != hipSuccess) return nullptr;
    if (hipHostGetDevicePointer((void**)&d.dev_ptr, d.host_ptr, 0) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&d.ev, hipEventDisableTiming) != hipSuccess) return nullptr;
    d.dev = dev;
  }
  d.host_ptr[0] = 0u; d.host_ptr[1] = 0u; d.host_ptr[2] = 0u;
  d.state = 0; d.result = 0;
  d.generation = (d.generation + 1) & 0xFFFFF;
  *ticket = d.generation * DEFER_SLOTS + idx;
  return &d;
}

int check_segments(const grpg_model_segment* segs, int nseg, int M, long long* P_out) {
  if (!segs || nseg <= 0 || nseg > GRPG_MAX_SEGMENTS)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "need 1..GRPG_MAX_SEGMENTS segments");
  long long P = 0;
  for (int i = 0; i < nseg; i++) {
    const grpg_model_segment& g = segs[i];
    if (g.count <= 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "segment with count <= 0");
    if (!g.xyz || !g.scaling || !g.rotation || !g.opacity || !g.features_dc || (M > 1 && !g.features_rest))
      return fail(GRPG_ERR_INVALID_ARGUMENT, "segment with a NULL parameter array");
    if (g.fourier_dim < 1 || g.fourier_dim > GRPG_MAX_FOURIER)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "fourier_dim must be in 1..GRPG_MAX_FOURIER");
    P += g.count;
  }
  if (P > (long long)ID_MASK) return fail(GRPG_ERR_INVALID_ARGUMENT, "P must be < 2^28");
  if (g_pose_cur.set) {   // the device poses bound for this call (grpg_bind_device_poses) must fit its segments
    if (g_pose_cur.n != nseg)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "device poses were bound for another number of segments");
    for (int i = 0; i < nseg; i++)
      if (g_pose_cur.row[i] >= 0 && segs[i].rigid == 0)
        return fail(GRPG_ERR_INVALID_ARGUMENT, "a device pose row names a static segment (rigid == 0)");
  }
  *P_out = P;
  return GRPG_OK;
}

// the model of a composed entry point: its segments and the SH degree they share -> P
int check_composed_model(const grpg_model_segment* segs, int nseg, int D, int M, long long* P_out) {
  if (int rc = check_segments(segs, nseg, M, P_out)) return rc;
  if (M < 1 || M > 16 || D < 0 || D > 3 || (D + 1) * (D + 1) > M)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "SH degree needs (D+1)^2 <= M <= 16");
  return GRPG_OK;
}

// The layer arguments of an entry point -> *out: &la for a layered frame, NULL for a plain one.  The layer planes
// come all four or not at all; `optional` (grpg_forward_frame / _composed_frame): none of them is a plain frame,
// otherwise (the _layers entries) all four are required.  `flat`: layer_class classes the Gaussians (a composed
// frame's segment_class may be NULL).
int check_layers(const LayerArgs& la, long long P, bool flat, bool optional, const LayerArgs** out) {
  const int n = (la.out_color_bg != nullptr) + (la.out_alpha_bg != nullptr) + (la.out_color_obj != nullptr) +
                (la.out_alpha_obj != nullptr);
  *out = nullptr;
  if (optional) {
    if (n == 0) return GRPG_OK;
    if (n != 4) return fail(GRPG_ERR_INVALID_ARGUMENT, "layer planes: give all four or none");
    if (!la.layer_background || (flat && P > 0 && !la.layer_class))
      return fail(GRPG_ERR_INVALID_ARGUMENT, flat ? "a layered frame needs layer_class and layer_background"
                                                  : "a layered frame needs layer_background");
  } else {
    if (!la.layer_background || n != 4)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL layer background / layer plane pointer");
    if (flat && P > 0 && !la.layer_class) return fail(GRPG_ERR_INVALID_ARGUMENT, "layer_class NULL");
  }
  if ((unsigned long long)P >= (1ull << 27))   // (a negative P of a flat entry as well)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "a layered frame needs P < 2^27 (the class travels in bit 27 of the point list)");
  *out = &la;
  return GRPG_OK;
}

}  // namespace

extern "C" {

int grpg_forward(grpg_alloc_fn geometry_alloc, void* geometry_user, grpg_alloc_fn binning_alloc,
                 void* binning_user, grpg_alloc_fn image_alloc, void* image_user, int P, int D,
                 int M, int S, const float* background, int width, int height,
                 const float* means3D, const float* shs, const float* colors_precomp,
                 const float* semantics, const float* opacities, const float* scales,
                 float scale_modifier, const float* rotations, const float* cov3D_precomp,
                 const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                 float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                 float* out_depth, float* out_alpha, float* out_semantic, int* radii, int debug,
                 void* hip_stream) {
  // (prefiltered -- reference: __trap() on a culled point when set; always False in practice)
  return grpg_forward_flags(geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user, P, D,
                            M, S, background, width, height, means3D, shs, colors_precomp, semantics, opacities,
                            scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos,
                            tan_fovx, tan_fovy, prefiltered, out_color, out_depth, out_alpha, out_semantic, radii,
                            debug, hip_stream, 0u);
}

int grpg_forward_flags(grpg_alloc_fn geometry_alloc, void* geometry_user, grpg_alloc_fn binning_alloc,
                       void* binning_user, grpg_alloc_fn image_alloc, void* image_user, int P, int D,
                       int M, int S, const float* background, int width, int height,
                       const float* means3D, const float* shs, const float* colors_precomp,
                       const float* semantics, const float* opacities, const float* scales,
                       float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                       float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                       float* out_depth, float* out_alpha, float* out_semantic, int* radii, int debug,
                       void* hip_stream, unsigned flags) {
  (void)prefiltered;
  FrameRequest q;
  set_allocators(q, geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user);
  set_model(q, P, D, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp);
  set_camera(q, background, width, height, scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
             out_color, out_depth, out_alpha, radii, debug, hip_stream, flags);
  q.S = S; q.semantics = semantics; q.out_semantic = out_semantic;
  return forward_impl(q);
}

int grpg_forward_layers(grpg_alloc_fn geometry_alloc, void* geometry_user, grpg_alloc_fn binning_alloc,
                        void* binning_user, grpg_alloc_fn image_alloc, void* image_user, int P, int D, int M,
                        const float* background, int width, int height, const float* means3D,
                        const float* shs, const float* colors_precomp, const float* opacities,
                        const float* scales, float scale_modifier, const float* rotations,
                        const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                        const float* cam_pos, float tan_fovx, float tan_fovy,
                        const unsigned char* layer_class, const float* layer_background, float* out_color,
                        float* out_depth, float* out_alpha, float* out_color_bg, float* out_alpha_bg,
                        float* out_color_obj, float* out_alpha_obj, int* radii, int debug, void* hip_stream) {
  g_last_error.clear();
  const LayerArgs la = {nullptr, layer_class, layer_background, out_color_bg, out_alpha_bg, out_color_obj, out_alpha_obj};
  FrameRequest q;
  if (int rc = check_layers(la, P, true, false, &q.layers)) return rc;
  set_allocators(q, geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user);
  set_model(q, P, D, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp);
  set_camera(q, background, width, height, scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
             out_color, out_depth, out_alpha, radii, debug, hip_stream, GRPG_FORWARD_NO_BACKWARD);
  return forward_impl(q);
}

int grpg_forward_deferred(grpg_alloc_fn geometry_alloc, void* geometry_user, grpg_alloc_fn binning_alloc,
                          void* binning_user, grpg_alloc_fn image_alloc, void* image_user, int P, int D,
                          int M, int S, const float* background, int width, int height,
                          const float* means3D, const float* shs, const float* colors_precomp,
                          const float* semantics, const float* opacities, const float* scales,
                          float scale_modifier, const float* rotations, const float* cov3D_precomp,
                          const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                          float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                          float* out_depth, float* out_alpha, float* out_semantic, int* radii, int debug,
                          void* hip_stream, unsigned flags, int* ticket) {
  (void)prefiltered;
  if (int rc = begin_call()) return rc;
  if (!ticket) return fail(GRPG_ERR_INVALID_ARGUMENT, "ticket must not be NULL");
  DeferSlot* d = defer_acquire(ticket);
  if (!d) return fail(GRPG_ERR_HIP, "pinned status words / event allocation failed");
  FrameRequest q;
  set_allocators(q, geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user);
  set_model(q, P, D, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp);
  set_camera(q, background, width, height, scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
             out_color, out_depth, out_alpha, radii, debug, hip_stream, flags);
  q.S = S; q.semantics = semantics; q.out_semantic = out_semantic; q.defer = d;
  const int rc = forward_impl(q);
  if (rc < 0) { d->state = 2; d->result = rc; return rc; }
  return GRPG_OK;
}

int grpg_frame_status(int ticket, int wait, int* num_rendered) {
  g_last_error.clear();
  if (ticket < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "no such ticket");
  DeferSlot& slot = g_defer[ticket % DEFER_SLOTS];
  if (slot.generation != ticket / DEFER_SLOTS || slot.state == 0)
    return fail(GRPG_ERR_INVALID_ARGUMENT,
                "no such ticket on this thread: tickets are valid only on the thread that enqueued the "
                "frame, and only until GRPG_MAX_DEFERRED_FRAMES (64) later frames have been enqueued there");
  for (auto& hw : g_host_words)
    if (int rc = check_async_error(&hw)) return rc;
  const int r = defer_resolve(slot, wait != 0);
  if (r >= 0) { if (num_rendered) *num_rendered = r; return GRPG_OK; }
  if (r == GRPG_ERR_CAPACITY)
    g_last_error = "the frame overflowed the capacity it was enqueued with; render it again";
  return r;
}

// Pure host bookkeeping: needs no device (the consuming call looks for one).  A bad binding is refused here and
// replaces nothing -- but a binding that was pending is dropped either way: the caller meant to replace it.
int grpg_bind_device_poses(const float* pose_rot, const float* pose_trans, const int* pose_row, int num_segments) {
  g_last_error.clear();
  g_pose_pending.clear();
  if (!pose_row || num_segments <= 0 || num_segments > GRPG_MAX_SEGMENTS)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "device poses: need pose_row and 1..GRPG_MAX_SEGMENTS segments");
  bool any = false;
  for (int i = 0; i < num_segments; i++) {
    if (pose_row[i] < -1 || pose_row[i] >= (1 << 28))
      return fail(GRPG_ERR_INVALID_ARGUMENT, "device poses: a pose_row entry is -1 or a row index below 2^28");
    any = any || pose_row[i] >= 0;
  }
  if (any && (!pose_rot || !pose_trans))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "device poses: NULL pose_rot / pose_trans with a row bound");
  g_pose_pending.set = true; g_pose_pending.any = any;
  g_pose_pending.rot = pose_rot; g_pose_pending.trans = pose_trans; g_pose_pending.n = num_segments;
  memcpy(g_pose_pending.row, pose_row, sizeof(int) * (size_t)num_segments);
  return GRPG_OK;
}

int grpg_device_poses_bound(void) { return g_pose_pending.set ? 1 : 0; }

// Pure host bookkeeping as well.  A refused bind leaves no binding (the caller meant to replace the pending one).
int grpg_bind_frame_correction(const float* affine_device) {
  g_last_error.clear();
  g_affine_pending = nullptr;
  if (!affine_device) return fail(GRPG_ERR_INVALID_ARGUMENT, "frame correction: NULL affine matrix");
  g_affine_pending = affine_device;
  return GRPG_OK;
}

int grpg_frame_correction_bound(void) { return g_affine_pending ? 1 : 0; }

size_t grpg_frame_tables_bytes(long long total_rows) {
  return total_rows > 0 ? sizeof(SegmentDev) * (size_t)total_rows : 0;
}

// Bind time: the static part of every frame's rows through fill_segments itself (so a baked row and a staged row are
// the same bytes by construction), one upload, one launch for the tracked poses, one wait.
int grpg_frame_tables_bake(void* rows_device, const grpg_model_segment* models, int num_models, const int* frame_first,
                           int num_frames, const int* row_model, const int* row_pose, const float* row_idft,
                           const unsigned char* row_class, const float* pose_rot, const float* pose_trans,
                           long long num_pose_rows, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (!rows_device || ((uintptr_t)rows_device & 15u) || !models || num_models <= 0 || !frame_first || num_frames <= 0 ||
      !row_model || !row_pose || !row_idft)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "frame tables: NULL or misaligned pointer, or no models / frames");
  if (num_pose_rows < 0 || num_pose_rows >= (1ll << 28))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "frame tables: num_pose_rows must be in 0..2^28-1");
  if (frame_first[0] != 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "frame tables: frame_first[0] must be 0");
  for (int k = 0; k < num_frames; k++) {
    const long long n = (long long)frame_first[k + 1] - frame_first[k];
    if (n < 1 || n > GRPG_MAX_SEGMENTS)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "frame tables: every frame needs 1..GRPG_MAX_SEGMENTS rows");
  }
  const long long R = frame_first[num_frames];
  bool any = false;
  for (long long i = 0; i < R; i++) {
    if (row_model[i] < 0 || row_model[i] >= num_models)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "frame tables: a row names a model outside the scene");
    if (row_pose[i] < -1 || row_pose[i] >= num_pose_rows)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "frame tables: a pose row is neither -1 nor a row of the pose tables");
    if (row_pose[i] >= 0 && models[row_model[i]].rigid == 0)
      return fail(GRPG_ERR_INVALID_ARGUMENT, "frame tables: a pose row names a static model (rigid == 0)");
    any = any || row_pose[i] >= 0;
  }
  if (any && (!pose_rot || !pose_trans))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "frame tables: NULL pose_rot / pose_trans with a pose row given");
  const hipStream_t stream = (hipStream_t)hip_stream;
  SegmentDev* host = nullptr;
  HIP_TRY(hipHostMalloc((void**)&host, sizeof(SegmentDev) * (size_t)R, hipHostMallocDefault));
  std::vector<grpg_model_segment> segs;
  int rc = GRPG_OK;
  for (int k = 0; k < num_frames && rc == GRPG_OK; k++) {
    const int first = frame_first[k], n = frame_first[k + 1] - first;
    segs.resize((size_t)n);
    for (int i = 0; i < n; i++) {
      segs[i] = models[row_model[first + i]];
      memcpy(segs[i].idft, row_idft + (size_t)GRPG_MAX_FOURIER * (size_t)(first + i), sizeof(float) * GRPG_MAX_FOURIER);
    }
    long long P = 0;
    // the checks of a composed call on these segments (features_rest: the consuming call knows M); outside a
    // PoseScope no device-pose binding is current, so fill_segments parks nothing: the tape's own rows follow
    rc = check_segments(segs.data(), n, 1, &P);
    if (rc != GRPG_OK) break;
    const LayerArgs la = {row_class ? row_class + first : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    fill_segments(host + first, segs.data(), n, row_class ? &la : nullptr);
    for (int i = 0; i < n; i++)
      if (row_pose[first + i] >= 0) {
        const int parked = row_pose[first + i] + 1;
        memcpy(&host[first + i].pad0, &parked, sizeof(parked));
      }
  }
  hipError_t e = hipSuccess;
  if (rc == GRPG_OK) {
    e = hipMemcpyAsync(rows_device, host, sizeof(SegmentDev) * (size_t)R, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && any) {
      launch_frame_table_bake(stream, (SegmentDev*)rows_device, R, pose_rot, pose_trans);
      e = hipGetLastError();
    }
    const hipError_t w = hipStreamSynchronize(stream);   // the staging is freed below
    if (e == hipSuccess) e = w;
  }
  (void)hipHostFree(host);
  if (rc != GRPG_OK) return rc;
  if (e != hipSuccess) return fail(GRPG_ERR_HIP, std::string("frame tables: ") + hipGetErrorString(e));
  return GRPG_OK;
}

// A refused bind leaves no binding (the caller meant to replace the pending one).
int grpg_bind_frame_table(const void* rows_device, int num_segments, int P) {
  g_table_pending = TableBinding{};
  if (int rc = begin_call()) return rc;
  if (!rows_device || ((uintptr_t)rows_device & 15u))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "frame table: NULL or misaligned rows");
  if (num_segments <= 0 || num_segments > GRPG_MAX_SEGMENTS || P <= 0 || (unsigned)P > ID_MASK)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "frame table: need 1..GRPG_MAX_SEGMENTS segments and 0 < P < 2^28");
  g_table_pending.rows = (const SegmentDev*)rows_device;
  g_table_pending.n = num_segments;
  g_table_pending.P = P;
  return GRPG_OK;
}

int grpg_frame_tables_bound(void) { return g_table_pending.rows ? 1 : 0; }

int grpg_forward_composed_flags(grpg_alloc_fn geometry_alloc, void* geometry_user,
                                grpg_alloc_fn binning_alloc, void* binning_user,
                                grpg_alloc_fn image_alloc, void* image_user,
                                const grpg_model_segment* segments, int num_segments, int D, int M,
                                const float* background, int width, int height, float scale_modifier,
                                const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                                float tan_fovx, float tan_fovy, float* out_color, float* out_depth,
                                float* out_alpha, int* radii, int debug, void* hip_stream, unsigned flags) {
  PoseScope poses;
  const TableBinding table = take_frame_table();
  if (int rc = begin_call()) return rc;
  long long P = 0;
  if (int rc = check_composed_model(segments, num_segments, D, M, &P)) return rc;
  FrameRequest q;
  set_allocators(q, geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user);
  set_model(q, segments, num_segments, P, D, M);
  set_camera(q, background, width, height, scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
             out_color, out_depth, out_alpha, radii, debug, hip_stream, flags);
  if (int rc = attach_frame_table(table, q)) return rc;
  return forward_impl(q);
}

int grpg_forward_composed_layers(grpg_alloc_fn geometry_alloc, void* geometry_user,
                                 grpg_alloc_fn binning_alloc, void* binning_user,
                                 grpg_alloc_fn image_alloc, void* image_user,
                                 const grpg_model_segment* segments, int num_segments,
                                 const unsigned char* segment_class, int D, int M,
                                 const float* background, const float* layer_background, int width, int height,
                                 float scale_modifier, const float* viewmatrix, const float* projmatrix,
                                 const float* cam_pos, float tan_fovx, float tan_fovy, float* out_color,
                                 float* out_depth, float* out_alpha, float* out_color_bg, float* out_alpha_bg,
                                 float* out_color_obj, float* out_alpha_obj, int* radii, int debug,
                                 void* hip_stream) {
  PoseScope poses;
  const TableBinding table = take_frame_table();
  if (int rc = begin_call()) return rc;
  long long P = 0;
  if (int rc = check_composed_model(segments, num_segments, D, M, &P)) return rc;
  const LayerArgs la = {segment_class, nullptr, layer_background, out_color_bg, out_alpha_bg, out_color_obj, out_alpha_obj};
  FrameRequest q;
  if (int rc = check_layers(la, P, false, false, &q.layers)) return rc;
  set_allocators(q, geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user);
  set_model(q, segments, num_segments, P, D, M);
  set_camera(q, background, width, height, scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
             out_color, out_depth, out_alpha, radii, debug, hip_stream, GRPG_FORWARD_NO_BACKWARD);
  if (int rc = attach_frame_table(table, q)) return rc;
  return forward_impl(q);
}

// grpg_frame_epilogue -> FrameEpilogue (pointers checked); returns GRPG_OK or fails
static int resolve_epilogue(const grpg_frame_epilogue* e, bool planes, FrameEpilogue* out) {
  if (e->sky_cube != nullptr && (e->sky_res <= 0 || e->ray_matrix == nullptr))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "frame epilogue: the sky composite needs sky_res > 0 and a ray matrix");
  out->sky_cube = e->sky_cube; out->sky_res = e->sky_res;
  out->ray_m_dev = (e->sky_cube && e->ray_matrix_on_device) ? e->ray_matrix : nullptr;
  for (int i = 0; i < 9; i++) out->ray_m[i] = (e->sky_cube && !e->ray_matrix_on_device) ? e->ray_matrix[i] : 0.f;
  out->sky_fill = e->sky_fill; out->clamp = e->clamp; out->rgb8 = e->out_rgb8; out->truncate = e->truncate;
  out->rgb8_host = (e->out_rgb8 != nullptr && e->out_rgb8_on_host) ? 1 : 0;
  out->planes = planes ? 1 : 0;
  return GRPG_OK;
}

int grpg_forward_frame(grpg_alloc_fn geometry_alloc, void* geometry_user, grpg_alloc_fn binning_alloc,
                       void* binning_user, grpg_alloc_fn image_alloc, void* image_user, int P, int D, int M,
                       const float* background, int width, int height, const float* means3D, const float* shs,
                       const float* colors_precomp, const float* opacities, const float* scales,
                       float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                       float tan_fovy, const unsigned char* layer_class, const float* layer_background,
                       float* out_color, float* out_depth, float* out_alpha, float* out_color_bg,
                       float* out_alpha_bg, float* out_color_obj, float* out_alpha_obj, int* radii, int debug,
                       void* hip_stream, const grpg_frame_epilogue* epilogue) {
  g_last_error.clear();
  const float* affine = take_frame_correction();
  const LayerArgs la = {nullptr, layer_class, layer_background, out_color_bg, out_alpha_bg, out_color_obj, out_alpha_obj};
  FrameRequest q;
  if (int rc = check_layers(la, P, true, true, &q.layers)) return rc;
  FrameEpilogue fe{};
  if (epilogue) {
    if (int rc = resolve_epilogue(epilogue, out_color && out_depth && out_alpha, &fe)) return rc;
    q.epi = &fe;
  }
  if (int rc = attach_frame_correction(affine, epilogue ? &fe : nullptr)) return rc;
  set_allocators(q, geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user);
  set_model(q, P, D, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp);
  set_camera(q, background, width, height, scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
             out_color, out_depth, out_alpha, radii, debug, hip_stream, GRPG_FORWARD_NO_BACKWARD);
  return forward_impl(q);
}

int grpg_forward_composed_frame(grpg_alloc_fn geometry_alloc, void* geometry_user, grpg_alloc_fn binning_alloc,
                                void* binning_user, grpg_alloc_fn image_alloc, void* image_user,
                                const grpg_model_segment* segments, int num_segments,
                                const unsigned char* segment_class, int D, int M, const float* background,
                                const float* layer_background, int width, int height, float scale_modifier,
                                const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                                float tan_fovx, float tan_fovy, float* out_color, float* out_depth,
                                float* out_alpha, float* out_color_bg, float* out_alpha_bg, float* out_color_obj,
                                float* out_alpha_obj, int* radii, int debug, void* hip_stream,
                                const grpg_frame_epilogue* epilogue) {
  PoseScope poses;
  const float* affine = take_frame_correction();
  const TableBinding table = take_frame_table();
  if (int rc = begin_call()) return rc;
  long long P = 0;
  if (int rc = check_composed_model(segments, num_segments, D, M, &P)) return rc;
  const LayerArgs la = {segment_class, nullptr, layer_background, out_color_bg, out_alpha_bg, out_color_obj, out_alpha_obj};
  FrameRequest q;
  if (int rc = check_layers(la, P, false, true, &q.layers)) return rc;
  FrameEpilogue fe{};
  if (epilogue) {
    if (int rc = resolve_epilogue(epilogue, out_color && out_depth && out_alpha, &fe)) return rc;
    q.epi = &fe;
  }
  if (int rc = attach_frame_correction(affine, epilogue ? &fe : nullptr)) return rc;
  set_allocators(q, geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user);
  set_model(q, segments, num_segments, P, D, M);
  set_camera(q, background, width, height, scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
             out_color, out_depth, out_alpha, radii, debug, hip_stream, GRPG_FORWARD_NO_BACKWARD);
  if (int rc = attach_frame_table(table, q)) return rc;
  return forward_impl(q);
}

int grpg_forward_composed(grpg_alloc_fn geometry_alloc, void* geometry_user,
                          grpg_alloc_fn binning_alloc, void* binning_user,
                          grpg_alloc_fn image_alloc, void* image_user,
                          const grpg_model_segment* segments, int num_segments, int D, int M,
                          const float* background, int width, int height, float scale_modifier,
                          const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                          float tan_fovx, float tan_fovy, float* out_color, float* out_depth,
                          float* out_alpha, int* radii, int debug, void* hip_stream) {
  PoseScope poses;
  return grpg_forward_composed_flags(geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc,
                                     image_user, segments, num_segments, D, M, background, width, height,
                                     scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
                                     out_color, out_depth, out_alpha, radii, debug, hip_stream,
                                     GRPG_FORWARD_NO_BACKWARD);
}

// the channel split of a composed frame's feature planes: S >= 0, normals 0 / 1 -> F
static int check_feature_split(int S, int normals, int* F) {
  if (S < 0 || (normals != 0 && normals != 1))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "feature planes: S must be >= 0 and normals 0 or 1");
  *F = 3 * normals + S;
  return GRPG_OK;
}

int grpg_forward_composed_features(grpg_alloc_fn geometry_alloc, void* geometry_user, grpg_alloc_fn binning_alloc,
                                   void* binning_user, grpg_alloc_fn image_alloc, void* image_user,
                                   grpg_alloc_fn feature_alloc, void* feature_user,
                                   const grpg_model_segment* segments, int num_segments,
                                   const float* const* seg_semantic, int S, int normals, int D, int M,
                                   const float* background, int width, int height, float scale_modifier,
                                   const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                                   float tan_fovx, float tan_fovy, float* out_color, float* out_depth,
                                   float* out_alpha, float* out_features, int* radii, int debug, void* hip_stream,
                                   unsigned flags) {
  PoseScope poses;
  if (take_frame_table().rows != nullptr) {   // (gone, like every binding its call refuses)
    g_last_error.clear();
    return fail(GRPG_ERR_INVALID_ARGUMENT, "a frame table was bound in front of a frame with feature planes");
  }
  if (int rc = begin_call()) return rc;
  long long P = 0;
  if (int rc = check_composed_model(segments, num_segments, D, M, &P)) return rc;
  int F = 0;
  if (int rc = check_feature_split(S, normals, &F)) return rc;
  if (!feature_alloc) return fail(GRPG_ERR_INVALID_ARGUMENT, "buffer allocators must not be NULL");
  if (F > 0 && !out_features) return fail(GRPG_ERR_INVALID_ARGUMENT, "semantics/out_semantic NULL with S>0");
  if (normals && !cam_pos) return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL camera/background/output pointer");
  const FeatLayout FL = feat_layout((size_t)P, (size_t)F);
  char* blob = feature_alloc(FL.total, feature_user);
  if (!blob) return fail(GRPG_ERR_ALLOC, "feature buffer allocation failed");
  FrameRequest q;
  set_allocators(q, geometry_alloc, geometry_user, binning_alloc, binning_user, image_alloc, image_user);
  set_model(q, segments, num_segments, P, D, M);
  set_camera(q, background, width, height, scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy,
             out_color, out_depth, out_alpha, radii, debug, hip_stream, flags);
  q.seg_semantic = seg_semantic; q.feat_S = S; q.feat_normals = normals; q.feat_blob = blob;
  q.S = F; q.semantics = (const float*)(blob + FL.features); q.out_semantic = out_features;
  return forward_impl(q);
}

// Shared body of grpg_backward_composed (F = 0), grpg_backward_composed_features and grpg_backward_composed_objects:
// the blend backward over the frame's F feature channels, the object-alpha plane's gradient added to the gradient
// records (q.alpha_object), the composed preprocess backward, and -- F > 0 -- the feature gradient back to the models.
static int backward_composed_impl(const BackwardRequest& q) {
  if (int rc = begin_call()) return rc;
  int F = 0;   // (== q.F)
  if (int rc = check_feature_split(q.S, q.normals, &F)) return rc;
  if (F > GRPG_MAX_SEMANTIC_BACKWARD)   // the blend backward carries the channels in registers
    return fail(GRPG_ERR_INVALID_ARGUMENT,
                "backward supports at most 32 semantic channels (the reference: 20, config.h:16)");
  if (F > 0 && (!q.feature_buffer || !q.dL_dpix_features || !q.dL_dfeatures))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL semantic pointer with S>0");
  long long Pll = 0;
  if (int rc = check_composed_model(q.segs, q.nseg, q.D, q.M, &Pll)) return rc;
  const int P = (int)Pll;
  if (!q.grads || !q.geom_buffer || !q.binning_buffer || !q.image_buffer)
    return fail(GRPG_ERR_BAD_BUFFER, "NULL gradient table / state buffer");
  const hipStream_t stream = q.stream;
  const int debug = q.debug;
  if (int rc = check_backward_state(q.geom_buffer, P, stream)) return rc;
  if (!q.dL_dpix || !q.dL_dpix_depth || !q.dL_dalphas || !q.alphas || !q.dL_dmean2D || !q.dL_dposes || !q.radii ||
      !q.background || !q.viewmatrix || !q.projmatrix || !q.campos)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL pointer");
  for (int i = 0; i < q.nseg; i++) {
    const grpg_model_segment_grad& g = q.grads[i];
    if (!g.xyz || !g.scaling || !g.rotation || !g.opacity || !g.features_dc || (q.M > 1 && !g.features_rest))
      return fail(GRPG_ERR_INVALID_ARGUMENT, "segment gradient with a NULL array");
  }
  BlendBackward bb(q, P);
  // tables: the segments (as in the forward; re-uploaded: the caller may hand over other arrays of
  // the same values) and the six output pointers per segment, through pinned staging
  BwdStagingSlot* stg = bwd_staging_acquire();
  if (!stg) return fail(GRPG_ERR_HIP, "pinned staging allocation failed");
  fill_segments(stg->segs, q.segs, q.nseg, nullptr);
  for (int i = 0; i < q.nseg; i++) stg->grads[i] = q.grads[i];
  SegmentDev* seg_dev = (SegmentDev*)(q.geom_buffer + bb.GL.seg_table);
  void* seg_grad_dev = (void*)(q.geom_buffer + bb.GL.seg_grad_table);
  HIP_TRY(hipMemcpyAsync(seg_dev, stg->segs, sizeof(SegmentDev) * (size_t)q.nseg, hipMemcpyHostToDevice, stream));
  gather_device_poses(stream, seg_dev, q.nseg);
  HIP_TRY(hipMemcpyAsync(seg_grad_dev, stg->grads, sizeof(grpg_model_segment_grad) * (size_t)q.nseg,
                         hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(stg->ev, stream));
  if (int rc = bb.run(F > 0 ? (const float*)(q.feature_buffer + feat_layout(0, 0).features) : nullptr)) return rc;
  if (q.alpha_object) {
    const ObjAlphaLayout OL = obj_alpha_layout((size_t)bb.cam.gx * (size_t)bb.cam.gy, (size_t)q.width * q.height);
    launch_object_alpha_backward(stream, bb.ranges(), bb.point_list(), bb.rec,
                                 (const unsigned char*)(q.geom_buffer + bb.GL.aux_c),
                                 (const unsigned char*)(q.workspace + OL.tile_flags), q.width, q.height, bb.cam.gx,
                                 bb.cam.gy, q.alpha_object, (const uint32_t*)(q.workspace + OL.n_contrib),
                                 q.dL_dalpha_object, bb.grad_rec);
    STAGE_CHECK("object-alpha backward");
  }
  launch_preprocess_backward_composed(stream, P, q.D, q.M, seg_dev, seg_grad_dev, q.nseg, q.radii, bb.rec,
                                      q.scale_modifier, bb.cam, bb.grad_rec, q.dL_dmean2D,
                                      (float*)(q.geom_buffer + bb.GL.pose_acc), q.dL_dposes);
  if (int rc = bb.finish("preprocess backward (composed)")) return rc;
  if (F == 0) return GRPG_OK;
  // the feature gradient back to the models, behind the preprocess backward on the same stream (it ADDS to the
  // rotation and pose gradients that one has written).  Its table travels through a staging slot of its own: the
  // ring turns by two per feature backward.
  BwdStagingSlot* fstg = bwd_staging_acquire();
  if (!fstg) return fail(GRPG_ERR_HIP, "pinned staging allocation failed");
  for (int i = 0; i < q.nseg; i++)
    fstg->feats[i] = FeatureSegDev{nullptr, q.seg_dL_dsemantic ? q.seg_dL_dsemantic[i] : nullptr, q.grads[i].rotation,
                                   nullptr};
  const FeatLayout FL = feat_layout((size_t)P, (size_t)F);
  FeatureSegDev* fdev = (FeatureSegDev*)(q.feature_buffer + FL.table);
  HIP_TRY(hipMemcpyAsync(fdev, fstg->feats, sizeof(FeatureSegDev) * (size_t)q.nseg, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(fstg->ev, stream));
  launch_compose_features_backward(stream, P, seg_dev, fdev, q.nseg, q.S, q.normals, q.campos, q.dL_dfeatures,
                                   (float*)(q.feature_buffer + FL.partials), FL.nslots, q.dL_dposes);
  STAGE_CHECK("feature backward");
  return GRPG_OK;
}

int grpg_backward_composed(const grpg_model_segment* segments, const grpg_model_segment_grad* grads,
                           int num_segments, int D, int M, int R, const float* background, int width,
                           int height, float scale_modifier, const float* viewmatrix,
                           const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                           const int* radii, const float* alphas, char* geom_buffer, char* binning_buffer,
                           char* image_buffer, const float* dL_dpix, const float* dL_dpix_depth,
                           const float* dL_dalphas, float* dL_dmean2D, float* dL_dposes, int debug,
                           void* hip_stream) {
  PoseScope poses;
  BackwardRequest q;
  set_model(q, segments, grads, num_segments, D, M, dL_dposes);
  set_frame(q, R, background, width, height, scale_modifier, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii,
            alphas, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dpix_depth, dL_dalphas, dL_dmean2D, debug,
            hip_stream);
  return backward_composed_impl(q);
}

int grpg_backward_composed_features(const grpg_model_segment* segments, const grpg_model_segment_grad* grads,
                                    int num_segments, float* const* seg_dL_dsemantic, int S, int normals, int D,
                                    int M, int R, const float* background, int width, int height,
                                    float scale_modifier, const float* viewmatrix, const float* projmatrix,
                                    const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                                    const float* alphas, char* geom_buffer, char* binning_buffer, char* image_buffer,
                                    char* feature_buffer, const float* dL_dpix, const float* dL_dpix_depth,
                                    const float* dL_dalphas, const float* dL_dpix_features, float* dL_dfeatures,
                                    float* dL_dmean2D, float* dL_dposes, int debug, void* hip_stream) {
  PoseScope poses;
  BackwardRequest q;
  set_model(q, segments, grads, num_segments, D, M, dL_dposes);
  set_features(q, seg_dL_dsemantic, S, normals, feature_buffer, dL_dpix_features, dL_dfeatures);
  set_frame(q, R, background, width, height, scale_modifier, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii,
            alphas, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dpix_depth, dL_dalphas, dL_dmean2D, debug,
            hip_stream);
  return backward_composed_impl(q);
}

size_t grpg_object_alpha_workspace_bytes(int width, int height) {
  if (width <= 0 || height <= 0) return 0;
  const size_t gx = ((size_t)width + TILE - 1) / TILE, gy = ((size_t)height + TILE - 1) / TILE;
  return obj_alpha_layout(gx * gy, (size_t)width * (size_t)height).total;
}

int grpg_object_alpha_forward(int P, int width, int height, const unsigned char* layer_class, char* geom_buffer,
                              char* binning_buffer, char* image_buffer, float* out_alpha_object, char* workspace,
                              void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (P < 0 || width <= 0 || height <= 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "negative size");
  if (!out_alpha_object || !workspace || ((uintptr_t)workspace & 3u) != 0u)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL pointer (or a workspace that is not 4-byte aligned)");
  hipStream_t stream = (hipStream_t)hip_stream;
  const int debug = 0;
  const int gx = (width + TILE - 1) / TILE, gy = (height + TILE - 1) / TILE;
  const size_t N = (size_t)width * (size_t)height;
  const ObjAlphaLayout OL = obj_alpha_layout((size_t)gx * (size_t)gy, N);
  if (P == 0) {   // a frame without Gaussians: the plane and its n_contrib are zero, no tile is flagged
    HIP_TRY(hipMemsetAsync(out_alpha_object, 0, N * sizeof(float), stream));
    HIP_TRY(hipMemsetAsync(workspace, 0, OL.total, stream));
    return GRPG_OK;
  }
  if (!geom_buffer || !binning_buffer || !image_buffer)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL state buffer");
  // a training forward's blobs only: the backward adds to the gradient records an evaluation blob lacks, and the
  // class array lives in the geometry blob (the depth sort's third payload array, idle once the forward is through)
  if (int rc = check_backward_state(geom_buffer, P, stream)) return rc;
  const GeomLayout GL = geom_layout((size_t)P);
  const ImgLayout IL = img_layout((size_t)gx * (size_t)gy, N);
  HIP_TRY(hipMemsetAsync(workspace + OL.tile_flags, 0, (size_t)gx * (size_t)gy, stream));
  launch_object_alpha_forward(stream, P, layer_class, (const SegmentDev*)(geom_buffer + GL.seg_table),
                              (const uint2*)(image_buffer + IL.ranges),
                              (const uint32_t*)(binning_buffer + bin_layout(0).val_a),
                              RecView{(const float4*)(geom_buffer + GL.rec)},
                              (const uint32_t*)(geom_buffer + GL.tiles), width, height, gx, gy,
                              (unsigned char*)(geom_buffer + GL.aux_c), out_alpha_object,
                              (uint32_t*)(workspace + OL.n_contrib), (unsigned char*)(workspace + OL.tile_flags));
  STAGE_CHECK("object-alpha forward");
  return GRPG_OK;
}

int grpg_backward_composed_objects(const grpg_model_segment* segments, const grpg_model_segment_grad* grads,
                                   int num_segments, float* const* seg_dL_dsemantic, int S, int normals, int D,
                                   int M, int R, const float* background, int width, int height,
                                   float scale_modifier, const float* viewmatrix, const float* projmatrix,
                                   const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                                   const float* alphas, char* geom_buffer, char* binning_buffer, char* image_buffer,
                                   char* feature_buffer, const float* dL_dpix, const float* dL_dpix_depth,
                                   const float* dL_dalphas, const float* dL_dpix_features, float* dL_dfeatures,
                                   float* dL_dmean2D, float* dL_dposes, const float* alpha_object, char* workspace,
                                   const float* dL_dalpha_object, int debug, void* hip_stream) {
  PoseScope poses;
  if (int rc = begin_call()) return rc;
  if (!alpha_object || !workspace || !dL_dalpha_object || ((uintptr_t)workspace & 3u) != 0u || width <= 0 ||
      height <= 0)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "object-alpha backward: NULL pointer, misaligned workspace or bad size");
  BackwardRequest q;
  set_model(q, segments, grads, num_segments, D, M, dL_dposes);
  set_features(q, seg_dL_dsemantic, S, normals, feature_buffer, dL_dpix_features, dL_dfeatures);
  set_frame(q, R, background, width, height, scale_modifier, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii,
            alphas, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dpix_depth, dL_dalphas, dL_dmean2D, debug,
            hip_stream);
  q.alpha_object = alpha_object; q.workspace = workspace; q.dL_dalpha_object = dL_dalpha_object;
  return backward_composed_impl(q);
}

// the arguments the two stand-alone feature entries share
static int check_feature_call(const grpg_model_segment* segments, int num_segments, int S, int normals,
                              const float* cam_pos, long long* P, int* F) {
  if (int rc = check_segments(segments, num_segments, 1, P)) return rc;
  if (int rc = check_feature_split(S, normals, F)) return rc;
  if (normals && !cam_pos) return fail(GRPG_ERR_INVALID_ARGUMENT, "normals need cam_pos");
  return GRPG_OK;
}

// Stand-alone calls (grpg_compose, grpg_compose_features and its backward): the segment table -- and, with `feats`,
// the feature table of the three per-segment arrays (each may be NULL) and the backward's slots -- travel through a
// temporary device buffer.
typedef std::function<void(const SegmentDev*, const FeatureSegDev*, float*, uint32_t)> TempTableLaunch;
static int temp_table_call(const grpg_model_segment* segments, int num_segments, bool feats,
                           const float* const* seg_semantic, float* const* seg_dL_dsemantic,
                           float* const* seg_dL_drotation, long long P, hipStream_t stream, const char* what,
                           const TempTableLaunch& launch) {
  const size_t n = (size_t)num_segments;
  std::vector<SegmentDev> host(n);
  fill_segments(host.data(), segments, num_segments, nullptr);
  std::vector<FeatureSegDev> fhost(feats ? n : 0);
  for (size_t i = 0; i < fhost.size(); i++)
    fhost[i] = FeatureSegDev{seg_semantic ? seg_semantic[i] : nullptr, seg_dL_dsemantic ? seg_dL_dsemantic[i] : nullptr,
                             seg_dL_drotation ? seg_dL_drotation[i] : nullptr, nullptr};
  const FeatLayout FL = feats ? feat_layout((size_t)P, 0) : FeatLayout{};   // (no feature array: the caller's)
  const size_t seg_bytes = (sizeof(SegmentDev) * n + 255) / 256 * 256;
  char* dev = nullptr;
  HIP_TRY(hipMalloc((void**)&dev, seg_bytes + FL.total));
  char* const fdev = dev + seg_bytes;
  hipError_t e = hipMemcpyAsync(dev, host.data(), sizeof(SegmentDev) * n, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess && feats)
    e = hipMemcpyAsync(fdev + FL.table, fhost.data(), sizeof(FeatureSegDev) * n, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);   // pageable sources: the copies must finish before they die
  if (e == hipSuccess) {
    gather_device_poses(stream, (SegmentDev*)dev, num_segments);
    launch((const SegmentDev*)dev, feats ? (const FeatureSegDev*)(fdev + FL.table) : nullptr,
           feats ? (float*)(fdev + FL.partials) : nullptr, FL.nslots);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
  }
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(GRPG_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  return GRPG_OK;
}

int grpg_compose_features(const grpg_model_segment* segments, int num_segments, const float* const* seg_semantic,
                          int S, int normals, const float* cam_pos, float* features, void* hip_stream) {
  PoseScope poses;
  if (int rc = begin_call()) return rc;
  long long P = 0;
  int F = 0;
  if (int rc = check_feature_call(segments, num_segments, S, normals, cam_pos, &P, &F)) return rc;
  if (F == 0) return GRPG_OK;
  if (!features) return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL output pointer");
  hipStream_t stream = (hipStream_t)hip_stream;
  return temp_table_call(segments, num_segments, true, seg_semantic, nullptr, nullptr, P, stream, "grpg_compose_features",
                         [&](const SegmentDev* sd, const FeatureSegDev* fd, float*, uint32_t) {
                           launch_compose_features(stream, (int)P, sd, fd, num_segments, S, normals, cam_pos, features);
                         });
}

int grpg_compose_features_backward(const grpg_model_segment* segments, int num_segments, int S, int normals,
                                   const float* cam_pos, const float* dL_dfeatures, float* const* seg_dL_dsemantic,
                                   float* const* seg_dL_drotation, float* dL_dposes, void* hip_stream) {
  PoseScope poses;
  if (int rc = begin_call()) return rc;
  long long P = 0;
  int F = 0;
  if (int rc = check_feature_call(segments, num_segments, S, normals, cam_pos, &P, &F)) return rc;
  if (F == 0) return GRPG_OK;
  if (!dL_dfeatures || (normals && !dL_dposes)) return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL gradient pointer");
  hipStream_t stream = (hipStream_t)hip_stream;
  return temp_table_call(segments, num_segments, true, nullptr, seg_dL_dsemantic, seg_dL_drotation, P, stream,
                         "grpg_compose_features_backward",
                         [&](const SegmentDev* sd, const FeatureSegDev* fd, float* partials, uint32_t nslots) {
                           launch_compose_features_backward(stream, (int)P, sd, fd, num_segments, S, normals, cam_pos,
                                                            dL_dfeatures, partials, nslots, dL_dposes);
                         });
}

int grpg_compose(const grpg_model_segment* segments, int num_segments, int M, float* means3D,
                 float* scales, float* rotations, float* opacities, float* shs, void* hip_stream) {
  PoseScope poses;
  if (int rc = begin_call()) return rc;
  long long P = 0;
  if (int rc = check_segments(segments, num_segments, M, &P)) return rc;
  if (M < 1 || M > 16) return fail(GRPG_ERR_INVALID_ARGUMENT, "M must be in 1..16");
  if (!means3D || !scales || !rotations || !opacities || !shs)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL output pointer");
  hipStream_t stream = (hipStream_t)hip_stream;
  return temp_table_call(segments, num_segments, false, nullptr, nullptr, nullptr, P, stream, "grpg_compose",
                         [&](const SegmentDev* sd, const FeatureSegDev*, float*, uint32_t) {
                           launch_compose(stream, (int)P, M, sd, num_segments, means3D, scales, rotations, opacities, shs);
                         });
}

static int backward_flat_impl(const BackwardRequest& q) {
  if (int rc = begin_call()) return rc;
  if (q.P <= 0) return GRPG_OK;
  if (!q.geom_buffer || !q.binning_buffer || !q.image_buffer)
    return fail(GRPG_ERR_BAD_BUFFER, "NULL state buffer");
  const hipStream_t stream = q.stream;
  if (int rc = check_backward_state(q.geom_buffer, q.P, stream)) return rc;
  // dL_dconic / dL_ddepth (pure intermediates of the reference's binding) and dL_dcolor / dL_dcov3D
  // (gradients of the OPTIONAL inputs colors_precomp / cov3D_precomp) may be NULL: not written then
  if (!q.dL_dpix || !q.dL_dpix_depth || !q.dL_dalphas || !q.alphas || !q.dL_dmean2D || !q.dL_dopacity || !q.dL_dmean3D)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL gradient pointer");
  if ((q.colors_precomp && !q.dL_dcolor) || (q.cov3D_precomp && !q.dL_dcov3D))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "colors_precomp / cov3D_precomp given without their gradient array");
  // every gradient array is WRITTEN, not accumulated: the inputs in use need theirs
  if (!q.colors_precomp && (!q.shs || !q.dL_dsh))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "shs (no colors_precomp) needs shs and dL_dsh");
  if (!q.cov3D_precomp && (!q.scales || !q.rotations || !q.dL_dscale || !q.dL_drot))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "scales / rotations (no cov3D_precomp) need dL_dscale and dL_drot");
  if (!q.means3D || !q.background || !q.viewmatrix || !q.projmatrix || !q.campos)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL means3D / camera / background pointer");
  if (q.S > 0 && (!q.semantics || !q.dL_dpix_features || !q.dL_dfeatures))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL semantic pointer with S>0");
  if (q.S > GRPG_MAX_SEMANTIC_BACKWARD)   // the blend backward carries the channels in registers
    return fail(GRPG_ERR_INVALID_ARGUMENT,
                "backward supports at most 32 semantic channels (the reference: 20, config.h:16)");
  BlendBackward bb(q, q.P);
  if (q.debug) {  // validate the blobs (costs a sync; only in debug mode, like the reference's checks)
    BlobHeader h[3];
    HIP_TRY(hipMemcpyAsync(&h[0], q.geom_buffer, sizeof(BlobHeader), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&h[1], q.binning_buffer, sizeof(BlobHeader), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&h[2], q.image_buffer, sizeof(BlobHeader), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h[0].magic != GEOM_MAGIC || h[1].magic != BIN_MAGIC || h[2].magic != IMG_MAGIC ||
        h[0].P != (uint32_t)q.P || h[0].R != (uint32_t)q.R || h[1].Rcap < (uint32_t)q.R ||
        h[2].W != (uint32_t)q.width || h[2].H != (uint32_t)q.height)
      return fail(GRPG_ERR_BAD_BUFFER, "state buffers do not match this call (P/R/W/H or magic)");
    if (h[0].has_grad_rec == 0u)
      return fail(GRPG_ERR_BAD_BUFFER, "the geometry buffer was carved by an evaluation forward (no gradient records)");
    if (h[2].pc_timeout != 0u)
      return fail(GRPG_ERR_HIP, "the forward of this frame reported a producer/consumer timeout: its image is invalid");
  }
  const int* radii_int = q.radii ? q.radii : (const int*)(q.geom_buffer + bb.GL.radii);
  if (int rc = bb.run(q.semantics)) return rc;
  launch_preprocess_backward(stream, q.P, q.D, q.M, q.means3D, radii_int, q.colors_precomp ? nullptr : q.shs, bb.rec,
                             q.cov3D_precomp ? nullptr : q.scales, q.rotations, q.scale_modifier, q.cov3D_precomp,
                             bb.cam, bb.grad_rec, q.dL_dmean2D, q.dL_dconic, q.dL_dopacity, q.dL_dmean3D, q.dL_dcolor,
                             q.dL_ddepth, q.dL_dcov3D, q.colors_precomp ? nullptr : q.dL_dsh, q.dL_dscale, q.dL_drot);
  return bb.finish("preprocess backward");
}

int grpg_backward(int P, int D, int M, int R, int S, const float* background, int width,
                  int height, const float* means3D, const float* shs, const float* colors_precomp,
                  const float* semantics, const float* alphas, const float* scales,
                  float scale_modifier, const float* rotations, const float* cov3D_precomp,
                  const float* viewmatrix, const float* projmatrix, const float* campos,
                  float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer,
                  char* binning_buffer, char* image_buffer, const float* dL_dpix,
                  const float* dL_dpix_depth, const float* dL_dalphas,
                  const float* dL_dpix_semantic, float* dL_dmean2D, float* dL_dconic,
                  float* dL_dopacity, float* dL_dcolor, float* dL_ddepth, float* dL_dmean3D,
                  float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                  float* dL_dsemantic, int debug, void* hip_stream) {
  BackwardRequest q;
  set_frame(q, R, background, width, height, scale_modifier, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii,
            alphas, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dpix_depth, dL_dalphas, dL_dmean2D, debug,
            hip_stream);
  q.P = P; q.D = D; q.M = M; q.means3D = means3D; q.shs = shs; q.colors_precomp = colors_precomp; q.scales = scales;
  q.rotations = rotations; q.cov3D_precomp = cov3D_precomp;
  // the semantic channels are the blend's feature channels of a flat frame
  q.S = q.F = S; q.semantics = semantics; q.dL_dpix_features = dL_dpix_semantic; q.dL_dfeatures = dL_dsemantic;
  q.dL_dconic = dL_dconic; q.dL_dopacity = dL_dopacity; q.dL_dcolor = dL_dcolor; q.dL_ddepth = dL_ddepth;
  q.dL_dmean3D = dL_dmean3D; q.dL_dcov3D = dL_dcov3D; q.dL_dsh = dL_dsh; q.dL_dscale = dL_dscale; q.dL_drot = dL_drot;
  return backward_flat_impl(q);
}

int grpg_mark_visible(int P, const float* means3D, const float* viewmatrix,
                      const float* projmatrix, unsigned char* present, void* hip_stream) {
  (void)projmatrix;
  if (int rc = begin_call()) return rc;
  if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present)))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "bad argument");
  launch_mark_visible((hipStream_t)hip_stream, P, means3D, viewmatrix, present);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_visible_filter(int P, int M, int width, int height, const float* means3D,
                        const float* scales, float scale_modifier, const float* rotations,
                        const float* cov3D_precomp, const float* viewmatrix,
                        const float* projmatrix, float tan_fovx, float tan_fovy, int prefiltered,
                        int* radii, float* means2D, int debug, void* hip_stream) {
  (void)M; (void)prefiltered;
  if (int rc = begin_call()) return rc;
  if (P < 0 || width <= 0 || height <= 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "bad size");
  if (P == 0) return GRPG_OK;
  if (!means3D || !viewmatrix || !projmatrix || !radii || !means2D ||
      (!cov3D_precomp && (!scales || !rotations)))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL pointer");
  hipStream_t stream = (hipStream_t)hip_stream;
  const CameraArgs cam = make_camera(viewmatrix, projmatrix, nullptr, width, height, tan_fovx, tan_fovy);
  launch_visible_filter(stream, P, means3D, scales, scale_modifier, rotations, cov3D_precomp, cam,
                        radii, means2D);
  STAGE_CHECK("visible filter");
  return GRPG_OK;
}

int grpg_pack_rgb_u8(const float* src, unsigned char* dst, size_t n, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (n > 0 && (!src || !dst)) return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL pointer");
  if (((uintptr_t)src & 15) || ((uintptr_t)dst & 3))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "src must be 16-byte and dst 4-byte aligned");
  launch_pack_u8((hipStream_t)hip_stream, src, dst, n);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_pack_rgb_u8_hwc(const float* src_chw, unsigned char* dst_hwc, int height, int width,
                         int truncate, void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (height < 0 || width < 0) return fail(GRPG_ERR_INVALID_ARGUMENT, "negative size");
  const size_t npix = (size_t)height * (size_t)width;
  if (npix > 0 && (!src_chw || !dst_hwc)) return fail(GRPG_ERR_INVALID_ARGUMENT, "NULL pointer");
  if (((uintptr_t)src_chw & 15) || ((uintptr_t)dst_hwc & 3))
    return fail(GRPG_ERR_INVALID_ARGUMENT, "src must be 16-byte and dst 4-byte aligned");
  launch_pack_hwc((hipStream_t)hip_stream, src_chw, dst_hwc, npix, truncate);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

int grpg_debug_export(int P, int R, int width, int height, const char* geom_buffer,
                      const char* binning_buffer, const char* image_buffer, uint64_t* keys_sorted,
                      uint32_t* point_list, uint32_t* ranges, uint32_t* n_contrib, float* means2D,
                      float* depths, float* conic_opacity, float* rgb, uint32_t* tiles_touched,
                      void* hip_stream) {
  if (int rc = begin_call()) return rc;
  if (P < 0 || R < 0 || !geom_buffer || !binning_buffer || !image_buffer)
    return fail(GRPG_ERR_INVALID_ARGUMENT, "bad argument");
  hipStream_t stream = (hipStream_t)hip_stream;
  const int gx = (width + TILE - 1) / TILE, gy = (height + TILE - 1) / TILE;
  const GeomLayout GL = geom_layout((size_t)P);
  // the binning blob was carved for a capacity >= R: read it from the blob's header
  BlobHeader bh;
  HIP_TRY(hipMemcpyAsync(&bh, binning_buffer, sizeof(BlobHeader), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (bh.magic != BIN_MAGIC || bh.Rcap < (uint32_t)R)
    return fail(GRPG_ERR_BAD_BUFFER, "binning buffer does not match this call");
  // An evaluation frame of the hierarchical binning lists fewer instances than its num_rendered (binned rectangles,
  // preprocess.hip): the point list holds what the tile scan counted (the geometry header's R), and the entries
  // behind that were never written -- they must not be decoded as Gaussian ids.
  BlobHeader gh;
  HIP_TRY(hipMemcpyAsync(&gh, geom_buffer, sizeof(BlobHeader), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (gh.magic != GEOM_MAGIC) return fail(GRPG_ERR_BAD_BUFFER, "geometry buffer does not match this call");
  const uint32_t R_listed = bh.hier && gh.R < (uint32_t)R ? gh.R : (uint32_t)R;
  // hierarchical blob: the header's Rc is the coarse capacity it was carved for
  const BinLayout BL = bh.hier ? bin_layout((size_t)bh.Rcap, (size_t)gx * gy, super_tiles(gx, gy), (size_t)bh.Rc)
                               : bin_layout((size_t)bh.Rcap);
  const ImgLayout IL = img_layout((size_t)gx * gy, (size_t)width * height);
  launch_debug_export(stream, P, R_listed, width, height, gx, gy,
                      RecView{(const float4*)(geom_buffer + GL.rec)},
                      (const uint32_t*)(geom_buffer + GL.tiles),
                      (const uint32_t*)(binning_buffer + BL.key_a),
                      bh.hier ? (const uint32_t*)(binning_buffer + BL.tile_start) : nullptr,
                      (const uint32_t*)(binning_buffer + BL.val_a),
                      (const uint2*)(image_buffer + IL.ranges),
                      (const uint32_t*)(image_buffer + IL.n_contrib), keys_sorted, point_list,
                      ranges, n_contrib, means2D, depths, conic_opacity, rgb, tiles_touched);
  HIP_TRY(hipGetLastError());
  return GRPG_OK;
}

}  // extern "C"
