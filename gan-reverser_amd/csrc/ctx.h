// ctx.h — what the net runtime (net.hip) and the context-level operators (ops.hip) share: the owning types of device memory, events
// and streams, the context, the error macros and the workspace helpers.  Internal: not installed, not part of the ABI (that is include/ganrev.h).
#pragma once
#include "../../include/ganrev.h"
#include "kernels.h"
#include <rccl/rccl.h>
#include <string>
#include <vector>

// ------------------------------------------------------------------ owners
// The owner of device and pinned-host allocations: it records each one it makes and frees them all in release(), which its destructor
// calls.  Every allocation is a hipMalloc / hipHostMalloc of its own.  Built on a stream, release() first waits for that stream when
// something is held (a call's temporaries, which its kernels may still read); otherwise whoever releases has drained what reads them.
struct DevMem {
  explicit DevMem(hipStream_t wait_for = nullptr) : wait(wait_for) {}
  DevMem(const DevMem&) = delete; DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { release(); }
  template <class T> hipError_t dev(T** p, size_t bytes) { return keep((void**)p, hipMalloc((void**)p, bytes), false); }
  template <class T> hipError_t pinned(T** p, size_t bytes) { return keep((void**)p, hipHostMalloc((void**)p, bytes), true); }
  void drop(void* p) {       // one allocation goes early (a buffer that grows); null and foreign pointers are left alone
    for (size_t i = 0; i < held.size(); ++i) if (p && held[i].first == p) { free_one(held[i]); held.erase(held.begin() + i); return; }
  }
  void release() {
    if (wait && !held.empty()) (void)hipStreamSynchronize(wait);
    for (auto& h : held) free_one(h); held.clear();
  }
 private:
  typedef std::pair<void*, bool> Held;       // (pointer, pinned)
  static void free_one(const Held& h) { if (h.second) (void)hipHostFree(h.first); else (void)hipFree(h.first); }
  hipError_t keep(void** p, hipError_t e, bool pinned) { if (e == hipSuccess) held.push_back(Held(*p, pinned)); else *p = nullptr; return e; }
  std::vector<Held> held; hipStream_t wait;
};
// A HIP event / stream that goes with its owner.  create() is checked by the caller; the handle converts to the plain HIP type.
template <class H, hipError_t (*Destroy)(H)> struct Handle {
  H h = nullptr;
  Handle() = default; Handle(const Handle&) = delete;
  Handle(Handle&& o) : h(o.h) { o.h = nullptr; }
  ~Handle() { if (h) (void)Destroy(h); }
  operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> { hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&h, flags); } };
struct Stream : Handle<hipStream_t, hipStreamDestroy> { hipError_t create() { return hipStreamCreateWithFlags(&h, hipStreamNonBlocking); } };

// ------------------------------------------------------------------ context
struct gr_ctx {
  int device = 0;
  Stream stream;
  DevMem mem;                                 // every device / pinned buffer below, the lazily created ones included (gr_shutdown releases it)
  std::string err;
  ncclComm_t comm = nullptr;
  ncclComm_t stat_comm = nullptr;             // synchronised BatchNorm's own communicator (ncclCommSplit of comm): its collectives run on the COMPUTE stream while the gradient
                                              // buckets run on comm_stream - two streams never share one communicator
  int nranks = 1, rank = 0;
  Stream comm_stream;                         // gradient buckets are reduced here, behind the rest of backward
  Event ev_ready, ev_done;
  void* ws = nullptr; size_t ws_bytes = 0;
  // weight gradients run beside the rest of backward (backward_impl): their own stream, workspace and events
  Stream side_stream; void* ws2 = nullptr; size_t ws2_bytes = 0;
  Event ev_dy_ready, ev_wgrad_done[2];
  // R's head in one launch (gr_train_r_step, elem.hip head_fwd_bwd_kernel): grid-barrier counter (monotonic) and per-workgroup loss partials
  unsigned* head_bar = nullptr; unsigned head_bar_count = 0; double* head_loss_part = nullptr;
  bool head_unchecked = false;         // a head kernel has been launched since the sticky fault word (d_loss + 48) was last read: head_fault_check
  int head_fault_inject = 0;           // gr_set_tuning "head_fault_inject" (test hook): the NEXT head launch waits at its barriers for an arrival count that never comes
  int cu_count = 0;                    // the grid barrier needs every workgroup of the head kernel resident at once: head_plan refuses devices with fewer CUs than workgroups
  int fused_head = 1;                  // gr_set_tuning "fused_head" (1 default; 0 = the stage-by-stage path: the A/B control and what every other entry point runs)
  int side_wgrad = -1;                 // gr_set_tuning "side_wgrad" / GR_SIDE_WGRAD: 1 on, 0 off, -1 (default) by size.  The MFMA kernels take the whole register file of a
                                       // CU (2 waves x 256 VGPRs per SIMD), so nothing becomes resident beside a weight gradient and only kernel tails overlap.  Round 5,
                                       // same box, interleaved (profiles/r05_ab_side_wgrad_*.txt): cfg2 1.976 -> 1.998 ms (slower: the tails are a few us and two streams
                                       // cost an event hand-over per stage), cfg3 12.005 -> 11.875 ms (faster: the slab write + reduction tail of a 0.3 ms launch hides
                                       // behind the data gradient).  Auto = on for stages of >= 2^26 activations (cfg3's layers; cfg2's have 2^24).  Bit-identical
                                       // either way.  Per-kernel timing (gr_set_timing 2) forces it off, so that kernel durations are not inflated by overlap.
  double* d_loss = nullptr;     // device scalar (64-byte block: +0 the loss, +16 the range guard's alarm word, +32 the search's arrival counter, +48 the head kernel's sticky fault word)
  double* h_loss = nullptr;     // pinned host scalar
  bool timing = false;
  int conv_mode = 2;            // 2 = f16x3 split (fp32-accurate, f16 MFMA; default), 1 = bf16x6 split (fp32-accurate, bf16 MFMA), 0 = exact fp32 MFMA
  unsigned* amax = nullptr;     // 4 scratch slots for the single-kernel entry points (f16x3 scales)
  Event ev[7];
  std::vector<Event> marks;      // gr_event_record slots (bench: per-step times on THIS stream)
  float times[6] = {0, 0, 0, 0, 0, 0};
  // f16x3 range guard (kernels.h "range guard"): the alarm word lives behind the loss scalar (d_loss + 16 bytes,
  // mirrored at h_loss + 16), chmax is the per-channel scratch of the scans
  int range_guard = 1;                 // 1: on (gr_set_tuning "range_guard")
  unsigned* guard_chmax = nullptr; size_t guard_chmax_cap = 0;     // (capacity in bytes)
  long guard_scans = 0, guard_fallbacks = 0;
  long search_reruns = 0;              // searches whose sample-bound filter overflowed and ran again unfiltered
  void* pin = nullptr; size_t pin_bytes = 0;   // pinned staging for small results (search)
  unsigned* search_state = nullptr;    // device words of the small search path (kernels.h SEARCH_STATE_WORDS)
  unsigned* pin_done = nullptr; unsigned search_seq = 0;   // per-needle completion words of the small search path (pinned, 64 bytes) and the sequence number they carry
  Event ev_guard; bool guard_pending = false;   // device-resident trainer: sampled scans, verdict read one call later
  bool guard_tripped = false;          // ... which found a hostile range: the context stays on bf16x6
  // synchronised BatchNorm (gr_set_tuning "sync_bn", SURVEY.md 8e optional) and the host-exchange hook that can stand in for RCCL
  int sync_bn = 0;
  double* sync_buf = nullptr; size_t sync_cap = 0;     // compact per-channel pairs that travel through the collective
  gr_exchange_fn xchg = nullptr; void* xchg_user = nullptr;
  int coll_rc = 0;                     // first failure of a collective issued from inside a kernel launcher (StatSync callbacks)
};

int fail(gr_ctx* c, int code, const char* fmt, ...);      // (net.hip) sets gr_last_error and returns code
#define HIPCHK(ctx, call)                                                                             \
  do { hipError_t e_ = (call); if (e_ != hipSuccess)                                                  \
      return fail(ctx, GR_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define LAUNCHCHK(ctx)                                                                                \
  do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess)                                       \
      return fail(ctx, GR_ERR_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

// Device buffers p[0..nbuf) of owner `own` that share the capacity `cap` (bytes) get `bytes` each when they hold less.  The old ones are freed
// once stream s, the one that may still read them, has drained (a buffer of capacity 0 was never handed to a kernel).  Contents are not kept.
template <class T> static int grow_dev(gr_ctx* c, DevMem& own, T** p, size_t& cap, size_t bytes, hipStream_t s, int nbuf = 1) {
  if (bytes <= cap) return GR_OK;
  if (cap) HIPCHK(c, hipStreamSynchronize(s));
  for (int i = 0; i < nbuf; ++i) { own.drop(p[i]); p[i] = nullptr; }
  cap = 0;
  for (int i = 0; i < nbuf; ++i) HIPCHK(c, own.dev(&p[i], bytes));
  cap = bytes;
  return GR_OK;
}
// the workspaces grow past the next MiB boundary
static size_t past_next_mib(size_t bytes) { return (bytes + (1u << 20)) & ~(size_t)((1u << 20) - 1); }
static int ensure_ws(gr_ctx* c, size_t bytes) { return bytes <= c->ws_bytes ? GR_OK : grow_dev(c, c->mem, &c->ws, c->ws_bytes, past_next_mib(bytes), c->stream); }
