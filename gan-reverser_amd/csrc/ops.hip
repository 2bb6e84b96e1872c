// ops.hip — the context-level operators of the C ABI (include/ganrev.h): entry points that take a gr_ctx and no gr_net.  The criteria,
// the nn.Concat helpers, colour spaces, image.scale and the dataset loader, the searches, k-means, the picture grids and the single-kernel
// convolution calls.  Host code only: the kernels are in the files kernels.h names.
#include "ctx.h"
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>

using namespace gr;

#define TRY(call) do { int r_ = (call); if (r_) return r_; } while (0)

// ------------------------------------------------------------------ staging and temporaries
// One call's share of the context workspace: reserve typed regions (each starts on a 256-byte boundary), grow() once, then ask for
// pointers.  A kernel that takes c->ws itself as its scratch gets the first region.  Copies go on c->stream; finish() is the one wait.
template <class T> struct Region { size_t off, count; };
struct Staging {
  gr_ctx* c; size_t bytes = 0;
  explicit Staging(gr_ctx* ctx) : c(ctx) {}
  template <class T> Region<T> reserve(size_t count) { Region<T> r{bytes, count}; bytes += (sizeof(T) * count + 255) & ~(size_t)255; return r; }
  int grow() { HIPCHK(c, hipSetDevice(c->device)); return ensure_ws(c, bytes); }
  template <class T> T* ptr(Region<T> r) const { return reinterpret_cast<T*>(static_cast<char*>(c->ws) + r.off); }
  template <class T> int upload(Region<T> r, const T* host) { HIPCHK(c, hipMemcpyAsync(ptr(r), host, sizeof(T) * r.count, hipMemcpyHostToDevice, c->stream)); return GR_OK; }
  template <class T> int download(T* host, Region<T> r) { HIPCHK(c, hipMemcpyAsync(host, ptr(r), sizeof(T) * r.count, hipMemcpyDeviceToHost, c->stream)); return GR_OK; }
  int finish() { HIPCHK(c, hipStreamSynchronize(c->stream)); return GR_OK; }
  // a host array that is the caller's own again (or dies) when the call returns
  template <class T> int upload_now(Region<T> r, const T* host) { TRY(upload(r, host)); return finish(); }
};
// (a call's hipMalloc temporaries live in a DevMem tmp(c->stream), ctx.h: they go on every exit path, once the work enqueued on the stream has finished)

// a criterion on host tensors: launch(x, t, loss_dev, grad) runs on staged copies
template <class Launch> static int criterion_host(gr_ctx* c, const float* x, const float* t, int64_t n, double* loss, float* grad, Launch launch) {
  Staging s(c);
  auto dx = s.reserve<float>(n), dt = s.reserve<float>(n), dg = s.reserve<float>(n);
  TRY(s.grow()); TRY(s.upload(dx, x)); TRY(s.upload(dt, t));
  launch(s.ptr(dx), s.ptr(dt), c->d_loss, grad ? s.ptr(dg) : nullptr); LAUNCHCHK(c);
  if (grad) TRY(s.download(grad, dg));
  HIPCHK(c, hipMemcpyAsync(c->h_loss, c->d_loss, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  TRY(s.finish());
  if (loss) *loss = *c->h_loss;
  return GR_OK;
}
// one host tensor in, one out: launch(in, out) runs on staged copies (gr_colorspace_host, gr_image_scale_host)
template <class Launch> static int map_host(gr_ctx* c, const float* in, size_t nin, float* out, size_t nout, Launch launch) {
  Staging s(c);
  auto din = s.reserve<float>(nin), dout = s.reserve<float>(nout);
  TRY(s.grow()); TRY(s.upload(din, in));
  launch(s.ptr(din), s.ptr(dout)); LAUNCHCHK(c);
  TRY(s.download(out, dout));
  return s.finish();
}
// a device entry point that is "scratch, launch, map the status": launch(scratch) gets `bytes` of the context workspace and returns its launcher's
// status; 1 (any other non-zero) and 2 become the caller's own code and text - a format of at most one int, which a text without one ignores
struct LaunchError { int code; const char* fmt; int arg; };
template <class Launch> static int scratch_launch(gr_ctx* c, size_t bytes, Launch launch, LaunchError on1, LaunchError on2 = {0, nullptr, 0}) {
  Staging s(c);
  auto scratch = s.reserve<char>(bytes);
  TRY(s.grow());
  const int r = launch(static_cast<void*>(s.ptr(scratch)));
  if (r == 2 && on2.fmt) return fail(c, on2.code, on2.fmt, on2.arg);
  if (r) return fail(c, on1.code, on1.fmt, on1.arg);
  LAUNCHCHK(c);
  return GR_OK;
}

// ------------------------------------------------------------------ criterion
extern "C" int gr_mse_dev(gr_ctx* c, const float* x, const float* t, int64_t n, int64_t ng, double* loss_dev, float* grad) {
  if (!c || !x || !t || n <= 0 || ng <= 0) return GR_ERR_INVALID;
  launch_mse(x, t, n, ng, loss_dev, grad, c->stream); LAUNCHCHK(c);
  return GR_OK;
}
extern "C" int gr_mse_host(gr_ctx* c, const float* x, const float* t, int64_t n, int64_t ng, double* loss, float* grad) {
  if (!c || !x || !t || n <= 0 || ng <= 0) return GR_ERR_INVALID;
  return criterion_host(c, x, t, n, loss, grad, [&](const float* dx, const float* dt, double* dl, float* dg) { launch_mse(dx, dt, n, ng, dl, dg, c->stream); });
}
// noise refinement: the per-row criterion and the per-row best-keeping + Adam step (kernels in elem.hip)
extern "C" int gr_mse_rows_dev(gr_ctx* c, const float* x, const float* t, int64_t rows, int64_t n, float* loss_rows, float* grad) {
  if (!c || !x || !t || !loss_rows || rows <= 0 || n <= 0) return GR_ERR_INVALID;
  launch_mse_rows(x, t, rows, n, loss_rows, grad, c->stream); LAUNCHCHK(c);
  return GR_OK;
}
extern "C" int gr_adam_rows_step_dev(gr_ctx* c, float* z, float* g, float* m, float* v, int64_t rows, int64_t nd, const gr_adam_hyper* h, int t, float clamp,
                                     const float* loss_rows, float* best_loss, float* best_z, int update) {
  if (!c || !z || !loss_rows || !best_loss || !best_z || rows <= 0 || nd <= 0 || rows > INT32_MAX || nd > INT32_MAX || clamp < 0) return GR_ERR_INVALID;
  if (update && (!g || !m || !v || !h || t < 1)) return GR_ERR_INVALID;
  const AdamConsts k = update ? adam_consts_plain(h->lr, h->beta1, h->beta2, h->eps, t) : AdamConsts{};
  launch_adam_rows(z, g, m, v, (int)rows, (int)nd, k, clamp, loss_rows, best_loss, best_z, update ? 1 : 0, c->stream); LAUNCHCHK(c);
  return GR_OK;
}
// nn.BCECriterion (sizeAverage): train.lua:173's CRITERION, used by adversarial.lua (the GAN step's loss; first pieces of SURVEY.md 8f rank 4)
extern "C" int gr_bce_dev(gr_ctx* c, const float* x, const float* t, int64_t n, double* loss_dev, float* grad) {
  if (!c || !x || !t || n <= 0) return GR_ERR_INVALID;
  launch_bce(x, t, n, loss_dev, grad, c->stream); LAUNCHCHK(c);
  return GR_OK;
}
extern "C" int gr_bce_host(gr_ctx* c, const float* x, const float* t, int64_t n, double* loss, float* grad) {
  if (!c || !x || !t || n <= 0) return GR_ERR_INVALID;
  return criterion_host(c, x, t, n, loss, grad, [&](const float* dx, const float* dt, double* dl, float* dg) { launch_bce(dx, dt, n, dl, dg, c->stream); });
}

// ------------------------------------------------------------------ nn.Concat on device-resident tensors (models.lua:293-321)
// The container stays on the host (it is a module that calls its children, not an operator); these two move its data
// without leaving the GPU: rows of one matrix into a column range of another (join the branch outputs / slice gradOutput),
// and the sum of the branches' gradInputs.
extern "C" int gr_copy2d_dev(gr_ctx* c, float* dst, int64_t dst_pitch, const float* src, int64_t src_pitch, int64_t rows, int64_t cols) {
  if (!c || !dst || !src || rows <= 0 || cols <= 0 || dst_pitch < cols || src_pitch < cols) return GR_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpy2DAsync(dst, sizeof(float) * (size_t)dst_pitch, src, sizeof(float) * (size_t)src_pitch, sizeof(float) * (size_t)cols, (size_t)rows,
                             hipMemcpyDeviceToDevice, c->stream));
  return GR_OK;
}
extern "C" int gr_add_dev(gr_ctx* c, float* y, const float* x, int64_t n) {
  if (!c || !y || !x || n <= 0) return GR_ERR_INVALID;
  launch_add_inplace(y, x, (long)n, c->stream); LAUNCHCHK(c);
  return GR_OK;
}

// ------------------------------------------------------------------ NN_UTILS.switchColorSpace (utils/nn_utils.lua:133-246)
static int colorspace_check(gr_ctx* c, const float* in, int from, int to, int64_t batch, int h, int w, const float* out) {
  if (!c) return GR_ERR_INVALID;
  if (!in || !out) return fail(c, GR_ERR_INVALID, "gr_colorspace: null pointer");
  if (from < GR_CS_RGB || from > GR_CS_HSL) return fail(c, GR_ERR_INVALID, "gr_colorspace: unknown color space <from>: %d", from);
  if (to < GR_CS_RGB || to > GR_CS_HSL) return fail(c, GR_ERR_INVALID, "gr_colorspace: unknown color space <to>: %d", to);
  if (batch <= 0 || h <= 0 || w <= 0) return fail(c, GR_ERR_INVALID, "gr_colorspace: batch %lld, h %d, w %d must be positive", (long long)batch, h, w);
  if (in == out && (from == GR_CS_Y) != (to == GR_CS_Y)) return fail(c, GR_ERR_INVALID, "gr_colorspace: in place needs equal plane counts (from %d, to %d)", from, to);
  return GR_OK;
}
extern "C" int gr_colorspace_dev(gr_ctx* c, const float* in, int from, int to, int64_t batch, int h, int w, float* out) {
  int r = colorspace_check(c, in, from, to, batch, h, w, out); if (r) return r;
  const long hw = (long)h * w;
  if (from == GR_CS_RGB && to == GR_CS_RGB) {
    if (in != out) HIPCHK(c, hipMemcpyAsync(out, in, sizeof(float) * 3 * (size_t)batch * hw, hipMemcpyDeviceToDevice, c->stream));
    return GR_OK;
  }
  launch_colorspace(in, from, to, (long)batch, hw, out, c->stream); LAUNCHCHK(c);
  return GR_OK;
}
extern "C" int gr_colorspace_host(gr_ctx* c, const float* in, int from, int to, int64_t batch, int h, int w, float* out) {
  int r = colorspace_check(c, in, from, to, batch, h, w, out); if (r) return r;
  const size_t hw = (size_t)h * w, nin = (from == GR_CS_Y ? 1 : 3) * (size_t)batch * hw, nout = (to == GR_CS_Y ? 1 : 3) * (size_t)batch * hw;
  if (from == GR_CS_RGB && to == GR_CS_RGB) {
    if (in != out) memmove(out, in, sizeof(float) * nin);
    return GR_OK;
  }
  return map_host(c, in, nin, out, nout, [&](const float* din, float* dout) { launch_colorspace(din, from, to, (long)batch, (long)hw, dout, c->stream); });
}

// ------------------------------------------------------------------ dataset.lua:111-116,149-153: image.scale and the loader's fused path (dataset.hip)
// GR_SCALE_MAX_ELEMS bounds both tensors of a call: the kernels index with 64-bit integers, the bound keeps every product of the geometry far inside them
static const int64_t GR_SCALE_MAX_ELEMS = (int64_t)1 << 40;
static int scale_check(gr_ctx* c, const char* who, const void* in, const void* out, int64_t n, int64_t per_in, int sh, int sw, int dh, int dw, int64_t per_out) {
  if (!c) return GR_ERR_INVALID;
  if (!in || !out) return fail(c, GR_ERR_INVALID, "%s: null pointer", who);
  if (n < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1) return fail(c, GR_ERR_INVALID, "%s: n %lld, source %d x %d, target %d x %d must be positive", who, (long long)n, sh, sw, dh, dw);
  if (sh > SCALE_MAX_LEN || sw > SCALE_MAX_LEN || dh > SCALE_MAX_LEN || dw > SCALE_MAX_LEN)
    return fail(c, GR_ERR_INVALID, "%s: source %d x %d, target %d x %d: a side is too large (at most %d)", who, sh, sw, dh, dw, SCALE_MAX_LEN);
  const int64_t ein = per_in * sh * sw, eout = per_out * dh * dw;              // per_* <= 2^31, a side <= 2^15: below 2^61
  if (n > GR_SCALE_MAX_ELEMS / ein || n > GR_SCALE_MAX_ELEMS / eout) return fail(c, GR_ERR_INVALID, "%s: %lld images are too large a batch (at most 2^40 elements per tensor)", who, (long long)n);
  return GR_OK;
}
extern "C" int gr_image_scale_dev(gr_ctx* c, const float* in, int64_t n, int planes, int sh, int sw, int dh, int dw, float* out) {
  if (c && planes < 1) return fail(c, GR_ERR_INVALID, "gr_image_scale: planes %d must be positive", planes);
  int r = scale_check(c, "gr_image_scale", in, out, n, planes, sh, sw, dh, dw, planes); if (r) return r;
  if (in == out) return fail(c, GR_ERR_INVALID, "gr_image_scale: in place is not supported");
  HIPCHK(c, hipSetDevice(c->device));
  launch_image_scale(in, (long)n * planes, scale_axis(sh, dh), scale_axis(sw, dw), out, c->stream); LAUNCHCHK(c);
  return GR_OK;
}
extern "C" int gr_image_scale_host(gr_ctx* c, const float* in, int64_t n, int planes, int sh, int sw, int dh, int dw, float* out) {
  if (c && planes < 1) return fail(c, GR_ERR_INVALID, "gr_image_scale: planes %d must be positive", planes);
  int r = scale_check(c, "gr_image_scale", in, out, n, planes, sh, sw, dh, dw, planes); if (r) return r;
  if (in == out) return fail(c, GR_ERR_INVALID, "gr_image_scale: in place is not supported");
  const size_t nin = (size_t)n * planes * sh * sw, nout = (size_t)n * planes * dh * dw;
  return map_host(c, in, nin, out, nout, [&](const float* din, float* dout) { launch_image_scale(din, (long)n * planes, scale_axis(sh, dh), scale_axis(sw, dw), dout, c->stream); });
}
extern "C" int gr_dataset_images_dev(gr_ctx* c, const uint8_t* in, int64_t n, int sh, int sw, int sc, int dh, int dw, int to_space, int normalize, float* out) {
  if (c && sc != 1 && sc != 3 && sc != 4) return fail(c, GR_ERR_INVALID, "gr_dataset_images: %d source channels (1, 3 or 4)", sc);
  if (c && (to_space < GR_CS_RGB || to_space > GR_CS_HSL)) return fail(c, GR_ERR_INVALID, "gr_dataset_images: unknown color space <to>: %d", to_space);
  int r = scale_check(c, "gr_dataset_images", in, out, n, sc, sh, sw, dh, dw, to_space == GR_CS_Y ? 1 : 3); if (r) return r;
  HIPCHK(c, hipSetDevice(c->device));
  launch_dataset_images(in, (long)n, sc, scale_axis(sh, dh), scale_axis(sw, dw), to_space, normalize != 0, out, c->stream); LAUNCHCHK(c);
  return GR_OK;
}

// ------------------------------------------------------------------ the decoded files of a dataset, kept on the device (gr_dataset_cache_*)
// An arena of chunks: an image is uploaded once, behind the last one of the open chunk (on a 4-byte boundary, padded to a dword, the chunk
// keeps a spare dword at its end), or into a new chunk when it does not fit; bytes that were uploaded never move.  The records (address,
// size) are kept on the host, where every call validates against them, and mirrored on the device for the gather kernel: the mirror is
// brought up to date by the first load after an append.  Like a net, the cache has a DevMem of its own and points at its context: it is
// destroyed before the context is shut down, or left alone after that.
struct DatasetCache {
  gr_ctx* ctx = nullptr;
  DevMem mem;                                             // the chunks, the record mirror, the index buffers
  size_t chunk_bytes = 0;                                 // what a new chunk gets (an image that needs more gets what it needs)
  uint8_t* chunk = nullptr; size_t chunk_cap = 0, chunk_used = 0;      // the open chunk
  std::vector<CachedImage> recs;
  int64_t bytes = 0;                                      // decoded bytes held (without the padding)
  CachedImage* d_recs = nullptr; size_t d_recs_bytes = 0, d_recs_n = 0;      // the mirror holds the first d_recs_n records
  long* d_idx = nullptr; size_t d_idx_bytes = 0;          // a load's index list on the device ...
  long* h_idx = nullptr; size_t h_idx_count = 0;          // ... and the pinned block it is copied from, free again once ev_idx has passed
  Event ev_idx;
};
static const int64_t GR_DATASET_CHUNK_DEFAULT = (int64_t)64 << 20;

extern "C" int gr_dataset_cache_create(gr_ctx* c, int64_t chunk_bytes, void** out) {
  if (!c) return GR_ERR_INVALID;
  if (!out) return fail(c, GR_ERR_INVALID, "gr_dataset_cache_create: null pointer");
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  DatasetCache* k = new DatasetCache();
  k->ctx = c;
  k->chunk_bytes = (size_t)(chunk_bytes > 0 ? chunk_bytes : GR_DATASET_CHUNK_DEFAULT);
  const hipError_t e = k->ev_idx.create(hipEventDisableTiming);
  if (e != hipSuccess) { delete k; return fail(c, GR_ERR_HIP, "gr_dataset_cache_create: %s", hipGetErrorString(e)); }
  *out = k;
  return GR_OK;
}
extern "C" int gr_dataset_cache_destroy(void* cache) {
  DatasetCache* k = static_cast<DatasetCache*>(cache);
  if (!k) return GR_ERR_INVALID;
  (void)hipSetDevice(k->ctx->device);
  (void)hipStreamSynchronize(k->ctx->stream);             // the one stream a load is enqueued on
  delete k;
  return GR_OK;
}
extern "C" int gr_dataset_cache_append(void* cache, const uint8_t* bytes, int sh, int sw, int sc) {
  DatasetCache* k = static_cast<DatasetCache*>(cache);
  if (!k) return GR_ERR_INVALID;
  gr_ctx* c = k->ctx;
  if (!bytes) return fail(c, GR_ERR_INVALID, "gr_dataset_cache_append: null pointer");
  if (sc != 1 && sc != 3 && sc != 4) return fail(c, GR_ERR_INVALID, "gr_dataset_cache_append: %d source channels (1, 3 or 4)", sc);
  if (sh < 1 || sw < 1 || sh > SCALE_MAX_LEN || sw > SCALE_MAX_LEN)
    return fail(c, GR_ERR_INVALID, "gr_dataset_cache_append: source %d x %d: a side must be in [1, %d]", sh, sw, SCALE_MAX_LEN);
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nbytes = (size_t)sh * sw * sc, padded = (nbytes + 3) & ~(size_t)3;      // at most 2^32
  if (k->chunk_used + padded + 4 > k->chunk_cap) {        // a new chunk; the open one keeps its images (nothing is copied)
    const size_t cap = padded + 4 > k->chunk_bytes ? padded + 4 : k->chunk_bytes;
    uint8_t* p = nullptr;
    const hipError_t e = k->mem.dev(&p, cap);
    if (e != hipSuccess) {
      (void)hipGetLastError();                            // (an allocation failure is not sticky: the cache and the context go on)
      return fail(c, GR_ERR_HIP, "gr_dataset_cache_append: a chunk of %zu bytes: %s (the cache keeps its %zu images)", cap, hipGetErrorString(e), k->recs.size());
    }
    HIPCHK(c, hipMemsetAsync(p, 0, cap, c->stream));      // the padding and the spare dword read as zeros
    k->chunk = p; k->chunk_cap = cap; k->chunk_used = 0;
  }
  uint8_t* dst = k->chunk + k->chunk_used;
  HIPCHK(c, hipMemcpyAsync(dst, bytes, nbytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));             // the caller's array is its own again
  k->chunk_used += padded;
  k->recs.push_back(CachedImage{dst, sh, sw, sc, 0});
  k->bytes += (int64_t)nbytes;
  return GR_OK;
}
extern "C" int gr_dataset_cache_size(void* cache, int64_t* n_images, int64_t* bytes) {
  DatasetCache* k = static_cast<DatasetCache*>(cache);
  if (!k) return GR_ERR_INVALID;
  if (n_images) *n_images = (int64_t)k->recs.size();
  if (bytes) *bytes = k->bytes;
  return GR_OK;
}
extern "C" int gr_dataset_cache_image(void* cache, int64_t i, int* sh, int* sw, int* sc) {
  DatasetCache* k = static_cast<DatasetCache*>(cache);
  if (!k) return GR_ERR_INVALID;
  if (i < 0 || i >= (int64_t)k->recs.size()) return fail(k->ctx, GR_ERR_INVALID, "gr_dataset_cache_image: image %lld is outside [0, %zu)", (long long)i, k->recs.size());
  const CachedImage& r = k->recs[(size_t)i];
  if (sh) *sh = r.sh;
  if (sw) *sw = r.sw;
  if (sc) *sc = r.sc;
  return GR_OK;
}
extern "C" int gr_dataset_cache_load_dev(void* cache, const int64_t* indices, int64_t n, int dh, int dw, int to_space, int normalize, float* out) {
  DatasetCache* k = static_cast<DatasetCache*>(cache);
  if (!k) return GR_ERR_INVALID;
  gr_ctx* c = k->ctx;
  if (!indices || !out) return fail(c, GR_ERR_INVALID, "gr_dataset_cache_load: null pointer");
  if (to_space < GR_CS_RGB || to_space > GR_CS_HSL) return fail(c, GR_ERR_INVALID, "gr_dataset_cache_load: unknown color space <to>: %d", to_space);
  if (n < 1 || dh < 1 || dw < 1) return fail(c, GR_ERR_INVALID, "gr_dataset_cache_load: n %lld, target %d x %d must be positive", (long long)n, dh, dw);
  if (dh > SCALE_MAX_LEN || dw > SCALE_MAX_LEN) return fail(c, GR_ERR_INVALID, "gr_dataset_cache_load: target %d x %d: a side is too large (at most %d)", dh, dw, SCALE_MAX_LEN);
  if (n > GR_SCALE_MAX_ELEMS / ((int64_t)3 * dh * dw)) return fail(c, GR_ERR_INVALID, "gr_dataset_cache_load: %lld images are too large a batch (at most 2^40 elements per tensor)", (long long)n);
  const int64_t held = (int64_t)k->recs.size();
  double bytes_in = 0;
  for (int64_t j = 0; j < n; ++j) {
    if (indices[j] < 0 || indices[j] >= held)
      return fail(c, GR_ERR_INVALID, "gr_dataset_cache_load: indices[%lld] = %lld is outside [0, %lld)", (long long)j, (long long)indices[j], (long long)held);
    const CachedImage& r = k->recs[(size_t)indices[j]];
    bytes_in += (double)r.sh * r.sw * r.sc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (k->d_recs_n < k->recs.size()) {                      // images were appended since the mirror was written: all records again, then a wait (the vector may grow)
    TRY(grow_dev(c, k->mem, &k->d_recs, k->d_recs_bytes, past_next_mib(sizeof(CachedImage) * k->recs.size()), c->stream));
    HIPCHK(c, hipMemcpyAsync(k->d_recs, k->recs.data(), sizeof(CachedImage) * k->recs.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    k->d_recs_n = k->recs.size();
  }
  TRY(grow_dev(c, k->mem, &k->d_idx, k->d_idx_bytes, sizeof(long) * (size_t)n, c->stream));
  // the list travels through a pinned block of the cache's own, so that the copy is asynchronous and the caller's array is its own again on
  // return; the block is written again only after the previous load's copy has left it (an event that has long passed in a training loop)
  HIPCHK(c, hipEventSynchronize(k->ev_idx));
  if ((size_t)n > k->h_idx_count) {
    k->mem.drop(k->h_idx); k->h_idx = nullptr; k->h_idx_count = 0;
    HIPCHK(c, k->mem.pinned(&k->h_idx, sizeof(long) * (size_t)n));
    k->h_idx_count = (size_t)n;
  }
  for (int64_t j = 0; j < n; ++j) k->h_idx[j] = (long)indices[j];
  HIPCHK(c, hipMemcpyAsync(k->d_idx, k->h_idx, sizeof(long) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(k->ev_idx, c->stream));
  launch_dataset_gather(k->d_recs, k->d_idx, (long)n, dh, dw, to_space, normalize != 0, out, bytes_in, c->stream); LAUNCHCHK(c);
  return GR_OK;
}

// ------------------------------------------------------------------ search
// The search behind both needle sources: rows of the table (qrows, host) or vectors of their own (queries_dev [Q][d], device); exactly one is given
static int cosine_topk_run(gr_ctx* c, const float* emb, int64_t N, int d, const int64_t* qrows, const float* queries_dev, int Q, int k,
                           int64_t* idx_out, float* score_out, int accf) {
  if (!c || !emb || (!qrows && !queries_dev) || !idx_out || N <= 0 || d <= 0 || Q <= 0 || k <= 0) return GR_ERR_INVALID;
  if (k > N) k = (int)N;
  if (qrows) for (int q = 0; q < Q; ++q) if (qrows[q] < 0 || qrows[q] >= N) return fail(c, GR_ERR_INVALID, "query row %lld out of range", (long long)qrows[q]);
  if (k > 1024) return fail(c, GR_ERR_UNSUPPORTED, "k > 1024");
  Staging s(c);
  s.reserve<char>(cosine_topk_workspace_bytes(N, d, Q, k));          // launch_cosine_topk takes c->ws itself: the first region
  auto tail = s.reserve<char>(sizeof(long) * (size_t)Q * (k + 1) + sizeof(float) * (size_t)Q * k + sizeof(unsigned));
  TRY(s.grow());
  char* base = s.ptr(tail);
  // results [idx | scores | status] are contiguous on the device: ONE copy into pinned memory and one wait per search (three
  // copies into pageable memory cost about 30 us of the 0.25 ms a cfg5 search takes)
  long* d_q = (long*)base; long* d_idx = d_q + Q; float* d_sc = (float*)(d_idx + (size_t)Q * k); unsigned* d_status = (unsigned*)(d_sc + (size_t)Q * k);
  const size_t res_bytes = sizeof(long) * (size_t)Q * k + sizeof(float) * (size_t)Q * k + sizeof(unsigned);
  if (res_bytes > c->pin_bytes) {
    c->mem.drop(c->pin);
    c->pin = nullptr; c->pin_bytes = 0;
    HIPCHK(c, c->mem.pinned(&c->pin, res_bytes * 2));
    c->pin_bytes = res_bytes * 2;
  }
  // A handful of needles (the reference's five): their rows travel in the kernel arguments and the kernels write idx | scores | status
  // straight into the pinned result block (host memory the device can address): no upload, no copy-out - launches, one wait.
  if (cosine_topk_small_path(N, d, Q, k)) {
    void* pin_dev = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&pin_dev, c->pin, 0));
    char* pd = static_cast<char*>(pin_dev);
    long* p_idx = reinterpret_cast<long*>(pd); float* p_sc = reinterpret_cast<float*>(pd + sizeof(long) * (size_t)Q * k);
    unsigned* p_status = reinterpret_cast<unsigned*>(pd + res_bytes - sizeof(unsigned));
    if (!c->pin_done) { HIPCHK(c, c->mem.pinned(&c->pin_done, 64)); memset(c->pin_done, 0, 64); }
    void* done_dev = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&done_dev, c->pin_done, 0));
    if (++c->search_seq == 0u) c->search_seq = 1u;                                  // never 0: a fresh block reads 0
    const unsigned seq = c->search_seq;
    if (!c->search_state) {       // the sample launch's arrival counter and histogram: zero now, left zero by every search
      HIPCHK(c, c->mem.dev(&c->search_state, sizeof(unsigned) * SEARCH_STATE_WORDS));
      HIPCHK(c, hipMemsetAsync(c->search_state, 0, sizeof(unsigned) * SEARCH_STATE_WORDS, c->stream));
    }
    const int lr = launch_cosine_topk(emb, N, d, d_q, Q, k, p_idx, p_sc, accf, c->ws, c->stream, p_status, 0, qrows, c->search_state,
                                      static_cast<unsigned*>(done_dev), seq, queries_dev);
    if (lr < 0) return fail(c, GR_ERR_UNSUPPORTED, "cosine_topk: unsupported size");
    LAUNCHCHK(c);
    // The selection kernel publishes one completion word per needle behind its results (system-scope release): poll them instead of
    // synchronising the stream (measured: 1-3 us of a 0.15 ms search).  Bounded: after 20 ms the stream is synchronised after all (a fault
    // shows up there).
    bool seen = false;
    if (lr == 2) {
      volatile unsigned* dw = c->pin_done;
      const auto t0 = std::chrono::steady_clock::now();
      for (unsigned spins = 0;; ++spins) {
        bool all = true;
        for (int q = 0; q < Q; ++q) if (dw[q] != seq) { all = false; break; }
        if (all) { seen = true; break; }
        if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
        __builtin_ia32_pause();
      }
      std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!seen) HIPCHK(c, hipStreamSynchronize(c->stream));
    const char* hres = (const char*)c->pin;
    unsigned status; memcpy(&status, hres + res_bytes - sizeof(unsigned), sizeof status);
    if (status == 0) {
      memcpy(idx_out, hres, sizeof(long) * (size_t)Q * k);
      if (score_out) memcpy(score_out, hres + sizeof(long) * (size_t)Q * k, sizeof(float) * (size_t)Q * k);
      return GR_OK;
    }
    c->search_reruns++;       // a candidate list overflowed (adversarial row order): the unfiltered search below decides
  }
  if (qrows) HIPCHK(c, hipMemcpyAsync(d_q, qrows, sizeof(long) * Q, hipMemcpyHostToDevice, c->stream));
  const bool small_failed = cosine_topk_small_path(N, d, Q, k);
  for (int unfiltered = small_failed ? 1 : 0; unfiltered < 2; ++unfiltered) {
    if (launch_cosine_topk(emb, N, d, d_q, Q, k, d_idx, d_sc, accf, c->ws, c->stream, d_status, unfiltered, qrows, nullptr, nullptr, 0, queries_dev)) return fail(c, GR_ERR_UNSUPPORTED, "cosine_topk: unsupported size");
    LAUNCHCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->pin, d_idx, res_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const char* h = (const char*)c->pin;
    unsigned status; memcpy(&status, h + res_bytes - sizeof(unsigned), sizeof status);
    if (status == 0 || unfiltered) {
      memcpy(idx_out, h, sizeof(long) * (size_t)Q * k);
      if (score_out) memcpy(score_out, h + sizeof(long) * (size_t)Q * k, sizeof(float) * (size_t)Q * k);
      break;
    }
    c->search_reruns++;       // 1: the sample-bound filter overflowed (adversarial row order): rerun on every key
  }
  return GR_OK;
}
extern "C" int gr_cosine_topk_dev(gr_ctx* c, const float* emb, int64_t N, int d, const int64_t* qrows, int Q, int k,
                                  int64_t* idx_out, float* score_out, int accf) {
  if (!qrows) return GR_ERR_INVALID;
  return cosine_topk_run(c, emb, N, d, qrows, nullptr, Q, k, idx_out, score_out, accf);
}
extern "C" int gr_cosine_topk_queries_dev(gr_ctx* c, const float* emb, int64_t N, int d, const float* queries, int Q, int k,
                                          int64_t* idx_out, float* score_out, int accf) {
  if (!queries) return GR_ERR_INVALID;
  return cosine_topk_run(c, emb, N, d, nullptr, queries, Q, k, idx_out, score_out, accf);
}
extern "C" int gr_cosine_topk_host(gr_ctx* c, const float* emb, int64_t N, int d, const int64_t* qrows, int Q, int k,
                                   int64_t* idx_out, float* score_out, int accf) {
  if (!c || !emb || N <= 0 || d <= 0) return GR_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  DevMem tmp(c->stream); float* dev = nullptr;
  HIPCHK(c, tmp.dev(&dev, sizeof(float) * (size_t)N * d));
  if (hipMemcpyAsync(dev, emb, sizeof(float) * (size_t)N * d, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(c, GR_ERR_HIP, "upload failed");
  return gr_cosine_topk_dev(c, dev, N, d, qrows, Q, k, idx_out, score_out, accf);
}
extern "C" int gr_cosine_topk_queries_host(gr_ctx* c, const float* emb, int64_t N, int d, const float* queries, int Q, int k,
                                           int64_t* idx_out, float* score_out, int accf) {
  if (!c || !emb || !queries || !idx_out || N <= 0 || d <= 0 || Q <= 0 || k <= 0) return GR_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  DevMem tmp(c->stream); float* dev = nullptr; float* qdev = nullptr;
  HIPCHK(c, tmp.dev(&dev, sizeof(float) * (size_t)N * d));
  HIPCHK(c, tmp.dev(&qdev, sizeof(float) * (size_t)Q * d));
  if (hipMemcpyAsync(dev, emb, sizeof(float) * (size_t)N * d, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(c, GR_ERR_HIP, "upload failed");
  if (hipMemcpyAsync(qdev, queries, sizeof(float) * (size_t)Q * d, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(c, GR_ERR_HIP, "upload failed");
  return gr_cosine_topk_queries_dev(c, dev, N, d, qdev, Q, k, idx_out, score_out, accf);
}
extern "C" int gr_cosine_similarity_host(gr_ctx* c, const float* a, const float* b, int d, float* out) {
  if (!c || !a || !b || !out || d <= 0) return GR_ERR_INVALID;
  std::vector<float> two((size_t)2 * d);
  memcpy(two.data(), a, sizeof(float) * d); memcpy(two.data() + d, b, sizeof(float) * d);
  int64_t q = 0, idx[2]; float sc[2];
  int r = gr_cosine_topk_host(c, two.data(), 2, d, &q, 1, 2, idx, sc, 0); if (r) return r;
  *out = idx[0] == 1 ? sc[0] : sc[1];   // score of row 1 against needle row 0
  return GR_OK;
}

// ------------------------------------------------------------------ apply_r.lua:197-217 clustering of the recovered noise
extern "C" int gr_kmeans_host(gr_ctx* c, const float* x, int64_t n, int d, int k, int niter, float* cent, float* totalcounts, int32_t* labels) {
  if (!c || !x || !cent || n <= 0 || d <= 0 || k <= 0 || niter < 0) return GR_ERR_INVALID;
  Staging s(c);
  auto scratch = s.reserve<char>(kmeans_workspace_bytes(n, d, k));   // launch_kmeans takes c->ws itself: the first region
  auto dx = s.reserve<float>((size_t)n * d), dc = s.reserve<float>((size_t)k * d), dc2 = s.reserve<float>(k), dcnt = s.reserve<float>(k), dtot = s.reserve<float>(k);
  auto dlab = s.reserve<int>(n);
  TRY(s.grow()); TRY(s.upload(dx, x)); TRY(s.upload(dc, cent));
  if (launch_kmeans(s.ptr(dx), n, d, k, niter, s.ptr(dc), s.ptr(dc2), s.ptr(dcnt), s.ptr(dtot), s.ptr(dlab), s.ptr(scratch), c->stream)) return fail(c, GR_ERR_UNSUPPORTED, "kmeans: k <= 32 and d <= 256 only");
  LAUNCHCHK(c);
  TRY(s.download(cent, dc));
  if (totalcounts) TRY(s.download(totalcounts, dtot));
  if (labels && niter > 0) TRY(s.download(labels, dlab));
  return s.finish();
}
extern "C" int gr_cosine_assign_host(gr_ctx* c, const float* x, int64_t n, int d, const float* cent, int k, int take_min, int32_t* labels, float* sims) {
  if (!c || !x || !cent || !labels || !sims || n <= 0 || d <= 0 || k <= 0) return GR_ERR_INVALID;
  Staging s(c);
  auto dx = s.reserve<float>((size_t)n * d), dc = s.reserve<float>((size_t)k * d), dw = s.reserve<float>(k), dsim = s.reserve<float>(n);
  auto dlab = s.reserve<int>(n);
  TRY(s.grow()); TRY(s.upload(dx, x)); TRY(s.upload(dc, cent));
  if (launch_cosine_assign(s.ptr(dx), n, d, s.ptr(dc), k, take_min, s.ptr(dw), s.ptr(dlab), s.ptr(dsim), c->stream)) return fail(c, GR_ERR_UNSUPPORTED, "cosine_assign: unsupported size");
  LAUNCHCHK(c);
  TRY(s.download(labels, dlab)); TRY(s.download(sims, dsim));
  return s.finish();
}
// the same two on device-resident tables, and the steps that follow them (apply_r.lua:218-243): enqueued on c->stream, no wait
extern "C" int gr_kmeans_dev(gr_ctx* c, const float* x, int64_t n, int d, int k, int niter, float* cent, float* totalcounts, int32_t* labels) {
  if (!c || !x || !cent || n <= 0 || d <= 0 || k <= 0 || niter < 0) return GR_ERR_INVALID;
  Staging s(c);
  auto scratch = s.reserve<char>(kmeans_workspace_bytes(n, d, k));   // launch_kmeans takes c->ws itself: the first region
  auto dc2 = s.reserve<float>(k), dcnt = s.reserve<float>(k), dtot = s.reserve<float>(k);
  TRY(s.grow());
  if (launch_kmeans(x, n, d, k, niter, cent, s.ptr(dc2), s.ptr(dcnt), totalcounts ? totalcounts : s.ptr(dtot), labels, s.ptr(scratch), c->stream))
    return fail(c, GR_ERR_UNSUPPORTED, "kmeans: k <= 32 and d <= 256 only");
  LAUNCHCHK(c);
  return GR_OK;
}
extern "C" int gr_cosine_assign_dev(gr_ctx* c, const float* x, int64_t n, int d, const float* cent, int k, int take_min, int32_t* labels, float* sims) {
  if (!c || !x || !cent || !labels || !sims || n <= 0 || d <= 0 || k <= 0) return GR_ERR_INVALID;
  Staging s(c);
  auto dw = s.reserve<float>(k);
  TRY(s.grow());
  if (launch_cosine_assign(x, n, d, cent, k, take_min, s.ptr(dw), labels, sims, c->stream)) return fail(c, GR_ERR_UNSUPPORTED, "cosine_assign: unsupported size");
  LAUNCHCHK(c);
  return GR_OK;
}
extern "C" int gr_cluster_members_dev(gr_ctx* c, const int32_t* labels, const float* sims, int64_t n, int k, int m, int64_t* rows_out, float* sims_out,
                                      int32_t* kept_out, int32_t* sizes_out) {
  if (!c) return GR_ERR_INVALID;
  if (!labels || !sims || !rows_out || !sims_out || !kept_out || !sizes_out) return fail(c, GR_ERR_INVALID, "gr_cluster_members_dev: null pointer");
  if (n <= 0 || k <= 0 || m <= 0) return fail(c, GR_ERR_INVALID, "gr_cluster_members_dev: n %lld, k %d, m %d must be positive", (long long)n, k, m);
  if (n >= ((int64_t)1 << 31) || k > 32 || m > 128)
    return fail(c, GR_ERR_UNSUPPORTED, "gr_cluster_members_dev: n %lld, k %d, m %d: n < 2^31, k <= 32 and m <= 128 only", (long long)n, k, m);
  return scratch_launch(c, cluster_members_workspace_bytes(n, k), [&](void* ws) {
    return launch_cluster_members(labels, sims, n, k, m, reinterpret_cast<long*>(rows_out), sims_out, kept_out, sizes_out, ws, c->stream);
  }, {GR_ERR_UNSUPPORTED, "gr_cluster_members_dev: unsupported size", 0});
}
extern "C" int gr_cluster_dev(gr_ctx* c, const float* x, int64_t n, int d, int k, int niter, float* cent, int take_min, int m, float* totalcounts,
                              int32_t* labels, float* sims, int64_t* rows_out, float* sims_out, int32_t* kept_out, int32_t* sizes_out) {
  if (!c) return GR_ERR_INVALID;
  if (!x || !cent || !labels || !sims || !rows_out || !sims_out || !kept_out || !sizes_out) return fail(c, GR_ERR_INVALID, "gr_cluster_dev: null pointer");
  if (n <= 0 || d <= 0 || k <= 0 || m <= 0 || niter < 0)
    return fail(c, GR_ERR_INVALID, "gr_cluster_dev: n %lld, d %d, k %d, m %d must be positive and niter %d not negative", (long long)n, d, k, m, niter);
  if (k > 4096) return fail(c, GR_ERR_UNSUPPORTED, "gr_cluster_dev: k %d: at most 4096 clusters", k);
  if (d > 256) return fail(c, GR_ERR_UNSUPPORTED, "gr_cluster_dev: d %d: at most 256 columns", d);
  if (m > 128) return fail(c, GR_ERR_UNSUPPORTED, "gr_cluster_dev: m %d: at most 128 rows per cluster", m);
  if (n >= ((int64_t)1 << 31)) return fail(c, GR_ERR_UNSUPPORTED, "gr_cluster_dev: n %lld: fewer than 2^31 rows", (long long)n);
  Staging s(c);
  auto scratch = s.reserve<char>(cluster_workspace_bytes(n, d, k));
  auto dc2 = s.reserve<float>(k), dcnt = s.reserve<float>(k), dtot = s.reserve<float>(k), dw = s.reserve<float>(k);
  TRY(s.grow());
  const int r = launch_cluster(x, n, d, k, niter, cent, take_min, m, s.ptr(dc2), s.ptr(dcnt), totalcounts ? totalcounts : s.ptr(dtot), s.ptr(dw), labels, sims,
                               reinterpret_cast<long*>(rows_out), sims_out, kept_out, sizes_out, s.ptr(scratch), c->stream);
  if (r == 2) return fail(c, GR_ERR_HIP, "gr_cluster_dev: the device refuses the assignment kernel's LDS (d %d)", d);
  if (r) return fail(c, GR_ERR_UNSUPPORTED, "gr_cluster_dev: unsupported size");
  LAUNCHCHK(c);
  return GR_OK;
}
extern "C" int gr_cluster_members_wide_dev(gr_ctx* c, const int32_t* labels, const float* sims, int64_t n, int k, int m, int64_t* rows_out, float* sims_out,
                                           int32_t* kept_out, int32_t* sizes_out) {
  if (!c) return GR_ERR_INVALID;
  if (!labels || !sims || !rows_out || !sims_out || !kept_out || !sizes_out) return fail(c, GR_ERR_INVALID, "gr_cluster_members_wide_dev: null pointer");
  if (n <= 0 || k <= 0 || m <= 0) return fail(c, GR_ERR_INVALID, "gr_cluster_members_wide_dev: n %lld, k %d, m %d must be positive", (long long)n, k, m);
  if (k > 4096) return fail(c, GR_ERR_UNSUPPORTED, "gr_cluster_members_wide_dev: k %d: at most 4096 clusters", k);
  if (m > 128) return fail(c, GR_ERR_UNSUPPORTED, "gr_cluster_members_wide_dev: m %d: at most 128 rows per cluster", m);
  if (n >= ((int64_t)1 << 31)) return fail(c, GR_ERR_UNSUPPORTED, "gr_cluster_members_wide_dev: n %lld: fewer than 2^31 rows", (long long)n);
  return scratch_launch(c, cluster_members_wide_workspace_bytes(n, k), [&](void* ws) {
    return launch_cluster_members_wide(labels, sims, n, k, m, reinterpret_cast<long*>(rows_out), sims_out, kept_out, sizes_out, ws, c->stream);
  }, {GR_ERR_UNSUPPORTED, "gr_cluster_members_wide_dev: unsupported size", 0});
}
extern "C" int gr_cluster_faces_dev(gr_ctx* c, const float* table, int64_t n_rows, int64_t d, const int64_t* rows, const int32_t* kept, int k, int m, float* out) {
  if (!c) return GR_ERR_INVALID;
  if (!table || !rows || !kept || !out) return fail(c, GR_ERR_INVALID, "gr_cluster_faces_dev: null pointer");
  if (n_rows <= 0 || d <= 0 || k <= 0 || m <= 0 || k > 65535)
    return fail(c, GR_ERR_INVALID, "gr_cluster_faces_dev: n_rows %lld, d %lld, k %d (at most 65535), m %d must be positive", (long long)n_rows, (long long)d, k, m);
  HIPCHK(c, hipSetDevice(c->device));
  launch_cluster_faces(table, (long)n_rows, (long)d, reinterpret_cast<const long*>(rows), kept, k, m, out, c->stream); LAUNCHCHK(c);
  return GR_OK;
}

// ------------------------------------------------------------------ principal axes of a device table (pca.hip)
extern "C" int gr_pca_dev(gr_ctx* c, const float* x, int64_t n, int d, double* mean, double* cov, double* eigvals, float* axes, int32_t* info) {
  if (!c) return GR_ERR_INVALID;
  if (!x || !mean || !eigvals || !axes || !info) return fail(c, GR_ERR_INVALID, "gr_pca_dev: null pointer");
  if (n <= 0 || d <= 0) return fail(c, GR_ERR_INVALID, "gr_pca_dev: n %lld and d %d must be positive", (long long)n, d);
  if (n < 2) return fail(c, GR_ERR_UNSUPPORTED, "gr_pca_dev: n %lld: at least 2 rows", (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(c, GR_ERR_UNSUPPORTED, "gr_pca_dev: n %lld: fewer than 2^31 rows", (long long)n);
  if (d > 256) return fail(c, GR_ERR_UNSUPPORTED, "gr_pca_dev: d %d: at most 256 columns", d);
  return scratch_launch(c, pca_workspace_bytes(n, d), [&](void* ws) { return launch_pca(x, n, d, mean, cov, eigvals, axes, info, ws, c->stream); },
                        {GR_ERR_UNSUPPORTED, "gr_pca_dev: unsupported size", 0});
}
extern "C" int gr_pca_project_dev(gr_ctx* c, const float* x, int64_t n, int d, const double* mean, const float* axes, const double* eigvals, int k, int whiten,
                                  float* out) {
  if (!c) return GR_ERR_INVALID;
  if (!x || !mean || !axes || !out || (whiten && !eigvals)) return fail(c, GR_ERR_INVALID, "gr_pca_project_dev: null pointer");
  if (n <= 0 || d <= 0 || k <= 0) return fail(c, GR_ERR_INVALID, "gr_pca_project_dev: n %lld, d %d and k %d must be positive", (long long)n, d, k);
  if (n >= ((int64_t)1 << 31)) return fail(c, GR_ERR_UNSUPPORTED, "gr_pca_project_dev: n %lld: fewer than 2^31 rows", (long long)n);
  if (d > 256) return fail(c, GR_ERR_UNSUPPORTED, "gr_pca_project_dev: d %d: at most 256 columns", d);
  if (k > d) return fail(c, GR_ERR_UNSUPPORTED, "gr_pca_project_dev: k %d: at most d = %d axes", k, d);
  HIPCHK(c, hipSetDevice(c->device));
  const int r = launch_pca_project(x, n, d, mean, axes, eigvals, k, whiten, out, c->stream);
  if (r == 2) return fail(c, GR_ERR_HIP, "gr_pca_project_dev: the device refuses the projection kernel's LDS (d %d)", d);
  if (r) return fail(c, GR_ERR_UNSUPPORTED, "gr_pca_project_dev: unsupported size");
  LAUNCHCHK(c);
  return GR_OK;
}

// ------------------------------------------------------------------ diagonal Gaussian mixture of a device table (mixture.hip)
extern "C" int gr_mixture_dev(gr_ctx* c, const float* x, int64_t n, int d, int k, int niter, float var_floor, float* weights, float* means, float* vars,
                              double* loglik, int32_t* labels, float* post, float* rowll) {
  if (!c) return GR_ERR_INVALID;
  if (!x || !weights || !means || !vars || !loglik) return fail(c, GR_ERR_INVALID, "gr_mixture_dev: null pointer");
  if (n <= 0 || d <= 0 || k <= 0) return fail(c, GR_ERR_INVALID, "gr_mixture_dev: n %lld, d %d and k %d must be positive", (long long)n, d, k);
  if (niter < 0) return fail(c, GR_ERR_INVALID, "gr_mixture_dev: niter %d: an iteration count", niter);
  if (!(var_floor > 0.f)) return fail(c, GR_ERR_INVALID, "gr_mixture_dev: var_floor %g must be positive", (double)var_floor);
  if (n >= ((int64_t)1 << 31)) return fail(c, GR_ERR_UNSUPPORTED, "gr_mixture_dev: n %lld: fewer than 2^31 rows", (long long)n);
  if (d > 256) return fail(c, GR_ERR_UNSUPPORTED, "gr_mixture_dev: d %d: at most 256 columns", d);
  if (k > 256) return fail(c, GR_ERR_UNSUPPORTED, "gr_mixture_dev: k %d: at most 256 components", k);
  return scratch_launch(c, mixture_workspace_bytes(n, d, k), [&](void* ws) {
    return launch_mixture(x, n, d, k, niter, var_floor, weights, means, vars, loglik, labels, post, rowll, ws, c->stream);
  }, {GR_ERR_UNSUPPORTED, "gr_mixture_dev: unsupported size", 0}, {GR_ERR_HIP, "gr_mixture_dev: the device refuses the kernels' LDS (d %d)", d});
}
// ------------------------------------------------------------------ silhouette coefficients of a labelled device table (silhouette.hip)
extern "C" int gr_silhouette_dev(gr_ctx* c, const float* x, int64_t n, int d, const int32_t* labels, int k, int metric, double* sv, double* a, double* b,
                                 int32_t* nearest, double* cluster_mean, int32_t* sizes, double* mean) {
  if (!c) return GR_ERR_INVALID;
  if (!x || !labels || !sv || !cluster_mean || !sizes || !mean) return fail(c, GR_ERR_INVALID, "gr_silhouette_dev: null pointer");
  if (n <= 0 || d <= 0 || k <= 0) return fail(c, GR_ERR_INVALID, "gr_silhouette_dev: n %lld, d %d and k %d must be positive", (long long)n, d, k);
  if (metric != 0 && metric != 1) return fail(c, GR_ERR_INVALID, "gr_silhouette_dev: metric %d: 0 (euclidean) or 1 (cosine)", metric);
  if (n < 2 || n > GR_SILHOUETTE_MAX_N)
    return fail(c, GR_ERR_UNSUPPORTED, "gr_silhouette_dev: n %lld: between 2 and %d rows", (long long)n, GR_SILHOUETTE_MAX_N);
  if (d > 256) return fail(c, GR_ERR_UNSUPPORTED, "gr_silhouette_dev: d %d: at most 256 columns", d);
  if (k > 4096) return fail(c, GR_ERR_UNSUPPORTED, "gr_silhouette_dev: k %d: at most 4096 clusters", k);
  return scratch_launch(c, silhouette_workspace_bytes(n, k), [&](void* ws) {
    return launch_silhouette(x, n, d, labels, k, metric, sv, a, b, nearest, cluster_mean, sizes, mean, ws, c->stream);
  }, {GR_ERR_UNSUPPORTED, "gr_silhouette_dev: unsupported size", 0});
}

// ------------------------------------------------------------------ the k-nearest-neighbour graph of a device table (knn.hip)
static int knn_graph_check(gr_ctx* c, const char* who, int64_t n, int k) {
  if (n <= 0 || k <= 0) return fail(c, GR_ERR_INVALID, "%s: n %lld and k %d must be positive", who, (long long)n, k);
  if (n < 2 || n > GR_KNN_MAX_N) return fail(c, GR_ERR_UNSUPPORTED, "%s: n %lld: between 2 and %d rows", who, (long long)n, GR_KNN_MAX_N);
  if (k > GR_KNN_MAX_K) return fail(c, GR_ERR_UNSUPPORTED, "%s: k %d: at most %d neighbours", who, k, GR_KNN_MAX_K);
  if (k > n - 1) return fail(c, GR_ERR_UNSUPPORTED, "%s: k %d: at most n - 1 = %lld neighbours (a row is not its own)", who, k, (long long)(n - 1));
  return GR_OK;
}
extern "C" int gr_knn_dev(gr_ctx* c, const float* x, int64_t n, int d, int k, int metric, int32_t* idx, double* dist) {
  if (!c) return GR_ERR_INVALID;
  if (!x || !idx || !dist) return fail(c, GR_ERR_INVALID, "gr_knn_dev: null pointer");
  if (d <= 0) return fail(c, GR_ERR_INVALID, "gr_knn_dev: d %d must be positive", d);
  if (metric != 0 && metric != 1) return fail(c, GR_ERR_INVALID, "gr_knn_dev: metric %d: 0 (euclidean) or 1 (cosine)", metric);
  TRY(knn_graph_check(c, "gr_knn_dev", n, k));
  if (d > GR_KNN_MAX_D) return fail(c, GR_ERR_UNSUPPORTED, "gr_knn_dev: d %d: at most %d columns", d, GR_KNN_MAX_D);
  return scratch_launch(c, knn_workspace_bytes(n), [&](void* ws) { return launch_knn(x, n, d, k, metric, idx, dist, ws, c->stream); },
                        {GR_ERR_UNSUPPORTED, "gr_knn_dev: unsupported size", 0});
}
extern "C" int gr_lof_dev(gr_ctx* c, const int32_t* idx, const double* dist, int64_t n, int k, double* lrd, double* lof) {
  if (!c) return GR_ERR_INVALID;
  if (!idx || !dist || !lof) return fail(c, GR_ERR_INVALID, "gr_lof_dev: null pointer");
  TRY(knn_graph_check(c, "gr_lof_dev", n, k));
  return scratch_launch(c, lof_workspace_bytes(n), [&](void* ws) { return launch_lof(idx, dist, n, k, lrd, lof, ws, c->stream); },
                        {GR_ERR_UNSUPPORTED, "gr_lof_dev: unsupported size", 0});
}
extern "C" int gr_knn_overlap_dev(gr_ctx* c, const int32_t* idx_a, const int32_t* idx_b, int64_t n, int k, int32_t* count, double* mean) {
  if (!c) return GR_ERR_INVALID;
  if (!idx_a || !idx_b || !count || !mean) return fail(c, GR_ERR_INVALID, "gr_knn_overlap_dev: null pointer");
  TRY(knn_graph_check(c, "gr_knn_overlap_dev", n, k));
  return scratch_launch(c, knn_overlap_workspace_bytes(n), [&](void* ws) { return launch_knn_overlap(idx_a, idx_b, n, k, count, mean, ws, c->stream); },
                        {GR_ERR_UNSUPPORTED, "gr_knn_overlap_dev: unsupported size", 0});
}

// ------------------------------------------------------------------ density-based clustering of a device table (density.hip)
static int dbscan_rows_check(gr_ctx* c, const char* who, int64_t n) {
  if (n <= 0) return fail(c, GR_ERR_INVALID, "%s: n %lld must be positive", who, (long long)n);
  if (n < 2 || n > GR_DBSCAN_MAX_N) return fail(c, GR_ERR_UNSUPPORTED, "%s: n %lld: between 2 and %d rows", who, (long long)n, GR_DBSCAN_MAX_N);
  return GR_OK;
}
extern "C" int gr_eps_graph_dev(gr_ctx* c, const float* x, int64_t n, int d, double eps, int metric, uint64_t* adj, int32_t* count) {
  if (!c) return GR_ERR_INVALID;
  if (!x || !adj || !count) return fail(c, GR_ERR_INVALID, "gr_eps_graph_dev: null pointer");
  if (d <= 0) return fail(c, GR_ERR_INVALID, "gr_eps_graph_dev: d %d must be positive", d);
  if (metric != 0 && metric != 1) return fail(c, GR_ERR_INVALID, "gr_eps_graph_dev: metric %d: 0 (euclidean) or 1 (cosine)", metric);
  if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(c, GR_ERR_INVALID, "gr_eps_graph_dev: eps %g: a finite distance, not below 0", eps);
  TRY(dbscan_rows_check(c, "gr_eps_graph_dev", n));
  if (d > GR_DBSCAN_MAX_D) return fail(c, GR_ERR_UNSUPPORTED, "gr_eps_graph_dev: d %d: at most %d columns", d, GR_DBSCAN_MAX_D);
  return scratch_launch(c, eps_graph_workspace_bytes(n), [&](void* ws) {
    return launch_eps_graph(x, n, d, eps, metric, reinterpret_cast<unsigned long long*>(adj), count, ws, c->stream);
  }, {GR_ERR_UNSUPPORTED, "gr_eps_graph_dev: unsupported size", 0});
}
// (the one analysis call that waits on the stream: once per round, to read whether a label fell)
extern "C" int gr_dbscan_dev(gr_ctx* c, const uint64_t* adj, const int32_t* count, int64_t n, int min_pts, int32_t* labels, int32_t* core, int32_t* n_clusters) {
  if (!c) return GR_ERR_INVALID;
  if (!adj || !count || !labels || !n_clusters) return fail(c, GR_ERR_INVALID, "gr_dbscan_dev: null pointer");
  if (min_pts <= 0) return fail(c, GR_ERR_INVALID, "gr_dbscan_dev: min_pts %d must be positive", min_pts);
  TRY(dbscan_rows_check(c, "gr_dbscan_dev", n));
  if (min_pts > n) return fail(c, GR_ERR_UNSUPPORTED, "gr_dbscan_dev: min_pts %d: at most n = %lld rows (a neighbourhood holds no more)", min_pts, (long long)n);
  Staging s(c);
  auto scratch = s.reserve<char>(dbscan_workspace_bytes(n));
  TRY(s.grow());
  const DbscanScratch w = dbscan_carve(s.ptr(scratch), n);
  const unsigned long long* bitmap = reinterpret_cast<const unsigned long long*>(adj);
  if (launch_dbscan_begin(count, n, min_pts, w, c->stream)) return fail(c, GR_ERR_UNSUPPORTED, "gr_dbscan_dev: unsupported size");
  LAUNCHCHK(c);
  bool settled = false;
  for (int64_t round = 0; round < n && !settled; ++round) {             // n - 1 rounds carry a label along the longest path; the n-th changes nothing
    launch_dbscan_round(bitmap, n, w, c->stream); LAUNCHCHK(c);
    int changed = 1;
    HIPCHK(c, hipMemcpyAsync(&changed, w.changed, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    TRY(s.finish());
    settled = changed == 0;
  }
  if (!settled) return fail(c, GR_ERR_STATE, "gr_dbscan_dev: the labels did not settle in n = %lld rounds", (long long)n);
  launch_dbscan_finish(bitmap, n, w, labels, core, n_clusters, c->stream); LAUNCHCHK(c);
  return GR_OK;
}

// ------------------------------------------------------------------ the minimum spanning tree of a device table (mst.hip)
// (like gr_dbscan_dev it waits on the stream: once per Boruvka round, to read how many edges are out)
extern "C" int gr_mst_dev(gr_ctx* c, const float* x, int64_t n, int d, int metric, const double* core, int64_t core_stride, int32_t* eu, int32_t* ev,
                          double* ew, int32_t* rounds_host) {
  if (!c) return GR_ERR_INVALID;
  if (!x || !eu || !ev || !ew) return fail(c, GR_ERR_INVALID, "gr_mst_dev: null pointer");
  if (n <= 0) return fail(c, GR_ERR_INVALID, "gr_mst_dev: n %lld must be positive", (long long)n);
  if (d <= 0) return fail(c, GR_ERR_INVALID, "gr_mst_dev: d %d must be positive", d);
  if (metric != 0 && metric != 1) return fail(c, GR_ERR_INVALID, "gr_mst_dev: metric %d: 0 (euclidean) or 1 (cosine)", metric);
  if (core_stride < 1) return fail(c, GR_ERR_INVALID, "gr_mst_dev: core_stride %lld: at least 1 double from one row's core distance to the next", (long long)core_stride);
  if (n < 2 || n > GR_MST_MAX_N) return fail(c, GR_ERR_UNSUPPORTED, "gr_mst_dev: n %lld: between 2 and %d rows", (long long)n, GR_MST_MAX_N);
  if (d > GR_MST_MAX_D) return fail(c, GR_ERR_UNSUPPORTED, "gr_mst_dev: d %d: at most %d columns", d, GR_MST_MAX_D);
  Staging s(c);
  auto scratch = s.reserve<char>(mst_workspace_bytes(n));
  TRY(s.grow());
  const MstScratch w = mst_carve(s.ptr(scratch), n);
  if (launch_mst_begin(x, n, d, metric, w, c->stream)) return fail(c, GR_ERR_UNSUPPORTED, "gr_mst_dev: unsupported size");
  LAUNCHCHK(c);
  int cap = 0;
  while (((int64_t)1 << cap) < n) ++cap;                                // ceil(log2 n): every round at least halves the component count
  int rounds = 0, edges = 0;
  while (rounds < cap && edges < n - 1) {
    launch_mst_round(x, n, d, metric, core, core_stride, w, c->stream); LAUNCHCHK(c);
    HIPCHK(c, hipMemcpyAsync(&edges, w.n_edges, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    TRY(s.finish());
    ++rounds;
  }
  if (edges != n - 1) return fail(c, GR_ERR_STATE, "gr_mst_dev: %d of %lld edges after %d rounds (non-finite elements?)", edges, (long long)(n - 1), rounds);
  launch_mst_finish(n, w, eu, ev, ew, c->stream); LAUNCHCHK(c);
  if (rounds_host) *rounds_host = rounds;
  return GR_OK;
}

// ------------------------------------------------------------------ the sampling layer of a VAE (vae.hip)
static int vae_check(gr_ctx* c, const char* who, bool null_ptr, int64_t B, int nd) {
  if (null_ptr) return fail(c, GR_ERR_INVALID, "%s: null pointer", who);
  if (B <= 0 || nd <= 0) return fail(c, GR_ERR_INVALID, "%s: B %lld and nd %d must be positive", who, (long long)B, nd);
  if (nd > 256) return fail(c, GR_ERR_UNSUPPORTED, "%s: nd %d: at most 256 latent dimensions", who, nd);
  if (B >= ((int64_t)1 << 31)) return fail(c, GR_ERR_UNSUPPORTED, "%s: B %lld: fewer than 2^31 rows", who, (long long)B);
  return GR_OK;
}
extern "C" int gr_vae_sample_dev(gr_ctx* c, const float* h, const float* eps, int64_t B, int nd, float* z, float* kl_rows, double* kl) {
  if (!c) return GR_ERR_INVALID;
  TRY(vae_check(c, "gr_vae_sample_dev", !h || !z, B, nd));
  Staging s(c);
  auto scratch = s.reserve<char>(kl ? chain_mean_workspace_bytes(B) : 0);
  if (kl) TRY(s.grow());
  if (launch_vae_sample(h, eps, B, nd, z, kl_rows, kl, kl ? s.ptr(scratch) : nullptr, c->stream)) return fail(c, GR_ERR_UNSUPPORTED, "gr_vae_sample_dev: unsupported size");
  LAUNCHCHK(c);
  return GR_OK;
}
extern "C" int gr_vae_sample_backward_dev(gr_ctx* c, const float* h, const float* eps, const float* gz, int64_t B, int nd, double kl_weight, float* gh) {
  if (!c) return GR_ERR_INVALID;
  TRY(vae_check(c, "gr_vae_sample_backward_dev", !h || !gz || !gh, B, nd));
  if (launch_vae_sample_backward(h, eps, gz, B, nd, kl_weight / (double)B, gh, c->stream)) return fail(c, GR_ERR_UNSUPPORTED, "gr_vae_sample_backward_dev: unsupported size");
  LAUNCHCHK(c);
  return GR_OK;
}
// the same kernels on staged copies of host tensors
extern "C" int gr_vae_sample_host(gr_ctx* c, const float* h, const float* eps, int64_t B, int nd, float* z, float* kl_rows, double* kl) {
  if (!c) return GR_ERR_INVALID;
  TRY(vae_check(c, "gr_vae_sample_host", !h || !z, B, nd));
  const size_t n = (size_t)B * nd;
  Staging s(c);
  auto scratch = s.reserve<char>(chain_mean_workspace_bytes(B));
  auto dh = s.reserve<float>(2 * n), de = s.reserve<float>(n), dz = s.reserve<float>(n), dr = s.reserve<float>((size_t)B);
  auto dk = s.reserve<double>(1);
  TRY(s.grow()); TRY(s.upload(dh, h));
  if (eps) TRY(s.upload(de, eps));
  if (launch_vae_sample(s.ptr(dh), eps ? s.ptr(de) : nullptr, B, nd, s.ptr(dz), kl_rows ? s.ptr(dr) : nullptr, kl ? s.ptr(dk) : nullptr, s.ptr(scratch), c->stream))
    return fail(c, GR_ERR_UNSUPPORTED, "gr_vae_sample_host: unsupported size");
  LAUNCHCHK(c);
  TRY(s.download(z, dz));
  if (kl_rows) TRY(s.download(kl_rows, dr));
  if (kl) TRY(s.download(kl, dk));
  return s.finish();
}
extern "C" int gr_vae_sample_backward_host(gr_ctx* c, const float* h, const float* eps, const float* gz, int64_t B, int nd, double kl_weight, float* gh) {
  if (!c) return GR_ERR_INVALID;
  TRY(vae_check(c, "gr_vae_sample_backward_host", !h || !gz || !gh, B, nd));
  const size_t n = (size_t)B * nd;
  Staging s(c);
  auto dh = s.reserve<float>(2 * n), de = s.reserve<float>(n), dg = s.reserve<float>(n), dout = s.reserve<float>(2 * n);
  TRY(s.grow()); TRY(s.upload(dh, h)); TRY(s.upload(dg, gz));
  if (eps) TRY(s.upload(de, eps));
  if (launch_vae_sample_backward(s.ptr(dh), eps ? s.ptr(de) : nullptr, s.ptr(dg), B, nd, kl_weight / (double)B, s.ptr(dout), c->stream))
    return fail(c, GR_ERR_UNSUPPORTED, "gr_vae_sample_backward_host: unsupported size");
  LAUNCHCHK(c);
  TRY(s.download(gh, dout));
  return s.finish();
}

// ------------------------------------------------------------------ SSIM and MSE per image (quality.hip)
static int ssim_check(gr_ctx* c, const char* who, bool null_ptr, int64_t n, int channels, int h, int w, int win, double data_range) {
  if (null_ptr) return fail(c, GR_ERR_INVALID, "%s: null pointer", who);
  if (n <= 0 || n >= ((int64_t)1 << 31) || channels <= 0) return fail(c, GR_ERR_INVALID, "%s: n %lld (1 .. 2^31 - 1) and channels %d must be positive", who, (long long)n, channels);
  if (win < 3 || win > GR_SSIM_MAX_WIN || !(win & 1)) return fail(c, GR_ERR_INVALID, "%s: win %d: an odd window of 3 .. %d", who, win, GR_SSIM_MAX_WIN);
  if (h < win || w < win || h > GR_SSIM_MAX_HW || w > GR_SSIM_MAX_HW)
    return fail(c, GR_ERR_INVALID, "%s: h %d, w %d: images of win = %d .. %d pixels a side", who, h, w, win, GR_SSIM_MAX_HW);
  if (!(data_range > 0)) return fail(c, GR_ERR_INVALID, "%s: data_range %g must be positive", who, data_range);
  return ssim_args_ok((long)n, channels, h, w, win) ? GR_OK : fail(c, GR_ERR_INVALID, "%s: unsupported size", who);
}
static int ssim_launch_status(gr_ctx* c, const char* who, int r) {
  if (r == 2) return fail(c, GR_ERR_HIP, "%s: the device refuses the kernel's LDS", who);
  if (r) return fail(c, GR_ERR_INVALID, "%s: unsupported size", who);
  LAUNCHCHK(c);
  return GR_OK;
}
extern "C" int gr_ssim_dev(gr_ctx* c, const float* a, const float* b, int64_t n, int channels, int h, int w, int win, double sigma, double data_range,
                           float* ssim_rows, float* mse_rows, double* mean) {
  if (!c) return GR_ERR_INVALID;
  TRY(ssim_check(c, "gr_ssim_dev", !a || !b || !ssim_rows, n, channels, h, w, win, data_range));
  Staging s(c);
  auto scratch = s.reserve<char>(mean ? chain_mean_workspace_bytes((long)n) : 0);
  if (mean) TRY(s.grow());
  return ssim_launch_status(c, "gr_ssim_dev", launch_ssim(a, b, (long)n, channels, h, w, win, sigma, data_range, ssim_rows, mse_rows, mean,
                                                          mean ? s.ptr(scratch) : nullptr, c->stream));
}
// the same kernels on staged copies of host tensors
extern "C" int gr_ssim_host(gr_ctx* c, const float* a, const float* b, int64_t n, int channels, int h, int w, int win, double sigma, double data_range,
                            float* ssim_rows, float* mse_rows, double* mean) {
  if (!c) return GR_ERR_INVALID;
  TRY(ssim_check(c, "gr_ssim_host", !a || !b || !ssim_rows, n, channels, h, w, win, data_range));
  const size_t elems = (size_t)n * channels * h * w;
  Staging s(c);
  auto scratch = s.reserve<char>(chain_mean_workspace_bytes((long)n));
  auto da = s.reserve<float>(elems), db = s.reserve<float>(elems), ds = s.reserve<float>((size_t)n), dm = s.reserve<float>((size_t)n);
  auto dq = s.reserve<double>(1);
  TRY(s.grow()); TRY(s.upload(da, a)); TRY(s.upload(db, b));
  TRY(ssim_launch_status(c, "gr_ssim_host", launch_ssim(s.ptr(da), s.ptr(db), (long)n, channels, h, w, win, sigma, data_range, s.ptr(ds),
                                                        mse_rows ? s.ptr(dm) : nullptr, mean ? s.ptr(dq) : nullptr, s.ptr(scratch), c->stream)));
  TRY(s.download(ssim_rows, ds));
  if (mse_rows) TRY(s.download(mse_rows, dm));
  if (mean) TRY(s.download(mean, dq));
  return s.finish();
}

// ------------------------------------------------------------------ exact t-SNE of a device table (tsne.hip)
static int tsne_n_check(gr_ctx* c, const char* who, int64_t n, int64_t least) {
  if (n < least) return fail(c, GR_ERR_INVALID, "%s: n %lld: at least %lld rows", who, (long long)n, (long long)least);
  if (n > GR_TSNE_MAX_N) return fail(c, GR_ERR_UNSUPPORTED, "%s: n %lld: at most GR_TSNE_MAX_N = %d rows", who, (long long)n, GR_TSNE_MAX_N);
  return GR_OK;
}
extern "C" int gr_tsne_affinities_dev(gr_ctx* c, const float* x, int64_t n, int d, double perplexity, float* p, double* beta, int32_t* info) {
  if (!c) return GR_ERR_INVALID;
  if (!x || !p || !info) return fail(c, GR_ERR_INVALID, "gr_tsne_affinities_dev: null pointer");
  TRY(tsne_n_check(c, "gr_tsne_affinities_dev", n, 4));
  if (d < 1) return fail(c, GR_ERR_INVALID, "gr_tsne_affinities_dev: d %d must be positive", d);
  if (!(perplexity >= 1.0 && perplexity <= (double)(n - 1) / 3.0))
    return fail(c, GR_ERR_INVALID, "gr_tsne_affinities_dev: perplexity %g: 1 to (n - 1) / 3 = %g", perplexity, (double)(n - 1) / 3.0);
  return scratch_launch(c, tsne_affinities_workspace_bytes((int)n, d), [&](void* ws) {
    return launch_tsne_affinities(x, (int)n, d, perplexity, p, beta, info, ws, c->stream);
  }, {GR_ERR_UNSUPPORTED, "gr_tsne_affinities_dev: unsupported size", 0}, {GR_ERR_HIP, "gr_tsne_affinities_dev: hipMemsetAsync failed", 0});
}
extern "C" int gr_tsne_gradient_dev(gr_ctx* c, const float* p, const float* y, int64_t n, float exaggeration, float* grad, double* z) {
  if (!c) return GR_ERR_INVALID;
  if (!p || !y || !grad) return fail(c, GR_ERR_INVALID, "gr_tsne_gradient_dev: null pointer");
  TRY(tsne_n_check(c, "gr_tsne_gradient_dev", n, 1));
  return scratch_launch(c, tsne_iter_workspace_bytes((int)n), [&](void* ws) { return launch_tsne_gradient(p, y, (int)n, exaggeration, grad, z, ws, c->stream); },
                        {GR_ERR_UNSUPPORTED, "gr_tsne_gradient_dev: unsupported size", 0});
}
extern "C" int gr_tsne_update_dev(gr_ctx* c, float* y, const float* grad, float* inc, float* gains, int64_t n, float eta, float momentum, float min_gain) {
  if (!c) return GR_ERR_INVALID;
  if (!y || !grad || !inc || !gains) return fail(c, GR_ERR_INVALID, "gr_tsne_update_dev: null pointer");
  TRY(tsne_n_check(c, "gr_tsne_update_dev", n, 1));
  return scratch_launch(c, tsne_iter_workspace_bytes((int)n), [&](void* ws) { return launch_tsne_update(y, grad, inc, gains, (int)n, eta, momentum, min_gain, ws, c->stream); },
                        {GR_ERR_UNSUPPORTED, "gr_tsne_update_dev: unsupported size", 0});
}
extern "C" int gr_tsne_kl_dev(gr_ctx* c, const float* p, const float* y, int64_t n, double* kl) {
  if (!c) return GR_ERR_INVALID;
  if (!p || !y || !kl) return fail(c, GR_ERR_INVALID, "gr_tsne_kl_dev: null pointer");
  TRY(tsne_n_check(c, "gr_tsne_kl_dev", n, 1));
  return scratch_launch(c, tsne_iter_workspace_bytes((int)n), [&](void* ws) { return launch_tsne_kl(p, y, (int)n, kl, ws, c->stream); },
                        {GR_ERR_UNSUPPORTED, "gr_tsne_kl_dev: unsupported size", 0});
}
extern "C" int gr_tsne_run_dev(gr_ctx* c, const float* p, int64_t n, const gr_tsne_config* cfg, float* y, float* inc, float* gains, int first_iter, int iters,
                               double* kl, int kl_every) {
  if (!c) return GR_ERR_INVALID;
  if (!p || !cfg || !y || !inc || !gains) return fail(c, GR_ERR_INVALID, "gr_tsne_run_dev: null pointer");
  TRY(tsne_n_check(c, "gr_tsne_run_dev", n, 1));
  if (first_iter < 0 || iters < 0 || kl_every < 0) return fail(c, GR_ERR_INVALID, "gr_tsne_run_dev: first_iter %d, iters %d and kl_every %d must not be negative", first_iter, iters, kl_every);
  if (first_iter > 0x7FFFFFFF - iters) return fail(c, GR_ERR_INVALID, "gr_tsne_run_dev: first_iter %d + iters %d: below 2^31", first_iter, iters);
  Staging s(c);
  auto scratch = s.reserve<char>(tsne_iter_workspace_bytes((int)n));
  auto grad = s.reserve<float>(2 * (size_t)n);
  TRY(s.grow());
  for (int t = first_iter; t < first_iter + iters; ++t) {                 // the public gradient and update launches, back to back on the stream
    const float ex = t < cfg->stop_lying_iter ? cfg->exaggeration : 1.0f, mom = t < cfg->mom_switch_iter ? cfg->momentum0 : cfg->momentum1;
    if (launch_tsne_gradient(p, y, (int)n, ex, s.ptr(grad), nullptr, s.ptr(scratch), c->stream) ||
        launch_tsne_update(y, s.ptr(grad), inc, gains, (int)n, cfg->eta, mom, cfg->min_gain, s.ptr(scratch), c->stream))
      return fail(c, GR_ERR_UNSUPPORTED, "gr_tsne_run_dev: unsupported size");
    if (kl && kl_every && (t + 1) % kl_every == 0 && launch_tsne_kl(p, y, (int)n, kl + ((t + 1) / kl_every - 1), s.ptr(scratch), c->stream))
      return fail(c, GR_ERR_UNSUPPORTED, "gr_tsne_run_dev: unsupported size");
    LAUNCHCHK(c);
  }
  return GR_OK;
}
extern "C" int gr_map_cells_dev(gr_ctx* c, const float* y, int64_t n, int grid_h, int grid_w, int64_t* rows_out, int32_t* counts) {
  if (!c) return GR_ERR_INVALID;
  if (!y || !rows_out) return fail(c, GR_ERR_INVALID, "gr_map_cells_dev: null pointer");
  if (n < 1) return fail(c, GR_ERR_INVALID, "gr_map_cells_dev: n %lld must be positive", (long long)n);
  if (grid_h < 1 || grid_w < 1) return fail(c, GR_ERR_INVALID, "gr_map_cells_dev: grid %d x %d must be positive", grid_h, grid_w);
  if (n >= ((int64_t)1 << 31)) return fail(c, GR_ERR_UNSUPPORTED, "gr_map_cells_dev: n %lld: fewer than 2^31 rows", (long long)n);
  if (grid_h > 1024 || grid_w > 1024) return fail(c, GR_ERR_UNSUPPORTED, "gr_map_cells_dev: grid %d x %d: at most 1024 cells a side", grid_h, grid_w);
  return scratch_launch(c, map_cells_workspace_bytes(grid_h * grid_w), [&](void* ws) {
    return launch_map_cells(y, (long)n, grid_h, grid_w, reinterpret_cast<long*>(rows_out), counts, ws, c->stream);
  }, {GR_ERR_UNSUPPORTED, "gr_map_cells_dev: unsupported size", 0});
}

// ------------------------------------------------------------------ apply_r.lua:355-372 detectAnomalies' distance
extern "C" int gr_l2_distance_rows_host(gr_ctx* c, const float* a, const float* b, int64_t n, int64_t d, double* out) {
  if (!c || !a || !b || !out || n <= 0 || d <= 0) return GR_ERR_INVALID;
  Staging s(c);
  auto da = s.reserve<float>((size_t)n * d), db = s.reserve<float>((size_t)n * d);
  auto dout = s.reserve<double>(n);
  TRY(s.grow()); TRY(s.upload(da, a)); TRY(s.upload(db, b));
  launch_l2_distance_rows(s.ptr(da), s.ptr(db), n, d, s.ptr(dout), c->stream); LAUNCHCHK(c);
  TRY(s.download(out, dout));
  return s.finish();
}
extern "C" int gr_l2_distance_rows_dev(gr_ctx* c, const float* a, const float* b, int64_t n, int64_t d, double* out) {
  if (!c || !a || !b || !out || n <= 0 || d <= 0) return GR_ERR_INVALID;
  Staging s(c);
  auto dout = s.reserve<double>(n);
  TRY(s.grow());
  launch_l2_distance_rows(a, b, n, d, s.ptr(dout), c->stream); LAUNCHCHK(c);
  TRY(s.download(out, dout));
  return s.finish();
}

// ------------------------------------------------------------------ the pictures of apply_r.lua / sample.lua (render.hip)
extern "C" int gr_rows_mean_dev(gr_ctx* c, const float* table, int64_t n_rows, int64_t d, const int64_t* rows, int n, float* out) {
  if (!c) return GR_ERR_INVALID;
  if (!table || !out || (n > 0 && !rows)) return fail(c, GR_ERR_INVALID, "gr_rows_mean_dev: null pointer");
  if (n_rows <= 0 || d <= 0 || n < 0) return fail(c, GR_ERR_INVALID, "gr_rows_mean_dev: n_rows %lld and d %lld must be positive, n %d not negative", (long long)n_rows, (long long)d, n);
  for (int j = 0; j < n; ++j)
    if (rows[j] < 0 || rows[j] >= n_rows) return fail(c, GR_ERR_INVALID, "gr_rows_mean_dev: rows[%d] = %lld is outside [0, %lld)", j, (long long)rows[j], (long long)n_rows);
  Staging s(c);
  auto drows = s.reserve<long>(n > 0 ? n : 1);
  TRY(s.grow());
  if (n > 0) TRY(s.upload_now(drows, rows));
  launch_rows_mean(table, (long)d, s.ptr(drows), n, out, c->stream); LAUNCHCHK(c);
  return GR_OK;
}
// what both picture grids ask of their outputs and source, and of the size of the picture
static int grid_source_check(gr_ctx* c, const char* who, const void* grid, const void* u8, int channels, int from_space) {
  if (!grid && !u8) return fail(c, GR_ERR_INVALID, "%s: both outputs are null", who);
  if (from_space < -1 || from_space > GR_CS_HSL) return fail(c, GR_ERR_INVALID, "%s: unknown color space <from>: %d", who, from_space);
  if ((channels != 1 && channels != 3) || (from_space >= 0 && channels != (from_space == GR_CS_Y ? 1 : 3)))
    return fail(c, GR_ERR_INVALID, "%s: %d channel(s) with from_space %d", who, channels, from_space);
  return GR_OK;
}
static int grid_size_check(gr_ctx* c, const char* who, long GH, long GW) {
  return GH > (1 << 20) || GW > (1 << 20) || GH * GW > (1L << 28) ? fail(c, GR_ERR_INVALID, "%s: a %ld x %ld grid is too large", who, GH, GW) : GR_OK;
}
extern "C" int gr_image_grid_dev(gr_ctx* c, const float* const* src, const int64_t* n_rows, int slots, int channels, int h, int w, int from_space,
                                 const int64_t* rows, int n_tiles, int nrow, int padding, int margin, const float* bg, const uint8_t* inset,
                                 const float* inset_rgb, float fill, int auto_range, float lo, float hi, float* grid, uint8_t* u8) {
  if (!c) return GR_ERR_INVALID;
  if (slots != 1 && slots != 2) return fail(c, GR_ERR_INVALID, "gr_image_grid_dev: slots %d (1 or 2)", slots);
  if (!src || !n_rows || !rows) return fail(c, GR_ERR_INVALID, "gr_image_grid_dev: null pointer");
  for (int s = 0; s < slots; ++s)
    if (!src[s] || n_rows[s] <= 0) return fail(c, GR_ERR_INVALID, "gr_image_grid_dev: table %d is null or has no rows", s);
  TRY(grid_source_check(c, "gr_image_grid_dev", grid, u8, channels, from_space));
  if (h <= 0 || w <= 0 || n_tiles <= 0 || nrow <= 0 || padding < 0 || padding > 64 || margin < 0 || margin > 1)
    return fail(c, GR_ERR_INVALID, "gr_image_grid_dev: bad geometry (h %d, w %d, n_tiles %d, nrow %d, padding %d in [0, 64], margin %d in {0, 1})", h, w, n_tiles, nrow, padding, margin);
  if (inset && !inset_rgb) return fail(c, GR_ERR_INVALID, "gr_image_grid_dev: inset flags without inset_rgb");
  if (!auto_range && !(lo <= hi)) return fail(c, GR_ERR_INVALID, "gr_image_grid_dev: display range [%g, %g]", (double)lo, (double)hi);
  GridGeom g{};
  g.slots = slots; g.C = channels; g.Cout = from_space >= 0 ? 3 : channels; g.H = h; g.W = w; g.from = from_space;
  g.n_tiles = n_tiles; g.xmaps = nrow < n_tiles ? nrow : n_tiles; g.padding = padding; g.margin = margin;
  const int ymaps = (n_tiles + g.xmaps - 1) / g.xmaps;
  const long TH = (long)h + 2 * margin, TW = (long)slots * w + 2 * margin, GH = (TH + padding) * ymaps, GW = (TW + padding) * g.xmaps;
  TRY(grid_size_check(c, "gr_image_grid_dev", GH, GW));
  g.TH = (int)TH; g.TW = (int)TW; g.cellH = (int)TH + padding; g.cellW = (int)TW + padding; g.GH = (int)GH; g.GW = (int)GW;
  std::vector<GridTile> tiles((size_t)n_tiles);
  for (int t = 0; t < n_tiles; ++t) {
    GridTile& tl = tiles[t];
    tl.row[0] = tl.row[1] = -1;
    for (int s = 0; s < slots; ++s) {
      const int64_t r = rows[(size_t)t * slots + s];
      if (r < -1 || r >= n_rows[s]) return fail(c, GR_ERR_INVALID, "gr_image_grid_dev: row %lld of tile %d, slot %d is outside [-1, %lld)", (long long)r, t, s, (long long)n_rows[s]);
      tl.row[s] = (long)r;
    }
    for (int k = 0; k < 3; ++k) tl.bg[k] = bg ? bg[(size_t)t * 3 + k] : 0.f;
    tl.inset = inset ? inset[t] != 0 : 0;
  }
  for (int k = 0; k < 3; ++k) g.inset_rgb[k] = inset_rgb ? inset_rgb[k] : 0.f;
  g.fill = fill; g.lo = lo; g.hi = hi;
  Staging s(c);
  auto parts = s.reserve<float>(2 * GRID_RANGE_BLOCKS);              // the auto-range blocks: the first region
  auto dtiles = s.reserve<GridTile>(n_tiles);
  TRY(s.grow()); TRY(s.upload_now(dtiles, tiles.data()));
  g.src[0] = src[0]; g.src[1] = slots == 2 ? src[1] : src[0]; g.tiles = s.ptr(dtiles);
  launch_image_grid(g, auto_range ? s.ptr(parts) : nullptr, grid, u8, c->stream); LAUNCHCHK(c);
  return GR_OK;
}

// ------------------------------------------------------------------ the trainers' progress pictures (render.hip)
extern "C" int gr_progress_grid_dev(gr_ctx* c, const float* table, int64_t n_rows, int channels, int h, int w, int from_space,
                                    const int64_t* rows, int n_show, int grid_h, int grid_w, int epoch, float* grid, uint8_t* u8) {
  if (!c) return GR_ERR_INVALID;
  if (!table) return fail(c, GR_ERR_INVALID, "gr_progress_grid_dev: the table is null");
  TRY(grid_source_check(c, "gr_progress_grid_dev", grid, u8, channels, from_space));
  if (n_rows < 1 || h < 1 || w < 1 || grid_h < 1 || grid_w < 1 || n_show < 0)
    return fail(c, GR_ERR_INVALID, "gr_progress_grid_dev: bad geometry (n_rows %lld, h %d, w %d, grid %d x %d, n_show %d)", (long long)n_rows, h, w, grid_h, grid_w, n_show);
  if (epoch < 0) return fail(c, GR_ERR_INVALID, "gr_progress_grid_dev: epoch %d is negative", epoch);
  const long GH = (long)grid_h * h + 7, GW = (long)grid_w * w;
  TRY(grid_size_check(c, "gr_progress_grid_dev", GH, GW));
  ProgressGeom g{};
  for (int e = epoch; g.ndig == 0 || e > 0; e /= 10) g.dig[g.ndig++] = (unsigned char)(e % 10);
  if (GW - 2 - 6L * g.ndig < 0)
    return fail(c, GR_ERR_INVALID, "gr_progress_grid_dev: the %d digit(s) of epoch %d do not fit a grid %ld pixels wide", g.ndig, epoch, GW);
  const long cells = (long)grid_h * grid_w;
  g.n_cells = (int)(n_show < cells ? n_show : cells);
  if (g.n_cells > 0 && !rows) return fail(c, GR_ERR_INVALID, "gr_progress_grid_dev: rows_host is null");
  for (int t = 0; t < g.n_cells; ++t)
    if (rows[t] < 0 || rows[t] >= n_rows) return fail(c, GR_ERR_INVALID, "gr_progress_grid_dev: rows[%d] = %lld is outside [0, %lld)", t, (long long)rows[t], (long long)n_rows);
  g.C = channels; g.Cout = from_space >= 0 ? 3 : channels; g.H = h; g.W = w; g.from = from_space;
  g.grid_w = grid_w; g.GH = (int)GH; g.GW = (int)GW;
  Staging s(c);
  auto drows = s.reserve<long>(g.n_cells > 0 ? g.n_cells : 1);
  TRY(s.grow());
  if (g.n_cells > 0) TRY(s.upload_now(drows, rows));
  g.src = table; g.rows = s.ptr(drows);
  const bool vec = w % 4 == 0 && (uintptr_t)table % 16 == 0 && (uintptr_t)grid % 16 == 0 && (uintptr_t)u8 % 4 == 0;
  launch_progress_grid(g, vec, grid, u8, c->stream); LAUNCHCHK(c);
  return GR_OK;
}

// ------------------------------------------------------------------ sample.lua:130-148 findClosestNeighboursOf (neighbours.hip)
static int l2_nearest_check(gr_ctx* c, const float* table, int64_t n, int64_t d, const float* queries, int Q, int k, const int64_t* idx_out, const double* dist_out) {
  if (!c) return GR_ERR_INVALID;
  if (!table || !queries || !idx_out || !dist_out || n <= 0 || d < 1 || d > 65536 || Q < 1 || Q > 64 || k < 1 || k > n)
    return fail(c, GR_ERR_INVALID, "gr_l2_nearest: bad arguments (n %lld, d %lld, q %d, k %d)", (long long)n, (long long)d, Q, k);
  if (k > 128) return fail(c, GR_ERR_UNSUPPORTED, "gr_l2_nearest: k > 128");
  if (n >= 0xFFFFFFFFll) return fail(c, GR_ERR_UNSUPPORTED, "gr_l2_nearest: n >= 2^32 - 1");
  return GR_OK;
}
extern "C" int gr_l2_nearest_dev(gr_ctx* c, const float* table, int64_t n, int64_t d, const float* queries, int Q, int k,
                                 int64_t* idx_out, double* dist_out) {
  TRY(l2_nearest_check(c, table, n, d, queries, Q, k, idx_out, dist_out));
  Staging s(c);
  auto scratch = s.reserve<char>(l2_nearest_workspace_bytes(n, Q));     // launch_l2_nearest takes c->ws itself: the first region
  const size_t res = sizeof(long) * (size_t)Q * k + sizeof(double) * (size_t)Q * k + sizeof(unsigned) * (size_t)Q;
  auto dres = s.reserve<char>(res);                                     // [idx | dist | status]: one copy back
  TRY(s.grow());
  long* d_idx = (long*)s.ptr(dres); double* d_dist = (double*)(d_idx + (size_t)Q * k); unsigned* d_status = (unsigned*)(d_dist + (size_t)Q * k);
  std::vector<char> h(res);
  for (int exact = l2_nearest_direct(n) ? 1 : 0; exact < 2; ++exact) {
    if (launch_l2_nearest(table, n, (int)d, queries, Q, k, d_idx, d_dist, d_status, s.ptr(scratch), exact, c->cu_count, c->stream))
      return fail(c, GR_ERR_UNSUPPORTED, "gr_l2_nearest: unsupported size");
    LAUNCHCHK(c);
    TRY(s.download(h.data(), dres)); TRY(s.finish());
    bool over = false;
    for (int q = 0; q < Q && !exact; ++q) { unsigned st; memcpy(&st, h.data() + res - sizeof(unsigned) * (size_t)(Q - q), sizeof st); over = over || st != 0u; }
    if (!over) break;             // (the exact path does not write the status words)
  }
  memcpy(idx_out, h.data(), sizeof(long) * (size_t)Q * k);
  memcpy(dist_out, h.data() + sizeof(long) * (size_t)Q * k, sizeof(double) * (size_t)Q * k);
  return GR_OK;
}
extern "C" int gr_l2_nearest_host(gr_ctx* c, const float* table, int64_t n, int64_t d, const float* queries, int Q, int k,
                                  int64_t* idx_out, double* dist_out) {
  TRY(l2_nearest_check(c, table, n, d, queries, Q, k, idx_out, dist_out));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t tb = sizeof(float) * (size_t)n * d, qb = sizeof(float) * (size_t)Q * d;
  DevMem tmp(c->stream); float *dt = nullptr, *dq = nullptr;
  HIPCHK(c, tmp.dev(&dt, tb)); HIPCHK(c, tmp.dev(&dq, qb));
  if (hipMemcpyAsync(dt, table, tb, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipMemcpyAsync(dq, queries, qb, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    return fail(c, GR_ERR_HIP, "upload failed");
  return gr_l2_nearest_dev(c, dt, n, d, dq, Q, k, idx_out, dist_out);
}

// ------------------------------------------------------------------ single-kernel entry points
static int with_prepped(gr_ctx* c, const float* w, int cin, int cout, bool bwd, DevMem& tmp, float** wt) {
  const ConvWeightLayout L = bwd ? conv_weight_layout(cout, cin) : conv_weight_layout(cin, cout);
  HIPCHK(c, tmp.dev(wt, sizeof(float) * L.elems()));
  launch_conv_weight_prep(w, *wt, cin, cout, bwd, c->stream);
  LAUNCHCHK(c);
  return GR_OK;
}
// f16x3: the weight maximum goes to c->amax[2]
static int conv_split_once(gr_ctx* c, const float* w, int cin, int cout, bool bwd, DevMem& tmp, void** ws) {
  HIPCHK(c, tmp.dev(ws, conv_weight_split_bytes(cin, cout, bwd)));
  launch_conv_weight_split(w, *ws, cin, cout, bwd, c->stream, c->conv_mode == 2 ? 2 : 3, c->amax + 2 * AMAX_WORDS);
  LAUNCHCHK(c);
  return GR_OK;
}
// how the gr_conv3_* calls end: the launch status is read first, then their weight image goes (tmp waits for the stream)
static int conv_launched(gr_ctx* c) { hipError_t e = hipGetLastError(); return e == hipSuccess ? GR_OK : fail(c, GR_ERR_HIP, "conv launch failed: %s", hipGetErrorString(e)); }
extern "C" int gr_conv3_forward_dev(gr_ctx* c, const float* in, const float* w, const float* bias, float* out, int B, int cin, int cout, int h, int wd, int up) {
  if (!c || !in || !w || !out) return GR_ERR_INVALID;
  DevMem tmp(c->stream); void* wt = nullptr; float* wt32 = nullptr;
  if (c->conv_mode == 2 && up && conv_up2_supported(cin, cout, h, wd)) {
    // the fused up-sampling layer as four 2x2 convolutions (the path a net takes for such a stage in f16x3 mode)
    HIPCHK(c, tmp.dev(&wt, conv_weight_up2_bytes(cin, cout)));
    launch_conv_weight_up2_split(w, wt, cin, cout, c->stream, c->amax + 2 * AMAX_WORDS, true);
    launch_absmax(in, (long)B * cin * (h / 2) * (wd / 2), c->amax, c->stream);
    launch_conv3x3_up2_f16x3(in, wt, bias, out, B, cin, cout, h, wd, c->stream, nullptr, c->amax, c->amax + 2 * AMAX_WORDS, nullptr);
  } else if (c->conv_mode >= 1 && cout > 4) {
    TRY(conv_split_once(c, w, cin, cout, false, tmp, &wt));
    if (c->conv_mode == 2) launch_absmax(in, (long)B * cin * (up ? (h / 2) * (wd / 2) : h * wd), c->amax, c->stream);
    launch_conv3x3_split(in, wt, bias, out, B, cin, cout, h, wd, up != 0, c->stream, nullptr, c->conv_mode == 2 ? 2 : 3, c->amax, c->amax + 2 * AMAX_WORDS);
  } else {
    TRY(with_prepped(c, w, cin, cout, false, tmp, &wt32));
    launch_conv3x3(in, wt32, bias, out, B, cin, cout, h, wd, up != 0, c->stream, w);
  }
  return conv_launched(c);
}
extern "C" int gr_conv3_backward_data_dev(gr_ctx* c, const float* gout, const float* w, float* gin, int B, int cin, int cout, int h, int wd) {
  if (!c || !gout || !w || !gin) return GR_ERR_INVALID;
  DevMem tmp(c->stream); void* wt = nullptr; float* wt32 = nullptr;
  if (c->conv_mode >= 1 && cin > 4) {
    TRY(conv_split_once(c, w, cin, cout, true, tmp, &wt));
    if (c->conv_mode == 2) launch_absmax(gout, (long)B * cout * h * wd, c->amax + AMAX_WORDS, c->stream);
    launch_conv3x3_split(gout, wt, nullptr, gin, B, cout, cin, h, wd, false, c->stream, nullptr, c->conv_mode == 2 ? 2 : 3, c->amax + AMAX_WORDS, c->amax + 2 * AMAX_WORDS);
  } else {
    TRY(with_prepped(c, w, cin, cout, true, tmp, &wt32));
    launch_conv3x3(gout, wt32, nullptr, gin, B, cout, cin, h, wd, false, c->stream);
  }
  return conv_launched(c);
}
extern "C" int gr_conv3_backward_weight_dev(gr_ctx* c, const float* in, const float* gout, float* gw, int B, int cin, int cout, int h, int wd) {
  if (!c || !in || !gout || !gw) return GR_ERR_INVALID;
  int r = ensure_ws(c, conv_wgrad_workspace_bytes(B, cin, cout, h, wd, c->conv_mode)); if (r) return r;
  if (c->conv_mode == 2 && conv_wgrad_is_split(2, cin, wd)) {
    launch_absmax(in, (long)B * cin * h * wd, c->amax, c->stream);
    launch_absmax(gout, (long)B * cout * h * wd, c->amax + AMAX_WORDS, c->stream);
  }
  launch_conv3x3_wgrad(in, gout, gw, c->ws, B, cin, cout, h, wd, c->stream, c->conv_mode, c->amax, c->amax + AMAX_WORDS);
  LAUNCHCHK(c);
  return GR_OK;
}
// Sustained rate of the bare f16x3 inner loop (mfmaloop.hip) on this device: `launches` back-to-back launches (>= 0.3 s of them
// before the timed ones so that the clock settles), HIP events on the ctx stream.  shape 0 = v_mfma_f32_32x32x16_f16 (what the
// convolution kernels issue), 1 = v_mfma_f32_16x16x32_f16.  tflops_out: fp32-accurate TFLOP/s (f16 MFMA rate / 3 products), the
// figure comparable with the 833 TFLOP/s ceiling bench.py prices the f16x3 kernels against.
extern "C" int gr_bench_mfma_loop(gr_ctx* c, int shape, int launches, float* tflops_out) {
  if (!c || !tflops_out || shape < 0 || shape > 1 || launches < 1) return GR_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  int r = ensure_ws(c, mfma_loop_workspace_bytes()); if (r) return r;
  launch_mfma_loop_fill(c->ws, c->stream);
  const int iters = 200;
  for (int i = 0; i < 300; ++i) launch_mfma_loop(shape, c->ws, iters, c->stream);     // ~0.35 s of warm-up under load
  LAUNCHCHK(c);
  Event e0, e1; HIPCHK(c, e0.create()); HIPCHK(c, e1.create());
  HIPCHK(c, hipEventRecord(e0, c->stream));
  for (int i = 0; i < launches; ++i) launch_mfma_loop(shape, c->ws, iters, c->stream);
  HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, hipEventSynchronize(e1));
  float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
  *tflops_out = (float)(mfma_loop_flops(iters) * launches / (ms * 1e-3) / 1e12 / 3.0);
  return GR_OK;
}
extern "C" int gr_bench_conv3(gr_ctx* c, int which, int B, int cin, int cout, int h, int wd, int iters, float* avg_ms) {
  if (!c || iters < 1 || !avg_ms) return GR_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nin = (size_t)B * cin * h * wd, nout = (size_t)B * cout * h * wd, nw = (size_t)cin * cout * 9;
  DevMem tmp(c->stream);
  float *x = nullptr, *y = nullptr, *w = nullptr, *gw = nullptr, *wt = nullptr; void *wsp = nullptr, *wup = nullptr, *xp16 = nullptr; double* statp = nullptr;
  HIPCHK(c, tmp.dev(&x, sizeof(float) * nin)); HIPCHK(c, tmp.dev(&y, sizeof(float) * nout)); HIPCHK(c, tmp.dev(&w, sizeof(float) * nw)); HIPCHK(c, tmp.dev(&gw, sizeof(float) * nw));
  launch_fill_normal(x, (long)nin, 11, c->stream); launch_fill_normal(y, (long)nout, 12, c->stream); launch_fill_normal(w, (long)nw, 13, c->stream);
  (void)hipMemsetAsync(gw, 0, sizeof(float) * nw, c->stream);
  TRY(with_prepped(c, w, cin, cout, which == 1, tmp, &wt));
  const bool split = c->conv_mode >= 1 && which != 2 && (which == 0 ? cout > 4 : cin > 4);
  const int nterm = c->conv_mode == 2 ? 2 : 3;
  if (split) TRY(conv_split_once(c, w, cin, cout, which == 1, tmp, &wsp));      // (which 4 and 5 launch on this image too: forward orientation, same term count)
  TRY(ensure_ws(c, conv_wgrad_workspace_bytes(B, cin, cout, h, wd, c->conv_mode)));
  // f16x3 scales: taken once outside the timed loop (in a net the producing kernel tracks them)
  if (c->conv_mode == 2) { launch_absmax(x, (long)nin, c->amax, c->stream); launch_absmax(y, (long)nout, c->amax + AMAX_WORDS, c->stream); }
  if (which == 3) {      // fused up-sampling layer: x is the source plane [B, cin, h/2, wd/2] (a quarter of the buffer), y the output
    if (c->conv_mode != 2 || !conv_up2_supported(cin, cout, h, wd)) return fail(c, GR_ERR_UNSUPPORTED, "up2 bench needs f16x3 mode and a supported shape");
    HIPCHK(c, tmp.dev(&wup, conv_weight_up2_bytes(cin, cout)));
    launch_conv_weight_up2_split(w, wup, cin, cout, c->stream, c->amax + 2 * AMAX_WORDS, true);
  }
  if (which == 4 || which == 5) {   // operand-ready forward (5: with the BatchNorm statistics epilogue): x converted once outside the loop
    if (c->conv_mode != 2 || !conv_p16_supported(B, cin, cout, h, wd)) return fail(c, GR_ERR_UNSUPPORTED, "p16 bench needs f16x3 mode and a supported shape");
    HIPCHK(c, tmp.dev(&xp16, sizeof(float) * nin));
    HIPCHK(c, tmp.dev(&statp, sizeof(double) * 2 * cout * conv_stat_tiles_max(B, h, wd)));
    launch_to_p16(x, xp16, B, cin, h * wd, c->amax, c->stream);
  }
  auto run = [&]() {
    if (which == 4 || which == 5) { int st = 0; launch_conv3x3_p16(xp16, wsp, nullptr, y, B, cin, cout, h, wd, c->stream, nullptr, c->amax, c->amax + 2 * AMAX_WORDS, nullptr, which == 5 ? statp : nullptr, which == 5 ? &st : nullptr); return; }
    if (which == 3) { launch_conv3x3_up2_f16x3(x, wup, nullptr, y, B, cin, cout, h, wd, c->stream, nullptr, c->amax, c->amax + 2 * AMAX_WORDS, nullptr); return; }
    if (split && which == 0) launch_conv3x3_split(x, wsp, nullptr, y, B, cin, cout, h, wd, false, c->stream, nullptr, nterm, c->amax, c->amax + 2 * AMAX_WORDS);
    else if (split && which == 1) launch_conv3x3_split(y, wsp, nullptr, x, B, cout, cin, h, wd, false, c->stream, nullptr, nterm, c->amax + AMAX_WORDS, c->amax + 2 * AMAX_WORDS);
    else if (which == 0) launch_conv3x3(x, wt, nullptr, y, B, cin, cout, h, wd, false, c->stream, w);
    else if (which == 1) launch_conv3x3(y, wt, nullptr, x, B, cout, cin, h, wd, false, c->stream);
    else launch_conv3x3_wgrad(x, y, gw, c->ws, B, cin, cout, h, wd, c->stream, c->conv_mode, c->amax, c->amax + AMAX_WORDS);
  };
  for (int i = 0; i < 3; ++i) run();
  Event e0, e1; HIPCHK(c, e0.create()); HIPCHK(c, e1.create());
  (void)hipEventRecord(e0, c->stream);
  for (int i = 0; i < iters; ++i) run();
  (void)hipEventRecord(e1, c->stream);
  HIPCHK(c, hipEventSynchronize(e1));
  float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
  *avg_ms = ms / iters;
  LAUNCHCHK(c);
  return GR_OK;
}
