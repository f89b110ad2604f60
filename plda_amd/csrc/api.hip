// plda_amd/csrc/api.hip -- the C ABI of libplda_hip.so (include/plda_hip.h).
// Host-pointer entry points stage through device buffers owned by the handle and
// call the *_device implementations; nothing here computes on the CPU.
#include "trial_source.hpp"
#include "hostio.hpp"

#include <mutex>

#include <algorithm>
#include <cstdarg>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <numeric>
#include <stdexcept>

namespace plda {

std::atomic<int64_t> g_device_bytes{0};
std::atomic<int64_t> g_device_bytes_peak{0};
std::atomic<int> g_scratch_poison{0};
thread_local hipStream_t g_call_stream = nullptr;
static thread_local std::string g_create_err;

int fail(plda_handle *h, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_create_err = buf;
  return code;
}

int refuse_on_cosine(plda_handle *h, const char *fn) {
  if (h->backend != PLDA_BACKEND_COSINE) return PLDA_OK;
  return fail(h, PLDA_E_INVAL, "%s: the cosine back-end is selected on this handle, which holds no PLDA model and takes none "
                               "(plda_backend_set(h, PLDA_BACKEND_PLDA, 0) returns it to the PLDA state)", fn);
}

int hip_fail(plda_handle *h, hipError_t e, const char *what, const char *file, int line) {
  (void)hipGetLastError();   // a failed call leaves its code behind: the next launch check would report it again
  return fail(h, PLDA_E_HIP, "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
}

void note_kernel(plda_handle *h, const char *name, int nargs, int a, int b, int c, const char *suffix) {
  char e[96];
  size_t n = 0;
  auto put = [&](const char *t) { while (*t && n + 1 < sizeof(e)) e[n++] = *t++; };
  auto num = [&](int v) {
    char d[12];
    int k = 0;
    unsigned u = v < 0 ? 0u : (unsigned)v;
    do { d[k++] = (char)('0' + u % 10); u /= 10; } while (u);
    while (k && n + 1 < sizeof(e)) e[n++] = d[--k];
  };
  put(name);
  if (nargs > 0) {
    const int v[3] = {a, b, c};
    put("<");
    for (int i = 0; i < nargs && i < 3; ++i) { if (i) put(","); num(v[i]); }
    put(">");
  }
  if (suffix) put(suffix);
  char *buf = h->linalg_kernels;
  const size_t len = (size_t)h->linalg_kernels_len, cap = sizeof(h->linalg_kernels);
  for (const char *p = buf, *end = buf + len; p < end;) {     // each entry once
    const char *q = static_cast<const char *>(std::memchr(p, ';', (size_t)(end - p)));
    if (!q) q = end;
    if ((size_t)(q - p) == n && std::memcmp(p, e, n) == 0) return;
    p = q + 1;
  }
  size_t at = len;
  if (len >= 3 && std::memcmp(buf + len - 3, "...", 3) == 0) return;   // ran full earlier: nothing after the mark
  if (len + 1 + n + 5 > cap) {   // full: the record ends in "..." (room for it is kept free by this very test)
    n = 0;
    put("...");
  }
  if (at) buf[at++] = ';';
  std::memcpy(buf + at, e, n);
  at += n;
  buf[at] = 0;
  h->linalg_kernels_len = (int)at;
}

int model_to_device(plda_handle *h) {
  const size_t Dout = h->Dout, Din = h->Din;
  PLDA_HIP(h, h->d_mean.reserve(Din * 8));
  PLDA_HIP(h, h->d_transform.reserve(Dout * Din * 8));
  PLDA_HIP(h, h->d_psi.reserve(Dout * 8));
  PLDA_HIP(h, h->d_offset.reserve(Dout * 8));
  PLDA_HIP(h, hipMemcpyAsync(h->d_mean.p, h->h_mean.data(), Din * 8, hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(h->d_transform.p, h->h_transform.data(), Dout * Din * 8, hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(h->d_psi.p, h->h_psi.data(), Dout * 8, hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(h->d_offset.p, h->h_offset.data(), Dout * 8, hipMemcpyHostToDevice, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  return PLDA_OK;
}

// the pinned ring + copy threads of the host-pointer entry points (hostio.hip), created on first use
static int host_pipe(plda_handle *h, HostPipe **out) {
  if (!h->hostpipe) {
    h->hostpipe = new HostPipe(default_host_threads());
  }
  PLDA_HIP(h, h->hostpipe->init());
  *out = h->hostpipe;
  return PLDA_OK;
}

// caller (pageable) memory -> a fresh device temporary; large arrays travel through the pinned ring
static int upload(plda_handle *h, Tmp &t, const void *src, size_t bytes) {
  PLDA_HIP(h, t.alloc(bytes));
  if (!bytes) return PLDA_OK;
  if (bytes >= ((size_t)4 << 20) && h->host_variant == 0) {
    HostPipe *hp = nullptr;
    PLDA_TRY(host_pipe(h, &hp));
    PLDA_HIP(h, hp->upload(h->stream, t.p, src, bytes));
    return PLDA_OK;
  }
  PLDA_HIP(h, hipMemcpyAsync(t.p, src, bytes, hipMemcpyHostToDevice, h->stream));
  return PLDA_OK;
}

// device -> caller (pageable) memory, contiguous; synchronises the stream
static int download(plda_handle *h, void *dst, const void *dsrc, size_t bytes) {
  if (bytes >= ((size_t)4 << 20) && h->host_variant == 0) {
    HostPipe *hp = nullptr;
    PLDA_TRY(host_pipe(h, &hp));
    advise_huge(dst, bytes);
    size_t i = 0;
    for (size_t off = 0; off < bytes; off += HostPipe::SLOT_BYTES, ++i) {
      const size_t n = std::min(HostPipe::SLOT_BYTES, bytes - off);
      const hipError_t e = hp->ship_slab(h->stream, i, static_cast<const char *>(dsrc) + off, n, static_cast<char *>(dst) + off, n, n, 1);
      if (e != hipSuccess) { (void)hp->finish(); return hip_fail(h, e, "ship_slab", __FILE__, __LINE__); }
    }
    PLDA_HIP(h, hp->finish());
    return PLDA_OK;
  }
  PLDA_HIP(h, hipMemcpyAsync(dst, dsrc, bytes, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  return PLDA_OK;
}

static int set_device(plda_handle *h) {
  g_call_stream = h->stream;
  PLDA_HIP(h, hipSetDevice(h->device));
  return PLDA_OK;
}

// Plda::SmoothWithinClassCovariance: psi /= wc, transform rows *= wc^-1/2
__global__ void smooth_kernel(double *__restrict__ T, double *__restrict__ psi, int Dout, int Din, double f) {
  const int o = blockIdx.x;
  const double wc = 1.0 + f * psi[o];
  const double sc = 1.0 / sqrt(wc);
  for (int d = threadIdx.x; d < Din; d += blockDim.x) T[(size_t)o * Din + d] *= sc;
  __syncthreads();
  if (threadIdx.x == 0) psi[o] = psi[o] / wc;
}

}  // namespace plda

using namespace plda;

// Nothing throws across the ABI: every entry point runs its body inside `guarded`, which turns a C++
// exception (std::bad_alloc / std::length_error from a host-side container, std::system_error from the
// mutex) into a status code + plda_last_error text.  (The reference lets Kaldi assertions abort the
// interpreter: pldamodule.cpp has no try/catch.)
namespace {
int fail_quiet(plda_handle *h, int code, const char *fn, const char *what) noexcept {
  try { return fail(h, code, "%s: %s", fn, what); } catch (...) { return code; }
}
// the stream a poison fill checks for a capture (common.hpp): this call's handle's, and nothing once the call returns
struct CallStream {
  hipStream_t prev;
  explicit CallStream(plda_handle *h) : prev(g_call_stream) { g_call_stream = h ? h->stream : nullptr; }
  ~CallStream() { g_call_stream = prev; }
};
template <typename F> int guarded(plda_handle *h, const char *fn, F &&body) noexcept {
  CallStream cs(h);
  try { return body(); }
  catch (const std::bad_alloc &) { return fail_quiet(h, PLDA_E_HIP, fn, "out of host memory"); }
  catch (const std::exception &e) { return fail_quiet(h, PLDA_E_HIP, fn, e.what()); }
  catch (...) { return fail_quiet(h, PLDA_E_HIP, fn, "unknown C++ exception"); }
}
// Every entry point that takes a handle runs through one of these two.  entry: NULL handle -> PLDA_E_INVAL, then the handle's
// lock (one handle = one GPU + one stream: calls on the same handle from several threads are serialised; taken inside guarded's
// try, so a std::system_error from the mutex becomes a status code), then body().  device_entry: the same, and set_device(h)
// before body() -- under the lock, because plda_set_stream on another thread may have changed h->stream since guarded read it.
template <typename F> int entry(plda_handle *h, const char *fn, F &&body) noexcept {
  return guarded(h, fn, [&]() -> int {
    if (!h) return PLDA_E_INVAL;
    std::lock_guard<std::recursive_mutex> lock(h->mu);
    const int rc = body();
    // the one place that says why a cosine handle has no model (every entry point that needs the model proper ends up here)
    if (rc == PLDA_E_NOT_FITTED && h->backend == PLDA_BACKEND_COSINE && h->err.find("(cosine back-end selected") == std::string::npos)
      h->err += " (cosine back-end selected: this entry point needs a PLDA model)";
    return rc;
  });
}
template <typename F> int device_entry(plda_handle *h, const char *fn, F &&body) noexcept {
  return entry(h, fn, [&]() -> int {
    PLDA_TRY(set_device(h));
    return body();
  });
}

// The device temporaries of one host-pointer call.  in(): a caller array uploaded into a fresh temporary (upload() above: the
// pinned ring from 4 MiB on); out(): a temporary for a caller output; finish(rc of the device call): every output copied
// back, whole, and one synchronisation.  An absent optional argument (NULL) gets no temporary and a NULL device pointer.
// The temporaries live until the object does, i.e. to the end of the call.
class Staged {
 public:
  explicit Staged(plda_handle *handle) : h(handle) {}
  int in(const void *src, size_t bytes, const void **d) {
    *d = nullptr;
    if (!src) return PLDA_OK;
    tmps.emplace_back();
    PLDA_TRY(upload(h, tmps.back(), src, bytes));
    *d = tmps.back().p;
    return PLDA_OK;
  }
  template <typename T> int in(const T *src, size_t count, const T **d) {
    const void *p = nullptr;
    const int rc = in(static_cast<const void *>(src), count * sizeof(T), &p);
    *d = static_cast<const T *>(p);
    return rc;
  }
  // ring: the output goes back through download() (the pinned ring from 4 MiB on), otherwise by a plain asynchronous copy
  template <typename T> int out(T *dst, size_t count, T **d, bool ring = false) {
    *d = nullptr;
    if (!dst) return PLDA_OK;
    tmps.emplace_back();
    PLDA_HIP(h, tmps.back().alloc(count * sizeof(T)));
    *d = tmps.back().template as<T>();
    outs.push_back(Out{dst, *d, count * sizeof(T), ring});
    return PLDA_OK;
  }
  // a failed device call: nothing is copied, h->err stays the callee's, and the stream is drained before the temporaries go
  int finish(int rc) {
    if (rc != PLDA_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
    bool drained = false;
    for (const Out &o : outs) {
      if (!o.bytes) continue;
      if (o.ring) PLDA_TRY(download(h, o.dst, o.src, o.bytes));
      else PLDA_HIP(h, hipMemcpyAsync(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost, h->stream));
      drained = o.ring;      // (download ends in a synchronisation of its own)
    }
    if (!drained) PLDA_HIP(h, hipStreamSynchronize(h->stream));
    return PLDA_OK;
  }

 private:
  struct Out { void *dst; const void *src; size_t bytes; bool ring; };
  plda_handle *h;
  std::deque<Tmp> tmps;      // (a deque: Tmp neither copies nor moves)
  std::vector<Out> outs;
};

// The host-list entry points (two lists of scores in caller memory): the argument check with the caller's message, both
// lists uploaded, then body(device targets, device non-targets).
template <typename F>
int with_host_lists(plda_handle *h, const char *fn, const float *pos, int64_t np, const float *neg, int64_t nn, bool outputs_ok,
                    const char *refusal, F &&body) noexcept {
  return entry(h, fn, [&]() -> int {
    if (!pos || !neg || !outputs_ok || np <= 0 || nn <= 0) return fail(h, PLDA_E_INVAL, "%s", refusal);
    PLDA_TRY(set_device(h));
    Staged st(h);
    const float *dpos, *dneg;
    PLDA_TRY(st.in(pos, (size_t)np, &dpos));
    PLDA_TRY(st.in(neg, (size_t)nn, &dneg));
    return body(dpos, dneg);
  });
}
// The device-list entry points (the two lists are on the device already): the same check and message, no upload, then body().
template <typename F>
int with_device_lists(plda_handle *h, const char *fn, const float *dpos, int64_t np, const float *dneg, int64_t nn, bool outputs_ok,
                      const char *refusal, F &&body) noexcept {
  return entry(h, fn, [&]() -> int {
    if (!dpos || !dneg || !outputs_ok || np <= 0 || nn <= 0) return fail(h, PLDA_E_INVAL, "%s", refusal);
    PLDA_TRY(set_device(h));
    return body();
  });
}
// the host-list forms: K target and K non-target arrays in caller memory, uploaded, then body(device pointer arrays)
template <typename F>
int with_host_fusion_lists(plda_handle *h, const char *fn, int32_t K, const float *const *pos, int64_t np, const float *const *neg,
                           int64_t nn, bool outputs_ok, F &&body) noexcept {
  return entry(h, fn, [&]() -> int {
    if (!outputs_ok) return fail(h, PLDA_E_INVAL, "%s: the output structure or the weight array is NULL", fn);
    PLDA_TRY(fusion_list_args_check(h, fn, K, pos, np, neg, nn));     // (fusion.hip: the one place that checks them)
    PLDA_TRY(set_device(h));
    Staged st(h);
    const float *pp[PLDA_FUSION_MAX_SYSTEMS], *pn[PLDA_FUSION_MAX_SYSTEMS];
    for (int k = 0; k < K; ++k) {
      PLDA_TRY(st.in(pos[k], (size_t)np, &pp[k]));
      PLDA_TRY(st.in(neg[k], (size_t)nn, &pn[k]));
    }
    return body(pp, pn);
  });
}
// the settings plda_create reads from the environment: whole numbers stored as they are ...
const struct { const char *name; int plda_handle::*member; } ENV_INT[] = {
    {"PLDA_PREP_VARIANT", &plda_handle::prep_variant},     {"PLDA_EM_VARIANT", &plda_handle::em_variant},
    {"PLDA_JACOBI_VARIANT", &plda_handle::jacobi_variant}, {"PLDA_GEMM64_VARIANT", &plda_handle::gemm64_variant},
    {"PLDA_EIG_VARIANT", &plda_handle::eig_variant},       {"PLDA_EIG_DEBUG", &plda_handle::eig_debug},
    {"PLDA_SORT_VARIANT", &plda_handle::sort_variant},     {"PLDA_ZNORM_VARIANT", &plda_handle::znorm_variant},
    {"PLDA_EER_VARIANT", &plda_handle::eer_variant},       {"PLDA_MINDCF_VARIANT", &plda_handle::mindcf_variant},
    {"PLDA_HOST_VARIANT", &plda_handle::host_variant},     {"PLDA_SWEEP_VARIANT", &plda_handle::sweep_variant},
    {"PLDA_ROCCH_VARIANT", &plda_handle::rocch_variant},
};
const struct { const char *name; int64_t plda_handle::*member; } ENV_INT64[] = {
    {"PLDA_EER_SLAB_ROWS", &plda_handle::eer_slab_rows},         {"PLDA_SNORM_SLAB_ROWS", &plda_handle::sn_slab_rows},
    {"PLDA_ADAPT_SLAB_ROWS", &plda_handle::ad_slab_rows},        {"PLDA_AHC_SCRATCH_BYTES", &plda_handle::ahc_scratch_bytes},
    {"PLDA_VBX_SCRATCH_BYTES", &plda_handle::vbx_scratch_bytes}, {"PLDA_DER_SCRATCH_BYTES", &plda_handle::der_scratch_bytes},
    {"PLDA_ROCCH_EDGE_CAP", &plda_handle::rocch_edge_cap},       {"PLDA_PARTITION_SLICE_ROWS", &plda_handle::partition_slice_rows},
    {"PLDA_AHC_WIDE_BATCH", &plda_handle::ahc_wide_batch},       {"PLDA_AHC_WIDE_PIECES", &plda_handle::ahc_wide_pieces},
};

// ... and the ones that are checked: a refused value fails plda_create (the text goes to plda_last_error(NULL))
int read_environment(plda_handle *h) {
  {   // tests only (common.hpp): process-wide, taken from the environment of the latest plda_create
    const char *v = std::getenv("PLDA_SCRATCH_POISON");
    g_scratch_poison.store(v && std::atoi(v) == 1 ? 1 : 0);
  }
  for (const auto &e : ENV_INT)
    if (const char *v = std::getenv(e.name)) h->*e.member = std::atoi(v);
  for (const auto &e : ENV_INT64)
    if (const char *v = std::getenv(e.name)) h->*e.member = std::atoll(v);
  if (const char *v = std::getenv("PLDA_HIP_TRACE")) h->trace_on = h->trace_print = std::atoi(v) != 0;
  if (const char *v = std::getenv("PLDA_GEMM_VARIANT")) {
    // one row of score.hip's table, or nothing: the numbers of A/B arms that are gone, and numbers nobody assigned, fail here
    // instead of timing the product kernel under another arm's name
    char *end = nullptr;
    const long n = std::strtol(v, &end, 10);
    const GemmArm *arm = *end == 0 && n == (int)n ? gemm_arm_lookup((int)n) : nullptr;      // (empty: arm 0)
    if (!arm) return fail(nullptr, PLDA_E_INVAL, "plda_create: PLDA_GEMM_VARIANT=%s: no such arm exists (profiles/SWITCHES.md lists them)", v);
    if (arm->diag && !PLDA_DIAG)   // measurement arms (garbage scores or clock stamps): not in this build
      return fail(nullptr, PLDA_E_INVAL, "plda_create: PLDA_GEMM_VARIANT=%d is a measurement arm of the diagnostic build (PLDA_DIAG=1, "
                                         "libplda_hip_diag.so); this library does not contain it", arm->variant);
    h->gemm_arm = *arm;
  }
  if (const char *v = std::getenv("PLDA_MIXED_VARIANT")) {
    if (*v && std::strcmp(v, "0") != 0 && std::strcmp(v, "1") != 0)
      return fail(nullptr, PLDA_E_INVAL, "plda_create: PLDA_MIXED_VARIANT=%s (0: mixed enrol counts bucketed by distinct count, 1: always "
                                         "the depth-2D form; no other arm exists)", v);
    h->mixed_variant = std::atoi(v);
  }
  if (const char *v = std::getenv("PLDA_SCORE_DTYPE")) {
    if (std::strcmp(v, "bf16x3") == 0) h->score_dtype = 1;
    else if (std::strcmp(v, "f32") != 0 && *v) return fail(nullptr, PLDA_E_INVAL, "plda_create: PLDA_SCORE_DTYPE=%s (f32 or bf16x3)", v);
  }
  if (const char *v = std::getenv("PLDA_TRANSFORM_VARIANT")) {
    // 0 or 1 only: the other numbers named A/B and timing arms that are gone -- a script that still sets one fails here
    // instead of timing the product kernel under the old arm's name
    if (*v && std::strcmp(v, "0") != 0 && std::strcmp(v, "1") != 0)
      return fail(nullptr, PLDA_E_INVAL, "plda_create: PLDA_TRANSFORM_VARIANT=%s (0: the one-pass kernel, 1: GEMM + length-norm "
                                         "pass; no other arm exists)", v);
    h->transform_variant = std::atoi(v);
  }
  if (const char *v = std::getenv("PLDA_EMBED_VARIANT")) {
    if (*v && std::strcmp(v, "0") != 0 && std::strcmp(v, "1") != 0)
      return fail(nullptr, PLDA_E_INVAL, "plda_create: PLDA_EMBED_VARIANT=%s (0: by shape, 1: row pass + GEMM + row pass always)", v);
    h->embed_variant = std::atoi(v);
  }
  if (const char *v = std::getenv("PLDA_EMBED_CUS")) {
    // tests only: the CU count the fused kernel's main / tail split is sized for; a whole number 1 ... 4096 (empty or 0: the device's)
    char *end = nullptr;
    const long n = std::strtol(v, &end, 10);
    if (*v && (*end != 0 || n < 0 || n > 4096))
      return fail(nullptr, PLDA_E_INVAL, "plda_create: PLDA_EMBED_CUS=%s (a whole number 1 ... 4096; 0 or empty: the device's count)", v);
    h->embed_cus = (int)n;
  }
  return PLDA_OK;
}

}  // namespace

// The argument record and the staging of the AHC host forms (plda_*ahc*), and the block range every *_matrix host form stages.
namespace {
// minc: the batched classes' min_clusters per recording; minc_wide: the wide class's one (each form passes the other as NULL / 1)
AhcArgs ahc_args(int32_t has_threshold, double threshold, const int32_t *minc, int32_t minc_wide, int32_t *labels, int32_t *n_clusters,
                 int32_t *merge_a, int32_t *merge_b, double *merge_cost) {
  AhcArgs a;
  a.has_thr = has_threshold; a.thr = threshold; a.minc = minc; a.minc_wide = minc_wide;
  a.labels = labels; a.n_clusters = n_clusters; a.merge_a = merge_a; a.merge_b = merge_b; a.merge_cost = merge_cost;
  return a;
}
// the device outputs of a host form: labels_len labels, merges_len entries of the merge record (nullable as a group) and one
// cluster count per recording, i.e. labels_len - merges_len of them (T, T - R, R; the wide class: N, N - 1, 1)
int ahc_stage_outputs(Staged &st, const AhcArgs &host, size_t labels_len, size_t merges_len, AhcArgs *dev) {
  *dev = host;
  PLDA_TRY(st.out(host.labels, labels_len, &dev->labels));
  PLDA_TRY(st.out(host.n_clusters, labels_len - merges_len, &dev->n_clusters));
  PLDA_TRY(st.out(host.merge_a, merges_len, &dev->merge_a));
  PLDA_TRY(st.out(host.merge_b, merges_len, &dev->merge_b));
  PLDA_TRY(st.out(host.merge_cost, merges_len, &dev->merge_cost));
  return PLDA_OK;
}
// the blocks' offsets relative to the first one: a host form stages the floats [block_off[0], block_off[R]) of the caller's
// array, rel[R] of them, and the device form addresses that copy
std::vector<int64_t> block_rel(const int64_t *block_off, int64_t R) {
  std::vector<int64_t> rel((size_t)R + 1);
  for (int64_t r = 0; r <= R; ++r) rel[(size_t)r] = block_off[r] - block_off[0];
  return rel;
}
}  // namespace

extern "C" {

int plda_abi_version(void) { return 2; }
int plda_build_flags(void) { return PLDA_DIAG ? 1 : 0; }
int64_t plda_device_bytes_held(void) { return g_device_bytes.load(std::memory_order_relaxed); }
int64_t plda_device_bytes_peak(int32_t reset) {
  const int64_t peak = g_device_bytes_peak.load(std::memory_order_relaxed);
  if (reset) g_device_bytes_peak.store(g_device_bytes.load(std::memory_order_relaxed), std::memory_order_relaxed);
  return peak;
}

int plda_create(int device, plda_handle **out) {
  return guarded(nullptr, "plda_create", [&]() -> int {
    if (!out) return fail(nullptr, PLDA_E_INVAL, "plda_create: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
      return fail(nullptr, PLDA_E_HIP, "plda_create: no HIP device available (%s); this engine has no CPU fallback",
                  e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= count) return fail(nullptr, PLDA_E_INVAL, "plda_create: device %d out of range [0,%d)", device, count);
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(nullptr, PLDA_E_HIP, "plda_create: hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      return fail(nullptr, PLDA_E_HIP, "plda_create: device %d is %s; libplda_hip is built for gfx950 only", device, prop.gcnArchName);
    plda_handle *h = new (std::nothrow) plda_handle();
    if (!h) return fail(nullptr, PLDA_E_HIP, "plda_create: out of host memory");
    h->device = device;
    e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
      int n = 0;
      if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) h->num_cus = n;
    }
    h->stream = h->own_stream;
    const int rc = e == hipSuccess ? read_environment(h) : fail(nullptr, PLDA_E_HIP, "plda_create: %s", hipGetErrorString(e));
    if (rc != PLDA_OK) {   // the one failure exit once the handle exists: the stream this call created goes with it
      if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
      delete h;
      return rc;
    }
    *out = h;
    return PLDA_OK;
  });
}

static int trace_summary(plda_handle *h, std::string &out, bool reset);

int plda_destroy(plda_handle *h) {
  return guarded(h, "plda_destroy", [&]() -> int {
    if (!h) return PLDA_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->trace_print && h->trace_used) {   // PLDA_HIP_TRACE=1: the summary goes to stderr when the handle dies
      std::string js;
      if (trace_summary(h, js, true) == PLDA_OK) std::fprintf(stderr, "[plda_hip trace] %s\n", js.c_str());
    }
    for (auto &sp : h->trace_spans) { (void)hipEventDestroy(sp.e0); (void)hipEventDestroy(sp.e1); }
    (void)comm_destroy(h);         // first: peers map comm_mm / comm_mc, which are freed with the handle below
    delete h->hostpipe;
    h->hostpipe = nullptr;
    if (h->cs_pin) (void)hipHostFree(h->cs_pin);
    if (h->one_host) (void)hipHostFree(h->one_host);
    if (h->pin_model) (void)hipHostFree(h->pin_model);
    for (hipEvent_t e : h->fit_ev) if (e) (void)hipEventDestroy(e);
    if (h->jac_exec) (void)hipGraphExecDestroy(h->jac_exec);
    for (auto &ev : h->prof_events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;                      // every DevBuf member frees its memory in its destructor
    return PLDA_OK;
  });
}

const char *plda_last_error(const plda_handle *h) {
  // a per-thread copy taken under the handle's lock: another thread failing at the same moment
  // reassigns h->err, so the handle's own buffer must not be handed out
  static thread_local std::string tl_err;
  try {
    if (!h) return g_create_err.c_str();
    plda_handle *hm = const_cast<plda_handle *>(h);
    std::lock_guard<std::recursive_mutex> g(hm->mu);
    tl_err = h->err;
    return tl_err.c_str();
  } catch (...) { return "plda_last_error: out of host memory"; }
}

int plda_set_stream(plda_handle *h, void *hip_stream) {
  return entry(h, "plda_set_stream", [&]() -> int {
    h->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return PLDA_OK;
  });
}

int plda_reset_stream(plda_handle *h) {
  return entry(h, "plda_reset_stream", [&]() -> int {
    h->stream = h->own_stream;
    return PLDA_OK;
  });
}

int plda_synchronize(plda_handle *h) {
  return device_entry(h, "plda_synchronize", [&]() -> int {
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    return comm_check(h);      // a peer-provider wait that gave up is reported where the caller synchronises
  });
}

// ---------------------------------------------------------------- fit
int plda_fit_dev(plda_handle *h, const double *dX, int64_t N, int32_t D, const uint64_t *dlabels, int64_t K,
                 int32_t iters) {
  return device_entry(h, "plda_fit_dev", [&] { return fit_device(h, dX, N, D, dlabels, K, iters); });
}

int plda_fit(plda_handle *h, const double *X, int64_t N, int32_t D, const uint64_t *labels, int32_t iters) {
  return entry(h, "plda_fit", [&]() -> int {
    if (!X || !labels || N <= 0 || D <= 0) return fail(h, PLDA_E_INVAL, "fit: bad argument");
    PLDA_TRY(set_device(h));
    uint64_t mx = 0;
    for (int64_t r = 0; r < N; ++r) mx = std::max(mx, labels[r]);
    if (mx >= (uint64_t)N) return fail(h, PLDA_E_LABELS, "fit: labels must be dense 0..K-1");
    const int64_t K = (int64_t)mx + 1;
    Staged st(h);
    const double *dX;
    const uint64_t *dL;
    PLDA_TRY(st.in(X, (size_t)N * D, &dX));
    PLDA_TRY(st.in(labels, (size_t)N, &dL));
    return fit_device(h, dX, N, D, dL, K, iters);
  });
}

int plda_fit_stats_dev(plda_handle *h, const double *dX, int64_t N, int32_t D, const uint64_t *dlabels, int64_t K) {
  return device_entry(h, "plda_fit_stats_dev", [&] { return fit_stats_device(h, dX, N, D, dlabels, K); });
}

int plda_fit_get_stats_dev(plda_handle *h, double *dmeans, int64_t *dcounts, double *dscatter) {
  return entry(h, "plda_fit_get_stats_dev", [&]() -> int {
    if (h->fit_K <= 0) return fail(h, PLDA_E_NOT_FITTED, "fit_get_stats_dev: no statistics pass has run on this handle");
    PLDA_TRY(set_device(h));
    const size_t K = (size_t)h->fit_K, D = (size_t)h->fit_D;
    if (dmeans) PLDA_HIP(h, hipMemcpyAsync(dmeans, h->f_means.p, K * D * 8, hipMemcpyDeviceToDevice, h->stream));
    if (dcounts) PLDA_HIP(h, hipMemcpyAsync(dcounts, h->f_counts.p, K * 8, hipMemcpyDeviceToDevice, h->stream));
    if (dscatter) PLDA_HIP(h, hipMemcpyAsync(dscatter, h->f_scatter.p, D * D * 8, hipMemcpyDeviceToDevice, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    return PLDA_OK;
  });
}

int plda_fit_em_dev(plda_handle *h, const double *dmeans, const int64_t *dcounts, int64_t K, const double *dscatter,
                    int32_t D, int32_t iters) {
  return entry(h, "plda_fit_em_dev", [&]() -> int {
    if (!dmeans || !dcounts || !dscatter || K <= 0 || D <= 0) return fail(h, PLDA_E_INVAL, "fit_em: bad argument");
    if (D > 2048) return fail(h, PLDA_E_INVAL, "fit: featdim %d > 2048 unsupported", D);
    PLDA_TRY(set_device(h));
    PLDA_HIP(h, h->f_means.reserve((size_t)K * D * 8));
    PLDA_HIP(h, h->f_counts.reserve((size_t)K * 8));
    PLDA_HIP(h, h->f_scatter.reserve((size_t)D * D * 8));
    if (dmeans != h->f_means.p)
      PLDA_HIP(h, hipMemcpyAsync(h->f_means.p, dmeans, (size_t)K * D * 8, hipMemcpyDeviceToDevice, h->stream));
    if ((const void *)dcounts != h->f_counts.p)
      PLDA_HIP(h, hipMemcpyAsync(h->f_counts.p, dcounts, (size_t)K * 8, hipMemcpyDeviceToDevice, h->stream));
    if (dscatter != h->f_scatter.p)
      PLDA_HIP(h, hipMemcpyAsync(h->f_scatter.p, dscatter, (size_t)D * D * 8, hipMemcpyDeviceToDevice, h->stream));
    h->fit_ms[0] = 0.0;
    return fit_em_device(h, K, D, iters);
  });
}

int plda_fit_timings(plda_handle *h, double out_ms[4]) {
  return entry(h, "plda_fit_timings", [&]() -> int {
    if (!out_ms) return PLDA_E_INVAL;
    for (int i = 0; i < 4; ++i) out_ms[i] = h->fit_ms[i];
    return PLDA_OK;
  });
}

int plda_fit_plan(plda_handle *h, int32_t out[2]) {
  return entry(h, "plda_fit_plan", [&]() -> int {
    if (!out) return PLDA_E_INVAL;
    out[0] = h->em_groups;
    out[1] = h->em_form;
    return PLDA_OK;
  });
}

int plda_fit_num_classes(plda_handle *h, int64_t *K) {
  return entry(h, "plda_fit_num_classes", [&]() -> int {
    if (!K) return PLDA_E_INVAL;
    *K = h->fit_K;
    return PLDA_OK;
  });
}

int plda_fit_get_stats(plda_handle *h, double *means, int64_t *counts, double *scatter, double *sum,
                       double *W, double *B) {
  return entry(h, "plda_fit_get_stats", [&]() -> int {
    if (h->fit_K <= 0) return fail(h, PLDA_E_NOT_FITTED, "fit_get_stats: no fit has run on this handle");
    PLDA_TRY(set_device(h));
    const size_t K = (size_t)h->fit_K, D = (size_t)h->fit_D;
    if (means) PLDA_HIP(h, hipMemcpyAsync(means, h->f_means.p, K * D * 8, hipMemcpyDeviceToHost, h->stream));
    if (counts) PLDA_HIP(h, hipMemcpyAsync(counts, h->f_counts.p, K * 8, hipMemcpyDeviceToHost, h->stream));
    if (scatter) PLDA_HIP(h, hipMemcpyAsync(scatter, h->f_scatter.p, D * D * 8, hipMemcpyDeviceToHost, h->stream));
    if (sum) PLDA_HIP(h, hipMemcpyAsync(sum, h->f_sum.p, D * 8, hipMemcpyDeviceToHost, h->stream));
    if (W) PLDA_HIP(h, hipMemcpyAsync(W, h->f_W.p, D * D * 8, hipMemcpyDeviceToHost, h->stream));
    if (B) PLDA_HIP(h, hipMemcpyAsync(B, h->f_B.p, D * D * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    return PLDA_OK;
  });
}

// ---------------------------------------------------------------- model
int plda_get_dims(plda_handle *h, int32_t *Dout, int32_t *Din) {
  return entry(h, "plda_get_dims", [&]() -> int {
    if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "model not fitted");
    if (Dout) *Dout = h->Dout;
    if (Din) *Din = h->Din;
    return PLDA_OK;
  });
}

// ---------------------------------------------------------------- back-end (cosine.hip)
int plda_backend_set(plda_handle *h, int32_t kind, int32_t D) {
  return entry(h, "plda_backend_set", [&]() -> int {
    if (kind != PLDA_BACKEND_PLDA && kind != PLDA_BACKEND_COSINE) return fail(h, PLDA_E_INVAL, "backend_set: kind = %d (must be 0: PLDA, or 1: cosine)", kind);
    if (kind == PLDA_BACKEND_PLDA && D != 0) return fail(h, PLDA_E_INVAL, "backend_set: D = %d with the PLDA back-end (must be 0: the model brings its dimensions)", D);
    if (kind == PLDA_BACKEND_COSINE && (D < 1 || D > 2048)) return fail(h, PLDA_E_INVAL, "backend_set: D = %d (must be in 1 ... 2048)", D);
    if (kind == PLDA_BACKEND_COSINE && h->fitted)
      return fail(h, PLDA_E_INVAL, "backend_set: the handle holds a PLDA model; the cosine back-end takes a handle without one (create another handle)");
    if (kind == PLDA_BACKEND_PLDA && h->backend == PLDA_BACKEND_PLDA) return PLDA_OK;      // nothing to leave: the handle and its model stay as they are
    h->backend = kind;
    h->fitted = false;                 // (a cosine handle never had one; back to the EMPTY PLDA state)
    h->Dout = h->Din = kind == PLDA_BACKEND_COSINE ? D : 0;
    ++h->model_epoch;                  // whatever is keyed on the model -- the prepared test side among it -- is stale
    h->prep_valid = false;
    h->ucoef_ptr = nullptr; h->gcoef_ptr = nullptr;
    return PLDA_OK;
  });
}

int plda_backend_get(plda_handle *h, int32_t *kind, int32_t *D) {
  return entry(h, "plda_backend_get", [&]() -> int {
    if (kind) *kind = h->backend;
    if (D) *D = h->backend == PLDA_BACKEND_COSINE ? h->Dout : 0;
    return PLDA_OK;
  });
}

int plda_get_model(plda_handle *h, double *mean, double *transform, double *psi, double *offset) {
  return entry(h, "plda_get_model", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "model not fitted");
    if (mean) std::memcpy(mean, h->h_mean.data(), h->h_mean.size() * 8);
    if (transform) std::memcpy(transform, h->h_transform.data(), h->h_transform.size() * 8);
    if (psi) std::memcpy(psi, h->h_psi.data(), h->h_psi.size() * 8);
    if (offset) std::memcpy(offset, h->h_offset.data(), h->h_offset.size() * 8);
    return PLDA_OK;
  });
}

static int refresh_offset(plda_handle *h) {
  // offset = -transform . mean on the device (Plda::ComputeDerivedVars), mirrored back to the host
  PLDA_TRY(compute_offset_device(h));
  h->h_offset.resize(h->Dout);
  PLDA_HIP(h, hipMemcpyAsync(h->h_offset.data(), h->d_offset.p, (size_t)h->Dout * 8, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  return PLDA_OK;
}

int plda_set_model(plda_handle *h, int32_t Dout, int32_t Din, const double *mean, const double *transform,
                   const double *psi) {
  return entry(h, "plda_set_model", [&]() -> int {
    if (Dout <= 0 || Din <= 0 || Dout > Din || !mean || !transform || !psi)
      return fail(h, PLDA_E_INVAL, "set_model: bad argument");
    PLDA_TRY(refuse_on_cosine(h, "set_model"));
    PLDA_TRY(set_device(h));
    h->Dout = Dout; h->Din = Din;
    h->h_mean.assign(mean, mean + Din);
    h->h_transform.assign(transform, transform + (size_t)Dout * Din);
    h->h_psi.assign(psi, psi + Dout);
    h->h_offset.assign(Dout, 0.0);
    PLDA_TRY(model_to_device(h));
    h->fitted = true;
    ++h->model_epoch;
    return refresh_offset(h);
  });
}

int plda_truncate(plda_handle *h, int32_t targetdim) {
  return entry(h, "plda_truncate", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "model not fitted");
    if (targetdim <= 0 || targetdim > h->Dout) return fail(h, PLDA_E_INVAL, "truncate: targetdim %d not in [1,%d]", targetdim, h->Dout);
    PLDA_TRY(set_device(h));
    h->Dout = targetdim;
    h->h_transform.resize((size_t)targetdim * h->Din);
    h->h_psi.resize(targetdim);
    h->h_offset.resize(targetdim);
    ++h->model_epoch;
    return PLDA_OK;  // device arrays are row-major prefixes: nothing to move
  });
}

int plda_smooth(plda_handle *h, double factor) {
  return entry(h, "plda_smooth", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "model not fitted");
    if (!(factor >= 0.0 && factor <= 1.0)) return fail(h, PLDA_E_INVAL, "smooth: factor must be in [0,1]");
    PLDA_TRY(set_device(h));
    smooth_kernel<<<h->Dout, 256, 0, h->stream>>>(h->d_transform.as<double>(), h->d_psi.as<double>(), h->Dout, h->Din, factor);
    PLDA_LAUNCH_CHECK(h);
    PLDA_HIP(h, hipMemcpyAsync(h->h_transform.data(), h->d_transform.p, (size_t)h->Dout * h->Din * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipMemcpyAsync(h->h_psi.data(), h->d_psi.p, (size_t)h->Dout * 8, hipMemcpyDeviceToHost, h->stream));
    ++h->model_epoch;
    return refresh_offset(h);
  });
}

// ---------------------------------------------------------------- domain adaptation (adapt.hip)
int plda_adapt_reset(plda_handle *h) {
  return entry(h, "plda_adapt_reset", [&] { return adapt_reset(h); });
}

int plda_adapt_accumulate_dev(plda_handle *h, const double *dX, int64_t N, int32_t Din, const double *dweights) {
  return device_entry(h, "plda_adapt_accumulate_dev", [&] { return adapt_accumulate(h, dX, N, Din, dweights, false); });
}

int plda_adapt_accumulate(plda_handle *h, const double *X, int64_t N, int32_t Din, const double *weights) {
  return device_entry(h, "plda_adapt_accumulate", [&] { return adapt_accumulate(h, X, N, Din, weights, true); });
}

int plda_adapt_get_stats(plda_handle *h, double *tw, int64_t *rows, double *pilot, double *s1, double *s2) {
  return device_entry(h, "plda_adapt_get_stats", [&] { return adapt_get_stats(h, tw, rows, pilot, s1, s2); });
}

int plda_adapt_add_stats(plda_handle *h, double tw, int64_t rows, const double *pilot, const double *s1, const double *s2) {
  return device_entry(h, "plda_adapt_add_stats", [&] { return adapt_add_stats(h, tw, rows, pilot, s1, s2); });
}

int plda_adapt_update(plda_handle *h, double within_scale, double between_scale, double mean_diff_scale, double *eig,
                      plda_adapt_info *info) {
  return device_entry(h, "plda_adapt_update", [&] { return adapt_update(h, within_scale, between_scale, mean_diff_scale, eig, info); });
}

int plda_blend_model(plda_handle *h, int32_t D, const double *mean2, const double *transform2, const double *psi2, double alpha,
                     double alpha_mean) {
  return device_entry(h, "plda_blend_model", [&] { return blend_model(h, D, mean2, transform2, psi2, alpha, alpha_mean); });
}

// ---------------------------------------------------------------- transform
int plda_transform_rows_dev(plda_handle *h, const double *dXbar, int64_t R, int32_t Din, const int32_t *dn,
                            int32_t n_uniform, double *dout) {
  return entry(h, "plda_transform_rows_dev", [&]() -> int {
    if (!dn && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "transform_rows: need num_examples or n_uniform > 0");
    PLDA_TRY(set_device(h));
    return transform_rows_device(h, dXbar, R, Din, dn, n_uniform, dout);
  });
}

int plda_transform_rows(plda_handle *h, const double *Xbar, int64_t R, int32_t Din, const int32_t *num_examples,
                        int32_t n_uniform, double *out) {
  return entry(h, "plda_transform_rows", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "transform: model not fitted");
    if (R <= 0) return PLDA_OK;
    if (!Xbar || !out) return fail(h, PLDA_E_INVAL, "transform_rows: bad argument");
    if (!num_examples && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "transform_rows: need num_examples or n_uniform > 0");
    if (num_examples) {      // (Kaldi asserts num_examples > 0; here the counts are in host memory: look at them before anything is written)
      int64_t bad = 0, first = -1;
      for (int64_t r = 0; r < R; ++r)
        if (num_examples[r] <= 0 && bad++ == 0) first = r;
      if (bad) return fail(h, PLDA_E_INVAL, "transform_rows: %lld of %lld rows have num_examples <= 0 (the first is row %lld)", (long long)bad, (long long)R, (long long)first);
    }
    PLDA_TRY(set_device(h));
    Staged st(h);
    const double *dX;
    const int32_t *dN;
    double *dO;
    PLDA_TRY(st.in(Xbar, (size_t)R * Din, &dX));
    PLDA_TRY(st.in(num_examples, (size_t)R, &dN));
    PLDA_TRY(st.out(out, (size_t)R * h->Dout, &dO, true));
    return st.finish(transform_rows_device(h, dX, R, Din, dN, n_uniform, dO));
  });
}

int plda_transform_plan(plda_handle *h, int64_t R, int64_t out[8]) {
  return entry(h, "plda_transform_plan", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "transform: model not fitted");
    if (!out) return fail(h, PLDA_E_INVAL, "transform_plan: out is NULL");
    if (R < 0) return fail(h, PLDA_E_INVAL, "transform_plan: R = %lld (must be >= 0)", (long long)R);
    const TfPlan p = transform_plan(h, R);
    out[0] = p.arm; out[1] = p.cls; out[2] = p.main_rows; out[3] = p.main_block; out[4] = p.tail_rows; out[5] = p.tail_block;
    out[6] = h->num_cus; out[7] = 0;
    return PLDA_OK;
  });
}

// grouping, per-label means and TransformIvector on device-resident rows; results stay on the device
// (out arrays sized by the caller's capacity *Ku; PLDA_E_CAPACITY reports the needed size in *Ku)
static int transform_groups_device(plda_handle *h, const double *dX, int64_t N, int32_t Din, const uint64_t *dlabels,
                                   uint64_t *dout_labels, int32_t *dcounts32, double *dout_vecs, int64_t *Ku,
                                   Tmp &dM) {
  uint32_t *perm = nullptr;
  int *offsets = nullptr;
  uint64_t *uniq = nullptr;
  int64_t G = 0;
  // label compaction on the device (the reference does it with std::map, pldamodule.cpp:118,147-156)
  PLDA_TRY(group_by_label_device(h, dlabels, N, &perm, &offsets, &uniq, &G));
  if (G > *Ku) { *Ku = G; return fail(h, PLDA_E_CAPACITY, "transform_groups: %lld groups > capacity", (long long)G); }
  PLDA_HIP(h, dM.alloc((size_t)G * Din * 8));
  PLDA_TRY(group_centroids_device(h, dX, N, Din, perm, offsets, G, dM.as<double>(), dcounts32));
  PLDA_TRY(transform_rows_device(h, dM.as<double>(), G, Din, dcounts32, 0, dout_vecs));
  PLDA_HIP(h, hipMemcpyAsync(dout_labels, uniq, (size_t)G * 8, hipMemcpyDeviceToDevice, h->stream));
  *Ku = G;
  return PLDA_OK;
}

int plda_transform_groups_dev(plda_handle *h, const double *dX, int64_t N, int32_t Din, const uint64_t *dlabels,
                              uint64_t *dout_labels, int32_t *dout_counts, double *dout_vecs, int64_t *Ku) {
  return entry(h, "plda_transform_groups_dev", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "transform: model not fitted");
    if (!Ku) return fail(h, PLDA_E_INVAL, "transform_groups: Ku is NULL");
    if (N <= 0) { *Ku = 0; return PLDA_OK; }
    if (!dX || !dlabels || !dout_labels || !dout_counts || !dout_vecs) return fail(h, PLDA_E_INVAL, "transform_groups: bad argument");
    if (Din != h->Din) return fail(h, PLDA_E_INVAL, "transform: feature dim %d != model dim %d", Din, h->Din);
    PLDA_TRY(set_device(h));
    Tmp dM;
    PLDA_TRY(transform_groups_device(h, dX, N, Din, dlabels, dout_labels, dout_counts, dout_vecs, Ku, dM));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));   // dM is released on return
    return PLDA_OK;
  });
}

int plda_transform_groups(plda_handle *h, const double *X, int64_t N, int32_t Din, const uint64_t *labels,
                          uint64_t *out_labels, int64_t *out_counts, double *out_vecs, int64_t *Ku) {
  return entry(h, "plda_transform_groups", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "transform: model not fitted");
    if (!Ku) return fail(h, PLDA_E_INVAL, "transform_groups: Ku is NULL");
    if (N <= 0) { *Ku = 0; return PLDA_OK; }
    if (!X || !labels || !out_labels || !out_counts || !out_vecs) return fail(h, PLDA_E_INVAL, "transform_groups: bad argument");
    if (Din != h->Din) return fail(h, PLDA_E_INVAL, "transform: feature dim %d != model dim %d", Din, h->Din);
    PLDA_TRY(set_device(h));
    const int64_t cap = *Ku;
    if (cap <= 0) return fail(h, PLDA_E_CAPACITY, "transform_groups: capacity must be > 0");
    Staged st(h);
    const double *dX;
    const uint64_t *dL;
    Tmp dM, dC, dO, dU;
    PLDA_TRY(st.in(X, (size_t)N * Din, &dX));
    PLDA_TRY(st.in(labels, (size_t)N, &dL));
    const int64_t gmax = std::min(cap, N);
    PLDA_HIP(h, dC.alloc((size_t)gmax * 4));
    PLDA_HIP(h, dO.alloc((size_t)gmax * h->Dout * 8));
    PLDA_HIP(h, dU.alloc((size_t)gmax * 8));
    int64_t G = gmax;
    const int rc = transform_groups_device(h, dX, N, Din, dL, dU.as<uint64_t>(),
                                           dC.as<int32_t>(), dO.as<double>(), &G, dM);
    if (rc != PLDA_OK) { if (rc == PLDA_E_CAPACITY) *Ku = G; return rc; }
    std::vector<int32_t> c32((size_t)G);
    PLDA_HIP(h, hipMemcpyAsync(c32.data(), dC.p, (size_t)G * 4, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipMemcpyAsync(out_labels, dU.p, (size_t)G * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_TRY(download(h, out_vecs, dO.p, (size_t)G * h->Dout * 8));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    for (int64_t g = 0; g < G; ++g) out_counts[g] = c32[g];
    *Ku = G;
    return PLDA_OK;
  });
}

// ---------------------------------------------------------------- score
int plda_score_matrix_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                          const double *dV, int64_t Nt, const double *dzmean, const double *dzstd, float *dout,
                          int64_t ld_out) {
  return device_entry(h, "plda_score_matrix_dev", [&] {
    return score_matrix_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, dout, ld_out);
  });
}

int plda_score_prepare_dev(plda_handle *h, const double *dV, int64_t Nt, int32_t mixed_counts, int32_t n_uniform) {
  return device_entry(h, "plda_score_prepare_dev", [&] { return score_prepare_device(h, dV, Nt, mixed_counts != 0 ? 1 : 0, n_uniform, nullptr); });
}

int plda_score_prepare_counts_dev(plda_handle *h, const double *dV, int64_t Nt, const int32_t *counts, int32_t num_counts) {
  return device_entry(h, "plda_score_prepare_counts_dev", [&]() -> int {
    if (!counts || num_counts <= 0) return fail(h, PLDA_E_INVAL, "score_prepare_counts: empty count list");
    CountSet cs;
    score_count_set_host(counts, num_counts, &cs);     // (sorted, duplicates dropped; G = 0: outside what the bucketed form takes)
    if (cs.G == 0) return score_prepare_device(h, dV, Nt, 1, 0, nullptr);
    return score_prepare_device(h, dV, Nt, 2, 0, &cs);
  });
}

int plda_score_unprepare(plda_handle *h) {
  return entry(h, "plda_score_unprepare", [&]() -> int {
    h->prep_valid = false;
    return PLDA_OK;
  });
}

// the round-1/2 form of the host-pointer trials matrix: one slab buffer, the runtime's pageable copy, a
// synchronisation per slab.  Kept as the A/B arm (PLDA_HOST_VARIANT=1) and for test sets so wide that a
// single row of scores does not fit a slot of the pinned ring.
static int score_matrix_host_serial(plda_handle *h, const double *U, const int32_t *n_enrol, int32_t n_uniform, int64_t M,
                                    const double *V, int64_t Nt, const double *zmean, const double *zstd, float *out,
                                    int64_t ld_out) {
  const int D = h->Dout;
  Staged st(h);
  const double *dV;
  Tmp dU, dN, dZm, dZs, dO;
  CountSet cs;                                           // the distinct counts of ALL rows: every slab sees the same set
  if (n_enrol) score_count_set_host(n_enrol, M, &cs);
  PLDA_TRY(st.in(V, (size_t)Nt * D, &dV));
  // row slabs so that the device score block stays <= 1 GiB
  int64_t slab = std::max<int64_t>(128, ((1ll << 30) / 4 / Nt) / 128 * 128);
  slab = std::min(slab, round_up(M, 128));
  PLDA_HIP(h, dU.alloc((size_t)slab * D * 8));
  PLDA_HIP(h, dO.alloc((size_t)slab * Nt * 4));
  if (n_enrol) PLDA_HIP(h, dN.alloc((size_t)slab * 4));
  if (zmean && zstd) { PLDA_HIP(h, dZm.alloc((size_t)slab * 8)); PLDA_HIP(h, dZs.alloc((size_t)slab * 8)); }
  for (int64_t r0 = 0; r0 < M; r0 += slab) {
    const int64_t m = std::min(slab, M - r0);
    PLDA_HIP(h, hipMemcpyAsync(dU.p, U + r0 * D, (size_t)m * D * 8, hipMemcpyHostToDevice, h->stream));
    if (n_enrol) PLDA_HIP(h, hipMemcpyAsync(dN.p, n_enrol + r0, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
    if (zmean && zstd) {
      PLDA_HIP(h, hipMemcpyAsync(dZm.p, zmean + r0, (size_t)m * 8, hipMemcpyHostToDevice, h->stream));
      PLDA_HIP(h, hipMemcpyAsync(dZs.p, zstd + r0, (size_t)m * 8, hipMemcpyHostToDevice, h->stream));
    }
    PLDA_TRY(score_matrix_device(h, dU.as<double>(), n_enrol ? dN.as<int32_t>() : nullptr, n_uniform, m,
                                 dV, Nt, (zmean && zstd) ? dZm.as<double>() : nullptr,
                                 (zmean && zstd) ? dZs.as<double>() : nullptr, dO.as<float>(), Nt,
                                 /*reuse_packed_B=*/r0 > 0, n_enrol ? &cs : nullptr));   // the test side is packed once, not per slab
    if (ld_out == Nt)
      PLDA_HIP(h, hipMemcpyAsync(out + r0 * ld_out, dO.p, (size_t)m * Nt * 4, hipMemcpyDeviceToHost, h->stream));
    else
      PLDA_HIP(h, hipMemcpy2DAsync(out + r0 * ld_out, (size_t)ld_out * 4, dO.p, (size_t)Nt * 4, (size_t)Nt * 4,
                                   (size_t)m, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
  }
  return PLDA_OK;
}

// Host-pointer trials matrix.  What bounds it is PCIe, not the GEMM (1.4 TB/s of scores against <= 64 GB/s of
// link): slabs of <= 64 MiB of scores alternate between two device buffers; while the GEMM of slab i + 1 runs,
// slab i crosses the link into a pinned slot on the copy stream and slab i - 1 is copied from its slot into the
// caller's array by the host threads, which also take the page faults of a freshly allocated output in
// parallel (hostio.hip).  Enrol vectors, counts and z-norm maps are uploaded once, not per slab.
int plda_score_matrix(plda_handle *h, const double *U, const int32_t *n_enrol, int32_t n_uniform, int64_t M,
                      const double *V, int64_t Nt, const double *zmean, const double *zstd, float *out,
                      int64_t ld_out) {
  return entry(h, "plda_score_matrix", [&]() -> int {
    if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "score_matrix: model not fitted");
    if (M <= 0 || Nt <= 0) return PLDA_OK;
    if (!U || !V || !out || ld_out < Nt) return fail(h, PLDA_E_INVAL, "score_matrix: bad argument");
    if (!n_enrol && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "score_matrix: n_uniform must be > 0 when n_enrol is NULL");
    PLDA_TRY(set_device(h));
    const int D = h->Dout;
    const bool zn = zmean && zstd;
    h->last_M = M;
    const int64_t fit_rows = (int64_t)(HostPipe::SLOT_BYTES / 4) / Nt;      // rows of scores per pinned slot
    if (h->host_variant == 1 || fit_rows < 1 || (size_t)M * D * 8 > ((size_t)2 << 30)) {
      const int rc = score_matrix_host_serial(h, U, n_enrol, n_uniform, M, V, Nt, zmean, zstd, out, ld_out);
      h->last_M = M;
      return rc;
    }
    HostPipe *hp = nullptr;
    PLDA_TRY(host_pipe(h, &hp));
    const int64_t slab = fit_rows >= 256 ? fit_rows / 128 * 128 : fit_rows;
    Staged st(h);
    const double *dV, *dU, *dZm, *dZs;
    const int32_t *dN;
    CountSet cs;                                         // the distinct counts of ALL rows, from the host array: no device pass
    if (n_enrol) score_count_set_host(n_enrol, M, &cs);
    PLDA_TRY(st.in(V, (size_t)Nt * D, &dV));
    PLDA_TRY(st.in(U, (size_t)M * D, &dU));
    PLDA_TRY(st.in(n_enrol, (size_t)M, &dN));
    PLDA_TRY(st.in(zn ? zmean : nullptr, (size_t)M, &dZm));
    PLDA_TRY(st.in(zn ? zstd : nullptr, (size_t)M, &dZs));
    for (auto &b : h->hio_O) PLDA_HIP(h, b.reserve((size_t)std::min(slab, M) * Nt * 4));
    advise_huge(out, (size_t)((M - 1) * ld_out + Nt) * 4);
    size_t i = 0;
    int rc = PLDA_OK;
    for (int64_t r0 = 0; r0 < M && rc == PLDA_OK; r0 += slab, ++i) {
      const int64_t m = std::min(slab, M - r0);
      float *dO = h->hio_O[i & 1].as<float>();
      hipError_t e = hp->begin_slab(h->stream, i);
      if (e != hipSuccess) { rc = hip_fail(h, e, "begin_slab", __FILE__, __LINE__); break; }
      rc = score_matrix_device(h, dU + r0 * D, dN ? dN + r0 : nullptr, n_uniform, m, dV, Nt, zn ? dZm + r0 : nullptr,
                               zn ? dZs + r0 : nullptr, dO, Nt, /*reuse_packed_B=*/r0 > 0, n_enrol ? &cs : nullptr);
      if (rc != PLDA_OK) break;
      e = hp->ship_slab(h->stream, i, dO, (size_t)m * Nt * 4, reinterpret_cast<char *>(out + r0 * ld_out), (size_t)ld_out * 4,
                        (size_t)Nt * 4, (size_t)m);
      if (e != hipSuccess) rc = hip_fail(h, e, "ship_slab", __FILE__, __LINE__);
    }
    const hipError_t ef = hp->finish();                       // also on failure: nothing of this call stays in flight
    if (rc == PLDA_OK && ef != hipSuccess) rc = hip_fail(h, ef, "HostPipe::finish", __FILE__, __LINE__);
    PLDA_HIP(h, hipStreamSynchronize(h->stream));              // the temporaries go out of scope
    h->last_M = M;
    return rc;
  });
}

// spans aggregated by name, in order of first appearance: [{"name": .., "calls": n, "ms": total, "work": w, "unit": "flop"|"bytes"|""}, ..]
static int trace_summary(plda_handle *h, std::string &out, bool reset) {
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  struct Agg { const char *name; long calls; double ms, work; int unit; };
  std::vector<Agg> agg;
  for (size_t i = 0; i < h->trace_used; ++i) {
    auto &sp = h->trace_spans[i];
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, sp.e0, sp.e1) != hipSuccess) { (void)hipGetLastError(); continue; }
    Agg *a = nullptr;
    for (auto &x : agg)
      if (std::strcmp(x.name, sp.name) == 0) { a = &x; break; }
    if (!a) { agg.push_back(Agg{sp.name, 0, 0.0, 0.0, sp.unit}); a = &agg.back(); }
    a->calls++; a->ms += ms; a->work += sp.work;
  }
  out = "[";
  char buf[256];
  for (size_t i = 0; i < agg.size(); ++i) {
    std::snprintf(buf, sizeof buf, "%s{\"name\": \"%s\", \"calls\": %ld, \"ms\": %.6f, \"work\": %.6g, \"unit\": \"%s\"}", i ? ", " : "",
                  agg[i].name, agg[i].calls, agg[i].ms, agg[i].work, agg[i].unit == 1 ? "flop" : agg[i].unit == 2 ? "bytes" : "");
    out += buf;
  }
  out += "]";
  if (reset) h->trace_used = 0;
  return PLDA_OK;
}

int plda_trace_enable(plda_handle *h, int32_t on) {
  return entry(h, "plda_trace_enable", [&]() -> int {
    h->trace_on = on != 0;
    return PLDA_OK;
  });
}

int plda_trace_read(plda_handle *h, char *json, int64_t cap, int32_t reset) {
  return entry(h, "plda_trace_read", [&]() -> int {
    if (!json || cap <= 0) return fail(h, PLDA_E_INVAL, "trace_read: bad argument");
    PLDA_TRY(set_device(h));
    std::string js;
    PLDA_TRY(trace_summary(h, js, false));
    if ((int64_t)js.size() + 1 > cap) return fail(h, PLDA_E_CAPACITY, "trace_read: need %zu bytes", js.size() + 1);
    std::memcpy(json, js.c_str(), js.size() + 1);
    if (reset) h->trace_used = 0;
    return PLDA_OK;
  });
}

int plda_profile_enable(plda_handle *h, int32_t on) {
  return entry(h, "plda_profile_enable", [&]() -> int {
    h->prof_on = on != 0;
    return PLDA_OK;
  });
}

int plda_profile_read(plda_handle *h, double *gemm_ms, int64_t *launches, double *gemm_flop, int32_t reset) {
  return device_entry(h, "plda_profile_read", [&]() -> int {
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    double total = 0.0;
    for (size_t i = 0; i < h->prof_used; ++i) {
      float ms = 0.f;
      PLDA_HIP(h, hipEventElapsedTime(&ms, h->prof_events[i].first, h->prof_events[i].second));
      total += ms;
    }
    if (gemm_ms) *gemm_ms = total;
    if (launches) *launches = (int64_t)h->prof_used;
    if (gemm_flop) *gemm_flop = h->prof_flop;
    if (reset) { h->prof_used = 0; h->prof_flop = 0.0; }
    return PLDA_OK;
  });
}

int plda_profile_timeline(plda_handle *h, uint64_t *out, int64_t cap_words) {
  return entry(h, "plda_profile_timeline", [&]() -> int {
    if (!out || cap_words < (int64_t)TIMELINE_WORDS) return fail(h, PLDA_E_CAPACITY, "profile_timeline: need %zu words", TIMELINE_WORDS);
    if (!h->timeline_valid) return fail(h, PLDA_E_INVAL, "profile_timeline: no launch of a timeline arm (PLDA_GEMM_VARIANT, diagnostic build) has run on this handle");
    PLDA_TRY(set_device(h));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    PLDA_HIP(h, hipMemcpy(out, h->timeline.p, TIMELINE_WORDS * 8, hipMemcpyDeviceToHost));
    return PLDA_OK;
  });
}

int plda_gemm_f64(plda_handle *h, int64_t M, int64_t N, int64_t K, double alpha, const double *A, int32_t transA,
                  const double *B, int32_t transB, const double *kw, double beta, double *C, int32_t batch) {
  return entry(h, "plda_gemm_f64", [&]() -> int {
    note_kernels_clear(h);
    if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || batch <= 0 || (kw && batch != 1))
      return fail(h, PLDA_E_INVAL, "gemm_f64: bad argument");
    PLDA_TRY(set_device(h));
    const size_t nA = (size_t)M * K, nB = (size_t)K * N, nC = (size_t)M * N;
    Tmp dA, dB, dC, dW;
    // the same host array on both sides (X^T diag(w) X: the scatter's product) stays ONE device array, so that the
    // dispatch sees what fit's statistics pass hands it and takes the symmetric kernels
    const bool same = A == B && nA == nB && batch == 1;
    PLDA_HIP(h, dA.alloc(nA * batch * 8));
    if (!same) PLDA_HIP(h, dB.alloc(nB * batch * 8));
    PLDA_HIP(h, dC.alloc(nC * batch * 8));
    PLDA_HIP(h, hipMemcpyAsync(dA.p, A, nA * batch * 8, hipMemcpyHostToDevice, h->stream));
    if (!same) PLDA_HIP(h, hipMemcpyAsync(dB.p, B, nB * batch * 8, hipMemcpyHostToDevice, h->stream));
    PLDA_HIP(h, hipMemcpyAsync(dC.p, C, nC * batch * 8, hipMemcpyHostToDevice, h->stream));
    if (kw) {
      PLDA_HIP(h, dW.alloc((size_t)K * 8));
      PLDA_HIP(h, hipMemcpyAsync(dW.p, kw, (size_t)K * 8, hipMemcpyHostToDevice, h->stream));
    }
    // element (m, k) of op(A): m * sam + k * sak; element (k, n) of op(B): k * sbk + n * sbn
    const int64_t sam = transA ? 1 : K, sak = transA ? M : 1, sbk = transB ? 1 : N, sbn = transB ? K : 1;
    PLDA_TRY(gemm_f64_batched(h, M, N, K, alpha, dA.as<double>(), sam, sak, (int64_t)nA, same ? dA.as<double>() : dB.as<double>(), sbk, sbn, (int64_t)nB,
                              kw ? dW.as<double>() : nullptr, beta, dC.as<double>(), N, (int64_t)nC, batch));
    PLDA_HIP(h, hipMemcpyAsync(C, dC.p, nC * batch * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    return PLDA_OK;
  });
}

int plda_spd_inverse(plda_handle *h, const double *A, int32_t D, double *inverse) {
  return entry(h, "plda_spd_inverse", [&]() -> int {
    note_kernels_clear(h);
    if (!A || !inverse || D <= 0 || D > 2048) return fail(h, PLDA_E_INVAL, "spd_inverse: bad argument");
    PLDA_TRY(set_device(h));
    const size_t DD = (size_t)D * D;
    Staged st(h);
    Tmp dA, dS, dF;
    double *dO;
    PLDA_HIP(h, dA.alloc(DD * 8));
    PLDA_TRY(st.out(inverse, DD, &dO));
    PLDA_HIP(h, dS.alloc(3 * DD * 8));
    PLDA_HIP(h, dF.alloc(sizeof(int)));
    PLDA_HIP(h, hipMemcpyAsync(dA.p, A, DD * 8, hipMemcpyHostToDevice, h->stream));
    PLDA_HIP(h, hipMemsetAsync(dF.p, 0, sizeof(int), h->stream));
    PLDA_TRY(spd_inverse_blocked(h, dA.as<double>(), D, D, (int64_t)DD, dO, D, (int64_t)DD, dS.as<double>(), (int64_t)(3 * DD),
                                 dF.as<int>(), 1));
    int bad = 0;
    PLDA_HIP(h, hipMemcpyAsync(&bad, dF.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PLDA_TRY(st.finish(PLDA_OK));
    if (bad) return fail(h, PLDA_E_NUMERIC, "spd_inverse: the matrix is not positive definite");
    return PLDA_OK;
  });
}

int plda_sym_eig(plda_handle *h, const double *G, int32_t D, int32_t method, double *eigenvalues, double *eigenvectors,
                 int32_t *method_used) {
  return entry(h, "plda_sym_eig", [&]() -> int {
    note_kernels_clear(h);
    if (!G || !eigenvalues || !eigenvectors || D <= 0 || D > 2048) return fail(h, PLDA_E_INVAL, "sym_eig: bad argument");
    if (method < 0 || method > 2) return fail(h, PLDA_E_INVAL, "sym_eig: method must be 0 (default), 1 (Jacobi) or 2 (direct)");
    if (method == 1 && D > 1024) return fail(h, PLDA_E_INVAL, "sym_eig: the block Jacobi solver (method 1) stops at D = 1024; D = %d needs method 0 or 2", D);
    PLDA_TRY(set_device(h));
    const size_t DD = (size_t)D * D;
    Staged st(h);
    Tmp dG;
    double *dS, *dV;
    PLDA_HIP(h, dG.alloc(DD * 8));
    PLDA_TRY(st.out(eigenvalues, (size_t)D, &dS));
    PLDA_TRY(st.out(eigenvectors, DD, &dV));
    PLDA_HIP(h, hipMemcpyAsync(dG.p, G, DD * 8, hipMemcpyHostToDevice, h->stream));
    const bool keep = h->eig_keep_sign;
    const int variant = h->eig_variant;
    h->eig_keep_sign = true;                       // signed eigenvalues: this entry point floors nothing
    int rc = PLDA_OK, status = 1;
    if (method == 2 || (method == 0 && variant != 1)) {
      rc = sym_eig_dc_f64(h, dG.as<double>(), D, dS, dV, &status);
      if (rc == PLDA_OK && status != 0 && method == 2) {
        h->eig_keep_sign = keep;
        return fail(h, PLDA_E_NUMERIC, "sym_eig: the direct method does not handle this input (status %d)", status);
      }
    }
    if (rc == PLDA_OK && status != 0) {
      rc = sym_eig_f64(h, dG.as<double>(), D, dS, dV, nullptr, nullptr);
      if (method_used) *method_used = 1;
    } else if (method_used) {
      *method_used = 2;
    }
    h->eig_keep_sign = keep;
    PLDA_TRY(rc);
    return st.finish(PLDA_OK);
  });
}

int plda_score_last_shape(plda_handle *h, int64_t *M, int64_t *Nt, int32_t *gemm_k) {
  return entry(h, "plda_score_last_shape", [&]() -> int {
    if (M) *M = h->last_M;
    if (Nt) *Nt = h->last_Nt;
    if (gemm_k) *gemm_k = h->last_k;
    return PLDA_OK;
  });
}

int plda_score_last_kernel(plda_handle *h, char *name, int64_t cap) {
  return entry(h, "plda_score_last_kernel", [&]() -> int {
    if (!name || cap <= 0) return PLDA_E_INVAL;
    const char *k = h->last_kernel ? h->last_kernel : "";
    if ((int64_t)std::strlen(k) + 1 > cap) return fail(h, PLDA_E_CAPACITY, "score_last_kernel: need %zu bytes", std::strlen(k) + 1);
    std::memcpy(name, k, std::strlen(k) + 1);
    return PLDA_OK;
  });
}

int plda_linalg_last_kernels(plda_handle *h, char *out, int64_t cap) {
  return entry(h, "plda_linalg_last_kernels", [&]() -> int {
    if (!out || cap <= 0) return PLDA_E_INVAL;
    const size_t need = (size_t)h->linalg_kernels_len + 1;
    if ((int64_t)need > cap) return fail(h, PLDA_E_CAPACITY, "linalg_last_kernels: need %zu bytes", need);
    std::memcpy(out, h->linalg_kernels, need);
    return PLDA_OK;
  });
}

int plda_score_pairs(plda_handle *h, const double *U, const int32_t *n_enrol, int64_t M, const double *V,
                     int64_t Nt, const int64_t *e_idx, const int64_t *t_idx, int64_t P, const double *zmean,
                     const double *zstd, double *out) {
  return entry(h, "plda_score_pairs", [&]() -> int {
    if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "score: model not fitted");
    if (P <= 0) return PLDA_OK;
    if (!U || !n_enrol || !V || !e_idx || !t_idx || !out || M <= 0 || Nt <= 0) return fail(h, PLDA_E_INVAL, "score_pairs: bad argument");
    const bool long_list = P >= 16384;      // (long lists: the indices are checked on the device, below -- 10^7 pairs are 10 ms of this loop)
    if (!long_list)
      for (int64_t p = 0; p < P; ++p)
        if (e_idx[p] < 0 || e_idx[p] >= M || t_idx[p] < 0 || t_idx[p] >= Nt)
          return fail(h, PLDA_E_INVAL, "score_pairs: trial %lld indexes outside the enrol/test sets", (long long)p);
    for (int64_t i = 0; i < M; ++i)
      if (n_enrol[i] <= 0) return fail(h, PLDA_E_INVAL, "score_pairs: num_examples must be > 0");
    PLDA_TRY(set_device(h));
    const int D = h->Dout;
    if (P == 1 && M == 1 && Nt == 1) {
      // One trial -- the reference's MPlda_score call (pldamodule.cpp:258-277).  No allocation and no copy
      // engine: the operands go into a host buffer that is mapped into the GPU's address space, the kernel
      // reads them and writes the score back through that mapping, and one stream synchronisation ends the call.
      const size_t need = ((size_t)2 * D + 8) * 8;
      if (h->one_cap < need) {
        if (h->one_host) (void)hipHostFree(h->one_host);
        h->one_host = nullptr; h->one_cap = 0;
        PLDA_HIP(h, hipHostMalloc(&h->one_host, need, hipHostMallocMapped));
        PLDA_HIP(h, hipHostGetDevicePointer(&h->one_dev, h->one_host, 0));
        h->one_cap = need;
      }
      double *hb = static_cast<double *>(h->one_host);
      double *db = static_cast<double *>(h->one_dev);
      // layout: u[D] v[D] zmean zstd out | e_idx t_idx (int64) | n (int32)
      std::memcpy(hb, U, (size_t)D * 8);
      std::memcpy(hb + D, V, (size_t)D * 8);
      const bool zn1 = zmean && zstd;
      hb[2 * D] = zn1 ? zmean[0] : 0.0;
      hb[2 * D + 1] = zn1 ? zstd[0] : 0.0;
      int64_t *hi = reinterpret_cast<int64_t *>(hb + 2 * D + 3);
      hi[0] = 0; hi[1] = 0;
      *reinterpret_cast<int32_t *>(hb + 2 * D + 5) = n_enrol[0];
      PLDA_TRY(score_pairs_device(h, db, reinterpret_cast<const int32_t *>(db + 2 * D + 5), db + D,
                                  reinterpret_cast<const int64_t *>(db + 2 * D + 3),
                                  reinterpret_cast<const int64_t *>(db + 2 * D + 4), 1, zn1 ? db + 2 * D : nullptr,
                                  zn1 ? db + 2 * D + 1 : nullptr, db + 2 * D + 2));
      PLDA_HIP(h, hipStreamSynchronize(h->stream));
      out[0] = hb[2 * D + 2];
      return PLDA_OK;
    }
    Staged st(h);
    const double *dU, *dV, *dZm, *dZs;
    const int32_t *dN;
    const int64_t *dE, *dT;
    double *dO;
    PLDA_TRY(st.in(U, (size_t)M * D, &dU));
    PLDA_TRY(st.in(n_enrol, (size_t)M, &dN));
    PLDA_TRY(st.in(V, (size_t)Nt * D, &dV));
    PLDA_TRY(st.in(e_idx, (size_t)P, &dE));
    PLDA_TRY(st.in(t_idx, (size_t)P, &dT));
    const bool zn = zmean && zstd;
    PLDA_TRY(st.in(zn ? zmean : nullptr, (size_t)M, &dZm));
    PLDA_TRY(st.in(zn ? zstd : nullptr, (size_t)M, &dZs));
    PLDA_TRY(st.out(out, (size_t)P, &dO, true));
    if (long_list) {
      long long bad = -1;
      PLDA_TRY(plda::pairs_validate_device(h, dE, dT, P, M, Nt, &bad));
      if (bad >= 0) return fail(h, PLDA_E_INVAL, "score_pairs: trial %lld indexes outside the enrol/test sets", bad);
    }
    plda::CountSet cs;                                   // the distinct enrol counts: long lists run on per-count tables (score.hip)
    if (P >= 16384) plda::score_count_set_host(n_enrol, M, &cs);
    return st.finish(score_pairs_device(h, dU, dN, dV, dE, dT, P, dZm, dZs, dO, M, &cs));
  });
}

// One trial on the HOST -- the reference's MPlda_score call (pldamodule.cpp:258-277: Plda::LogLikelihoodRatio at :266,
// z-norm at :269-273) for callers that score one pair per Python call (scoring/scorePLDA.py:302-318,
// tests/pldatest.py:29-33).  A single trial is 2 D numbers and ~5 D flop: any trip to the GPU (>= 30 us of launch and
// synchronisation latency) costs ten times what the arithmetic does, so this entry point evaluates
//   -1/2 [ sum_d log var_d - log(1 + psi_d) + (v_d - c_d u_d)^2 / var_d - v_d^2 / (1 + psi_d) ],
//   c_d = n psi_d / (n psi_d + 1),  var_d = 1 + psi_d / (n psi_d + 1)
// on the handle's host mirror of psi, with the per-count terms (c, 1/var, 1/(1 + psi), the log sum) cached for the last
// n.  fp64; own code of the library (the oracle is not involved); callers with more than a handful of trials belong
// on plda_score_pairs / plda_score_matrix.
int plda_score_one(plda_handle *h, const double *u, int32_t n, const double *v, int32_t has_z, double zmean, double zstd,
                   double *out) {
  return entry(h, "plda_score_one", [&]() -> int {
    if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "score: model not fitted");
    if (!u || !v || !out) return fail(h, PLDA_E_INVAL, "score_one: bad argument");
    if (n <= 0) return fail(h, PLDA_E_INVAL, "score_one: num_examples must be > 0");
    const int D = h->Dout;
    if (h->backend == PLDA_BACKEND_COSINE) { *out = cosine_one_host(u, v, D, has_z != 0, zmean, zstd); return PLDA_OK; }
    auto &o = h->one;
    if (o.epoch != h->model_epoch || o.n != n || o.D != D) {
      o.c.resize(D); o.ivar.resize(D); o.ipsi1.resize(D);
      double lt = 0.0;
      for (int d = 0; d < D; ++d) {
        const double ps = h->h_psi[d], den = (double)n * ps + 1.0;
        const double var = 1.0 + ps / den;
        o.c[d] = (double)n * ps / den;
        o.ivar[d] = 1.0 / var;
        o.ipsi1[d] = 1.0 / (1.0 + ps);
        lt += std::log(var) - std::log(1.0 + ps);
      }
      o.logterm = lt; o.epoch = h->model_epoch; o.n = n; o.D = D;
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;     // four partial sums: the loop vectorises
    const double *c = o.c.data(), *iv = o.ivar.data(), *ip = o.ipsi1.data();
    int d = 0;
    for (; d + 4 <= D; d += 4) {
      const double e0 = v[d] - c[d] * u[d], e1 = v[d + 1] - c[d + 1] * u[d + 1];
      const double e2 = v[d + 2] - c[d + 2] * u[d + 2], e3 = v[d + 3] - c[d + 3] * u[d + 3];
      a0 += e0 * e0 * iv[d] - v[d] * v[d] * ip[d];
      a1 += e1 * e1 * iv[d + 1] - v[d + 1] * v[d + 1] * ip[d + 1];
      a2 += e2 * e2 * iv[d + 2] - v[d + 2] * v[d + 2] * ip[d + 2];
      a3 += e3 * e3 * iv[d + 3] - v[d + 3] * v[d + 3] * ip[d + 3];
    }
    for (; d < D; ++d) { const double e = v[d] - c[d] * u[d]; a0 += e * e * iv[d] - v[d] * v[d] * ip[d]; }
    double sc = -0.5 * (o.logterm + ((a0 + a1) + (a2 + a3)));
    if (has_z && zstd != 0.0) sc = (sc - zmean) / zstd;   // zstd == 0: left un-normalised, as the trial-list kernel does
    *out = sc;
    return PLDA_OK;
  });
}

// ---------------------------------------------------------------- z-norm
int plda_znorm_stats_dev(plda_handle *h, const double *dbkg, int64_t Nb, int32_t num_examples, int32_t Din,
                         const double *dmodels, int64_t M, double *dout_mean, double *dout_std) {
  return device_entry(h, "plda_znorm_stats_dev", [&] { return znorm_stats_device(h, dbkg, Nb, num_examples, Din, dmodels, M, dout_mean, dout_std); });
}

int plda_znorm_stats(plda_handle *h, const double *bkg, int64_t Nb, int32_t num_examples, int32_t Din,
                     const double *models, int64_t M, double *out_mean, double *out_std) {
  return entry(h, "plda_znorm_stats", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "norm: model not fitted");
    if (!bkg || !models || !out_mean || !out_std || Nb <= 0 || M <= 0) return fail(h, PLDA_E_INVAL, "norm: bad argument");
    if (Din != h->Din) return fail(h, PLDA_E_INVAL, "norm: feature dim %d != model dim %d", Din, h->Din);
    PLDA_TRY(set_device(h));
    Staged st(h);
    const double *dB, *dM;
    double *dMean, *dStd;
    PLDA_TRY(st.in(bkg, (size_t)Nb * Din, &dB));
    PLDA_TRY(st.in(models, (size_t)M * h->Dout, &dM));
    PLDA_TRY(st.out(out_mean, (size_t)M, &dMean));
    PLDA_TRY(st.out(out_std, (size_t)M, &dStd));
    return st.finish(znorm_stats_device(h, dB, Nb, num_examples, Din, dM, M, dMean, dStd));
  });
}

// ---------------------------------------------------------------- AS-norm (snorm.hip)
int plda_cohort_stats_dev(plda_handle *h, const double *dX, const int32_t *dn, int32_t n_uniform, int64_t R, const double *dC,
                          int64_t Nc, int64_t top_k, double *dmean, double *dstd) {
  return device_entry(h, "plda_cohort_stats_dev", [&] { return cohort_stats_device(h, dX, dn, n_uniform, R, dC, Nc, top_k, dmean, dstd); });
}

int plda_cohort_stats(plda_handle *h, const double *X, const int32_t *n, int32_t n_uniform, int64_t R, const double *Cv,
                      int64_t Nc, int64_t top_k, double *mean, double *std_) {
  return entry(h, "plda_cohort_stats", [&]() -> int {
    if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "cohort_stats: model not fitted");
    if (R < 1 || Nc < 1) return fail(h, PLDA_E_INVAL, "cohort_stats: R = %lld, Nc = %lld (both must be >= 1)", (long long)R, (long long)Nc);
    if (top_k < 1 || top_k > Nc) return fail(h, PLDA_E_INVAL, "cohort_stats: top_k = %lld (must be in 1 ... Nc = %lld)", (long long)top_k, (long long)Nc);
    if (!X || !Cv || !mean || !std_) return fail(h, PLDA_E_INVAL, "cohort_stats: %s is NULL", !X ? "X" : !Cv ? "cohort" : !mean ? "mean" : "std");
    if (!n && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "cohort_stats: n_uniform must be > 0 when n is NULL");
    PLDA_TRY(set_device(h));
    const int D = h->Dout;
    Staged st(h);
    const double *dX, *dC;
    const int32_t *dN;
    double *dMean, *dStd;
    CountSet cs;                                         // from the host array: no device pass, no wait
    if (n) score_count_set_host(n, R, &cs);
    PLDA_TRY(st.in(Cv, (size_t)Nc * D, &dC));
    PLDA_TRY(st.in(X, (size_t)R * D, &dX));
    PLDA_TRY(st.in(n, (size_t)R, &dN));
    PLDA_TRY(st.out(mean, (size_t)R, &dMean));
    PLDA_TRY(st.out(std_, (size_t)R, &dStd));
    return st.finish(cohort_stats_device(h, dX, dN, n_uniform, R, dC, Nc, top_k, dMean, dStd, n ? &cs : nullptr));
  });
}

int plda_score_matrix_snorm_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                                const double *dV, int64_t Nt, const double *demean, const double *destd, const double *dtmean,
                                const double *dtstd, float *dout, int64_t ld_out) {
  return device_entry(h, "plda_score_matrix_snorm_dev", [&] {
    return score_matrix_snorm_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, demean, destd, dtmean, dtstd, dout, ld_out);
  });
}

// Host pointers: everything but the scores is uploaded once; the scores cross in row slabs of <= 1 GiB through one device buffer.
int plda_score_matrix_snorm(plda_handle *h, const double *U, const int32_t *n_enrol, int32_t n_uniform, int64_t M, const double *V,
                            int64_t Nt, const double *emean, const double *estd, const double *tmean, const double *tstd,
                            float *out, int64_t ld_out) {
  return entry(h, "plda_score_matrix_snorm", [&]() -> int {
    if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "score_matrix_snorm: model not fitted");
    if ((emean == nullptr) != (estd == nullptr)) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: %s is NULL but its partner is not", emean ? "estd" : "emean");
    if ((tmean == nullptr) != (tstd == nullptr)) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: %s is NULL but its partner is not", tmean ? "tstd" : "tmean");
    if (!emean && !tmean) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: both statistic pairs are NULL (emean/estd or tmean/tstd must be given)");
    if (M < 1 || Nt < 1) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: M = %lld, Nt = %lld (both must be >= 1)", (long long)M, (long long)Nt);
    if (!U || !V || !out) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: %s is NULL", !U ? "U" : !V ? "V" : "out");
    if (ld_out < Nt) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: ld_out = %lld < Nt = %lld", (long long)ld_out, (long long)Nt);
    if (!n_enrol && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "score_matrix_snorm: n_uniform must be > 0 when n_enrol is NULL");
    PLDA_TRY(set_device(h));
    const int D = h->Dout;
    Staged st(h);
    const double *dV, *dU, *dEm, *dEs, *dTm, *dTs;
    const int32_t *dN;
    Tmp dO;
    CountSet cs;                                         // the distinct counts of ALL rows: every slab sees the same set
    if (n_enrol) score_count_set_host(n_enrol, M, &cs);
    PLDA_TRY(st.in(V, (size_t)Nt * D, &dV));
    PLDA_TRY(st.in(U, (size_t)M * D, &dU));
    PLDA_TRY(st.in(n_enrol, (size_t)M, &dN));
    PLDA_TRY(st.in(emean, (size_t)M, &dEm));
    PLDA_TRY(st.in(estd, (size_t)M, &dEs));
    PLDA_TRY(st.in(tmean, (size_t)Nt, &dTm));
    PLDA_TRY(st.in(tstd, (size_t)Nt, &dTs));
    const int64_t ld = round_up(Nt, 4);
    int64_t slab = std::max<int64_t>(1, std::min<int64_t>(M, ((int64_t)1 << 30) / 4 / ld));
    PLDA_HIP(h, dO.alloc((size_t)slab * ld * 4));
    int rc = PLDA_OK;
    for (int64_t r0 = 0; r0 < M && rc == PLDA_OK; r0 += slab) {
      const int64_t m = std::min(slab, M - r0);
      rc = score_matrix_snorm_device(h, dU + r0 * D, dN ? dN + r0 : nullptr, n_uniform, m, dV, Nt, dEm ? dEm + r0 : nullptr,
                                     dEs ? dEs + r0 : nullptr, dTm, dTs, dO.as<float>(), ld, n_enrol ? &cs : nullptr,
                                     /*reuse_packed_B=*/r0 > 0);
      if (rc != PLDA_OK) break;
      const hipError_t e = hipMemcpy2DAsync(out + r0 * ld_out, (size_t)ld_out * 4, dO.p, (size_t)ld * 4, (size_t)Nt * 4, (size_t)m,
                                            hipMemcpyDeviceToHost, h->stream);
      if (e != hipSuccess) rc = hip_fail(h, e, "hipMemcpy2DAsync", __FILE__, __LINE__);
      else if ((rc = (hipStreamSynchronize(h->stream) == hipSuccess) ? PLDA_OK : PLDA_E_HIP) != PLDA_OK) fail(h, rc, "score_matrix_snorm: stream synchronisation failed");
    }
    (void)hipStreamSynchronize(h->stream);                // the temporaries go out of scope
    h->last_M = M;
    return rc;
  });
}

// ---------------------------------------------------------------- top-N retrieval (topn.hip)
int plda_topn_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, int32_t axis, int64_t top_n,
                         float *dout_scores, int64_t *dout_index) {
  return device_entry(h, "plda_topn_matrix_dev", [&] { return topn_matrix_device(h, dscores, ld, M, Nt, axis, top_n, dout_scores, dout_index); });
}

int plda_score_topn_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M, const double *dV,
                        int64_t Nt, const double *dzmean, const double *dzstd, const double *demean, const double *destd,
                        const double *dtmean, const double *dtstd, int32_t axis, int64_t top_n, float *dout_scores,
                        int64_t *dout_index) {
  return device_entry(h, "plda_score_topn_dev", [&] {
    return score_topn_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, demean, destd, dtmean, dtstd, axis, top_n,
                             dout_scores, dout_index);
  });
}

// Host pointers: the operands and statistics are uploaded once, the [L, top_n] results come back in two copies.
int plda_score_topn(plda_handle *h, const double *U, const int32_t *n_enrol, int32_t n_uniform, int64_t M, const double *V,
                    int64_t Nt, const double *zmean, const double *zstd, const double *emean, const double *estd,
                    const double *tmean, const double *tstd, int32_t axis, int64_t top_n, float *out_scores, int64_t *out_index) {
  return entry(h, "plda_score_topn", [&]() -> int {
    if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "score_topn: model not fitted");
    if (M < 1 || Nt < 1) return fail(h, PLDA_E_INVAL, "score_topn: M = %lld, Nt = %lld (both must be >= 1)", (long long)M, (long long)Nt);
    if (axis != 0 && axis != 1) return fail(h, PLDA_E_INVAL, "score_topn: axis = %d (must be 0: per row, or 1: per column)", axis);
    if (top_n < 1 || top_n > PLDA_TOPN_MAX) return fail(h, PLDA_E_INVAL, "score_topn: top_n = %lld (must be in 1 ... %d)", (long long)top_n, PLDA_TOPN_MAX);
    if (!U || !V || !out_scores || !out_index) return fail(h, PLDA_E_INVAL, "score_topn: %s is NULL", !U ? "U" : !V ? "V" : !out_scores ? "out_scores" : "out_index");
    if ((zmean == nullptr) != (zstd == nullptr)) return fail(h, PLDA_E_INVAL, "score_topn: %s is NULL but its partner is not", zmean ? "zstd" : "zmean");
    if ((emean == nullptr) != (estd == nullptr)) return fail(h, PLDA_E_INVAL, "score_topn: %s is NULL but its partner is not", emean ? "estd" : "emean");
    if ((tmean == nullptr) != (tstd == nullptr)) return fail(h, PLDA_E_INVAL, "score_topn: %s is NULL but its partner is not", tmean ? "tstd" : "tmean");
    if (!n_enrol && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "score_topn: n_uniform must be > 0 when n_enrol is NULL");
    PLDA_TRY(set_device(h));
    const int D = h->Dout;
    const int64_t L = axis == 0 ? M : Nt;
    Staged st(h);
    const double *dV, *dU, *dZm, *dZs, *dEm, *dEs, *dTm, *dTs;
    const int32_t *dN;
    float *dOs;
    int64_t *dOi;
    CountSet cs;                                         // from the host array: no device pass, no wait
    if (n_enrol) score_count_set_host(n_enrol, M, &cs);
    PLDA_TRY(st.in(V, (size_t)Nt * D, &dV));
    PLDA_TRY(st.in(U, (size_t)M * D, &dU));
    PLDA_TRY(st.in(n_enrol, (size_t)M, &dN));
    PLDA_TRY(st.in(zmean, (size_t)M, &dZm));
    PLDA_TRY(st.in(zstd, (size_t)M, &dZs));
    PLDA_TRY(st.in(emean, (size_t)M, &dEm));
    PLDA_TRY(st.in(estd, (size_t)M, &dEs));
    PLDA_TRY(st.in(tmean, (size_t)Nt, &dTm));
    PLDA_TRY(st.in(tstd, (size_t)Nt, &dTs));
    PLDA_TRY(st.out(out_scores, (size_t)L * top_n, &dOs));
    PLDA_TRY(st.out(out_index, (size_t)L * top_n, &dOi));
    return st.finish(score_topn_device(h, dU, dN, n_uniform, M, dV, Nt, dZm, dZs, dEm, dEs, dTm, dTs, axis, top_n, dOs, dOi,
                                       n_enrol ? &cs : nullptr));
  });
}

// ---------------------------------------------------------------- d-vector front-end
int plda_dvector_pool_dev(plda_handle *h, const void *dframes, int32_t dtype, int64_t T, int32_t D,
                          const int64_t *doffsets, int64_t U, int32_t method, int32_t l2norm, double *dout) {
  return device_entry(h, "plda_dvector_pool_dev", [&] { return dvector_pool_device(h, dframes, dtype, T, D, doffsets, U, method, l2norm, dout); });
}

int plda_dvector_pool(plda_handle *h, const void *frames, int32_t dtype, int64_t T, int32_t D, const int64_t *offsets,
                      int64_t U, int32_t method, int32_t l2norm, double *out) {
  return entry(h, "plda_dvector_pool", [&]() -> int {
    if (U <= 0) return PLDA_OK;
    if (!frames || !offsets || !out || T < 0 || D <= 0 || (dtype != 0 && dtype != 1))
      return fail(h, PLDA_E_INVAL, "dvector_pool: bad argument");
    for (int64_t u = 0; u < U; ++u)
      if (offsets[u] < 0 || offsets[u + 1] < offsets[u] || offsets[u + 1] > T)
        return fail(h, PLDA_E_INVAL, "dvector_pool: offsets must be non-decreasing within [0, T]");
    PLDA_TRY(set_device(h));
    Staged st(h);
    const void *dF;
    const int64_t *dO;
    double *dOut;
    PLDA_TRY(st.in(frames, (size_t)T * D * (dtype == 0 ? 4 : 8), &dF));
    PLDA_TRY(st.in(offsets, (size_t)(U + 1), &dO));
    PLDA_TRY(st.out(out, (size_t)U * D, &dOut));
    return st.finish(dvector_pool_device(h, dF, dtype, T, D, dO, U, method, l2norm, dOut));
  });
}

// ---------------------------------------------------------------- LDA (python/liblda/lda.py)
int plda_lda_fit_dev(plda_handle *h, const double *dX, int64_t N, int32_t D, const uint64_t *dlabels, int64_t K,
                     int32_t solver, const double *priors) {
  return device_entry(h, "plda_lda_fit_dev", [&] { return lda_fit_device(h, dX, N, D, dlabels, K, solver, priors); });
}

int plda_lda_fit(plda_handle *h, const double *X, int64_t N, int32_t D, const uint64_t *labels, int32_t solver,
                 const double *priors) {
  return entry(h, "plda_lda_fit", [&]() -> int {
    if (!X || !labels || N <= 0 || D <= 0) return fail(h, PLDA_E_INVAL, "lda_fit: bad argument");
    uint64_t mx = 0;
    for (int64_t r = 0; r < N; ++r) mx = std::max(mx, labels[r]);
    if (mx >= (uint64_t)N) return fail(h, PLDA_E_LABELS, "lda_fit: labels must be dense 0..K-1");
    PLDA_TRY(set_device(h));
    Staged st(h);
    const double *dX;
    const uint64_t *dL;
    PLDA_TRY(st.in(X, (size_t)N * D, &dX));
    PLDA_TRY(st.in(labels, (size_t)N, &dL));
    return lda_fit_device(h, dX, N, D, dL, (int64_t)mx + 1, solver, priors);
  });
}

int plda_lda_dims(plda_handle *h, int64_t *K, int32_t *D, int32_t *rank, int32_t *solver) {
  return entry(h, "plda_lda_dims", [&]() -> int {
    if (!h->lda_fitted) return fail(h, PLDA_E_NOT_FITTED, "This LDA instance is not fitted yet");
    if (K) *K = h->lda_K;
    if (D) *D = h->lda_D;
    if (rank) *rank = h->lda_rank;
    if (solver) *solver = h->lda_solver;
    return PLDA_OK;
  });
}

int plda_lda_get_model(plda_handle *h, double *priors, double *means, double *xbar, double *scalings, double *coef,
                       double *intercept, double *evr) {
  return entry(h, "plda_lda_get_model", [&]() -> int {
    if (!h->lda_fitted) return fail(h, PLDA_E_NOT_FITTED, "This LDA instance is not fitted yet");
    PLDA_TRY(set_device(h));
    const size_t K = (size_t)h->lda_K, D = (size_t)h->lda_D, R = (size_t)h->lda_rank;
    auto get = [&](double *dst, const DevBuf &src, size_t n) -> hipError_t {
      return (dst && n) ? hipMemcpyAsync(dst, src.p, n * 8, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
    };
    PLDA_HIP(h, get(priors, h->l_priors, K));
    PLDA_HIP(h, get(means, h->l_means, K * D));
    PLDA_HIP(h, get(coef, h->l_coef, K * D));
    PLDA_HIP(h, get(intercept, h->l_intercept, K));
    if (h->lda_solver == 0) PLDA_HIP(h, get(xbar, h->l_xbar, D));
    if (h->lda_solver != 2) PLDA_HIP(h, get(scalings, h->l_scalings, D * R));
    if (h->lda_solver == 1) PLDA_HIP(h, get(evr, h->l_evr, D));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    return PLDA_OK;
  });
}

int plda_lda_set_model(plda_handle *h, int32_t solver, int64_t K, int32_t D, int32_t rank, const double *priors,
                       const double *means, const double *xbar, const double *scalings, const double *coef,
                       const double *intercept) {
  return entry(h, "plda_lda_set_model", [&]() -> int {
    if (solver < 0 || solver > 2 || K <= 0 || D <= 0 || rank < 0 || rank > D || !coef || !intercept)
      return fail(h, PLDA_E_INVAL, "lda_set_model: bad argument");
    if (solver != 2 && (!scalings || rank == 0)) return fail(h, PLDA_E_INVAL, "lda_set_model: scalings required");
    if (solver == 0 && !xbar) return fail(h, PLDA_E_INVAL, "lda_set_model: xbar required for the svd solver");
    PLDA_TRY(set_device(h));
    auto put = [&](DevBuf &dst, const double *src, size_t n) -> hipError_t {
      hipError_t e = dst.reserve((n ? n : 1) * 8);
      if (e != hipSuccess || !src || !n) return e;
      return hipMemcpyAsync(dst.p, src, n * 8, hipMemcpyHostToDevice, h->stream);
    };
    const size_t k = (size_t)K, d = (size_t)D;
    PLDA_HIP(h, put(h->l_priors, priors, k));
    PLDA_HIP(h, put(h->l_means, means, k * d));
    PLDA_HIP(h, put(h->l_xbar, xbar, d));
    PLDA_HIP(h, put(h->l_scalings, scalings, d * (size_t)rank));
    PLDA_HIP(h, put(h->l_coef, coef, k * d));
    PLDA_HIP(h, put(h->l_intercept, intercept, k));
    PLDA_HIP(h, h->l_evr.reserve(d * 8));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    h->lda_fitted = true; h->lda_solver = solver; h->lda_K = K; h->lda_D = D; h->lda_rank = rank;
    return PLDA_OK;
  });
}

int plda_lda_predict_dev(plda_handle *h, const double *dX, int64_t N, int32_t mode, double *dout) {
  return device_entry(h, "plda_lda_predict_dev", [&] { return lda_predict_device(h, dX, N, mode, dout); });
}

int plda_lda_predict(plda_handle *h, const double *X, int64_t N, int32_t D, int32_t mode, double *out) {
  return entry(h, "plda_lda_predict", [&]() -> int {
    if (!h->lda_fitted) return fail(h, PLDA_E_NOT_FITTED, "This LDA instance is not fitted yet");
    if (D != h->lda_D)
      return fail(h, PLDA_E_INVAL, "X has %d features per sample; expecting %d", D, h->lda_D);   // lda.py:264-266
    if (N <= 0) return PLDA_OK;
    if (!X || !out) return fail(h, PLDA_E_INVAL, "lda_predict: bad argument");
    PLDA_TRY(set_device(h));
    // row slabs bound the device footprint of the [N, K] result
    const int64_t slab = std::max<int64_t>(1, std::min<int64_t>(N, ((int64_t)1 << 28) / std::max<int64_t>(h->lda_K, D)));
    Tmp dX, dO;
    PLDA_HIP(h, dX.alloc((size_t)slab * D * 8));
    PLDA_HIP(h, dO.alloc((size_t)slab * h->lda_K * 8));
    for (int64_t r0 = 0; r0 < N; r0 += slab) {
      const int64_t r = std::min(slab, N - r0);
      PLDA_HIP(h, hipMemcpyAsync(dX.p, X + r0 * D, (size_t)r * D * 8, hipMemcpyHostToDevice, h->stream));
      PLDA_TRY(lda_predict_device(h, dX.as<double>(), r, mode, dO.as<double>()));
      PLDA_HIP(h, hipMemcpyAsync(out + r0 * h->lda_K, dO.p, (size_t)r * h->lda_K * 8, hipMemcpyDeviceToHost, h->stream));
      PLDA_HIP(h, hipStreamSynchronize(h->stream));
    }
    return PLDA_OK;
  });
}

int plda_lda_transform_dev(plda_handle *h, const double *dX, int64_t N, int32_t ncomp, double *dout) {
  return device_entry(h, "plda_lda_transform_dev", [&] { return lda_transform_device(h, dX, N, ncomp, dout); });
}

int plda_lda_transform(plda_handle *h, const double *X, int64_t N, int32_t D, int32_t ncomp, double *out) {
  return entry(h, "plda_lda_transform", [&]() -> int {
    if (!h->lda_fitted) return fail(h, PLDA_E_NOT_FITTED, "This LDA instance is not fitted yet");
    if (D != h->lda_D) return fail(h, PLDA_E_INVAL, "X has %d features per sample; expecting %d", D, h->lda_D);
    if (N <= 0 || ncomp <= 0) return PLDA_OK;
    if (!X || !out) return fail(h, PLDA_E_INVAL, "lda_transform: bad argument");
    PLDA_TRY(set_device(h));
    Staged st(h);
    const double *dX;
    double *dO;
    PLDA_TRY(st.in(X, (size_t)N * D, &dX));
    PLDA_TRY(st.out(out, (size_t)N * ncomp, &dO, true));
    return st.finish(lda_transform_device(h, dX, N, ncomp, dO));
  });
}

// ---------------------------------------------------------------- HTK feature files
int plda_htk_frames_dev(plda_handle *h, const void *dblob, const int64_t *dfile_off, const int64_t *dframe_off,
                        int64_t U, int64_t T, int32_t samplesize, int32_t frm_ext, float *dout) {
  return device_entry(h, "plda_htk_frames_dev", [&] { return htk_frames_device(h, dblob, dfile_off, dframe_off, U, T, samplesize, frm_ext, dout); });
}

int plda_htk_frames(plda_handle *h, const void *blob, int64_t blob_bytes, const int64_t *file_off,
                    const int64_t *frame_off, int64_t U, int32_t samplesize, int32_t frm_ext, float *out) {
  return entry(h, "plda_htk_frames", [&]() -> int {
    if (U <= 0) return PLDA_OK;
    if (!blob || !file_off || !frame_off || !out || blob_bytes < 0 || samplesize <= 0 || frm_ext < 0)
      return fail(h, PLDA_E_INVAL, "htk_frames: bad argument");
    if (samplesize % 4) return fail(h, PLDA_E_INVAL, "htk_frames: samplesize %d is not a multiple of 4", samplesize);
    const int64_t W = samplesize / 4;
    for (int64_t u = 0; u < U; ++u) {
      const int64_t n = frame_off[u + 1] - frame_off[u];
      if (n < 0 || file_off[u] < 0 || (file_off[u] + n * W) * 4 > blob_bytes)
        return fail(h, PLDA_E_INVAL, "htk_frames: file %lld does not fit the blob (pad short files with zeros)", (long long)u);
    }
    const int64_t T = frame_off[U] - frame_off[0];
    if (frame_off[0] != 0) return fail(h, PLDA_E_INVAL, "htk_frames: frame_off[0] must be 0");
    if (T <= 0) return PLDA_OK;
    PLDA_TRY(set_device(h));
    Staged st(h);
    const void *dB;
    const int64_t *dF, *dO;
    float *dOut;
    PLDA_TRY(st.in(blob, (size_t)blob_bytes, &dB));
    PLDA_TRY(st.in(file_off, (size_t)U, &dF));
    PLDA_TRY(st.in(frame_off, (size_t)(U + 1), &dO));
    PLDA_TRY(st.out(out, (size_t)T * (2 * frm_ext + 1) * W, &dOut, true));     // (W floats per sample: samplesize bytes)
    return st.finish(htk_frames_device(h, dB, dF, dO, U, T, samplesize, frm_ext, dOut));
  });
}

// ---------------------------------------------------------------- multi-GPU (comm.hip)
int plda_comm_init(plda_handle *h, int32_t nranks, int32_t rank, const void *unique_id) {
  return device_entry(h, "plda_comm_init", [&] { return comm_init(h, nranks, rank, unique_id); });
}

int plda_comm_init_custom(plda_handle *h, int32_t nranks, int32_t rank, const plda_collectives *table) {
  return device_entry(h, "plda_comm_init_custom", [&] { return comm_init_custom(h, nranks, rank, table); });
}

int plda_comm_init_peer(plda_handle *h, int32_t nranks, int32_t rank, const plda_host_collectives *bootstrap) {
  return device_entry(h, "plda_comm_init_peer", [&] { return comm_init_peer(h, nranks, rank, bootstrap); });
}

int plda_comm_init_host(plda_handle *h, int32_t nranks, int32_t rank, const plda_host_collectives *table) {
  return device_entry(h, "plda_comm_init_host", [&] { return comm_init_host(h, nranks, rank, table); });
}

int plda_comm_destroy(plda_handle *h) {
  return device_entry(h, "plda_comm_destroy", [&] { return comm_destroy(h); });
}

int plda_comm_describe(plda_handle *h, char *json, int64_t cap) {
  return entry(h, "plda_comm_describe", [&]() -> int {
    if (!json || cap <= 0) return fail(h, PLDA_E_INVAL, "comm_describe: bad argument");
    PLDA_TRY(set_device(h));
    std::string js;
    PLDA_TRY(comm_describe(h, js));
    if ((int64_t)js.size() + 1 > cap) return fail(h, PLDA_E_CAPACITY, "comm_describe: need %zu bytes", js.size() + 1);
    std::memcpy(json, js.c_str(), js.size() + 1);
    return PLDA_OK;
  });
}

int plda_comm_emulate(plda_handle *h, int32_t nranks, int32_t rank) {
  return entry(h, "plda_comm_emulate", [&]() -> int {
    if (h->comm) return fail(h, PLDA_E_INVAL, "comm_emulate: this handle has a real communicator");
    if (nranks <= 0 || rank < 0 || rank >= nranks) return fail(h, PLDA_E_INVAL, "comm_emulate: bad argument");
    h->comm_nranks = nranks; h->comm_rank = rank;
    return PLDA_OK;
  });
}

int plda_comm_info(plda_handle *h, int32_t *nranks, int32_t *rank) {
  return entry(h, "plda_comm_info", [&]() -> int {
    if (nranks) *nranks = h->comm_nranks;
    if (rank) *rank = h->comm_rank;
    return PLDA_OK;
  });
}

int plda_score_matrix_sharded_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                                  const double *dV, int64_t Nt, const double *dzmean, const double *dzstd, float *dout,
                                  int64_t ld_out, int64_t block_rows, int32_t gather) {
  return entry(h, "plda_score_matrix_sharded_dev", [&]() -> int {
    if (!dn_enrol && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "score_matrix_sharded: n_uniform must be > 0 when n_enrol is NULL");
    PLDA_TRY(set_device(h));
    return score_matrix_sharded_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, nullptr, 0, dout, ld_out,
                                       block_rows, gather);
  });
}

int plda_score_matrix_sharded_local_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform,
                                        int64_t M, const double *dV, int64_t Nt, const double *dzmean, const double *dzstd,
                                        float *dlocal, int64_t ld_local, int64_t block_rows, float *dfull, int64_t ld_full) {
  return entry(h, "plda_score_matrix_sharded_local_dev", [&]() -> int {
    if (!dn_enrol && n_uniform <= 0) return fail(h, PLDA_E_INVAL, "score_matrix_sharded: n_uniform must be > 0 when n_enrol is NULL");
    if (!dlocal) return fail(h, PLDA_E_INVAL, "score_matrix_sharded_local: dlocal is NULL");
    PLDA_TRY(set_device(h));
    return score_matrix_sharded_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, dlocal, ld_local, dfull, ld_full,
                                       block_rows, dfull ? 1 : 0);
  });
}

int plda_znorm_stats_sharded_dev(plda_handle *h, const double *dbkg, int64_t Nb, int32_t num_examples, int32_t Din,
                                 const double *dmodels, int64_t M, double *dout_mean, double *dout_std) {
  return entry(h, "plda_znorm_stats_sharded_dev", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "norm: model not fitted");
    if (!dbkg || !dmodels || !dout_mean || !dout_std || Nb <= 0 || M <= 0) return fail(h, PLDA_E_INVAL, "norm: bad argument");
    PLDA_TRY(set_device(h));
    return znorm_stats_sharded_device(h, dbkg, Nb, num_examples, Din, dmodels, M, dout_mean, dout_std);
  });
}

int plda_cohort_stats_sharded_dev(plda_handle *h, const double *dX, const int32_t *dn, int32_t n_uniform, int64_t R, const double *dC,
                                  int64_t Nc, int64_t top_k, double *dmean, double *dstd) {
  return entry(h, "plda_cohort_stats_sharded_dev", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "cohort_stats: model not fitted");
    if (!dX || !dC || !dmean || !dstd || R < 1 || Nc < 1 || top_k < 1 || top_k > Nc) return fail(h, PLDA_E_INVAL, "cohort_stats_sharded: bad argument");
    PLDA_TRY(set_device(h));
    return cohort_stats_sharded_device(h, dX, dn, n_uniform, R, dC, Nc, top_k, dmean, dstd);
  });
}

int plda_fit_sharded_dev(plda_handle *h, const double *dX, int64_t N, int32_t D, const uint64_t *dlabels, int64_t K,
                         int32_t iters) {
  return device_entry(h, "plda_fit_sharded_dev", [&] { return fit_sharded_device(h, dX, N, D, dlabels, K, iters); });
}

int plda_eer_matrix_comm_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                             const int64_t *denrol_spk, const int64_t *dtest_spk, double *out) {
  return device_entry(h, "plda_eer_matrix_comm_dev", [&] { return eer_matrix_comm_device(h, dscores, ld, M, Nt, denrol_spk, dtest_spk, out); });
}

// ---------------------------------------------------------------- EER
int plda_eer_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                        const int64_t *denrol_spk, const int64_t *dtest_spk, double *out) {
  return device_entry(h, "plda_eer_matrix_dev", [&] { return eer_matrix_device(h, dscores, ld, M, Nt, denrol_spk, dtest_spk, out); });
}

int plda_score_eer_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M, const double *dV,
                       int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *denrol_spk, const int64_t *dtest_spk,
                       double *out) {
  return device_entry(h, "plda_score_eer_dev", [&] {
    return score_eer_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, denrol_spk, dtest_spk, out);
  });
}

int plda_eer_matrix_sharded_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt,
                                const int64_t *denrol_spk, const int64_t *dtest_spk, plda_eer_reduce_fn reduce, void *ctx,
                                double *out) {
  return entry(h, "plda_eer_matrix_sharded_dev", [&]() -> int {
    if (!reduce) return fail(h, PLDA_E_INVAL, "eer_matrix_sharded: a reduction callback is required");
    PLDA_TRY(set_device(h));
    return eer_matrix_device(h, dscores, ld, M, Nt, denrol_spk, dtest_spk, out, reduce, ctx);
  });
}

int plda_det_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                        const int64_t *dtest_spk, int32_t n_points, double *far, double *frr, double *thresholds) {
  return device_entry(h, "plda_det_matrix_dev", [&] {
    return det_matrix_device(h, dscores, ld, M, Nt, denrol_spk, dtest_spk, n_points, far, frr, thresholds);
  });
}

int plda_det_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, int32_t n_points, double *far,
                   double *frr, double *thresholds) {
  return with_host_lists(h, "plda_det_lists", pos, np, neg, nn, far && frr, "det: need at least one target and one impostor score",
                         [&](const float *dpos, const float *dneg) -> int {
    const int rc = det_lists_device(h, dpos, np, dneg, nn, n_points, far, frr, thresholds);
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    return rc;
  });
}

int plda_eer_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, double *out) {
  return with_host_lists(h, "plda_eer_lists", pos, np, neg, nn, out != nullptr, "eer: need at least one target and one impostor score",
                         [&](const float *dpos, const float *dneg) { return eer_lists_device(h, dpos, np, dneg, nn, out); });
}

// ---------------------------------------------------------------- ROC convex hull, minCllr, PAV (rocch.hip)
int plda_rocch_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                          const int64_t *dtest_spk, int64_t cap_vertices, plda_rocch *out, plda_rocch_vertex *vertices, double *llr,
                          plda_rocch_points *points, plda_rocch_info *info) {
  return device_entry(h, "plda_rocch_matrix_dev", [&] {
    return rocch_matrix_device(h, dscores, ld, M, Nt, denrol_spk, dtest_spk, cap_vertices, out, vertices, llr, points, info);
  });
}

int plda_rocch_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, int64_t cap_vertices, plda_rocch *out,
                     plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points, plda_rocch_info *info) {
  return with_host_lists(h, "plda_rocch_lists", pos, np, neg, nn, out != nullptr, "rocch: need at least one target and one non-target score",
                         [&](const float *dpos, const float *dneg) {
                           return rocch_lists_device(h, dpos, np, dneg, nn, cap_vertices, out, vertices, llr, points, info);
                         });
}

int plda_score_rocch_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M, const double *dV,
                         int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *denrol_spk, const int64_t *dtest_spk,
                         int64_t cap_vertices, plda_rocch *out, plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points,
                         plda_rocch_info *info) {
  return device_entry(h, "plda_score_rocch_dev", [&] {
    return score_rocch_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, denrol_spk, dtest_spk, cap_vertices, out, vertices, llr,
                              points, info);
  });
}

int plda_pav_map_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, int64_t n_vertices,
                     const plda_rocch_vertex *vertices, const double *llr, double bound, float *dout, int64_t ld_out) {
  return device_entry(h, "plda_pav_map_dev", [&] { return pav_map_device(h, dscores, ld, M, Nt, n_vertices, vertices, llr, bound, dout, ld_out); });
}

// the host steps: pure functions, no handle (the CPU suite drives them with NumPy ranks)
int plda_rocch_hull(int64_t T, const uint32_t *edge_key, const uint64_t *other_lt, const uint64_t *other_le, const uint64_t *edge_lt,
                    const uint64_t *edge_le, int32_t edge_class, uint64_t np, uint64_t nn, int64_t cap_vertices, plda_rocch *out,
                    plda_rocch_vertex *vertices, double *llr) {
  try { return rocch_hull(T, edge_key, other_lt, other_le, edge_lt, edge_le, edge_class, np, nn, cap_vertices, out, vertices, llr); }
  catch (...) { return PLDA_E_HIP; }      // (std::bad_alloc of the vertex stack)
}
int plda_rocch_finish(int64_t n_vertices, plda_rocch_vertex *vertices, const uint32_t *below, const uint32_t *above) {
  return rocch_finish(n_vertices, vertices, below, above);
}

// ---------------------------------------------------------------- trial keys: the partition (partition.hip) and the device-list forms
int plda_partition_plan(const int64_t *enrol_spk, int64_t M, const int64_t *test_spk, int64_t Nt, const plda_trial_key *key,
                        plda_partition_record *plan) {
  return guarded(nullptr, "plda_partition_plan", [&]() -> int { return partition_plan(nullptr, "partition_plan", enrol_spk, M, test_spk, Nt, key, plan); });
}

int plda_partition_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                              const int64_t *dtest_spk, const plda_trial_key *key, float *dtar, int64_t cap_tar, float *dnon,
                              int64_t cap_non, plda_partition_record *plan_out) {
  return device_entry(h, "plda_partition_matrix_dev", [&] {
    return partition_matrix_device(h, dscores, ld, M, Nt, denrol_spk, dtest_spk, key, dtar, cap_tar, dnon, cap_non, plan_out);
  });
}

int plda_score_partition_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M, const double *dV,
                             int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *denrol_spk, const int64_t *dtest_spk,
                             const plda_trial_key *key, float *dtar, int64_t cap_tar, float *dnon, int64_t cap_non,
                             plda_partition_record *plan_out) {
  return device_entry(h, "plda_score_partition_dev", [&] {
    return score_partition_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, denrol_spk, dtest_spk, key, dtar, cap_tar, dnon,
                                  cap_non, plan_out);
  });
}

// each is its _lists sibling without the upload: the same check, the same message, the same *_lists_device call
int plda_eer_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double *out) {
  return with_device_lists(h, "plda_eer_lists_dev", dpos, np, dneg, nn, out != nullptr, "eer: need at least one target and one impostor score",
                           [&] { return eer_lists_device(h, dpos, np, dneg, nn, out); });
}
int plda_det_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int32_t n_points, double *far,
                       double *frr, double *thresholds) {
  return with_device_lists(h, "plda_det_lists_dev", dpos, np, dneg, nn, far && frr, "det: need at least one target and one impostor score",
                           [&]() -> int {
    const int rc = det_lists_device(h, dpos, np, dneg, nn, n_points, far, frr, thresholds);
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    return rc;
  });
}
int plda_min_dcf_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int32_t n_points,
                           const plda_dcf_point *points, plda_min_dcf *out, plda_min_dcf_info *info) {
  return with_device_lists(h, "plda_min_dcf_lists_dev", dpos, np, dneg, nn, out != nullptr, "min_dcf: need at least one target and one non-target score",
                           [&] { return min_dcf_lists_device(h, dpos, np, dneg, nn, n_points, points, out, info); });
}
int plda_calib_pass_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double a, double c,
                              double theta, plda_calib_record *out_record) {
  return with_device_lists(h, "plda_calib_pass_lists_dev", dpos, np, dneg, nn, out_record != nullptr, "calib_pass: need at least one target and one non-target score",
                           [&] { return calib_pass_lists_device(h, dpos, np, dneg, nn, a, c, theta, out_record); });
}
int plda_calib_fit_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, double prior, double tol,
                             int32_t max_iter, plda_calib_fit *out_fit) {
  return with_device_lists(h, "plda_calib_fit_lists_dev", dpos, np, dneg, nn, out_fit != nullptr, "calib_fit: need at least one target and one non-target score",
                           [&] { return calib_fit_lists_device(h, dpos, np, dneg, nn, prior, tol, max_iter, out_fit); });
}
int plda_rocch_lists_dev(plda_handle *h, const float *dpos, int64_t np, const float *dneg, int64_t nn, int64_t cap_vertices,
                         plda_rocch *out, plda_rocch_vertex *vertices, double *llr, plda_rocch_points *points, plda_rocch_info *info) {
  return with_device_lists(h, "plda_rocch_lists_dev", dpos, np, dneg, nn, out != nullptr, "rocch: need at least one target and one non-target score",
                           [&] { return rocch_lists_device(h, dpos, np, dneg, nn, cap_vertices, out, vertices, llr, points, info); });
}
int plda_fusion_pass_lists_dev(plda_handle *h, int32_t n_systems, const float *const *dpos, int64_t np, const float *const *dneg,
                               int64_t nn, const double *a, double c, double theta, plda_fusion_record *out_record) {
  return entry(h, "plda_fusion_pass_lists_dev", [&]() -> int {
    if (!out_record || !a) return fail(h, PLDA_E_INVAL, "%s: the output structure or the weight array is NULL", "plda_fusion_pass_lists_dev");
    PLDA_TRY(fusion_list_args_check(h, "plda_fusion_pass_lists_dev", n_systems, dpos, np, dneg, nn));
    PLDA_TRY(set_device(h));
    return fusion_pass_lists_device(h, n_systems, dpos, np, dneg, nn, a, c, theta, out_record);
  });
}
int plda_fusion_fit_lists_dev(plda_handle *h, int32_t n_systems, const float *const *dpos, int64_t np, const float *const *dneg,
                              int64_t nn, double prior, double tol, int32_t max_iter, plda_fusion_fit *out_fit) {
  return entry(h, "plda_fusion_fit_lists_dev", [&]() -> int {
    if (!out_fit) return fail(h, PLDA_E_INVAL, "%s: the output structure or the weight array is NULL", "plda_fusion_fit_lists_dev");
    PLDA_TRY(fusion_list_args_check(h, "plda_fusion_fit_lists_dev", n_systems, dpos, np, dneg, nn));
    PLDA_TRY(set_device(h));
    return fusion_fit_lists_device(h, n_systems, dpos, np, dneg, nn, prior, tol, max_iter, out_fit);
  });
}

// ---------------------------------------------------------------- minimum detection cost (dcf.hip)
int plda_min_dcf_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                            const int64_t *dtest_spk, int32_t n_points, const plda_dcf_point *points, plda_min_dcf *out,
                            plda_min_dcf_info *info) {
  return entry(h, "plda_min_dcf_matrix_dev", [&]() -> int {
    if (M <= 0) return fail(h, PLDA_E_INVAL, "min_dcf: bad argument");
    PLDA_TRY(set_device(h));
    return min_dcf_matrix_device(h, dscores, ld, M, Nt, denrol_spk, dtest_spk, n_points, points, out, info, nullptr, nullptr);
  });
}

int plda_min_dcf_matrix_comm_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                                 const int64_t *dtest_spk, int32_t n_points, const plda_dcf_point *points, plda_min_dcf *out,
                                 plda_min_dcf_info *info) {
  return device_entry(h, "plda_min_dcf_matrix_comm_dev", [&] {
    return min_dcf_matrix_comm_device(h, dscores, ld, M, Nt, denrol_spk, dtest_spk, n_points, points, out, info);
  });
}

int plda_min_dcf_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, int32_t n_points,
                       const plda_dcf_point *points, plda_min_dcf *out, plda_min_dcf_info *info) {
  return with_host_lists(h, "plda_min_dcf_lists", pos, np, neg, nn, out != nullptr, "min_dcf: need at least one target and one non-target score",
                         [&](const float *dpos, const float *dneg) { return min_dcf_lists_device(h, dpos, np, dneg, nn, n_points, points, out, info); });
}

int plda_score_min_dcf_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M, const double *dV,
                           int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *denrol_spk, const int64_t *dtest_spk,
                           int32_t n_points, const plda_dcf_point *points, plda_min_dcf *out, plda_min_dcf_info *info) {
  return device_entry(h, "plda_score_min_dcf_dev", [&] {
    return score_min_dcf_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, denrol_spk, dtest_spk, n_points, points, out, info);
  });
}

// the host step: pure functions, no handle (include/plda_hip.h)
int plda_min_dcf_step(int32_t level, int64_t n_nodes, const plda_min_dcf_node *nodes, const uint64_t *hist, int32_t n_points,
                      const plda_dcf_point *points, plda_min_dcf_state *state, int64_t cap_next, plda_min_dcf_node *next,
                      int64_t *n_next) {
  return min_dcf_step(level, n_nodes, nodes, hist, n_points, points, state, cap_next, next, n_next);
}
int plda_min_dcf_finish(const plda_min_dcf_state *state, int32_t n_points, const plda_dcf_point *points, const uint32_t *below,
                        const uint32_t *above, plda_min_dcf *out) {
  return min_dcf_finish(state, n_points, points, below, above, out);
}

// ---------------------------------------------------------------- score calibration (calib.hip)
int plda_calib_pass_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                               const int64_t *dtest_spk, double a, double c, double theta, plda_calib_record *out_record) {
  return device_entry(h, "plda_calib_pass_matrix_dev", [&] {
    return calib_pass_matrix_device(h, dscores, ld, M, Nt, denrol_spk, dtest_spk, a, c, theta, out_record);
  });
}

int plda_calib_fit_matrix_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                              const int64_t *dtest_spk, double prior, double tol, int32_t max_iter, plda_calib_fit *out_fit) {
  return device_entry(h, "plda_calib_fit_matrix_dev", [&] {
    return calib_fit_matrix_device(h, dscores, ld, M, Nt, denrol_spk, dtest_spk, prior, tol, max_iter, out_fit);
  });
}

int plda_calib_pass_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, double a, double c,
                          double theta, plda_calib_record *out_record) {
  return with_host_lists(h, "plda_calib_pass_lists", pos, np, neg, nn, out_record != nullptr, "calib_pass: need at least one target and one non-target score",
                         [&](const float *dpos, const float *dneg) { return calib_pass_lists_device(h, dpos, np, dneg, nn, a, c, theta, out_record); });
}

int plda_calib_fit_lists(plda_handle *h, const float *pos, int64_t np, const float *neg, int64_t nn, double prior, double tol,
                         int32_t max_iter, plda_calib_fit *out_fit) {
  return with_host_lists(h, "plda_calib_fit_lists", pos, np, neg, nn, out_fit != nullptr, "calib_fit: need at least one target and one non-target score",
                         [&](const float *dpos, const float *dneg) { return calib_fit_lists_device(h, dpos, np, dneg, nn, prior, tol, max_iter, out_fit); });
}

int plda_score_calib_pass_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                              const double *dV, int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *denrol_spk,
                              const int64_t *dtest_spk, double a, double c, double theta, plda_calib_record *out_record) {
  return device_entry(h, "plda_score_calib_pass_dev", [&] {
    return score_calib_pass_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, denrol_spk, dtest_spk, a, c, theta, out_record);
  });
}

int plda_score_calib_fit_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                             const double *dV, int64_t Nt, const double *dzmean, const double *dzstd, const int64_t *denrol_spk,
                             const int64_t *dtest_spk, double prior, double tol, int32_t max_iter, plda_calib_fit *out_fit) {
  return device_entry(h, "plda_score_calib_fit_dev", [&] {
    return score_calib_fit_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, denrol_spk, dtest_spk, prior, tol, max_iter, out_fit);
  });
}

int plda_affine_map_dev(plda_handle *h, const float *dscores, int64_t ld, int64_t M, int64_t Nt, double a, double b, float *dout,
                        int64_t ld_out) {
  return device_entry(h, "plda_affine_map_dev", [&] { return affine_map_device(h, dscores, ld, M, Nt, a, b, dout, ld_out); });
}

// ---------------------------------------------------------------- multi-system score fusion (fusion.hip)
int plda_fusion_pass_matrices_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int64_t M,
                                  int64_t Nt, const int64_t *denrol_spk, const int64_t *dtest_spk, const double *a, double c,
                                  double theta, plda_fusion_record *out_record) {
  return device_entry(h, "plda_fusion_pass_matrices_dev", [&] {
    return fusion_pass_matrices_device(h, n_systems, dscores, ld, M, Nt, denrol_spk, dtest_spk, a, c, theta, out_record);
  });
}

int plda_fusion_fit_matrices_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int64_t M,
                                 int64_t Nt, const int64_t *denrol_spk, const int64_t *dtest_spk, double prior, double tol,
                                 int32_t max_iter, plda_fusion_fit *out_fit) {
  return device_entry(h, "plda_fusion_fit_matrices_dev", [&] {
    return fusion_fit_matrices_device(h, n_systems, dscores, ld, M, Nt, denrol_spk, dtest_spk, prior, tol, max_iter, out_fit);
  });
}

int plda_fusion_pass_lists(plda_handle *h, int32_t n_systems, const float *const *pos, int64_t np, const float *const *neg,
                           int64_t nn, const double *a, double c, double theta, plda_fusion_record *out_record) {
  return with_host_fusion_lists(h, "plda_fusion_pass_lists", n_systems, pos, np, neg, nn, out_record != nullptr && a != nullptr,
                                [&](const float *const *dpos, const float *const *dneg) {
                                  return fusion_pass_lists_device(h, n_systems, dpos, np, dneg, nn, a, c, theta, out_record);
                                });
}

int plda_fusion_fit_lists(plda_handle *h, int32_t n_systems, const float *const *pos, int64_t np, const float *const *neg,
                          int64_t nn, double prior, double tol, int32_t max_iter, plda_fusion_fit *out_fit) {
  return with_host_fusion_lists(h, "plda_fusion_fit_lists", n_systems, pos, np, neg, nn, out_fit != nullptr,
                                [&](const float *const *dpos, const float *const *dneg) {
                                  return fusion_fit_lists_device(h, n_systems, dpos, np, dneg, nn, prior, tol, max_iter, out_fit);
                                });
}

int plda_fusion_map_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int64_t M, int64_t Nt,
                        const double *a, double b, float *dout, int64_t ld_out) {
  return device_entry(h, "plda_fusion_map_dev", [&] { return fusion_map_device(h, n_systems, dscores, ld, M, Nt, a, b, dout, ld_out); });
}

// the Newton step: a pure function, no handle (include/plda_hip.h)
int plda_fusion_newton(const plda_fusion_record *record, double prior, double *F, double *d, double *lambda2) {
  return guarded(nullptr, "plda_fusion_newton", [&]() -> int { return fusion_newton(record, prior, F, d, lambda2); });
}

// ---------------------------------------------------------------- quality-aware calibration (fusion.hip)
int plda_fusion_side_pass_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int32_t n_sides,
                              const plda_fusion_side *sides, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                              const int64_t *dtest_spk, const double *a, double c, double theta, plda_fusion_record *out_record) {
  return device_entry(h, "plda_fusion_side_pass_dev", [&] {
    return fusion_side_pass_device(h, n_systems, dscores, ld, n_sides, sides, M, Nt, denrol_spk, dtest_spk, a, c, theta, out_record);
  });
}

int plda_fusion_side_fit_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int32_t n_sides,
                             const plda_fusion_side *sides, int64_t M, int64_t Nt, const int64_t *denrol_spk,
                             const int64_t *dtest_spk, double prior, double tol, int32_t max_iter, plda_fusion_fit *out_fit) {
  return device_entry(h, "plda_fusion_side_fit_dev", [&] {
    return fusion_side_fit_device(h, n_systems, dscores, ld, n_sides, sides, M, Nt, denrol_spk, dtest_spk, prior, tol, max_iter, out_fit);
  });
}

int plda_fusion_side_map_dev(plda_handle *h, int32_t n_systems, const float *const *dscores, const int64_t *ld, int32_t n_sides,
                             const plda_fusion_side *sides, int64_t M, int64_t Nt, const double *a, double b, float *dout,
                             int64_t ld_out) {
  return device_entry(h, "plda_fusion_side_map_dev", [&] {
    return fusion_side_map_device(h, n_systems, dscores, ld, n_sides, sides, M, Nt, a, b, dout, ld_out);
  });
}

int plda_score_fusion_side_pass_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                                    const double *dV, int64_t Nt, const double *dzmean, const double *dzstd,
                                    const int64_t *denrol_spk, const int64_t *dtest_spk, int32_t n_sides,
                                    const plda_fusion_side *sides, const double *a, double c, double theta,
                                    plda_fusion_record *out_record) {
  return device_entry(h, "plda_score_fusion_side_pass_dev", [&] {
    return score_fusion_side_pass_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, denrol_spk, dtest_spk, n_sides, sides, a, c,
                                         theta, out_record);
  });
}

int plda_score_fusion_side_fit_dev(plda_handle *h, const double *dU, const int32_t *dn_enrol, int32_t n_uniform, int64_t M,
                                   const double *dV, int64_t Nt, const double *dzmean, const double *dzstd,
                                   const int64_t *denrol_spk, const int64_t *dtest_spk, int32_t n_sides,
                                   const plda_fusion_side *sides, double prior, double tol, int32_t max_iter,
                                   plda_fusion_fit *out_fit) {
  return device_entry(h, "plda_score_fusion_side_fit_dev", [&] {
    return score_fusion_side_fit_device(h, dU, dn_enrol, n_uniform, M, dV, Nt, dzmean, dzstd, denrol_spk, dtest_spk, n_sides, sides, prior,
                                        tol, max_iter, out_fit);
  });
}

// ---------------------------------------------------------------- speaker clustering (ahc.hip)
int plda_ahc_plan(plda_handle *h, int64_t N, int32_t out[3]) {
  return entry(h, "plda_ahc_plan", [&] { return ahc_plan(h, N, out); });
}

int plda_ahc_matrix_dev(plda_handle *h, const float *dscores, const int64_t *block_off, const int64_t *offsets, int64_t R,
                        int32_t has_threshold, double threshold, const int32_t *min_clusters, int32_t *dlabels,
                        int32_t *dn_clusters, int32_t *dmerge_a, int32_t *dmerge_b, double *dmerge_cost) {
  return device_entry(h, "plda_ahc_matrix_dev", [&] {
    return ahc_matrix_device(h, dscores, block_off, offsets, R,
                             ahc_args(has_threshold, threshold, min_clusters, 1, dlabels, dn_clusters, dmerge_a, dmerge_b, dmerge_cost));
  });
}

int plda_ahc_matrix(plda_handle *h, const float *scores, const int64_t *block_off, const int64_t *offsets, int64_t R,
                    int32_t has_threshold, double threshold, const int32_t *min_clusters, int32_t *labels, int32_t *n_clusters,
                    int32_t *merge_a, int32_t *merge_b, double *merge_cost) {
  return entry(h, "plda_ahc_matrix", [&]() -> int {
    const AhcArgs host = ahc_args(has_threshold, threshold, min_clusters, 1, labels, n_clusters, merge_a, merge_b, merge_cost);
    if (!scores) return fail(h, PLDA_E_INVAL, "ahc_matrix: scores is NULL");
    PLDA_TRY(ahc_validate(h, "ahc_matrix", block_off, true, offsets, R, host));
    PLDA_TRY(set_device(h));
    const size_t T = (size_t)offsets[R];
    const std::vector<int64_t> rel = block_rel(block_off, R);
    Staged st(h);
    const float *dS;
    AhcArgs dev;
    PLDA_TRY(st.in(scores + block_off[0], (size_t)rel[(size_t)R], &dS));
    PLDA_TRY(ahc_stage_outputs(st, host, T, T - (size_t)R, &dev));
    return st.finish(ahc_matrix_device(h, dS, rel.data(), offsets, R, dev));
  });
}

int plda_score_ahc_dev(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, int32_t has_threshold,
                       double threshold, const int32_t *min_clusters, int32_t *dlabels, int32_t *dn_clusters,
                       int32_t *dmerge_a, int32_t *dmerge_b, double *dmerge_cost) {
  return device_entry(h, "plda_score_ahc_dev", [&] {
    return score_ahc_device(h, dX, offsets, R,
                            ahc_args(has_threshold, threshold, min_clusters, 1, dlabels, dn_clusters, dmerge_a, dmerge_b, dmerge_cost));
  });
}

int plda_score_ahc(plda_handle *h, const double *X, const int64_t *offsets, int64_t R, int32_t has_threshold, double threshold,
                   const int32_t *min_clusters, int32_t *labels, int32_t *n_clusters, int32_t *merge_a, int32_t *merge_b,
                   double *merge_cost) {
  return entry(h, "plda_score_ahc", [&]() -> int {
    const AhcArgs host = ahc_args(has_threshold, threshold, min_clusters, 1, labels, n_clusters, merge_a, merge_b, merge_cost);
    if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "score_ahc: model not fitted");
    if (!X) return fail(h, PLDA_E_INVAL, "score_ahc: X is NULL");
    PLDA_TRY(ahc_validate(h, "score_ahc", nullptr, false, offsets, R, host));
    PLDA_TRY(set_device(h));
    const size_t T = (size_t)offsets[R];
    Staged st(h);
    const double *dX;
    AhcArgs dev;
    PLDA_TRY(st.in(X, T * h->Dout, &dX));
    PLDA_TRY(ahc_stage_outputs(st, host, T, T - (size_t)R, &dev));
    return st.finish(score_ahc_device(h, dX, offsets, R, dev));
  });
}

// ---------------------------------------------------------------- corpus-scale clustering (ahc.hip, the wide class)
int plda_ahc_wide_plan(plda_handle *h, int64_t N, int64_t out[4]) {
  return entry(h, "plda_ahc_wide_plan", [&] { return ahc_wide_plan(h, N, out); });
}

int plda_ahc_wide_matrix_dev(plda_handle *h, const float *dscores, int64_t N, int64_t ld, int32_t has_threshold, double threshold,
                             int32_t min_clusters, int32_t *dlabels, int32_t *dn_clusters, int32_t *dmerge_a, int32_t *dmerge_b,
                             double *dmerge_cost) {
  return device_entry(h, "plda_ahc_wide_matrix_dev", [&] {
    return ahc_wide_matrix_device(h, dscores, N, ld,
                                  ahc_args(has_threshold, threshold, nullptr, min_clusters, dlabels, dn_clusters, dmerge_a, dmerge_b,
                                           dmerge_cost));
  });
}

int plda_ahc_wide_matrix(plda_handle *h, const float *scores, int64_t N, int64_t ld, int32_t has_threshold, double threshold,
                         int32_t min_clusters, int32_t *labels, int32_t *n_clusters, int32_t *merge_a, int32_t *merge_b,
                         double *merge_cost) {
  return entry(h, "plda_ahc_wide_matrix", [&]() -> int {
    const AhcArgs host = ahc_args(has_threshold, threshold, nullptr, min_clusters, labels, n_clusters, merge_a, merge_b, merge_cost);
    if (!scores) return fail(h, PLDA_E_INVAL, "ahc_wide_matrix: scores is NULL");
    PLDA_TRY(ahc_wide_validate(h, "ahc_wide_matrix", N, ld, host));
    PLDA_TRY(set_device(h));
    Staged st(h);
    const float *dS;
    AhcArgs dev;
    PLDA_TRY(st.in(scores, (size_t)((N - 1) * ld + N), &dS));
    PLDA_TRY(ahc_stage_outputs(st, host, (size_t)N, (size_t)(N - 1), &dev));
    return st.finish(ahc_wide_matrix_device(h, dS, N, ld, dev));
  });
}

int plda_score_ahc_wide_dev(plda_handle *h, const double *dX, int64_t N, int32_t has_threshold, double threshold,
                            int32_t min_clusters, int32_t *dlabels, int32_t *dn_clusters, int32_t *dmerge_a, int32_t *dmerge_b,
                            double *dmerge_cost) {
  return device_entry(h, "plda_score_ahc_wide_dev", [&] {
    return score_ahc_wide_device(h, dX, N,
                                 ahc_args(has_threshold, threshold, nullptr, min_clusters, dlabels, dn_clusters, dmerge_a, dmerge_b,
                                          dmerge_cost));
  });
}

int plda_score_ahc_wide(plda_handle *h, const double *X, int64_t N, int32_t has_threshold, double threshold, int32_t min_clusters,
                        int32_t *labels, int32_t *n_clusters, int32_t *merge_a, int32_t *merge_b, double *merge_cost) {
  return entry(h, "plda_score_ahc_wide", [&]() -> int {
    const AhcArgs host = ahc_args(has_threshold, threshold, nullptr, min_clusters, labels, n_clusters, merge_a, merge_b, merge_cost);
    if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "score_ahc_wide: model not fitted");
    if (!X) return fail(h, PLDA_E_INVAL, "score_ahc_wide: X is NULL");
    PLDA_TRY(ahc_wide_validate(h, "score_ahc_wide", N, N, host));
    PLDA_TRY(set_device(h));
    Staged st(h);
    const double *dX;
    AhcArgs dev;
    PLDA_TRY(st.in(X, (size_t)N * h->Dout, &dX));
    PLDA_TRY(ahc_stage_outputs(st, host, (size_t)N, (size_t)(N - 1), &dev));
    return st.finish(score_ahc_wide_device(h, dX, N, dev));
  });
}

// ---------------------------------------------------------------- spectral clustering (spectral.hip)
namespace {
SpectralArgs spectral_args(const int64_t *offsets, int64_t R, const int32_t *p_table, int32_t P, int32_t max_speakers,
                           const int32_t *num_speakers, int32_t max_iters, int32_t *labels, int32_t *n_clusters, int32_t *p_used,
                           int32_t *k_gap, double *eig, double *embed, int32_t *deg2) {
  SpectralArgs a;
  a.offsets = offsets; a.R = R; a.p_table = p_table; a.P = P; a.max_spk = max_speakers; a.num_spk = num_speakers; a.max_iters = max_iters;
  a.labels = labels; a.n_clusters = n_clusters; a.p_used = p_used; a.k_gap = k_gap; a.eig = eig; a.embed = embed; a.deg2 = deg2;
  return a;
}
// the device outputs of a host form, sized from the (validated) host arguments
int spectral_stage_outputs(Staged &st, const SpectralArgs &host, SpectralArgs *dev) {
  const size_t T = (size_t)host.offsets[host.R], R = (size_t)host.R;
  *dev = host;
  PLDA_TRY(st.out(host.labels, T, &dev->labels));
  PLDA_TRY(st.out(host.n_clusters, R, &dev->n_clusters));
  PLDA_TRY(st.out(host.p_used, R, &dev->p_used));
  PLDA_TRY(st.out(host.k_gap, R, &dev->k_gap));
  PLDA_TRY(st.out(host.eig, R * (size_t)host.P * (size_t)(host.max_spk + 2), &dev->eig));
  PLDA_TRY(st.out(host.embed, T * (size_t)host.max_spk, &dev->embed));
  PLDA_TRY(st.out(host.deg2, T, &dev->deg2));
  return PLDA_OK;
}
}  // namespace

int plda_spectral_plan(plda_handle *h, int64_t N, int32_t k, int32_t out[5]) {
  return entry(h, "plda_spectral_plan", [&] { return spectral_plan(h, N, k, out); });
}

int plda_spectral_matrix_dev(plda_handle *h, const float *dscores, const int64_t *block_off, const int64_t *offsets, int64_t R,
                             const int32_t *p_table, int32_t P, int32_t max_speakers, const int32_t *num_speakers, int32_t max_iters,
                             int32_t *dlabels, int32_t *dn_clusters, int32_t *dp_used, int32_t *dk_gap, double *deig, double *dembed,
                             int32_t *ddeg2) {
  return device_entry(h, "plda_spectral_matrix_dev", [&] {
    return spectral_matrix_device(h, dscores, block_off,
                                  spectral_args(offsets, R, p_table, P, max_speakers, num_speakers, max_iters, dlabels, dn_clusters,
                                                dp_used, dk_gap, deig, dembed, ddeg2));
  });
}

int plda_spectral_matrix(plda_handle *h, const float *scores, const int64_t *block_off, const int64_t *offsets, int64_t R,
                         const int32_t *p_table, int32_t P, int32_t max_speakers, const int32_t *num_speakers, int32_t max_iters,
                         int32_t *labels, int32_t *n_clusters, int32_t *p_used, int32_t *k_gap, double *eig, double *embed,
                         int32_t *deg2) {
  return entry(h, "plda_spectral_matrix", [&]() -> int {
    const SpectralArgs host = spectral_args(offsets, R, p_table, P, max_speakers, num_speakers, max_iters, labels, n_clusters, p_used,
                                            k_gap, eig, embed, deg2);
    if (!scores) return fail(h, PLDA_E_INVAL, "spectral_matrix: scores is NULL");
    PLDA_TRY(spectral_validate(h, "spectral_matrix", block_off, true, host));
    PLDA_TRY(set_device(h));
    const std::vector<int64_t> rel = block_rel(block_off, R);
    Staged st(h);
    const float *dS;
    PLDA_TRY(st.in(scores + block_off[0], (size_t)rel[(size_t)R], &dS));
    SpectralArgs dev;
    PLDA_TRY(spectral_stage_outputs(st, host, &dev));
    return st.finish(spectral_matrix_device(h, dS, rel.data(), dev));
  });
}

int plda_score_spectral_dev(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, const int32_t *p_table, int32_t P,
                            int32_t max_speakers, const int32_t *num_speakers, int32_t max_iters, int32_t *dlabels,
                            int32_t *dn_clusters, int32_t *dp_used, int32_t *dk_gap, double *deig, double *dembed, int32_t *ddeg2) {
  return device_entry(h, "plda_score_spectral_dev", [&] {
    return score_spectral_device(h, dX, spectral_args(offsets, R, p_table, P, max_speakers, num_speakers, max_iters, dlabels,
                                                      dn_clusters, dp_used, dk_gap, deig, dembed, ddeg2));
  });
}

int plda_score_spectral(plda_handle *h, const double *X, const int64_t *offsets, int64_t R, const int32_t *p_table, int32_t P,
                        int32_t max_speakers, const int32_t *num_speakers, int32_t max_iters, int32_t *labels, int32_t *n_clusters,
                        int32_t *p_used, int32_t *k_gap, double *eig, double *embed, int32_t *deg2) {
  return entry(h, "plda_score_spectral", [&]() -> int {
    const SpectralArgs host = spectral_args(offsets, R, p_table, P, max_speakers, num_speakers, max_iters, labels, n_clusters, p_used,
                                            k_gap, eig, embed, deg2);
    if (!can_score(h)) return fail(h, PLDA_E_NOT_FITTED, "score_spectral: model not fitted");
    if (!X) return fail(h, PLDA_E_INVAL, "score_spectral: X is NULL");
    PLDA_TRY(spectral_validate(h, "score_spectral", nullptr, false, host));
    PLDA_TRY(set_device(h));
    Staged st(h);
    const double *dX;
    PLDA_TRY(st.in(X, (size_t)offsets[R] * h->Dout, &dX));
    SpectralArgs dev;
    PLDA_TRY(spectral_stage_outputs(st, host, &dev));
    return st.finish(score_spectral_device(h, dX, dev));
  });
}

// ---------------------------------------------------------------- dense scoring in a recording's PCA subspace (dense_pca.hip)
int plda_dense_pca_plan(plda_handle *h, int64_t N, int32_t D, int32_t out[4]) {
  return entry(h, "plda_dense_pca_plan", [&] { return dense_pca_plan(h, N, D, out); });
}

int plda_score_dense_pca_dev(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, double target_energy,
                             float *dscores, const int64_t *block_off, int32_t *ddims, double *deig) {
  return device_entry(h, "plda_score_dense_pca_dev", [&] {
    return score_dense_pca_device(h, dX, offsets, R, target_energy, dscores, block_off, ddims, deig);
  });
}

int plda_score_dense_pca(plda_handle *h, const double *X, const int64_t *offsets, int64_t R, double target_energy, float *scores,
                         const int64_t *block_off, int32_t *dims, double *eig) {
  return entry(h, "plda_score_dense_pca", [&]() -> int {
    PLDA_TRY(dense_pca_validate(h, "score_dense_pca", offsets, R, target_energy, block_off, true));
    if (!X) return fail(h, PLDA_E_INVAL, "score_dense_pca: X is NULL");
    if (!scores) return fail(h, PLDA_E_INVAL, "score_dense_pca: scores is NULL");
    PLDA_TRY(set_device(h));
    const int64_t T = offsets[R], first = block_off[0];
    const std::vector<int64_t> rel = block_rel(block_off, R);
    const int64_t floats = rel[(size_t)R];
    Staged st(h);
    const double *dX;
    Tmp dS, dD, dE;
    PLDA_TRY(st.in(X, (size_t)T * h->Din, &dX));
    PLDA_HIP(h, dS.alloc((size_t)floats * 4));
    if (dims) PLDA_HIP(h, dD.alloc((size_t)R * 4));
    if (eig) PLDA_HIP(h, dE.alloc((size_t)T * 8));
    bool packed = true;                        // every block exactly N_r^2 floats: one copy back; otherwise block by block
    for (int64_t r = 0; r < R; ++r) {
      const int64_t n = offsets[r + 1] - offsets[r];
      packed = packed && rel[(size_t)r + 1] - rel[(size_t)r] == n * n;
    }
    const int rc = score_dense_pca_device(h, dX, offsets, R, target_energy, dS.as<float>(), rel.data(),
                                          dims ? dD.as<int32_t>() : nullptr, eig ? dE.as<double>() : nullptr);
    if (rc != PLDA_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
    if (packed) {
      PLDA_HIP(h, hipMemcpyAsync(scores + first, dS.p, (size_t)floats * 4, hipMemcpyDeviceToHost, h->stream));
    } else {
      for (int64_t r = 0; r < R; ++r) {
        const int64_t n = offsets[r + 1] - offsets[r];
        PLDA_HIP(h, hipMemcpyAsync(scores + block_off[r], dS.as<float>() + rel[(size_t)r], (size_t)(n * n) * 4, hipMemcpyDeviceToHost,
                                   h->stream));
      }
    }
    if (dims) PLDA_HIP(h, hipMemcpyAsync(dims, dD.p, (size_t)R * 4, hipMemcpyDeviceToHost, h->stream));
    if (eig) PLDA_HIP(h, hipMemcpyAsync(eig, dE.p, (size_t)T * 8, hipMemcpyDeviceToHost, h->stream));
    PLDA_HIP(h, hipStreamSynchronize(h->stream));
    return PLDA_OK;
  });
}

int plda_score_dense_pca_ahc_dev(plda_handle *h, const double *dX, const int64_t *offsets, int64_t R, double target_energy,
                                 int32_t has_threshold, double threshold, const int32_t *min_clusters, int32_t *dlabels,
                                 int32_t *dn_clusters, int32_t *dmerge_a, int32_t *dmerge_b, double *dmerge_cost) {
  return device_entry(h, "plda_score_dense_pca_ahc_dev", [&] {
    return score_dense_pca_ahc_device(h, dX, offsets, R, target_energy,
                                      ahc_args(has_threshold, threshold, min_clusters, 1, dlabels, dn_clusters, dmerge_a, dmerge_b,
                                               dmerge_cost));
  });
}

int plda_score_dense_pca_ahc(plda_handle *h, const double *X, const int64_t *offsets, int64_t R, double target_energy,
                             int32_t has_threshold, double threshold, const int32_t *min_clusters, int32_t *labels,
                             int32_t *n_clusters, int32_t *merge_a, int32_t *merge_b, double *merge_cost) {
  return entry(h, "plda_score_dense_pca_ahc", [&]() -> int {
    const AhcArgs host = ahc_args(has_threshold, threshold, min_clusters, 1, labels, n_clusters, merge_a, merge_b, merge_cost);
    PLDA_TRY(dense_pca_validate(h, "score_dense_pca_ahc", offsets, R, target_energy, nullptr, false));
    if (!X) return fail(h, PLDA_E_INVAL, "score_dense_pca_ahc: X is NULL");
    PLDA_TRY(ahc_validate(h, "score_dense_pca_ahc", nullptr, false, offsets, R, host));
    PLDA_TRY(set_device(h));
    const size_t T = (size_t)offsets[R];
    Staged st(h);
    const double *dX;
    AhcArgs dev;
    PLDA_TRY(st.in(X, T * h->Din, &dX));
    PLDA_TRY(ahc_stage_outputs(st, host, T, T - (size_t)R, &dev));
    return st.finish(score_dense_pca_ahc_device(h, dX, offsets, R, target_energy, dev));
  });
}

// ---------------------------------------------------------------- diarisation error rate (der.hip, der_time.hip)
// Every entry point below fills a DerArgs by field name -- the group all forms of its family share through one of the two
// functions here, the rest by assignment -- and hands it to the device form (der_seg_device, der_timed_device) or to der_host.
namespace {
DerArgs der_seg_args(const int32_t *ref, const int32_t *dur, const int64_t *offsets, int64_t R, int64_t *counts) {
  DerArgs a;
  a.ref = ref; a.dur = dur; a.offsets = offsets; a.R = R; a.counts = counts;
  return a;
}

DerArgs der_timed_args(const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                       const int32_t *seg_start, const int32_t *seg_dur, const int64_t *offsets, int64_t R, const int32_t *uem_start,
                       const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags, int64_t *counts) {
  DerArgs a;
  a.tstart = turn_start; a.tdur = turn_dur; a.tspk = turn_spk; a.turn_off = turn_off;
  a.sstart = seg_start; a.sdur = seg_dur; a.offsets = offsets; a.R = R;
  a.ustart = uem_start; a.udur = uem_dur; a.uem_off = uem_off; a.collar = collar; a.flags = flags;
  a.counts = counts;
  return a;
}

// the sweep of a full merge record over Q thresholds
void der_sweep_args(DerArgs &a, const int32_t *merge_a, const int32_t *merge_b, const double *merge_cost, const double *thresholds,
                    int64_t Q, const int32_t *min_clusters, int32_t *n_clusters) {
  a.ma = merge_a; a.mb = merge_b; a.mc = merge_cost; a.thresholds = thresholds; a.Q = Q; a.minc = min_clusters;
  a.n_clusters = n_clusters;
}

// the JER form: jer behind the outputs of the plain form (a sweep has neither jmap nor spk)
void der_jer_args(DerArgs &a, int64_t *jer, int32_t *jmap = nullptr, int64_t *spk = nullptr) {
  a.jer_form = true;
  a.jo.jer = reinterpret_cast<long long *>(jer); a.jo.jmap = jmap; a.jo.spk = reinterpret_cast<long long *>(spk);
}

// the host form of every DER call: the check, every array uploaded, the outputs copied back (an array the form does not
// have is NULL and gets no temporary)
int der_host(plda_handle *h, const char *fn, DerArgs a, bool sweep, bool timed) {
  PLDA_TRY(timed ? der_timed_validate(h, fn, a, sweep) : der_seg_validate(h, fn, a, sweep));
  PLDA_TRY(set_device(h));
  const int64_t T = a.offsets[a.R], R = a.R, nt = timed ? a.turn_off[R] : 0, nu = a.uem_off ? a.uem_off[R] : 0;
  Staged st(h);
  int64_t *counts = a.counts;
  int32_t *ncl = a.n_clusters, *map = a.map;
  PLDA_TRY(st.in(a.ref, (size_t)T, &a.ref));
  PLDA_TRY(st.in(a.dur, (size_t)T, &a.dur));
  PLDA_TRY(st.in(a.tstart, (size_t)nt, &a.tstart));
  PLDA_TRY(st.in(a.tdur, (size_t)nt, &a.tdur));
  PLDA_TRY(st.in(a.tspk, (size_t)nt, &a.tspk));
  PLDA_TRY(st.in(a.sstart, (size_t)T, &a.sstart));
  PLDA_TRY(st.in(a.sdur, (size_t)T, &a.sdur));
  PLDA_TRY(st.in(a.hyp, (size_t)T, &a.hyp));
  PLDA_TRY(st.in(a.hyp2, (size_t)T, &a.hyp2));
  PLDA_TRY(st.in(a.ustart, (size_t)nu, &a.ustart));
  PLDA_TRY(st.in(a.udur, (size_t)nu, &a.udur));
  PLDA_TRY(st.in(a.ma, (size_t)(T - R), &a.ma));          // (all three may be NULL when no recording has a merge: T == R)
  PLDA_TRY(st.in(a.mb, (size_t)(T - R), &a.mb));
  PLDA_TRY(st.in(a.mc, (size_t)(T - R), &a.mc));
  PLDA_TRY(st.out(counts, (size_t)(sweep ? a.Q : 1) * R * 4, &a.counts));
  PLDA_TRY(st.out(ncl, (size_t)(sweep ? a.Q * R : 0), &a.n_clusters));
  PLDA_TRY(st.out(map, (size_t)R * PLDA_DER_MAX_REF, &a.map));
  long long *jer = a.jo.jer, *spk = a.jo.spk;               // (all three NULL outside the JER form)
  int *jmap = a.jo.jmap;
  PLDA_TRY(st.out(jer, (size_t)(sweep ? a.Q : 1) * R * 2, &a.jo.jer));
  PLDA_TRY(st.out(jmap, (size_t)R * PLDA_DER_MAX_REF, &a.jo.jmap));
  PLDA_TRY(st.out(spk, (size_t)R * PLDA_DER_MAX_REF * 3, &a.jo.spk));
  return st.finish(timed ? der_timed_device(h, fn, a, sweep) : der_seg_device(h, fn, a, sweep));
}
}  // namespace

int plda_der_plan(plda_handle *h, int64_t Sr, int64_t Sh, int32_t out[3]) {
  return entry(h, "plda_der_plan", [&] { return der_plan(h, Sr, Sh, out); });
}

int plda_der_dev(plda_handle *h, const int32_t *dref, const int32_t *dhyp, const int32_t *ddur, const int64_t *offsets, int64_t R,
                 int64_t *dcounts, int32_t *dmap) {
  return device_entry(h, "plda_der_dev", [&] {
    DerArgs a = der_seg_args(dref, ddur, offsets, R, dcounts);
    a.hyp = dhyp; a.map = dmap;
    return der_seg_device(h, "der", a, false);
  });
}

int plda_der(plda_handle *h, const int32_t *ref, const int32_t *hyp, const int32_t *dur, const int64_t *offsets, int64_t R,
             int64_t *counts, int32_t *map) {
  return entry(h, "plda_der", [&] {
    DerArgs a = der_seg_args(ref, dur, offsets, R, counts);
    a.hyp = hyp; a.map = map;
    return der_host(h, "der", a, false, false);
  });
}

int plda_der_sweep_dev(plda_handle *h, const int32_t *dmerge_a, const int32_t *dmerge_b, const double *dmerge_cost,
                       const int64_t *offsets, int64_t R, const int32_t *dref, const int32_t *ddur, const double *thresholds, int64_t Q,
                       const int32_t *min_clusters, int64_t *dcounts, int32_t *dn_clusters) {
  return device_entry(h, "plda_der_sweep_dev", [&] {
    DerArgs a = der_seg_args(dref, ddur, offsets, R, dcounts);
    der_sweep_args(a, dmerge_a, dmerge_b, dmerge_cost, thresholds, Q, min_clusters, dn_clusters);
    return der_seg_device(h, "der_sweep", a, true);
  });
}

int plda_der_sweep(plda_handle *h, const int32_t *merge_a, const int32_t *merge_b, const double *merge_cost, const int64_t *offsets,
                   int64_t R, const int32_t *ref, const int32_t *dur, const double *thresholds, int64_t Q, const int32_t *min_clusters,
                   int64_t *counts, int32_t *n_clusters) {
  return entry(h, "plda_der_sweep", [&] {
    DerArgs a = der_seg_args(ref, dur, offsets, R, counts);
    der_sweep_args(a, merge_a, merge_b, merge_cost, thresholds, Q, min_clusters, n_clusters);
    return der_host(h, "der_sweep", a, true, false);
  });
}

// ---------------------------------------------------------------- time-based diarisation error rate (der_time.hip)
int plda_der_timed_plan(plda_handle *h, int64_t n_turns, int64_t n_seg, int64_t n_uem, int32_t collar, int32_t out[3]) {
  return entry(h, "plda_der_timed_plan", [&] { return der_timed_plan(h, n_turns, n_seg, n_uem, collar, out); });
}

int plda_der_timed_dev(plda_handle *h, const int32_t *dturn_start, const int32_t *dturn_dur, const int32_t *dturn_spk,
                       const int64_t *turn_off, const int32_t *dseg_start, const int32_t *dseg_dur, const int32_t *dhyp,
                       const int64_t *offsets, int64_t R, const int32_t *duem_start, const int32_t *duem_dur, const int64_t *uem_off,
                       int32_t collar, int32_t flags, int64_t *dcounts, int32_t *dmap) {
  return device_entry(h, "plda_der_timed_dev", [&] {
    DerArgs a = der_timed_args(dturn_start, dturn_dur, dturn_spk, turn_off, dseg_start, dseg_dur, offsets, R, duem_start, duem_dur, uem_off,
                               collar, flags, dcounts);
    a.hyp = dhyp; a.map = dmap;
    return der_timed_device(h, "der_timed", a, false);
  });
}

int plda_der_timed(plda_handle *h, const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                   const int32_t *seg_start, const int32_t *seg_dur, const int32_t *hyp, const int64_t *offsets, int64_t R,
                   const int32_t *uem_start, const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags,
                   int64_t *counts, int32_t *map) {
  return entry(h, "plda_der_timed", [&] {
    DerArgs a = der_timed_args(turn_start, turn_dur, turn_spk, turn_off, seg_start, seg_dur, offsets, R, uem_start, uem_dur, uem_off, collar,
                               flags, counts);
    a.hyp = hyp; a.map = map;
    return der_host(h, "der_timed", a, false, true);
  });
}

int plda_der_timed_ovl_dev(plda_handle *h, const int32_t *dturn_start, const int32_t *dturn_dur, const int32_t *dturn_spk,
                           const int64_t *turn_off, const int32_t *dseg_start, const int32_t *dseg_dur, const int32_t *dhyp,
                           const int32_t *dhyp2, const int64_t *offsets, int64_t R, const int32_t *duem_start, const int32_t *duem_dur,
                           const int64_t *uem_off, int32_t collar, int32_t flags, int64_t *dcounts, int32_t *dmap) {
  return device_entry(h, "plda_der_timed_ovl_dev", [&] {
    DerArgs a = der_timed_args(dturn_start, dturn_dur, dturn_spk, turn_off, dseg_start, dseg_dur, offsets, R, duem_start, duem_dur, uem_off,
                               collar, flags, dcounts);
    a.hyp = dhyp; a.hyp2 = dhyp2; a.map = dmap;
    return der_timed_device(h, "der_timed_ovl", a, false);
  });
}

int plda_der_timed_ovl(plda_handle *h, const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                       const int32_t *seg_start, const int32_t *seg_dur, const int32_t *hyp, const int32_t *hyp2, const int64_t *offsets,
                       int64_t R, const int32_t *uem_start, const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags,
                       int64_t *counts, int32_t *map) {
  return entry(h, "plda_der_timed_ovl", [&] {
    DerArgs a = der_timed_args(turn_start, turn_dur, turn_spk, turn_off, seg_start, seg_dur, offsets, R, uem_start, uem_dur, uem_off, collar,
                               flags, counts);
    a.hyp = hyp; a.hyp2 = hyp2; a.map = map;
    return der_host(h, "der_timed_ovl", a, false, true);
  });
}

int plda_der_timed_sweep_dev(plda_handle *h, const int32_t *dmerge_a, const int32_t *dmerge_b, const double *dmerge_cost,
                             const int32_t *dturn_start, const int32_t *dturn_dur, const int32_t *dturn_spk, const int64_t *turn_off,
                             const int32_t *dseg_start, const int32_t *dseg_dur, const int64_t *offsets, int64_t R,
                             const int32_t *duem_start, const int32_t *duem_dur, const int64_t *uem_off, int32_t collar, int32_t flags,
                             const double *thresholds, int64_t Q, const int32_t *min_clusters, int64_t *dcounts, int32_t *dn_clusters) {
  return device_entry(h, "plda_der_timed_sweep_dev", [&] {
    DerArgs a = der_timed_args(dturn_start, dturn_dur, dturn_spk, turn_off, dseg_start, dseg_dur, offsets, R, duem_start, duem_dur, uem_off,
                               collar, flags, dcounts);
    der_sweep_args(a, dmerge_a, dmerge_b, dmerge_cost, thresholds, Q, min_clusters, dn_clusters);
    return der_timed_device(h, "der_timed_sweep", a, true);
  });
}

int plda_der_timed_sweep(plda_handle *h, const int32_t *merge_a, const int32_t *merge_b, const double *merge_cost,
                         const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                         const int32_t *seg_start, const int32_t *seg_dur, const int64_t *offsets, int64_t R, const int32_t *uem_start,
                         const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags, const double *thresholds,
                         int64_t Q, const int32_t *min_clusters, int64_t *counts, int32_t *n_clusters) {
  return entry(h, "plda_der_timed_sweep", [&] {
    DerArgs a = der_timed_args(turn_start, turn_dur, turn_spk, turn_off, seg_start, seg_dur, offsets, R, uem_start, uem_dur, uem_off, collar,
                               flags, counts);
    der_sweep_args(a, merge_a, merge_b, merge_cost, thresholds, Q, min_clusters, n_clusters);
    return der_host(h, "der_timed_sweep", a, true, true);
  });
}

// ---------------------------------------------------------------- Jaccard error rate (der.hip's JER form)
int plda_der_jer_plan(plda_handle *h, int64_t Sr, int64_t Sh, int32_t out[3]) {
  return entry(h, "plda_der_jer_plan", [&] { return der_jer_plan(h, Sr, Sh, out); });
}

int plda_der_jer_dev(plda_handle *h, const int32_t *dref, const int32_t *dhyp, const int32_t *ddur, const int64_t *offsets, int64_t R,
                     int64_t *dcounts, int32_t *dmap, int64_t *djer, int32_t *djmap, int64_t *dspk) {
  return device_entry(h, "plda_der_jer_dev", [&] {
    DerArgs a = der_seg_args(dref, ddur, offsets, R, dcounts);
    a.hyp = dhyp; a.map = dmap;
    der_jer_args(a, djer, djmap, dspk);
    return der_seg_device(h, "der_jer", a, false);
  });
}

int plda_der_jer(plda_handle *h, const int32_t *ref, const int32_t *hyp, const int32_t *dur, const int64_t *offsets, int64_t R,
                 int64_t *counts, int32_t *map, int64_t *jer, int32_t *jmap, int64_t *spk) {
  return entry(h, "plda_der_jer", [&] {
    DerArgs a = der_seg_args(ref, dur, offsets, R, counts);
    a.hyp = hyp; a.map = map;
    der_jer_args(a, jer, jmap, spk);
    return der_host(h, "der_jer", a, false, false);
  });
}

int plda_der_jer_sweep_dev(plda_handle *h, const int32_t *dmerge_a, const int32_t *dmerge_b, const double *dmerge_cost,
                           const int64_t *offsets, int64_t R, const int32_t *dref, const int32_t *ddur, const double *thresholds,
                           int64_t Q, const int32_t *min_clusters, int64_t *dcounts, int32_t *dn_clusters, int64_t *djer) {
  return device_entry(h, "plda_der_jer_sweep_dev", [&] {
    DerArgs a = der_seg_args(dref, ddur, offsets, R, dcounts);
    der_sweep_args(a, dmerge_a, dmerge_b, dmerge_cost, thresholds, Q, min_clusters, dn_clusters);
    der_jer_args(a, djer);
    return der_seg_device(h, "der_jer_sweep", a, true);
  });
}

int plda_der_jer_sweep(plda_handle *h, const int32_t *merge_a, const int32_t *merge_b, const double *merge_cost, const int64_t *offsets,
                       int64_t R, const int32_t *ref, const int32_t *dur, const double *thresholds, int64_t Q,
                       const int32_t *min_clusters, int64_t *counts, int32_t *n_clusters, int64_t *jer) {
  return entry(h, "plda_der_jer_sweep", [&] {
    DerArgs a = der_seg_args(ref, dur, offsets, R, counts);
    der_sweep_args(a, merge_a, merge_b, merge_cost, thresholds, Q, min_clusters, n_clusters);
    der_jer_args(a, jer);
    return der_host(h, "der_jer_sweep", a, true, false);
  });
}

int plda_der_timed_jer_dev(plda_handle *h, const int32_t *dturn_start, const int32_t *dturn_dur, const int32_t *dturn_spk,
                           const int64_t *turn_off, const int32_t *dseg_start, const int32_t *dseg_dur, const int32_t *dhyp,
                           const int32_t *dhyp2, const int64_t *offsets, int64_t R, const int32_t *duem_start, const int32_t *duem_dur,
                           const int64_t *uem_off, int32_t collar, int32_t flags, int64_t *dcounts, int32_t *dmap, int64_t *djer,
                           int32_t *djmap, int64_t *dspk) {
  return device_entry(h, "plda_der_timed_jer_dev", [&] {
    DerArgs a = der_timed_args(dturn_start, dturn_dur, dturn_spk, turn_off, dseg_start, dseg_dur, offsets, R, duem_start, duem_dur, uem_off,
                               collar, flags, dcounts);
    a.hyp = dhyp; a.hyp2 = dhyp2; a.map = dmap;
    der_jer_args(a, djer, djmap, dspk);
    return der_timed_device(h, "der_timed_jer", a, false);
  });
}

int plda_der_timed_jer(plda_handle *h, const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                       const int32_t *seg_start, const int32_t *seg_dur, const int32_t *hyp, const int32_t *hyp2, const int64_t *offsets,
                       int64_t R, const int32_t *uem_start, const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags,
                       int64_t *counts, int32_t *map, int64_t *jer, int32_t *jmap, int64_t *spk) {
  return entry(h, "plda_der_timed_jer", [&] {
    DerArgs a = der_timed_args(turn_start, turn_dur, turn_spk, turn_off, seg_start, seg_dur, offsets, R, uem_start, uem_dur, uem_off, collar,
                               flags, counts);
    a.hyp = hyp; a.hyp2 = hyp2; a.map = map;
    der_jer_args(a, jer, jmap, spk);
    return der_host(h, "der_timed_jer", a, false, true);
  });
}

int plda_der_timed_jer_sweep_dev(plda_handle *h, const int32_t *dmerge_a, const int32_t *dmerge_b, const double *dmerge_cost,
                                 const int32_t *dturn_start, const int32_t *dturn_dur, const int32_t *dturn_spk, const int64_t *turn_off,
                                 const int32_t *dseg_start, const int32_t *dseg_dur, const int64_t *offsets, int64_t R,
                                 const int32_t *duem_start, const int32_t *duem_dur, const int64_t *uem_off, int32_t collar,
                                 int32_t flags, const double *thresholds, int64_t Q, const int32_t *min_clusters, int64_t *dcounts,
                                 int32_t *dn_clusters, int64_t *djer) {
  return device_entry(h, "plda_der_timed_jer_sweep_dev", [&] {
    DerArgs a = der_timed_args(dturn_start, dturn_dur, dturn_spk, turn_off, dseg_start, dseg_dur, offsets, R, duem_start, duem_dur, uem_off,
                               collar, flags, dcounts);
    der_sweep_args(a, dmerge_a, dmerge_b, dmerge_cost, thresholds, Q, min_clusters, dn_clusters);
    der_jer_args(a, djer);
    return der_timed_device(h, "der_timed_jer_sweep", a, true);
  });
}

int plda_der_timed_jer_sweep(plda_handle *h, const int32_t *merge_a, const int32_t *merge_b, const double *merge_cost,
                             const int32_t *turn_start, const int32_t *turn_dur, const int32_t *turn_spk, const int64_t *turn_off,
                             const int32_t *seg_start, const int32_t *seg_dur, const int64_t *offsets, int64_t R,
                             const int32_t *uem_start, const int32_t *uem_dur, const int64_t *uem_off, int32_t collar, int32_t flags,
                             const double *thresholds, int64_t Q, const int32_t *min_clusters, int64_t *counts, int32_t *n_clusters,
                             int64_t *jer) {
  return entry(h, "plda_der_timed_jer_sweep", [&] {
    DerArgs a = der_timed_args(turn_start, turn_dur, turn_spk, turn_off, seg_start, seg_dur, offsets, R, uem_start, uem_dur, uem_off, collar,
                               flags, counts);
    der_sweep_args(a, merge_a, merge_b, merge_cost, thresholds, Q, min_clusters, n_clusters);
    der_jer_args(a, jer);
    return der_host(h, "der_timed_jer_sweep", a, true, true);
  });
}

// ---------------------------------------------------------------- VBx resegmentation (vbx.hip)
int plda_vbx_plan(plda_handle *h, int64_t T, int64_t S, int64_t D, int32_t out[3]) {
  return entry(h, "plda_vbx_plan", [&] { return vbx_plan(h, T, S, D, out); });
}

int plda_vbx_dev(plda_handle *h, const double *dY, int64_t D, const double *dPhi, const int32_t *dlabels_in, const int64_t *offsets,
                 int64_t R, double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon,
                 int32_t *dlabels, int32_t *dn_clusters, double *dgamma, const int64_t *gamma_off, double *dpi, const int64_t *pi_off,
                 double *delbo, int32_t *diters) {
  return device_entry(h, "plda_vbx_dev", [&] {
    return vbx_device(h, dY, D, dPhi, dlabels_in, offsets, R, Fa, Fb, loop_prob, init_smoothing, max_iters, epsilon, dlabels,
                      dn_clusters, dgamma, gamma_off, dpi, pi_off, delbo, diters);
  });
}

int plda_vbx_top2_dev(plda_handle *h, const double *dY, int64_t D, const double *dPhi, const int32_t *dlabels_in, const int64_t *offsets,
                      int64_t R, double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon,
                      int32_t *dlabels, int32_t *dn_clusters, double *dgamma, const int64_t *gamma_off, double *dpi, const int64_t *pi_off,
                      double *delbo, int32_t *diters, int32_t *dlabels2, double *dpost2) {
  return device_entry(h, "plda_vbx_top2_dev", [&] {
    return vbx_device(h, dY, D, dPhi, dlabels_in, offsets, R, Fa, Fb, loop_prob, init_smoothing, max_iters, epsilon, dlabels,
                      dn_clusters, dgamma, gamma_off, dpi, pi_off, delbo, diters, dlabels2, dpost2);
  });
}

namespace {
// the host form of plda_vbx and plda_vbx_top2 (labels2 and post2 NULL in the former)
int vbx_host(plda_handle *h, const double *Y, int64_t D, const double *Phi, const int32_t *labels_in, const int64_t *offsets, int64_t R,
             double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon, int32_t *labels,
             int32_t *n_clusters, double *gamma, const int64_t *gamma_off, double *pi, const int64_t *pi_off, double *elbo,
             int32_t *iters, int32_t *labels2, double *post2) {
  if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "vbx: model not fitted");
  if (!Y) return fail(h, PLDA_E_INVAL, "vbx: Y is NULL");
  if (!labels_in) return fail(h, PLDA_E_INVAL, "vbx: labels_in is NULL");
  PLDA_TRY(vbx_validate(h, "vbx", D, offsets, R, Fa, Fb, loop_prob, max_iters, labels, n_clusters, gamma, gamma_off, pi, pi_off));
  PLDA_TRY(set_device(h));
  const int64_t T = offsets[R];
  // the intervals of gamma and pi keep their layout, relative to their first entry, in device temporaries
  const int64_t g0 = gamma ? gamma_off[0] : 0, gn = gamma ? gamma_off[R] - g0 : 0;
  const int64_t p0 = pi ? pi_off[0] : 0, pn = pi ? pi_off[R] - p0 : 0;
  if (gn < 0 || pn < 0) return fail(h, PLDA_E_INVAL, "vbx: gamma_off / pi_off must ascend");
  std::vector<int64_t> grel, prel;
  if (gamma) { grel.resize((size_t)R + 1); for (int64_t r = 0; r <= R; ++r) grel[(size_t)r] = gamma_off[r] - g0; }
  if (pi) { prel.resize((size_t)R + 1); for (int64_t r = 0; r <= R; ++r) prel[(size_t)r] = pi_off[r] - p0; }
  Staged st(h);
  const double *dY, *dPhi;
  const int32_t *dLin;
  Tmp dL, dK, dG, dP, dE, dI, dL2, dP2;
  PLDA_TRY(st.in(Y, (size_t)T * D, &dY));
  PLDA_TRY(st.in(Phi, (size_t)D, &dPhi));
  PLDA_TRY(st.in(labels_in, (size_t)T, &dLin));
  PLDA_HIP(h, dL.alloc((size_t)T * 4));
  PLDA_HIP(h, dK.alloc((size_t)R * 4));
  if (gamma) PLDA_HIP(h, dG.alloc((size_t)gn * 8));
  if (pi) PLDA_HIP(h, dP.alloc((size_t)pn * 8));
  if (elbo) PLDA_HIP(h, dE.alloc((size_t)R * max_iters * 8));
  if (iters) PLDA_HIP(h, dI.alloc((size_t)R * 4));
  if (labels2) PLDA_HIP(h, dL2.alloc((size_t)T * 4));
  if (post2) PLDA_HIP(h, dP2.alloc((size_t)T * 8));
  const int rc = vbx_device(h, dY, D, dPhi, dLin, offsets, R, Fa, Fb, loop_prob,
                            init_smoothing, max_iters, epsilon, dL.as<int32_t>(), dK.as<int32_t>(), gamma ? dG.as<double>() : nullptr,
                            gamma ? grel.data() : nullptr, pi ? dP.as<double>() : nullptr, pi ? prel.data() : nullptr,
                            elbo ? dE.as<double>() : nullptr, iters ? dI.as<int32_t>() : nullptr,
                            labels2 ? dL2.as<int32_t>() : nullptr, post2 ? dP2.as<double>() : nullptr);
  if (rc != PLDA_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
  // gamma and pi: only T_r x S_r (S_r) entries of every interval are the call's to write
  std::vector<int32_t> hl((size_t)T);
  std::vector<double> hg((size_t)gn), hp((size_t)pn);
  PLDA_HIP(h, hipMemcpyAsync(labels, dL.p, (size_t)T * 4, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipMemcpyAsync(n_clusters, dK.p, (size_t)R * 4, hipMemcpyDeviceToHost, h->stream));
  if (gn) PLDA_HIP(h, hipMemcpyAsync(hg.data(), dG.p, (size_t)gn * 8, hipMemcpyDeviceToHost, h->stream));
  if (pn) PLDA_HIP(h, hipMemcpyAsync(hp.data(), dP.p, (size_t)pn * 8, hipMemcpyDeviceToHost, h->stream));
  if (elbo) PLDA_HIP(h, hipMemcpyAsync(elbo, dE.p, (size_t)R * max_iters * 8, hipMemcpyDeviceToHost, h->stream));
  if (iters) PLDA_HIP(h, hipMemcpyAsync(iters, dI.p, (size_t)R * 4, hipMemcpyDeviceToHost, h->stream));
  if (labels2) PLDA_HIP(h, hipMemcpyAsync(labels2, dL2.p, (size_t)T * 4, hipMemcpyDeviceToHost, h->stream));
  if (post2) PLDA_HIP(h, hipMemcpyAsync(post2, dP2.p, (size_t)T * 8, hipMemcpyDeviceToHost, h->stream));
  PLDA_HIP(h, hipStreamSynchronize(h->stream));
  for (int64_t r = 0; r < R && (gamma || pi); ++r) {
    int S = 0;
    for (int64_t t = offsets[r]; t < offsets[r + 1]; ++t) S = std::max(S, (int)labels_in[t] + 1);
    const int64_t n = offsets[r + 1] - offsets[r];
    if (gamma) std::copy(hg.begin() + grel[(size_t)r], hg.begin() + grel[(size_t)r] + n * S, gamma + gamma_off[r]);
    if (pi) std::copy(hp.begin() + prel[(size_t)r], hp.begin() + prel[(size_t)r] + S, pi + pi_off[r]);
  }
  return PLDA_OK;
}
}  // namespace

int plda_vbx(plda_handle *h, const double *Y, int64_t D, const double *Phi, const int32_t *labels_in, const int64_t *offsets, int64_t R,
             double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon, int32_t *labels,
             int32_t *n_clusters, double *gamma, const int64_t *gamma_off, double *pi, const int64_t *pi_off, double *elbo,
             int32_t *iters) {
  return entry(h, "plda_vbx", [&] {
    return vbx_host(h, Y, D, Phi, labels_in, offsets, R, Fa, Fb, loop_prob, init_smoothing, max_iters, epsilon, labels, n_clusters, gamma,
                    gamma_off, pi, pi_off, elbo, iters, nullptr, nullptr);
  });
}

int plda_vbx_top2(plda_handle *h, const double *Y, int64_t D, const double *Phi, const int32_t *labels_in, const int64_t *offsets,
                  int64_t R, double Fa, double Fb, double loop_prob, double init_smoothing, int64_t max_iters, double epsilon,
                  int32_t *labels, int32_t *n_clusters, double *gamma, const int64_t *gamma_off, double *pi, const int64_t *pi_off,
                  double *elbo, int32_t *iters, int32_t *labels2, double *post2) {
  return entry(h, "plda_vbx_top2", [&] {
    return vbx_host(h, Y, D, Phi, labels_in, offsets, R, Fa, Fb, loop_prob, init_smoothing, max_iters, epsilon, labels, n_clusters, gamma,
                    gamma_off, pi, pi_off, elbo, iters, labels2, post2);
  });
}

int plda_project_rows_dev(plda_handle *h, const double *dX, int64_t R, int32_t Din, double *dout) {
  return device_entry(h, "plda_project_rows_dev", [&] { return project_rows_device(h, dX, R, Din, dout); });
}

int plda_project_rows(plda_handle *h, const double *X, int64_t R, int32_t Din, double *out) {
  return entry(h, "plda_project_rows", [&]() -> int {
    if (!h->fitted) return fail(h, PLDA_E_NOT_FITTED, "project_rows: model not fitted");
    if (Din != h->Din) return fail(h, PLDA_E_INVAL, "project_rows: feature dim %d != model dim %d", (int)Din, h->Din);
    if (R <= 0) return R < 0 ? fail(h, PLDA_E_INVAL, "project_rows: R = %lld", (long long)R) : PLDA_OK;
    if (!X || !out) return fail(h, PLDA_E_INVAL, "project_rows: bad argument");
    PLDA_TRY(set_device(h));
    Staged st(h);
    const double *dX;
    double *dO;
    PLDA_TRY(st.in(X, (size_t)R * Din, &dX));
    PLDA_TRY(st.out(out, (size_t)R * h->Dout, &dO, true));
    return st.finish(project_rows_device(h, dX, R, Din, dO));
  });
}

// ---------------------------------------------------------------- embedding chain (embed.hip)
int plda_embed_set(plda_handle *h, int32_t Din, int32_t Dout, const double *m_in, double len_in, const double *A, const double *m_out,
                   double len_out) {
  return device_entry(h, "plda_embed_set", [&] { return embed_set(h, Din, Dout, m_in, len_in, A, m_out, len_out); });
}

int plda_embed_clear(plda_handle *h) {
  return entry(h, "plda_embed_clear", [&] { return embed_clear(h); });
}

int plda_embed_dims(plda_handle *h, int32_t *Din, int32_t *Dout, int32_t *flags) {
  return entry(h, "plda_embed_dims", [&]() -> int {
    if (!h->em_has) return fail(h, PLDA_E_NOT_FITTED, "embed_dims: no embedding chain is set");
    if (Din) *Din = h->em_Din;
    if (Dout) *Dout = h->em_Dout;
    if (flags) *flags = (h->em_has_min ? 1 : 0) | (h->em_has_A ? 2 : 0) | (h->em_has_mout ? 4 : 0);
    return PLDA_OK;
  });
}

int plda_embed_get(plda_handle *h, double *m_in, double *len_in, double *A, double *m_out, double *len_out) {
  return entry(h, "plda_embed_get", [&]() -> int {
    if (!h->em_has) return fail(h, PLDA_E_NOT_FITTED, "embed_get: no embedding chain is set");
    if (m_in && h->em_has_min) std::memcpy(m_in, h->em_h_min.data(), h->em_h_min.size() * 8);
    if (A && h->em_has_A) std::memcpy(A, h->em_h_A.data(), h->em_h_A.size() * 8);
    if (m_out && h->em_has_mout) std::memcpy(m_out, h->em_h_mout.data(), h->em_h_mout.size() * 8);
    if (len_in) *len_in = h->em_len_in;
    if (len_out) *len_out = h->em_len_out;
    return PLDA_OK;
  });
}

int plda_embed_plan(plda_handle *h, int32_t Din, int32_t Dout, int32_t has_A, int32_t dtype, int32_t out[3]) {
  return entry(h, "plda_embed_plan", [&] { return embed_plan(h, Din, Dout, has_A, dtype, out); });
}

int plda_embed_apply_dev(plda_handle *h, const void *dX, int32_t dtype, int64_t R, int32_t Din, double *dout) {
  return device_entry(h, "plda_embed_apply_dev", [&] { return embed_apply_device(h, dX, dtype, R, Din, dout); });
}

int plda_embed_apply(plda_handle *h, const void *X, int32_t dtype, int64_t R, int32_t Din, double *out) {
  return entry(h, "plda_embed_apply", [&]() -> int {
    if (!h->em_has) return fail(h, PLDA_E_NOT_FITTED, "embed_apply: no embedding chain is set");
    if (dtype != 0 && dtype != 1) return fail(h, PLDA_E_INVAL, "embed_apply: dtype %d (0 fp64, 1 fp32)", (int)dtype);
    if (Din != h->em_Din) return fail(h, PLDA_E_INVAL, "embed_apply: feature dim %d != the chain's input dim %d", (int)Din, h->em_Din);
    if (R <= 0) return PLDA_OK;
    if (!X || !out) return fail(h, PLDA_E_INVAL, "embed_apply: bad argument");
    PLDA_TRY(set_device(h));
    Staged st(h);
    const void *dX;
    double *dO;
    PLDA_TRY(st.in(X, (size_t)R * Din * (dtype == 1 ? 4 : 8), &dX));
    PLDA_TRY(st.out(out, (size_t)R * h->em_Dout, &dO, true));
    return st.finish(embed_apply_device(h, dX, dtype, R, Din, dO));
  });
}

int plda_embed_fit_dev(plda_handle *h, const void *dX, int32_t dtype, int64_t N, int32_t Din, const uint64_t *dlabels, int64_t K,
                       int32_t kind, int32_t Dout, double len_in, double len_out, double *eig) {
  return entry(h, "plda_embed_fit_dev", [&]() -> int {
    PLDA_TRY(embed_fit_validate(h, dtype, N, Din, dlabels != nullptr, K, kind, Dout, len_in, len_out));
    PLDA_TRY(set_device(h));
    return embed_fit_device(h, dX, dtype, N, Din, dlabels, K, kind, Dout, len_in, len_out, eig);
  });
}

int plda_embed_fit(plda_handle *h, const void *X, int32_t dtype, int64_t N, int32_t Din, const uint64_t *labels, int32_t kind,
                   int32_t Dout, double len_in, double len_out, double *eig) {
  return entry(h, "plda_embed_fit", [&]() -> int {
    int64_t K = 0;
    if (labels && kind == 2 && N > 0 && N < ((int64_t)1 << 31)) {
      uint64_t mx = 0;
      for (int64_t i = 0; i < N; ++i) mx = std::max(mx, labels[i]);
      if (mx >= (uint64_t)N) return fail(h, PLDA_E_LABELS, "embed_fit: labels must be dense 0..K-1");
      K = (int64_t)mx + 1;
    }
    PLDA_TRY(embed_fit_validate(h, dtype, N, Din, labels != nullptr, K, kind, Dout, len_in, len_out));
    if (!X) return fail(h, PLDA_E_INVAL, "embed_fit: X is NULL");
    PLDA_TRY(set_device(h));
    Staged st(h);
    const void *dX;
    const uint64_t *dL;
    PLDA_TRY(st.in(X, (size_t)N * Din * (dtype == 1 ? 4 : 8), &dX));
    PLDA_TRY(st.in(kind == 2 ? labels : nullptr, (size_t)N, &dL));
    return embed_fit_device(h, dX, dtype, N, Din, dL, K, kind, Dout, len_in, len_out, eig);
  });
}

}  // extern "C"
