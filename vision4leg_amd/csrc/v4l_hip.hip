// libv4l_hip.so — plans, launch drivers and the C ABI (include/v4l_hip.h) of the gfx950 PPO hot path.
#include <math.h>
#include <stdarg.h>

#include <algorithm>
#include <type_traits>

#include <dlfcn.h>

#include "net.h"
#include "infer.h"
#include "bwd.h"
#include "wps.h"
#include "wps_fb.h"
#include "rollout_dense.h"
#include "dense_stack.h"
#include "host_step.h"

namespace v4l {

// ------------------------------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";
// The library's switches (include/v4l_hip.h lists them): every one is read through these two, at the call that uses it
static bool sw_on(const char* name) { return getenv(name) != nullptr; }
// Run f(TypeTag<T>) with T = the operand type of compute mode `compute` (float | __bf16 | _Float16); by_half: the 16-bit modes only
template <typename T> struct TypeTag { typedef T type; };
#ifdef V4L_DEV_ONLY  // development builds (tools/probe/build_variant.sh only=<mode>): ONE operand type instantiated, a third of the compile time
template <class F> static inline int by_compute(int compute, F&& f) {
  typedef std::conditional<V4L_DEV_ONLY == V4L_BF16, __bf16, std::conditional<V4L_DEV_ONLY == V4L_F16, _Float16, float>::type>::type T;
  if (compute != V4L_DEV_ONLY) { set_error("this development build only holds compute mode %d", V4L_DEV_ONLY); return -1; }
  return f(TypeTag<T>());
}
template <class F> static inline int by_half(int compute, F&& f) {
  typedef std::conditional<V4L_DEV_ONLY == V4L_F16, _Float16, __bf16>::type T;
  if (compute != V4L_DEV_ONLY) { set_error("this development build only holds compute mode %d", V4L_DEV_ONLY); return -1; }
  return f(TypeTag<T>());
}
#else
template <class F> static inline int by_compute(int compute, F&& f) {
  return compute == V4L_BF16 ? f(TypeTag<__bf16>()) : compute == V4L_F16 ? f(TypeTag<_Float16>()) : f(TypeTag<float>());
}
template <class F> static inline int by_half(int compute, F&& f) {
  return compute == V4L_F16 ? f(TypeTag<_Float16>()) : f(TypeTag<__bf16>());
}
#endif
static inline bool is_half(int compute) { return compute == V4L_BF16 || compute == V4L_F16; }
// the 16-bit operand type a kernel family that only exists for 16-bit operands is instantiated with from a function templated on T
template <typename T> struct HalfOf { typedef typename std::conditional<sizeof(T) == 2, T, __bf16>::type type; };
// The dynamic-LDS limit of kernel instance K, raised to `bytes` once per process (a function-local static: its initialisation is
// thread-safe). Every call returns the stored result, so a failure is reported through V4L_HIP_CHECK on every launch path.
template <auto K> static hipError_t lds_limit(size_t bytes) {
  static const hipError_t e =
      hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  return e;
}
static int sw_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static const bool g_trace = sw_on("V4L_TRACE");
#define V4L_TRACE(...) do { if (v4l::g_trace) { fprintf(stderr, "[v4l] " __VA_ARGS__); fputc('\n', stderr); fflush(stderr); } } while (0)
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_err; }


// ------------------------------------------------------------------------------------------ built-in profiler
// Optional per-launch timing with HIP events on the launch stream (v4l_prof_enable). Off: zero overhead beyond a
// branch. Records (phase/op label, kernel family, algorithmic FLOPs); v4l_prof_collect aggregates and clears.
struct ProfRec { std::string label; hipEvent_t e0, e1; double flops; };
static bool g_prof = false;
static std::vector<ProfRec> g_recs;
static thread_local const char* g_phase = "";
static thread_local const char* g_op = "";
// roctx ranges (V4L_ROCTX=1): every phase and every launch call is bracketed by roctxRangePushA / roctxRangePop, labelled
// phase|op|kernel like the built-in profiler's records, so `rocprofv3 --marker-trace --kernel-trace` lines the launches up with
// the library's own structure. The roctx library (rocprofiler-sdk's, else libroctx64) is opened with dlopen: no link-time
// dependency; absent library = switch ignored.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  bool on = false;
  Roctx() {
    const char* e = getenv("V4L_ROCTX");
    if (e == nullptr || atoi(e) == 0) return;
    void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);  // what rocprofv3 --marker-trace listens to
    if (h == nullptr) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);   // the roctracer-era library (rocprof v1 / v2)
    if (h == nullptr) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (h == nullptr) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    on = push != nullptr && pop != nullptr;
  }
};
static Roctx& roctx() { static Roctx r; return r; }
struct PhaseScope {
  const char* prev;
  bool ranged;
  explicit PhaseScope(const char* p) : prev(g_phase), ranged(roctx().on) {
    g_phase = p;
    if (ranged) (void)roctx().push(p);
  }
  ~PhaseScope() {
    if (ranged) (void)roctx().pop();
    g_phase = prev;
  }
};
struct ProfGuard {
  hipStream_t s;
  bool on;
  bool ranged;
  ProfGuard(const char* kname, double flops, hipStream_t st) : s(st), on(g_prof), ranged(roctx().on) {
    if (ranged) (void)roctx().push((std::string(g_phase) + "|" + g_op + "|" + kname).c_str());
    if (!on) return;
    ProfRec r;
    r.label = std::string(g_phase) + "|" + g_op + "|" + kname;
    r.flops = flops;
    (void)hipEventCreate(&r.e0);
    (void)hipEventCreate(&r.e1);
    (void)hipEventRecord(r.e0, s);
    g_recs.push_back(r);
  }
  ~ProfGuard() {
    if (on) (void)hipEventRecord(g_recs.back().e1, s);
    if (ranged) (void)roctx().pop();
  }
};
#define V4L_KLAUNCH(kname, flops, s, ...)            \
  do {                                               \
    v4l::ProfGuard _pg(kname, (double)(flops), s);   \
    hipLaunchKernelGGL(__VA_ARGS__);                 \
  } while (0)

// ------------------------------------------------------------------------------------------ launch helpers
static inline ADense dense(const float* p, int lda, int M, int K, const int* rowidx = nullptr, int tokmap = 0,
                           const float* mask = nullptr) {
  ADense a;
  memset(&a, 0, sizeof(a));  // descriptors are compared bytewise (cached device tables): no stray padding
  a.p = p; a.lda = lda; a.M = M; a.K = K; a.rowidx = rowidx; a.tokmap = tokmap; a.mask = mask;
  return a;
}
static inline Epi mk_epi(float* C, int ldc, int N, const float* bias = nullptr, int act = EPI_ACT_NONE) {
  Epi e;
  memset(&e, 0, sizeof(e));
  e.C = C; e.ldc = ldc; e.N = N; e.bias = bias; e.act = act;
  e.rowmap = ROWMAP_IDENT;
  return e;
}

static inline bool epi_wants_tanh(const Epi& ep) {
  return ep.act == EPI_ACT_TANH || (ep.mask != nullptr && ep.mask_mode == EPI_MASK_TANH);
}
// C = epi(A * Bp^T): Bp is a packed [Np][Kp] operand (Np % 16 == 0, Kp % 64 == 0)
template <typename T, class AL>
static int launch_nt(hipStream_t s, const AL& al, int M, const T* Bp, int Np, int Kp, Epi ep, double flops) {
  if (M <= 0) return 0;
  ep.M = M;
  const int gx = cdiv(M, 128);
  if (epi_wants_tanh(ep)) {  // the kernels' TANH instantiations (csrc/gemm.h epi_activate): dense layers only
    if constexpr (std::is_same<AL, ADense>::value) {
      if (Np % 64 == 0) {
        V4L_KLAUNCH("gemm_nt", flops, s, (gemm_nt_kernel<T, 64, AL, true>), dim3(gx, Np / 64), dim3(256), 0, s, al, Bp, Kp, ep);
      } else if (Np % 32 == 0) {
        V4L_KLAUNCH("gemm_nt", flops, s, (gemm_nt_kernel<T, 32, AL, true>), dim3(gx, Np / 32), dim3(256), 0, s, al, Bp, Kp, ep);
      } else {
        V4L_KLAUNCH("gemm_nt", flops, s, (gemm_nt_kernel<T, 16, AL, true>), dim3(gx, Np / 16), dim3(256), 0, s, al, Bp, Kp, ep);
      }
      V4L_LAUNCH_CHECK();
      return 0;
    }
    V4L_REQUIRE(false, "internal: a Tanh epilogue on a GEMM that is not a dense layer");
  }
  if (Np % 64 == 0) {
    V4L_KLAUNCH("gemm_nt", flops, s, (gemm_nt_kernel<T, 64, AL>), dim3(gx, Np / 64), dim3(256), 0, s, al, Bp, Kp, ep);
  } else if (Np % 32 == 0) {
    V4L_KLAUNCH("gemm_nt", flops, s, (gemm_nt_kernel<T, 32, AL>), dim3(gx, Np / 32), dim3(256), 0, s, al, Bp, Kp, ep);
  } else {
    V4L_KLAUNCH("gemm_nt", flops, s, (gemm_nt_kernel<T, 16, AL>), dim3(gx, Np / 16), dim3(256), 0, s, al, Bp, Kp, ep);
  }
  V4L_LAUNCH_CHECK();
  return 0;
}

// ROCm 7.2: ending a capture that contains this library's fork/join pattern crashes inside hipStreamEndCapture
// (a stand-alone reproduction of the pattern does not — tools/probe/capture_fork.hip), so the aux stream is used
// for eager launches only; captured sequences stay on one stream.
static inline bool capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (s == nullptr || hipStreamIsCapturing(s, &st) != hipSuccess) return false;
  return st != hipStreamCaptureStatusNone;
}
// Weight-grad plan: tile shape, split count over the reduction (m) and slab geometry.
struct TnPlan { int BN, KT, gx, gy, splits, mpb, Npad, Kpad; int64_t slab_floats, bslab_floats; };
static inline TnPlan tn_plan(int M, int N, int Kx, bool bf16) {
  TnPlan p;
  p.BN = N <= 16 ? 16 : (N <= 32 ? 32 : 64);
  // wider k tiles amortise the staged Y rows over more MFMAs; the f32 operand tile of KT=4 would not fit the
  // 64 KiB static LDS budget
  p.KT = (Kx >= 256 && bf16 && M >= 4096) ? 4 : (Kx >= 128 ? 2 : 1);
  p.gy = cdiv(N, p.BN);
  p.gx = cdiv(Kx, 64 * p.KT);
  // these kernels are latency-bound chains (rowidx -> operand rows -> LDS -> MFMA per stage): many short blocks keep
  // more independent chains in flight per CU than few long ones
  int splits = std::max(1, 1024 / (p.gx * p.gy));
  splits = std::min(splits, std::max(1, M / 256));
  p.mpb = round_up(cdiv(M, splits), 64);
  p.splits = cdiv(M, p.mpb);
  p.Npad = p.gy * p.BN;
  p.Kpad = p.gx * 64 * p.KT;
  p.slab_floats = ((int64_t)p.splits * p.Npad * p.Kpad + 63) / 64 * 64;
  p.bslab_floats = ((int64_t)p.splits * p.Npad + 63) / 64 * 64;
  return p;
}

struct Ctx {  // per-call view of a bound net
  v4l_net* net;
  hipStream_t s;
  float* grads;
  float* slab;         // arena for weight-grad partials (inside the workspace)
  int64_t slab_used;
  hipStream_t tn;      // stream weight-grad kernels go to: s, or the net's aux stream inside par_begin/par_end
  // dW3's launch can be held back by conv_stack_bwd_fused and issued by the caller (next to the dense weight-grads)
  bool defer_conv3 = false, conv3_pending = false, conv3_a16 = false, conv3_tr = false;
  v4l::BwdConv conv3_args = {};
  int conv3_blocks = 0, conv3_n = 0;
  // the wave-per-sample layers' weight-grad launch (csrc/wps.h), issued with the other dense weight-grads
  bool wps_pending = false;
  bool wps_used = false;     // this backward pass runs the wave-per-sample layer kernels (stays set: sizes the dW3 launch)
  v4l::WpsWg wps_args = {};
  // the fused forward-loss-backward launch (csrc/wps_fb.h) left per-block partial statistics: fb_loss_finish_kernel, issued
  // with the dense weight-grads (auxiliary stream)
  bool fb_pending = false;
  v4l::FbLoss fb_args = {};
  int fb_blocks = 0, fb_n = 0;
  bool taps = false;  // LayerRoute::taps of the pass: bwd_conv_kernel writes dc2 / dc1 out too
};

// Fork/join of the net's auxiliary stream. Independent sibling kernels (a layer's weight-grad next to its data-grad,
// the proprio MLP next to the conv stack) run concurrently: most kernels of this workload fill only a fraction of
// the 256 CUs. Under stream capture the event record/wait pairs become plain graph dependencies.
static int par_begin(Ctx& c, bool in_capture_too = false) {
  v4l_net* n = c.net;
  if (n->aux == nullptr || (capturing(c.s) && !in_capture_too)) return 0;
  V4L_TRACE("par_begin net=%p s=%p aux=%p", (void*)n, (void*)c.s, (void*)n->aux);
  V4L_HIP_CHECK(hipEventRecord(n->ev_fork, c.s));
  V4L_HIP_CHECK(hipStreamWaitEvent(n->aux, n->ev_fork, 0));
  c.tn = n->aux;
  return 0;
}
static int par_end(Ctx& c) {
  v4l_net* n = c.net;
  if (n->aux == nullptr || c.tn == c.s) return 0;
  V4L_TRACE("par_end net=%p", (void*)n);
  V4L_HIP_CHECK(hipEventRecord(n->ev_join, n->aux));
  V4L_HIP_CHECK(hipStreamWaitEvent(c.s, n->ev_join, 0));
  c.tn = c.s;
  return 0;
}

// partial[z] = Y^T X over slab z of the rows; registers a reduce descriptor that wgrad_finish() executes
template <typename T, class YL, class XL>
static int launch_tn(Ctx& c, const YL& yl, const XL& xl, int M, int N, int Kx, RedDesc rd, double flops) {
  if (M <= 0) return 0;
  const TnPlan p = tn_plan(M, N, Kx, sizeof(T) == 2);
  float* slab = c.slab + c.slab_used;
  float* bslab = rd.db != nullptr ? slab + p.slab_floats : nullptr;
  c.slab_used += p.slab_floats + (rd.db != nullptr ? p.bslab_floats : 0);
  V4L_REQUIRE(c.slab_used <= c.net->slab_cap, "internal: weight-grad slab arena overflow");
  const dim3 grid(p.gx, p.gy, p.splits);
  hipStream_t s = c.tn;
#define V4L_TN(BN_, KT_) \
  V4L_KLAUNCH("gemm_tn", flops, s, (gemm_tn_kernel<T, BN_, KT_, YL, XL>), grid, dim3(256), 0, s, yl, xl, M, p.mpb, slab, bslab, p.Npad, p.Kpad)
  if constexpr (sizeof(T) == 2) {
    if (p.KT == 4) {
      if (p.BN == 64) V4L_TN(64, 4); else if (p.BN == 32) V4L_TN(32, 4); else V4L_TN(16, 4);
    }
  }
  if (p.KT == 2) { if (p.BN == 64) V4L_TN(64, 2); else if (p.BN == 32) V4L_TN(32, 2); else V4L_TN(16, 2); }
  else if (p.KT == 1) { if (p.BN == 64) V4L_TN(64, 1); else if (p.BN == 32) V4L_TN(32, 1); else V4L_TN(16, 1); }
#undef V4L_TN
  V4L_LAUNCH_CHECK();
  rd.slab = slab; rd.bslab = bslab; rd.nsplit = p.splits; rd.Npad = p.Npad; rd.Kpad = p.Kpad;
  c.net->red.push_back(rd);
  return 0;
}

// one launch: sum all registered slabs into the PyTorch-layout gradients
template <typename T> static int wgrad_dense(Ctx& c, hipStream_t ds, hipStream_t dg = nullptr);
template <typename T> static int wgrad_reduce_all(Ctx& c);
template <typename T>
static int wgrad_finish(Ctx& c) {
  int rc = wgrad_dense<T>(c, c.s);
  return rc ? rc : wgrad_reduce_all<T>(c);
}
// The statistics of a fused forward-loss-backward launch (csrc/wps_fb.h): one block, off the chain of the big launches — only
// clip_adam and the record's readers wait for it
static int fb_finish(Ctx& c, hipStream_t s) {
  if (!c.fb_pending) return 0;
  c.fb_pending = false;
  V4L_HIP_CHECK(lds_limit<&fb_loss_finish_kernel>(FbFinishLds::bytes));
  g_op = "loss";
  V4L_KLAUNCH("fb_loss_finish", 0, s, fb_loss_finish_kernel, dim3(1), dim3(256), FbFinishLds::bytes, s, c.fb_args, c.fb_blocks, c.fb_n);
  V4L_LAUNCH_CHECK();
  return 0;
}
// the deferred dense weight-grad launches (grouped + whole-output kernels) on stream ds: ONE launch when both kinds are
// present (gemm_tn_dense_kernel hosts both kinds of blocks; V4L_SPLIT_DENSE_WGRAD=1: one launch per kind)
// dg: stream of the grouped / whole-output launches when they run as a branch of their own (default: ds, after wps_wgrad)
template <typename T>
static int wgrad_dense(Ctx& c, hipStream_t ds, hipStream_t dg) {
  v4l_net* net = c.net;
  if (dg == nullptr) dg = ds;
  if (int rc = fb_finish(c, ds)) return rc;  // (schedules without a shorter branch to put it on)
  if (c.wps_pending) {
    c.wps_pending = false;
    const int jobs = c.wps_args.nsplit * WPS_ROLES * c.wps_args.nlayers;
    c.wps_args.wg_blocks = cdiv(jobs, 4);
    const int chain = c.wps_args.chain_blocks;
    // (the proprio chain's consumer — the grouped weight-grads below — must follow on the SAME stream)
    V4L_REQUIRE(chain == 0 || dg == ds, "internal: proprio chain in the weight-grad launch, but the grouped weight-grads run elsewhere");
    g_op = "layer.wgrad";
    V4L_KLAUNCH("wps_wgrad", 2.0 * c.wps_args.n * NTOK * (double)WPS_LAYER_ELEMS * c.wps_args.nlayers +
                                 (chain ? 2.0 * c.wps_args.n * (64 * 256 + 256 * 256) : 0.0),
                ds, wps_wgrad_kernel<T>, dim3((unsigned)(c.wps_args.wg_blocks + chain)), dim3(256),
                chain ? (RowsChainLds<T, RowsChainCfg<T>::MT_TOK0>::bytes2) : 0, ds, c.wps_args);
    V4L_LAUNCH_CHECK();
  }
  int64_t gb = 0;
  int wb = 0;
  if (!net->tnp.empty()) {
    V4L_REQUIRE(net->tnp.size() <= (size_t)v4l_net::MAX_TNP, "internal: too many deferred weight-grads");
    for (TnProb& q : net->tnp) { const int64_t nb = q.blk0; q.blk0 = gb; gb += nb; }
    const size_t bytes = net->tnp.size() * sizeof(TnProb);
    if (net->tnp_cached.size() != net->tnp.size() || memcmp(net->tnp_cached.data(), net->tnp.data(), bytes) != 0) {
      V4L_REQUIRE(!capturing(c.s), "internal: weight-grad geometry changed while capturing a graph");
      V4L_HIP_CHECK(hipStreamSynchronize(c.s));
      V4L_HIP_CHECK(hipMemcpy(net->d_tnp, net->tnp.data(), bytes, hipMemcpyHostToDevice));
      net->tnp_cached = net->tnp;
    }
  }
  if (!net->wide.empty()) {
    V4L_REQUIRE(net->wide.size() <= (size_t)v4l_net::MAX_WIDE, "internal: too many fused-layer weight-grads");
    for (TnWide& q : net->wide) { const int nb = q.blk0; q.blk0 = wb; wb += nb; }
    const size_t bytes = net->wide.size() * sizeof(TnWide);
    if (net->wide_cached.size() != net->wide.size() || memcmp(net->wide_cached.data(), net->wide.data(), bytes) != 0) {
      V4L_REQUIRE(!capturing(c.s), "internal: weight-grad geometry changed while capturing a graph");
      V4L_HIP_CHECK(hipStreamSynchronize(c.s));
      V4L_HIP_CHECK(hipMemcpy(net->d_wide, net->wide.data(), bytes, hipMemcpyHostToDevice));
      net->wide_cached = net->wide;
    }
  }
  constexpr size_t dense_lds = TnWideLds<T>::max_bytes > TnBodyLds<T, 64, 1>::bytes ? TnWideLds<T>::max_bytes : TnBodyLds<T, 64, 1>::bytes;
  V4L_HIP_CHECK(lds_limit<&gemm_tn_wide_kernel<T>>(TnWideLds<T>::max_bytes));
  V4L_HIP_CHECK(lds_limit<&gemm_tn_dense_kernel<T>>(dense_lds));
  if (gb > 0 && wb > 0) {
    g_op = "layer.wgrad";  // (the layers' share dominates: 8 of the ~20 problems, 2/3 of the blocks)
    V4L_KLAUNCH("gemm_tn_dense", net->wide_flops + net->tnp_flops, dg, gemm_tn_dense_kernel<T>, dim3((unsigned)(wb + gb)), dim3(256),
                dense_lds, dg, (const TnWide*)net->d_wide, (int)net->wide.size(), wb, (const TnProb*)net->d_tnp, (int)net->tnp.size());
    V4L_LAUNCH_CHECK();
    return 0;
  }
  if (gb > 0) {
    g_op = "dense.wgrad";
    V4L_KLAUNCH("gemm_tn_group", net->tnp_flops, dg, gemm_tn_group_kernel<T>, dim3((unsigned)gb), dim3(256), 0, dg,
                (const TnProb*)net->d_tnp, (int)net->tnp.size());
    V4L_LAUNCH_CHECK();
  }
  if (wb > 0) {
    g_op = "layer.wgrad";
    V4L_KLAUNCH("gemm_tn_wide", net->wide_flops, dg, gemm_tn_wide_kernel<T>, dim3((unsigned)wb), dim3(256),
                TnWideLds<T>::max_bytes, dg, (const TnWide*)net->d_wide, (int)net->wide.size());
    V4L_LAUNCH_CHECK();
  }
  return 0;
}
// one launch: sum all registered slabs into the PyTorch-layout gradients
// The reduce table: descriptors in a fixed order — the fused conv-stack backward's (group 1) first, then the others in
// registration order — with table-wide block numbers; refreshed on the device when the geometry changed (first call for a batch
// size; not capturable, by design). The order is the same in every launch schedule, so the per-block partials of the gradient
// norm are summed in the same order whether the reduction runs as one launch or two.
static int wgrad_reduce_prepare(Ctx& c, int64_t (&blocks)[2]) {
  v4l_net* net = c.net;
  std::stable_partition(net->red.begin(), net->red.end(), [](const RedDesc& d) { return d.group == 1; });
  int64_t blk = 0;
  blocks[0] = blocks[1] = 0;
  for (RedDesc& d : net->red) {
    d.blk0 = blk;
    const int64_t nb = cdiv64((int64_t)d.N * d.K + d.N, 64);
    blk += nb;
    blocks[d.group == 1 ? 0 : 1] += nb;  // [0]: the conv stack's blocks (first in the table), [1]: the rest
  }
  V4L_REQUIRE(net->red.size() <= (size_t)v4l_net::MAX_RED, "internal: too many weight-grad descriptors");
  const size_t bytes = net->red.size() * sizeof(RedDesc);
  if (net->red_cached.size() != net->red.size() || memcmp(net->red_cached.data(), net->red.data(), bytes) != 0) {
    V4L_REQUIRE(!capturing(c.s), "internal: weight-grad geometry changed while capturing a graph");
    V4L_HIP_CHECK(hipStreamSynchronize(c.s));
    if (c.tn != c.s) V4L_HIP_CHECK(hipStreamSynchronize(c.tn));
    V4L_HIP_CHECK(hipMemcpy(net->d_red, net->red.data(), bytes, hipMemcpyHostToDevice));
    net->red_cached = net->red;
  }
  float* sq = blk <= net->sq_cap() ? net->d_sq : nullptr;
  net->red_blocks = sq != nullptr ? (int)blk : 0;
  net->red_grads = c.grads;
  return 0;
}
// blocks [base, base + count) of the prepared table on stream s
static int wgrad_reduce_launch(Ctx& c, int64_t base, int64_t count, hipStream_t s) {
  v4l_net* net = c.net;
  if (count <= 0) return 0;
  g_op = "wgrad_reduce";
  float* sq = net->red_blocks > 0 ? net->d_sq : nullptr;
  V4L_KLAUNCH("wgrad_reduce", 0, s, wgrad_reduce_kernel, dim3((unsigned)count), dim3(256), 0, s, net->d_red, (int)net->red.size(), sq,
              (int)base, net->grad_unscale);
  V4L_LAUNCH_CHECK();
  return 0;
}
template <typename T>
static int wgrad_reduce_all(Ctx& c) {
  int64_t blocks[2];
  int rc = wgrad_reduce_prepare(c, blocks);
  if (rc) return rc;
  return wgrad_reduce_launch(c, 0, blocks[0] + blocks[1], c.s);
}

struct Act { float* p; int ld; int w; };

// minibatch-sized dense problems go to gemm_nt_deep_kernel (csrc/gemm.h): fragment-order weight, 32 x 64 blocks, 8 K-stages in flight
static inline bool nt_deep_shape(int M, int Kp) {
  const char* e = getenv("V4L_GEMM_DEEP_MIN_M");  // (read per call: tests lower it to run their small batches through it; 0 = off)
  const int min_m = e ? atoi(e) : 256;
  return min_m > 0 && M >= min_m && M <= 65536 && Kp <= 4096;
}
template <typename T>
static int launch_nt_deep(hipStream_t s, const ADense& al, const T* Bf, int Np, int Kp, Epi ep, double flops) {
  ep.M = al.M;
  if (epi_wants_tanh(ep))
    V4L_KLAUNCH("gemm_nt_deep", flops, s, (gemm_nt_deep_kernel<T, ADense, true>), dim3(cdiv(al.M, 32), cdiv(Np, 64)), dim3(256), 0, s,
                al, Bf, Np, Kp, ep);
  else
    V4L_KLAUNCH("gemm_nt_deep", flops, s, (gemm_nt_deep_kernel<T, ADense>), dim3(cdiv(al.M, 32), cdiv(Np, 64)), dim3(256), 0, s, al,
                Bf, Np, Kp, ep);
  V4L_LAUNCH_CHECK();
  return 0;
}
template <typename T>
static int lin_fwd(const Ctx& c, const Lin& L, const ADense& a, Epi ep) {
  ep.bias = c.net->p[L.b];
  g_op = L.tag_fwd.c_str();
  if (L.pkf >= 0 && nt_deep_shape(a.M, L.Kp))
    return launch_nt_deep<T>(c.s, a, (const T*)c.net->packed + L.pkf, L.Np, L.Kp, ep, 2.0 * a.M * L.N * L.K);
  return launch_nt<T>(c.s, a, a.M, (const T*)c.net->packed + L.pk, L.Np, L.Kp, ep, 2.0 * a.M * L.N * L.K);
}
// Dense weight-grads are not launched where they arise: they are collected and run as ONE grouped launch at the end
// of the backward pass (wgrad_finish), which is why every gradient tensor keeps its own buffer.
template <typename T>
static int lin_wgrad(Ctx& c, const Lin& L, const ADense& y, const ADense& x, int Kx) {
  v4l_net* net = c.net;
  const int M = y.M;
  if (M <= 0) return 0;
  TnProb p;
  memset(&p, 0, sizeof(p));
  p.y = y; p.x = x; p.M = M;
  p.gx = cdiv(Kx, 64); p.gy = cdiv(L.N, 64);
  constexpr int big_rows = 256;
#ifndef V4L_TN_SMALL_ROWS
#define V4L_TN_SMALL_ROWS 128  // rows per block of a grouped dense weight-grad below 4096 rows (probe builds: -DV4L_TN_SMALL_ROWS=64|256)
#endif
  int splits = M >= 4096 ? std::min(16384 / big_rows, M / big_rows) : std::max(1, M / V4L_TN_SMALL_ROWS);  // 2..4 staging rounds per block: latency-bound
  p.mpb = round_up(cdiv(M, splits), 64);
  splits = cdiv(M, p.mpb);
  p.Npad = p.gy * 64; p.Kpad = p.gx * 64;
  const int64_t slab_f = ((int64_t)splits * p.Npad * p.Kpad + 63) / 64 * 64;
  const int64_t bslab_f = ((int64_t)splits * p.Npad + 63) / 64 * 64;
  p.slab = c.slab + c.slab_used;
  p.bslab = p.slab + slab_f;
  c.slab_used += slab_f + bslab_f;
  V4L_REQUIRE(c.slab_used <= net->slab_cap, "internal: weight-grad slab arena overflow");
  p.blk0 = (int64_t)p.gx * p.gy * splits;  // block count for now; prefix-summed in wgrad_finish
  net->tnp.push_back(p);
  net->tnp_flops += 2.0 * M * L.N * L.K;
  RedDesc o;
  memset(&o, 0, sizeof(o));
  o.dW = c.grads + net->params[L.w].goff;
  o.db = c.grads + net->params[L.b].goff;
  o.N = L.N; o.K = L.K; o.Ktorch = L.K; o.Cin = L.cin; o.taps = L.taps;
  o.slab = p.slab; o.bslab = p.bslab; o.nsplit = splits; o.Npad = p.Npad; o.Kpad = p.Kpad;
  net->red.push_back(o);
  return 0;
}
// Weight-grad of a transformer-layer linear whose operands y [M][N], x [M][K] the fused layer kernels left in the
// contraction type: one block per row slab owns the whole N x K output (gemm_tn_wide_kernel)
static int lin_wgrad_wide(Ctx& c, const Lin& L, const void* y, const void* x, int M) {
  v4l_net* net = c.net;
  V4L_REQUIRE(tn_wide_shape(L.N, L.K), "internal: lin_wgrad_wide on an unsupported shape");
  TnWide p;
  memset(&p, 0, sizeof(p));
  p.y = y; p.x = x; p.M = M; p.N = L.N; p.K = L.K;
  constexpr int wide_splits = 64;
  int splits = std::max(1, std::min(wide_splits, M / 256));
  p.mpb = round_up(cdiv(M, splits), 64);
  splits = cdiv(M, p.mpb);
  const int64_t slab_f = ((int64_t)splits * p.N * p.K + 63) / 64 * 64;
  const int64_t bslab_f = ((int64_t)splits * p.N + 63) / 64 * 64;
  p.slab = c.slab + c.slab_used;
  p.bslab = p.slab + slab_f;
  c.slab_used += slab_f + bslab_f;
  V4L_REQUIRE(c.slab_used <= net->slab_cap, "internal: weight-grad slab arena overflow");
  p.blk0 = splits;  // block count for now; prefix-summed in wgrad_finish
  net->wide.push_back(p);
  net->wide_flops += 2.0 * M * L.N * L.K;
  RedDesc o;
  memset(&o, 0, sizeof(o));
  o.dW = c.grads + net->params[L.w].goff;
  o.db = c.grads + net->params[L.b].goff;
  o.N = L.N; o.K = L.K; o.Ktorch = L.K; o.Cin = L.cin; o.taps = L.taps;
  o.slab = p.slab; o.bslab = p.bslab; o.nsplit = splits; o.Npad = p.N; o.Kpad = p.K;
  net->red.push_back(o);
  return 0;
}
template <typename T>
static int lin_dgrad(const Ctx& c, const Lin& L, const ADense& y, Epi ep) {
  ep.N = L.K;
  g_op = L.tag_dgrad.c_str();
  if (L.pkft >= 0 && nt_deep_shape(y.M, L.Ct))
    return launch_nt_deep<T>(c.s, y, (const T*)c.net->packed + L.pkft, L.Rt, L.Ct, ep, 2.0 * y.M * L.N * L.K);
  return launch_nt<T>(c.s, y, y.M, (const T*)c.net->packed + L.pkt, L.Rt, L.Ct, ep, 2.0 * y.M * L.N * L.K);
}

// the net's hidden activation (cfg.activation) as the GEMM epilogue's selectors: forward side, backward side
static inline int epi_act(const v4l_net* n) { return n->cfg.activation == V4L_ACT_TANH ? EPI_ACT_TANH : EPI_ACT_RELU; }
static inline int epi_mask_mode(const v4l_net* n) { return n->cfg.activation == V4L_ACT_TANH ? EPI_MASK_TANH : EPI_MASK_RELU; }

// forward through Linear(+activation) layers; outs[i] receives layer i's output
template <typename T>
static int chain_fwd(const Ctx& c, const Lin* Ls, int k, ADense in, const Act* outs, bool act_last, bool zero_pad_last = false) {
  for (int i = 0; i < k; ++i) {
    Epi ep = mk_epi(outs[i].p, outs[i].ld, Ls[i].N, nullptr, (i < k - 1 || act_last) ? epi_act(c.net) : EPI_ACT_NONE);
    // the last layer of a head stack writes out_dim of its row's OUT_LD columns: the rest as zeros from the same epilogue
    // (its column tiles cover Np >= 16 = OUT_LD columns) instead of a memset launch ahead of the chain
    if (i == k - 1 && zero_pad_last && outs[i].ld <= Ls[i].Np) ep.npad = outs[i].ld;
    int rc = lin_fwd<T>(c, Ls[i], in, ep);
    if (rc) return rc;
    in = dense(outs[i].p, outs[i].ld, in.M, outs[i].w);
  }
  return 0;
}
// backward through the same chain. y: grad w.r.t. the last layer's pre-activation. acts[i]: output of layer i.
// dbufs[i]: where the grad w.r.t. layer i's pre-activation goes (i < k-1). din (optional): epilogue that receives the
// grad w.r.t. the chain input.
template <typename T>
static int chain_bwd(Ctx& c, const Lin* Ls, int k, const ADense& in, const Act* acts, ADense y, float* const* dbufs,
                     const Epi* din) {
  for (int i = k - 1; i >= 0; --i) {
    int rc;
    if (i == 0) rc = lin_wgrad<T>(c, Ls[0], y, in, in.K);
    else rc = lin_wgrad<T>(c, Ls[i], y, dense(acts[i - 1].p, acts[i - 1].ld, y.M, acts[i - 1].w), acts[i - 1].w);
    if (rc) return rc;
    if (i > 0) {
      Epi ep = mk_epi(dbufs[i - 1], acts[i - 1].w, acts[i - 1].w);
      ep.mask = acts[i - 1].p;
      ep.ldmask = acts[i - 1].ld;
      ep.mask_mode = epi_mask_mode(c.net);
      if ((rc = lin_dgrad<T>(c, Ls[i], y, ep))) return rc;
      y = dense(dbufs[i - 1], acts[i - 1].w, y.M, acts[i - 1].w);
    } else if (din != nullptr) {
      if ((rc = lin_dgrad<T>(c, Ls[0], y, *din))) return rc;
    }
  }
  return 0;
}

// LayerNorm backward: per-block dgamma/dbeta partials go to the slab arena and are summed by wgrad_finish
static int ln_bwd_launch(Ctx& c, int nblk, const float* dout, float* dz, const float* xhat, const float* rstd, const LNp& ln,
                         int rows) {
  v4l_net* net = c.net;
  float* gpart = c.slab + c.slab_used;
  float* bpart = gpart + (int64_t)nblk * TD;
  c.slab_used += 2 * (int64_t)nblk * TD;
  V4L_REQUIRE(c.slab_used <= net->slab_cap, "internal: weight-grad slab arena overflow");
  V4L_KLAUNCH("ln_bwd", 0, c.s, ln_bwd_kernel, dim3(nblk), dim3(256), 0, c.s, dout, xhat, rstd, net->p[ln.g], rows, dz, gpart,
              bpart);
  V4L_LAUNCH_CHECK();
  for (int k = 0; k < 2; ++k) {
    RedDesc d;
    memset(&d, 0, sizeof(d));
    d.slab = k == 0 ? gpart : bpart;
    d.dW = c.grads + net->params[k == 0 ? ln.g : ln.b].goff;
    d.nsplit = nblk; d.N = 1; d.K = TD; d.Npad = 1; d.Kpad = TD; d.Ktorch = TD;
    net->red.push_back(d);
  }
  return 0;
}

static inline AIm2colNHWC nhwc_loader(const float* p, const Conv& cv, int n) {
  AIm2colNHWC a;
  a.p = p; a.IH = cv.IH; a.IW = cv.IH; a.Cin = cv.Cin; a.OH = cv.OH; a.OW = cv.OH; a.KH = cv.KH; a.KW = cv.KH;
  a.stride = cv.stride; a.M = n * cv.OH * cv.OH; a.K = cv.K;
  return a;
}
template <typename T>
static inline AIm2colCHW<T> chw_loader(const T* img, const Conv& cv, int n, const int* rowidx) {
  AIm2colCHW<T> a;
  a.p = img; a.C = cv.Cin; a.IH = cv.IH; a.IW = cv.IH; a.OH = cv.OH; a.OW = cv.OH; a.stride = cv.stride;
  a.M = n * cv.OH * cv.OH; a.rowidx = rowidx;
  return a;
}

template <typename T>
static int conv_stack_fwd(const Ctx& c, const T* image, const int* rowidx, int n, float* c1, float* c2, float* c3) {
  const v4l_net* N = c.net;
  const Conv* cv = N->conv;
  int rc;
  {
    Epi ep = mk_epi(c1, cv[0].Cout, cv[0].Cout, N->p[cv[0].b], 1);
    auto al = chw_loader<T>(image, cv[0], n, rowidx);
    g_op = "conv1.fwd";
    rc = launch_nt<T>(c.s, al, al.M, (const T*)N->packed + cv[0].pk, cv[0].Np, cv[0].Kp, ep, 2.0 * al.M * cv[0].Cout * cv[0].K);
    if (rc) return rc;
  }
  float* ins[3] = {nullptr, c1, c2};
  float* outs[3] = {c1, c2, c3};
  for (int i = 1; i < 3; ++i) {
    Epi ep = mk_epi(outs[i], cv[i].Cout, cv[i].Cout, N->p[cv[i].b], 1);
    auto al = nhwc_loader(ins[i], cv[i], n);
    g_op = i == 1 ? "conv2.fwd" : "conv3.fwd";
    rc = launch_nt<T>(c.s, al, al.M, (const T*)N->packed + cv[i].pk, cv[i].Np, cv[i].Kp, ep, 2.0 * al.M * cv[i].Cout * cv[i].K);
    if (rc) return rc;
  }
  return 0;
}

// The whole conv-stack backward as one persistent launch (csrc/bwd.h) when the stack has the shipped NatureCNN geometry
static bool conv_bwd_fusable(const v4l_net* N) {
  const Conv* v = N->conv;
  return v[1].Rd == 32 && v[1].Kdp == 256 && v[2].Rd == 64 && v[2].Kdp == 576 && v[0].chw && v[0].Cin == 4 && v[0].IH == 64 && v[0].KH == 8 && v[0].stride == 4 && v[0].Cout == 32 &&
         v[1].Cin == 32 && v[1].KH == 4 && v[1].stride == 2 && v[1].Cout == 64 && v[1].OH == 6 &&
         v[2].Cin == 64 && v[2].KH == 3 && v[2].stride == 1 && v[2].Cout == 64 && v[2].OH == 4 &&
         !sw_on("V4L_NO_FUSED_CONV_BWD");
}
// dW3's launch (bwd_conv3_wgrad_kernel) of the conv-stack backward last set up in c.conv3_*, on stream s
template <typename T>
static int conv3_wgrad_launch(Ctx& c, hipStream_t s) {
  g_op = "conv3.wgrad";
  const double fl = 2.0 * c.conv3_n * 16 * 64 * 576;
  const dim3 grid(c.conv3_blocks), blk(256);
  const bool a16 = c.conv3_a16, tr = c.conv3_tr;
  if constexpr (sizeof(T) == 2) {
    if (a16 && tr) V4L_KLAUNCH("fused_conv3_wgrad", fl, s, (bwd_conv3_wgrad_kernel<T, true, true>), grid, blk, 0, s, c.conv3_args);
    else if (a16) V4L_KLAUNCH("fused_conv3_wgrad", fl, s, (bwd_conv3_wgrad_kernel<T, true>), grid, blk, 0, s, c.conv3_args);
    else if (tr) V4L_KLAUNCH("fused_conv3_wgrad", fl, s, (bwd_conv3_wgrad_kernel<T, false, true>), grid, blk, 0, s, c.conv3_args);
  }
  if (!a16 && !tr) V4L_KLAUNCH("fused_conv3_wgrad", fl, s, bwd_conv3_wgrad_kernel<T>, grid, blk, 0, s, c.conv3_args);
  V4L_LAUNCH_CHECK();
  return 0;
}
template <typename T>
static int conv_stack_bwd_fused(Ctx& c, const T* image, const int* rowidx, int n, const float* c1, const float* c2,
                                const float* dc3, float* dc2_tap, float* dc1_tap) {
  v4l_net* N = c.net;
  V4L_HIP_CHECK(lds_limit<&bwd_conv_kernel<T>>(BwdConvLds<T>::bytes));
  if constexpr (sizeof(T) == 2) {
    V4L_HIP_CHECK(lds_limit<&bwd_conv_kernel<T, true>>(BwdConvLds<T>::bytes));
    V4L_HIP_CHECK(lds_limit<&bwd_conv_kernel<T, false, true>>(BwdConvLds<T, true>::bytes));
    V4L_HIP_CHECK(lds_limit<&bwd_conv_kernel<T, true, true>>(BwdConvLds<T, true>::bytes));
  }
  // c1 / c2 in T: what the training encoder of THIS workspace's last forward wrote (the mark is the workspace's c1 address, so a
  // forward of the same net over another workspace in between — HipNet.value() at another batch size — does not change it)
  const bool a16 = sizeof(T) == 2 && N->acts16_c1 != nullptr && N->acts16_c1 == c1;
  int nblk = std::min(n, CONV_BWD_MAX_BLOCKS);
  if (const char* e = getenv("V4L_CONV_BWD_BLOCKS")) nblk = std::max(1, std::min(nblk, atoi(e)));
  // 16-bit modes: the conv weight-grads' operands by transposed LDS reads (csrc/bwd.h, TR). V4L_WGRAD_TR: 0 the gathers, 1 (default)
  // dW2 / dW1 and dW3, 2 dW2 / dW1 only, 3 dW3 only — the same bits whatever it says
  const int tr_sw = sizeof(T) == 2 ? sw_int("V4L_WGRAD_TR", 1) : 0;
  const bool tr = tr_sw == 1 || tr_sw == 2, tr3 = tr_sw == 1 || tr_sw == 3;
  // dW3's launch runs beside the dense weight-grads on the other stream: fewer, fatter blocks cut its partial slabs (147 KB
  // per block, written here and read again by wgrad_reduce) until the launch itself becomes the longer branch. The balance
  // moved with the other branch: when the dense weight-grads took ~54 us, 64 blocks (53 us) won (357.8 / 364.2 / 367.6 K
  // env-steps/s at 256 / 128 / 64); with wps_wgrad + gemm_tn_group at ~44 us, three interleaved runs per setting in one
  // session give 358 K (64) / 372 K (96) / 369 K (128) / 366 K (192).
  // Without wps_wgrad on the other branch (NatureCNN nets: gemm_tn_group alone, ~25 us) dW3 has to be shorter still: 316 K (96) /
  // 320 K (128, 192, 256) env-steps/s on ppo_nature_cnn.
  int nblk3 = std::min(nblk, c.wps_used ? 96 : 160);
  if (const char* e = getenv("V4L_CONV3_WGRAD_BLOCKS")) nblk3 = std::max(1, std::min(nblk, atoi(e)));
  const int Ns[3] = {32, 64, 64}, Ks[3] = {256, 512, 576};
  float* slab[3];
  float* bslab[3];
  for (int i = 0; i < 3; ++i) {
    const int nb = i == 2 ? nblk3 : nblk;
    const int64_t sf = ((int64_t)nb * Ns[i] * Ks[i] + 63) / 64 * 64, bf = ((int64_t)nb * Ns[i] + 63) / 64 * 64;
    slab[i] = c.slab + c.slab_used;
    bslab[i] = slab[i] + sf;
    c.slab_used += sf + bf;
    const Conv& v = N->conv[i];
    RedDesc o;
    memset(&o, 0, sizeof(o));
    o.dW = c.grads + N->params[v.w].goff;
    o.db = c.grads + N->params[v.b].goff;
    o.N = v.Cout; o.K = v.K; o.Ktorch = v.K;
    o.Cin = v.chw ? 0 : v.Cin; o.taps = v.chw ? 0 : v.KH * v.KH;
    o.slab = slab[i]; o.bslab = bslab[i]; o.nsplit = nb; o.Npad = Ns[i]; o.Kpad = Ks[i];
    o.group = 1;  // (reduced right behind dW3 on the main stream when the weight-grad section is forked)
    N->red.push_back(o);
  }
  V4L_REQUIRE(c.slab_used <= N->slab_cap, "internal: weight-grad slab arena overflow");
  BwdConv a;
  memset(&a, 0, sizeof(a));
  a.w3d = (const T*)N->packed + N->conv[2].pkd[0];
  for (int cls = 0; cls < 4; ++cls) a.w2d[cls] = (const T*)N->packed + N->conv[1].pkd[cls];
  a.image = image; a.rowidx = rowidx; a.c1 = c1; a.c2 = c2; a.dc3 = dc3;
  if (c.taps) { a.t_dc2 = dc2_tap; a.t_dc1 = dc1_tap; }  // (tests)
  a.slab1 = slab[0]; a.slab2 = slab[1]; a.slab3 = slab[2];
  a.bslab1 = bslab[0]; a.bslab2 = bslab[1]; a.bslab3 = bslab[2];
  a.n = n;
  g_op = "conv.bwd";
  const double fl = 2.0 * n * (16.0 * 64 * 576 + 2.0 * 36 * 64 * 512 + 225.0 * 32 * 256);
  if constexpr (sizeof(T) == 2) {
    if (a16 && tr) V4L_KLAUNCH("fused_conv_bwd", fl, c.s, (bwd_conv_kernel<T, true, true>), dim3(nblk), dim3(512), (BwdConvLds<T, true>::bytes), c.s, a);
    else if (a16) V4L_KLAUNCH("fused_conv_bwd", fl, c.s, (bwd_conv_kernel<T, true>), dim3(nblk), dim3(512), BwdConvLds<T>::bytes, c.s, a);
    else if (tr) V4L_KLAUNCH("fused_conv_bwd", fl, c.s, (bwd_conv_kernel<T, false, true>), dim3(nblk), dim3(512), (BwdConvLds<T, true>::bytes), c.s, a);
  }
  if (!a16 && !tr) V4L_KLAUNCH("fused_conv_bwd", fl, c.s, bwd_conv_kernel<T>, dim3(nblk), dim3(512), BwdConvLds<T>::bytes, c.s, a);
  V4L_LAUNCH_CHECK();
  c.conv3_args = a; c.conv3_blocks = nblk3; c.conv3_n = n; c.conv3_a16 = a16; c.conv3_tr = tr3;
  if (c.defer_conv3) {
    c.conv3_pending = true;
    return 0;
  }
  return conv3_wgrad_launch<T>(c, c.tn);
}
template <typename T>
static int conv3_wgrad_deferred(Ctx& c, hipStream_t s) {
  if (!c.conv3_pending) return 0;
  c.conv3_pending = false;
  return conv3_wgrad_launch<T>(c, s);
}

// dc3: grad w.r.t. conv3's pre-activation [n*16][64]. Scratch dc2 [n*36][64], dc1 [n*225][32].
template <typename T>
static int conv_stack_bwd(Ctx& c, const T* image, const int* rowidx, int n, const float* c1, const float* c2,
                          float* dc3, float* dc2, float* dc1) {
  if (conv_bwd_fusable(c.net)) return conv_stack_bwd_fused<T>(c, image, rowidx, n, c1, c2, dc3, dc2, dc1);
  const v4l_net* N = c.net;
  const Conv* cv = N->conv;
  const float* acts[3] = {nullptr, c1, c2};   // input activation of conv i
  float* dys[3] = {dc1, dc2, dc3};            // grad w.r.t. conv i pre-activation
  for (int i = 2; i >= 0; --i) {
    const Conv& v = cv[i];
    const int M = n * v.OH * v.OH;
    ADense y = dense(dys[i], v.Cout, M, v.Cout);
    RedDesc o;
    memset(&o, 0, sizeof(o));
    o.dW = c.grads + N->params[v.w].goff;
    o.db = c.grads + N->params[v.b].goff;
    o.N = v.Cout; o.K = v.K; o.Ktorch = v.K;
    int rc;
    if (i > 0 && (rc = par_begin(c))) return rc;  // weight-grad of conv i next to its data-grad
    if (v.chw) {
      o.Cin = 0; o.taps = 0;
      auto x = chw_loader<T>(image, v, n, rowidx);
      g_op = "conv1.wgrad";
      rc = launch_tn<T>(c, y, x, M, v.Cout, v.K, o, 2.0 * M * v.Cout * v.K);
    } else {
      o.Cin = v.Cin; o.taps = v.KH * v.KH;
      auto x = nhwc_loader(acts[i], v, n);
      g_op = i == 1 ? "conv2.wgrad" : "conv3.wgrad";
      rc = launch_tn<T>(c, y, x, M, v.Cout, v.K, o, 2.0 * M * v.Cout * v.K);
    }
    if (rc) return rc;
    if (i == 0) break;
    // gather-form data-grad into the input plane of conv i (= output plane of conv i-1), ReLU-masked: all
    // stride-parity classes in one launch (blockIdx.z)
    const int st = v.stride, TH = v.KH / st;
    DgradClasses<T> dc;
    memset(&dc, 0, sizeof(dc));
    dc.Kp = v.Kdp;
    int maxM = 0;
    for (int cls = 0; cls < v.ncls; ++cls) {
      const int py = cls / st, px = cls % st;
      ADgradNHWC& a = dc.a[cls];
      a.p = dys[i]; a.OH = v.OH; a.OW = v.OH; a.Cout = v.Cout; a.TH = TH; a.TW = TH;
      a.nIy = (v.IH - py + st - 1) / st; a.nIx = (v.IH - px + st - 1) / st;
      a.M = n * a.nIy * a.nIx; a.K = v.Kd;
      Epi ep = mk_epi(dys[i - 1], v.Cin, v.Cin);
      ep.M = a.M;
      ep.rowmap = ROWMAP_DGRAD;
      ep.py = py; ep.px = px; ep.s = st; ep.nIy = a.nIy; ep.nIx = a.nIx; ep.IH = v.IH; ep.IW = v.IH;
      ep.mask = acts[i]; ep.ldmask = v.Cin;
      dc.ep[cls] = ep;
      dc.B[cls] = (const T*)N->packed + v.pkd[cls];
      maxM = std::max(maxM, a.M);
    }
    g_op = i == 1 ? "conv2.dgrad" : "conv3.dgrad";
    const dim3 grid(cdiv(maxM, 128), 1, v.ncls);
    if (v.Rd % 64 == 0) {
      V4L_KLAUNCH("gemm_nt_dgrad", 2.0 * M * v.Cout * v.K, c.s, (gemm_nt_dgrad_kernel<T, 64>), dim3(grid.x, v.Rd / 64, grid.z),
                  dim3(256), 0, c.s, dc);
    } else {
      V4L_KLAUNCH("gemm_nt_dgrad", 2.0 * M * v.Cout * v.K, c.s, (gemm_nt_dgrad_kernel<T, 32>), dim3(grid.x, v.Rd / 32, grid.z),
                  dim3(256), 0, c.s, dc);
    }
    V4L_LAUNCH_CHECK();
    if ((rc = par_end(c))) return rc;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------ RCCL (data parallel)
// The collective library is bound at run time (dlopen of the soname PyTorch-ROCm and /opt/rocm both ship): the shared
// library has no link-time dependency on it and single-GPU users never load it. Only what the path needs is bound: one
// in-place fp32 sum all-reduce per optimiser step, issued on the caller's stream so that it is captured
// into the update's hipGraph like any kernel.
struct RcclUid { char internal[128]; };
struct Rccl {
  void* h = nullptr;
  int (*GetUniqueId)(RcclUid*) = nullptr;
  int (*CommInitRank)(void**, int, RcclUid, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;
  int (*CommUserRank)(void*, int*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
static Rccl g_rccl;
static int rccl_load() {
  if (g_rccl.h != nullptr) return 0;
  const char* names[] = {getenv("V4L_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;
  for (const char* nm : names) {
    if (nm == nullptr || *nm == 0) continue;
    h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (h != nullptr) break;
  }
  V4L_REQUIRE(h != nullptr, "v4l_comm: cannot load RCCL (librccl.so.1): %s", dlerror());
  Rccl r;
  r.h = h;
  r.GetUniqueId = (int (*)(RcclUid*))dlsym(h, "ncclGetUniqueId");
  r.CommInitRank = (int (*)(void**, int, RcclUid, int))dlsym(h, "ncclCommInitRank");
  r.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
  r.CommCount = (int (*)(void*, int*))dlsym(h, "ncclCommCount");
  r.CommUserRank = (int (*)(void*, int*))dlsym(h, "ncclCommUserRank");
  r.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclAllReduce");
  r.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
  V4L_REQUIRE(r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllReduce && r.GetErrorString && r.CommCount && r.CommUserRank,
              "v4l_comm: the loaded RCCL lacks a required symbol");
  g_rccl = r;
  return 0;
}
#define V4L_RCCL_CHECK(expr)                                                                      \
  do {                                                                                            \
    const int _e = (expr);                                                                        \
    if (_e != 0) {                                                                                \
      v4l::set_error("%s:%d: %s -> RCCL error %d (%s)", __FILE__, __LINE__, #expr, _e, v4l::g_rccl.GetErrorString(_e)); \
      return -3;                                                                                  \
    }                                                                                             \
  } while (0)

}  // namespace v4l

using namespace v4l;

// ------------------------------------------------------------------------------------------ plan
int v4l_net::build() {
  const v4l_net_cfg& c = cfg;
  V4L_REQUIRE(c.kind >= V4L_NET_MLP && c.kind <= V4L_NET_LOCO_VIS, "v4l_net_create: unknown net kind %d", c.kind);
  V4L_REQUIRE(c.compute == V4L_F32 || c.compute == V4L_BF16 || c.compute == V4L_F16, "v4l_net_create: unknown compute mode %d", c.compute);
  V4L_REQUIRE(c.activation == V4L_ACT_RELU || c.activation == V4L_ACT_TANH,
              "v4l_net_create: unknown activation %d (V4L_ACT_RELU 0 | V4L_ACT_TANH 1)", c.activation);
  V4L_REQUIRE(c.activation == V4L_ACT_RELU || c.kind == V4L_NET_MLP,
              "v4l_net_create: activation V4L_ACT_TANH runs on net kind V4L_NET_MLP only (got kind %d); the kinds V4L_NET_CNN, "
              "V4L_NET_LOCO, V4L_NET_CNN_VIS and V4L_NET_LOCO_VIS take V4L_ACT_RELU", c.kind);
  V4L_REQUIRE(c.out_dim > 0 && c.out_dim <= V4L_MAX_ACT, "v4l_net_create: 1<=out_dim<=%d (V4L_MAX_ACT) required, got %d", V4L_MAX_ACT,
              c.out_dim);
  V4L_REQUIRE(c.has_logstd >= V4L_LOGSTD_NONE && c.has_logstd <= V4L_LOGSTD_HEAD,
              "v4l_net_create: has_logstd must be 0 (none), 1 (a logstd parameter) or 2 (log sigma from the head's last layer), got %d",
              c.has_logstd);
  if (sd()) {  // GaussianContPolicy (continuous_policy.py:222-236): the last layer is [mean | raw log sigma]
    V4L_REQUIRE(c.kind == V4L_NET_MLP, "v4l_net_create: V4L_LOGSTD_HEAD runs on net kind V4L_NET_MLP only (got kind %d)", c.kind);
    V4L_REQUIRE(c.out_dim % 2 == 0, "v4l_net_create: V4L_LOGSTD_HEAD splits the head's output in two halves: out_dim must be even, "
                "got %d", c.out_dim);
    V4L_REQUIRE(c.out_dim <= OUT_LD, "v4l_net_create: V4L_LOGSTD_HEAD needs 2 A <= %d columns of the head row, got out_dim %d", OUT_LD,
                c.out_dim);
  }
  if (vis_only())  // vision-only nets have no proprio branch: the observation row is the depth stack alone
    V4L_REQUIRE(c.state_dim == 0 && c.n_enc_hidden == 0, "v4l_net_create: vision-only nets take state_dim 0 and no encoder MLP");
  else
    V4L_REQUIRE(c.state_dim > 0 && c.n_enc_hidden >= 1, "v4l_net_create: state_dim>0 and an encoder MLP required");
  V4L_REQUIRE(c.n_enc_hidden <= V4L_MAX_HIDDEN && c.n_head_hidden >= 0 && c.n_head_hidden <= V4L_MAX_HIDDEN,
              "v4l_net_create: hidden layer counts out of range");
  for (int i = 0; i < c.n_enc_hidden; ++i)
    V4L_REQUIRE(c.enc_hidden[i] > 0 && c.enc_hidden[i] % 8 == 0, "v4l_net_create: hidden widths must be multiples of 8");
  for (int i = 0; i < c.n_head_hidden; ++i)
    V4L_REQUIRE(c.head_hidden[i] > 0 && c.head_hidden[i] % 8 == 0, "v4l_net_create: hidden widths must be multiples of 8");
  if (c.kind != V4L_NET_MLP)
    V4L_REQUIRE(c.in_channels == 4 && c.img_hw == 64,
                "v4l_net_create: only the 4x64x64 depth stack is supported (got %dx%dx%d)", c.in_channels, c.img_hw, c.img_hw);
  if (is_tf())
    V4L_REQUIRE(c.token_dim == TD && c.n_layers >= 1 && c.n_layers <= 8 && c.ff_dim > 0 && c.ff_dim % 8 == 0,
                "v4l_net_create: LocoTransformer needs token_dim 64, 1..8 layers, ff_dim %% 8 == 0");
  if (c.kind == V4L_NET_CNN)
    V4L_REQUIRE(c.visual_dim > 0 && c.visual_dim % 8 == 0, "v4l_net_create: visual_dim must be a positive multiple of 8");
  Sp = std::max(32, round_up(c.state_dim, 32));  // vision-only: a 32-float all-zero dummy row keeps every array non-empty
  ntok = c.kind == V4L_NET_LOCO_VIS ? 16 : NTOK;

  auto add_param = [&](const std::string& name, std::initializer_list<int64_t> shp) {
    ParamInfo pi;
    pi.name = name;
    pi.ndim = (int)shp.size();
    pi.numel = 1;
    int d = 0;
    for (int64_t v : shp) { pi.shape[d++] = v; pi.numel *= v; }
    for (; d < 4; ++d) pi.shape[d] = 1;
    pi.goff = total_params;
    total_params += pi.numel;
    params.push_back(pi);
    return (int)params.size() - 1;
  };
  auto make_lin = [&](const std::string& wname, const std::string& bname, int N, int K, bool need_dgrad,
                      bool as_conv1x1 = false) {
    Lin L;
    if (as_conv1x1) L.w = add_param(wname, {N, K, 1, 1});
    else L.w = add_param(wname, {N, K});
    L.b = add_param(bname, {N});
    L.N = N; L.K = K; L.need_dgrad = need_dgrad;
    std::string t = wname;
    const size_t cut = t.rfind('.');
    if (cut != std::string::npos) t = t.substr(0, cut);
    L.tag_fwd = t + ".fwd"; L.tag_wgrad = t + ".wgrad"; L.tag_dgrad = t + ".dgrad";
    return L;
  };
  auto make_mlp = [&](const std::string& prefix, int in_dim, const int* widths, int nw, bool first_needs_dgrad,
                      std::vector<Lin>& out) {
    int k = in_dim;
    for (int i = 0; i < nw; ++i) {
      const std::string id = prefix + "." + std::to_string(2 * i);
      out.push_back(make_lin(id + ".weight", id + ".bias", widths[i], k, i > 0 || first_needs_dgrad));
      k = widths[i];
    }
    return k;
  };
  auto make_convs = [&](const std::string& prefix) {
    const int spec[3][5] = {{4, 32, 8, 4, 64}, {32, 64, 4, 2, 15}, {64, 64, 3, 1, 6}};  // base.py:317-324
    for (int i = 0; i < 3; ++i) {
      Conv& v = conv[i];
      v.Cin = spec[i][0]; v.Cout = spec[i][1]; v.KH = spec[i][2]; v.stride = spec[i][3]; v.IH = spec[i][4];
      v.OH = (v.IH - v.KH) / v.stride + 1;
      v.K = v.Cin * v.KH * v.KH;
      v.chw = (i == 0);
      const std::string id = prefix + ".layers." + std::to_string(2 * i);
      v.w = add_param(id + ".weight", {v.Cout, v.Cin, v.KH, v.KH});
      v.b = add_param(id + ".bias", {v.Cout});
    }
  };

  int head_in = 0;
  if (c.kind == V4L_NET_MLP) {
    head_in = make_mlp("base.seq_fcs", c.state_dim, c.enc_hidden, c.n_enc_hidden, false, enc);
  } else if (c.kind == V4L_NET_CNN) {
    make_convs("encoder.visual_base");
    proj = make_lin("encoder.visual_projector.projection.0.weight", "encoder.visual_projector.projection.0.bias",
                    c.visual_dim, 1024, true);
    proj.cin = 64; proj.taps = 16;
    const int e = make_mlp("encoder.base.seq_fcs", c.state_dim, c.enc_hidden, c.n_enc_hidden, false, enc);
    head_in = c.visual_dim + e;
  } else if (c.kind == V4L_NET_CNN_VIS) {
    make_convs("encoder");  // the NatureEncoder(flatten=True) itself is `encoder` (starter/ppo_nature_cnn_vision_only.py:80-83)
    head_in = 1024;
  } else {
    make_convs("encoder.depth_visual_base");
    upconv = make_lin("encoder.depth_up_conv.weight", "encoder.depth_up_conv.bias", TD, 64, true, true);
    if (c.kind == V4L_NET_LOCO) {
      const int e = make_mlp("encoder.base.seq_fcs", c.state_dim, c.enc_hidden, c.n_enc_hidden, false, enc);
      proj = make_lin("encoder.state_projector.projection.0.weight", "encoder.state_projector.projection.0.bias", TD, e, true);
    }
    if (c.token_norm) {  // (the reference creates them between the encoder and the layers: nets.py:815-818)
      tok_ln.g = add_param("token_ln.weight", {TD});
      tok_ln.b = add_param("token_ln.bias", {TD});
      stok_ln.g = add_param("state_token_ln.weight", {TD});
      stok_ln.b = add_param("state_token_ln.bias", {TD});
    }
    for (int l = 0; l < c.n_layers; ++l) {
      const std::string id = (c.pytorch_encoder ? "visual_trans_encoder.layers." : "visual_append_layers.") + std::to_string(l);
      TLayer t;
      t.inproj = make_lin(id + ".self_attn.in_proj_weight", id + ".self_attn.in_proj_bias", 3 * TD, TD, true);
      t.outproj = make_lin(id + ".self_attn.out_proj.weight", id + ".self_attn.out_proj.bias", TD, TD, true);
      t.ff1 = make_lin(id + ".linear1.weight", id + ".linear1.bias", c.ff_dim, TD, true);
      t.ff2 = make_lin(id + ".linear2.weight", id + ".linear2.bias", TD, c.ff_dim, true);
      t.ln1.g = add_param(id + ".norm1.weight", {TD});
      t.ln1.b = add_param(id + ".norm1.bias", {TD});
      t.ln2.g = add_param(id + ".norm2.weight", {TD});
      t.ln2.b = add_param(id + ".norm2.bias", {TD});
      layers.push_back(t);
    }
    if (c.pytorch_encoder) {
      fin_ln.g = add_param("visual_trans_encoder.norm.weight", {TD});
      fin_ln.b = add_param("visual_trans_encoder.norm.bias", {TD});
    }
    head_in = c.kind == V4L_NET_LOCO ? 2 * TD : TD;
  }
  {
    const std::string hp = is_tf() ? "visual_seq_append_fcs" : "seq_append_fcs";
    const int k = make_mlp(hp, head_in, c.head_hidden, c.n_head_hidden, true, head);
    const std::string id = hp + "." + std::to_string(2 * c.n_head_hidden);
    head.push_back(make_lin(id + ".weight", id + ".bias", c.out_dim, k, true));
    if (c.kind == V4L_NET_CNN_VIS) {  // the first head layer reads conv3's NHWC rows as PyTorch's NCHW flatten
      head[0].cin = 64;
      head[0].taps = 16;
    }
  }
  if (c.has_logstd == V4L_LOGSTD_PARAM) logstd = add_param("logstd", {c.out_dim});

  // ---- packed operand layout
  auto align64 = [](int64_t x) { return (x + 63) / 64 * 64; };
  auto add_pack = [&](int param, int kind, int R, int Cc, int N, int K, int cin, int taps, int KW, int s, int py, int px,
                      int TW) {
    PackDesc d;
    memset(&d, 0, sizeof(d));
    d.dst_off = packed_elems;
    d.kind = kind; d.R = R; d.Cc = Cc; d.N = N; d.K = K; d.Cin = cin; d.taps = taps; d.KW = KW;
    d.s = s; d.py = py; d.px = px; d.TW = TW;
    d.blk0 = pack_blocks;
    pack_blocks += cdiv64((int64_t)R * Cc, PACK_PER_BLOCK);
    packed_elems = align64(packed_elems + (int64_t)R * Cc);
    packs.push_back(d);
    pack_param.push_back(param);
    return d.dst_off;
  };
  auto pack_lin = [&](Lin& L) {
    L.Np = round_up(L.N, 16); L.Kp = round_up(L.K, 64);
    L.pk = add_pack(L.w, L.cin ? PK_CONV_NHWC : PK_NT, L.Np, L.Kp, L.N, L.K, L.cin, L.taps, 0, 0, 0, 0, 0);
    if (L.need_dgrad) {
      L.Rt = round_up(L.K, 16); L.Ct = round_up(L.N, 64);
      L.pkt = add_pack(L.w, L.cin ? PK_CONV_NHWC_T : PK_T, L.Rt, L.Ct, L.N, L.K, L.cin, L.taps, 0, 0, 0, 0, 0);
    }
  };
  if (c.kind != V4L_NET_MLP) {
    for (int i = 0; i < 3; ++i) {
      Conv& v = conv[i];
      v.Np = round_up(v.Cout, 16); v.Kp = round_up(v.K, 64);
      const int taps = v.KH * v.KH;
      v.pk = add_pack(v.w, v.chw ? PK_NT : PK_CONV_NHWC, v.Np, v.Kp, v.Cout, v.K, v.Cin, taps, v.KH, 0, 0, 0, 0);
      if (i > 0) {
        V4L_REQUIRE(v.KH % v.stride == 0, "conv data-grad needs kernel %% stride == 0");
        const int TH = v.KH / v.stride;
        v.ncls = v.stride * v.stride;
        v.Kd = TH * TH * v.Cout; v.Kdp = round_up(v.Kd, 64); v.Rd = round_up(v.Cin, 16);
        for (int cls = 0; cls < v.ncls; ++cls)
          v.pkd[cls] = add_pack(v.w, PK_CONV_DGRAD, v.Rd, v.Kdp, v.Cout, v.K, v.Cin, taps, v.KH, v.stride, cls / v.stride,
                                cls % v.stride, TH);
      }
    }
  }
  if (is_tf()) pack_lin(upconv);
  if (c.kind == V4L_NET_CNN || c.kind == V4L_NET_LOCO) pack_lin(proj);
  for (Lin& L : enc) pack_lin(L);
  for (TLayer& t : layers) { pack_lin(t.inproj); pack_lin(t.outproj); pack_lin(t.ff1); pack_lin(t.ff2); }
  for (Lin& L : head) pack_lin(L);
  if (is_tf() && c.ff_dim == 256) {
    // wave-per-sample layer kernels (csrc/wps.h): per layer ONE contiguous block [in_proj | out_proj | linear1 | linear2] of
    // k-permuted fragment-order packs (it is DMA'd into LDS as a whole), and the same of the transposed weights
    for (TLayer& t : layers) {
      Lin* ls[4] = {&t.inproj, &t.outproj, &t.ff1, &t.ff2};
      int64_t at = -1;
      for (Lin* L : ls) {
        L->pkp = add_pack(L->w, PK_FRAGP, L->N, L->K, L->N, L->K, 0, 0, 0, 0, 0, 0, 0);
        V4L_REQUIRE(at < 0 || L->pkp == at, "internal: a layer's fragment packs are not adjacent");
        at = L->pkp + (int64_t)L->N * L->K;
      }
      V4L_REQUIRE(t.outproj.pkp - t.inproj.pkp == WPS_OFF_WO && t.ff1.pkp - t.inproj.pkp == WPS_OFF_W1 &&
                      t.ff2.pkp - t.inproj.pkp == WPS_OFF_W2, "internal: wave-per-sample weight block layout");
      at = -1;
      for (Lin* L : ls) {  // the transposed block: rows = input features, contraction = output features
        L->pkpt = add_pack(L->w, PK_FRAGPT, L->K, L->N, L->N, L->K, 0, 0, 0, 0, 0, 0, 0);
        V4L_REQUIRE(at < 0 || L->pkpt == at, "internal: a layer's transposed fragment packs are not adjacent");
        at = L->pkpt + (int64_t)L->N * L->K;
      }
      V4L_REQUIRE(t.outproj.pkpt - t.inproj.pkpt == WPS_OFF_WO && t.ff1.pkpt - t.inproj.pkpt == WPS_OFF_W1 &&
                      t.ff2.pkpt - t.inproj.pkpt == WPS_OFF_W2, "internal: wave-per-sample transposed weight block layout");
    }
    upconv.pkpt = add_pack(upconv.w, PK_FRAGPT, upconv.K, upconv.N, upconv.N, upconv.K, 0, 0, 0, 0, 0, 0, 0);
    if (c.kind == V4L_NET_LOCO_VIS && head[0].K == TD) {
      // the first head layer against the 128-wide pooled operand [dummy row | mean of the 16 tokens]: K entries at offset 64
      Lin& h0 = head[0];
      h0.pko = add_pack(h0.w, PK_NT, h0.Np, 2 * TD, h0.N, h0.K, 0, 0, 0, 0, 0, TD, 0);
      h0.pkto = add_pack(h0.w, PK_T, 2 * TD, h0.Ct, h0.N, h0.K, 0, 0, 0, 0, 0, TD, 0);
    }
  }
  {
    // the rollout step streams these as whole MFMA fragments (rollout_stack_kernel, rollout_encoder2_kernel, csrc/rollout_dense.h);
    // a linear that reads conv3's NHWC rows keeps that k order (L.cin / L.taps, as in its PK_CONV_NHWC pack)
    auto pack_frag = [&](Lin& L) {
      L.pkf = add_pack(L.w, PK_FRAG, L.Np, L.Kp, L.N, L.K, L.cin, L.taps, 0, 0, 0, 0, 0);
      if (L.need_dgrad && c.kind != V4L_NET_LOCO)  // (the LocoTransformer's data-grads live in the fused kernels)
        L.pkft = add_pack(L.w, PK_FRAGT, L.Rt, L.Ct, L.N, L.K, L.cin, L.taps, 0, 0, 0, 0, 0);
    };
    for (TLayer& t : layers) { pack_frag(t.inproj); pack_frag(t.outproj); pack_frag(t.ff1); pack_frag(t.ff2); }
    for (Lin& L : head) pack_frag(L);
    if (is_tf()) pack_frag(upconv);
    if (c.kind == V4L_NET_CNN || c.kind == V4L_NET_LOCO) pack_frag(proj);
    for (Lin& L : enc) pack_frag(L);
    for (int i = 0; i < 3 && c.kind != V4L_NET_MLP; ++i) {
      Conv& v = conv[i];
      v.pkf = add_pack(v.w, PK_FRAG, v.Np, v.Kp, v.Cout, v.K, v.chw ? 0 : v.Cin, v.KH * v.KH, v.KH, 0, 0, 0, 0);
    }
  }

  seg_blocks = 0;
  for (const ParamInfo& pi : params) seg_blocks += cdiv64(pi.numel, 256);
  p.assign(params.size(), nullptr);
  return 0;
}

int64_t v4l_net::table_bytes() const {
  return (int64_t)(packs.size() * sizeof(PackDesc) + params.size() * sizeof(ParamSeg) + MAX_RED * sizeof(RedDesc) +
                   MAX_TNP * sizeof(TnProb) + MAX_WIDE * sizeof(TnWide) + sq_cap() * sizeof(float) + 1024);
}
// the NatureCNN nets' dense stack as one launch per direction (csrc/dense_stack.h): the shipped widths only
static bool dense_stack_shape(const v4l_net* N) {
  const v4l_net_cfg& c = N->cfg;
  if (sw_on("V4L_NO_DENSE_STACK")) return false;  // (read per call: tests switch it)
  if (c.n_head_hidden != 2 || c.head_hidden[0] != 256 || c.head_hidden[1] != 256 || c.out_dim > OUT_LD) return false;
  for (int i = 0; i < 3; ++i)
    if (N->head[i].pkf < 0 || N->head[i].pkft < 0) return false;
  if (c.kind == V4L_NET_CNN_VIS) return N->head[0].Kp == 1024 && N->head[0].Rt == 1024;
  if (c.kind != V4L_NET_CNN) return false;
  return c.visual_dim == 256 && c.n_enc_hidden == 2 && c.enc_hidden[0] == 256 && c.enc_hidden[1] == 256 && N->proj.pkf >= 0 &&
         N->proj.pkft >= 0 && N->proj.Kp == 1024 && N->enc[1].pkft >= 0 && N->head[0].Kp == 512;
}
// the shapes the fused kernels are specialised for: the proprio MLP 256-256 on at most 128 inputs, heads 256-256, 4 x 64 x 64 depth
static bool mlp_256(const v4l_net_cfg& c) {
  return c.n_enc_hidden == 2 && c.enc_hidden[0] == 256 && c.enc_hidden[1] == 256 && c.state_dim <= 128;
}
static bool head_256(const v4l_net_cfg& c) { return c.n_head_hidden == 2 && c.head_hidden[0] == 256 && c.head_hidden[1] == 256; }
static bool depth_64(const v4l_net_cfg& c) { return c.in_channels == 4 && c.img_hw == 64; }
bool v4l_net::wps_tail_shape() const {  // (mlp_256 without its bound on state_dim, which belongs to the encoder kernels)
  return cfg.n_enc_hidden == 2 && cfg.enc_hidden[0] == 256 && cfg.enc_hidden[1] == 256;
}
// The route of the Transformer layers (net.h LayerRoute). The wave-per-sample kernels (csrc/wps.h) serve two layers of ff_dim 256
// under 256-256 heads; what surrounds the layers picks the family. Everything else with ff_dim 256 and neither token_norm nor
// use_pytorch_encoder runs the block-cooperative kernels (csrc/infer.h, bwd.h), the rest layer by layer.
LayerRoute v4l_net::layer_route(bool whole_pass) const {
  const v4l_net_cfg& c = cfg;
  LayerRoute r;
  // (read per call: tests switch them)
  r.taps = sw_on("V4L_LAYER_TAPS");
  r.stack_ok = !sw_on("V4L_NO_LAYER_STACK");
  r.tok0_in = sw_on("V4L_WPS_TOK0_IN");
  r.par_wgrad = sw_int("V4L_PAR_WGRAD", 2);
  const bool no_wps = sw_on("V4L_NO_WPS_LAYERS"), vis17 = sw_on("V4L_VIS17"), no_fb = sw_on("V4L_NO_FB");
  const bool head_in = sw_on("V4L_WPS_HEAD_IN"), ext_critic = sw_on("V4L_WPS_HEAD_EXT_CRITIC");
  if (!is_tf()) return r;
  const bool vis = c.kind == V4L_NET_LOCO_VIS, opt = c.token_norm || c.pytorch_encoder;
  const bool heads = head_256(c) && c.out_dim <= OUT_LD;
  const bool wps = c.ff_dim == 256 && c.n_layers == 2 && heads && layers[0].inproj.pkp >= 0 && !no_wps &&
                   (!vis || head[0].pko >= 0);
  // the routes with layer-by-layer launches around the wave-per-sample pair: mean pooling only, no test taps, a pass of their own
  const bool around = wps && whole_pass && !c.max_pool && r.stack_ok && !r.taps;
  r.family = LayerFamily::LAYER_BY_LAYER;
  if (vis) {
    // V4L_VIS17=1 (a test switches it) and the tapped test build: the 17-row instantiation (dummy row 0) instead of the native
    // 16-token one — the two are cross-checked against each other
    if (wps && whole_pass && !opt) r.family = (vis17 || r.taps) ? LayerFamily::WPS_VIS17 : LayerFamily::WPS_VIS;
    else if (around && opt) r.family = LayerFamily::WPS_OPT_VIS;
    r.rows17 = r.wps();
    r.heads_in = r.wps() && !c.pytorch_encoder;
    r.tail_in = r.wps() && !c.token_norm;
    return r;
  }
  const bool plain = !opt && wps_tail_shape();  // the shipped net; max_pool=True pools inside the wave-per-sample pair only
  if (wps && plain && r.stack_ok) {
    r.family = LayerFamily::WPS_PLAIN;
    r.heads_in = r.tail_in = true;
    r.heads_ext_allowed = !head_in && !r.taps;
    r.heads_ext_critic = r.heads_ext_allowed && ext_critic;
    // (the fused forward-loss-backward launch holds a row's action dimensions in capacity-8 arrays and is not widened: one wave
    // per SIMD at 512 registers, launch time grows with code size. A wider policy takes the TanhNormal policies' route.)
    r.fb_allowed = r.heads_ext_allowed && !c.max_pool && !no_fb && !ext_critic && c.out_dim <= ACT_CAP_NARROW;
  } else if (around && !plain) {
    // (use_pytorch_encoder alone leaves the encoder-side data-grads inside the launch like the plain net; token_norm takes them
    // layer by layer from token_ln's backward, another proprio MLP from the layer-0 input gradient)
    r.family = LayerFamily::WPS_OPT;
    r.heads_in = !c.pytorch_encoder;
    r.tail_in = !c.token_norm && wps_tail_shape();
  } else if (c.ff_dim == 256 && !opt) {
    // the last layer's blocks also run the pooled heads of their samples (mean pooling), layer 0's continue into the proprio MLP
    r.heads_in = c.n_layers >= 1 && heads && !c.max_pool;
    r.tail_in = c.n_layers >= 1 && wps_tail_shape();
    r.family = (r.heads_in && c.n_layers == 2 && r.stack_ok) ? LayerFamily::BLOCK_STACK : LayerFamily::BLOCK_PER_LAYER;
  }
  return r;
}
// The operands of the pooled heads' data-grad chain over the workspace `ws` laid out for n rows, for a caller (the trainer's
// loss launch) that runs the chain itself right before v4l_net_backward(ws, n): -> 1 and the backward pass is told (it then
// starts from dpool), or 0 when that backward pass will not be the wave-per-sample one (or V4L_WPS_HEAD_IN / test taps ask for
// the in-kernel heads).
int v4l_net::heads_ext(float* ws, int n, v4l::RowsChain* out, bool critic) {
  heads_ext_ws = nullptr;
  const LayerRoute r = layer_route();
  if (!bound || out == nullptr || !(critic ? r.heads_ext_critic : r.heads_ext_allowed)) return 0;
  const Layout L = layout(n);
  const size_t es = is_half(cfg.compute) ? 2 : 4;
  const char* base = (const char*)packed;
  out->wa = base + (size_t)head[2].pkt * es; out->wb = base + (size_t)head[1].pkt * es; out->wc = base + (size_t)head[0].pkt * es;
  out->ma = ws + L.hh[1]; out->mb = ws + L.hh[0];
  out->oa = ws + L.dhh[1]; out->ob = ws + L.dhh[0];
  out->oc = ws + L.dpool;
  heads_ext_ws = ws; heads_ext_n = n;
  return 1;
}

// Upper bound of the weight-grad slab arena for a batch of n: every weight tensor with the row count its
// gradient contraction runs over.
int64_t v4l_net::slab_floats(int n) const {
  int64_t tot = 0;
  auto add = [&](int M, int N, int Kx) {   // conv weight-grads (tn_plan) and, conservatively, dense ones
    const TnPlan p = tn_plan(M, N, Kx, is_half(cfg.compute));
    const int64_t dense_splits = 256;  // (lin_wgrad: at most 16384 / V4L_TN_BIG_ROWS slabs, rows per block >= 64)
    const int64_t np = round_up(N, 64), kp = round_up(Kx, 64);
    tot += std::max<int64_t>(p.slab_floats + p.bslab_floats, dense_splits * np * (kp + 1) + 128);
  };
  if (cfg.kind != V4L_NET_MLP) {
    for (int i = 0; i < 3; ++i) add(n * conv[i].OH * conv[i].OH, conv[i].Cout, conv[i].K);
    tot += (int64_t)CONV_BWD_MAX_BLOCKS * (32 * 256 + 64 * 512 + 64 * 576 + 3 * 64);  // fused conv backward: one slab set per block
  }
  if (is_tf()) add(n * 16, upconv.N, 64);
  if (cfg.kind == V4L_NET_LOCO) add(n, proj.N, proj.K);
  if (cfg.kind == V4L_NET_CNN) add(n, proj.N, 1024);
  for (size_t i = 0; i < enc.size(); ++i) add(n, enc[i].N, i == 0 ? Sp : enc[i].K);
  for (const TLayer& t : layers) {
    add(n * NTOK, t.inproj.N, t.inproj.K); add(n * NTOK, t.outproj.N, t.outproj.K);
    add(n * NTOK, t.ff1.N, t.ff1.K); add(n * NTOK, t.ff2.N, t.ff2.K);
    // LayerNorm dgamma/dbeta partials: one [64] row per block (<= 128 ln_bwd blocks, or n/4 fused-layer blocks)
    tot += 2 * 2 * (int64_t)std::max(128, cdiv(n, 2)) * TD;
  }
  for (const Lin& L : head) add(n, L.N, L.K);
  if (!layers.empty() && layers[0].inproj.pkp >= 0)  // wave-per-sample weight-grads: one slab set per run of WPS_SPLIT samples
    tot += (int64_t)layers.size() * cdiv(n, WPS_SPLIT) * (WPS_LAYER_ELEMS + 576) + 1024;
  if (cfg.kind == V4L_NET_LOCO) tot += 2 * (int64_t)cdiv(n, WPS_WPB) * FB_PART + 8;  // fused launch: per-block partial statistics (doubles)
  return tot;
}

Layout v4l_net::layout(int n) const {
  Layout L;
  L.n = n;
  int64_t off = 0;
  auto take = [&](int64_t floats) { int64_t o = off; off += (floats + 63) / 64 * 64; return o; };
  const v4l_net_cfg& c = cfg;
  // (the vision-only Transformer's token tensors are sized for 17 rows per sample too: its wave-per-sample path keeps the 16
  // tokens in rows 1..16 of a 17-row stride, the layer-by-layer path packs them 16 per sample into the same buffers)
  const int64_t R = (int64_t)n * (is_tf() ? NTOK : ntok);
  int maxw = 2 * TD;
  for (int i = 0; i < c.n_enc_hidden; ++i) maxw = std::max(maxw, c.enc_hidden[i]);
  for (int i = 0; i < c.n_head_hidden; ++i) maxw = std::max(maxw, c.head_hidden[i]);
  if (c.kind == V4L_NET_CNN) maxw = std::max(maxw, c.visual_dim + c.enc_hidden[c.n_enc_hidden - 1]);
  if (c.kind != V4L_NET_MLP) {
    L.c1 = take((int64_t)n * 225 * 32);
    L.c2 = take((int64_t)n * 36 * 64);
    L.c3 = take((int64_t)n * 16 * 64);
  }
  for (int i = 0; i < c.n_enc_hidden; ++i) L.eh.push_back(take((int64_t)n * c.enc_hidden[i]));
  if (c.kind == V4L_NET_CNN) L.vis = take((int64_t)n * (c.visual_dim + c.enc_hidden[c.n_enc_hidden - 1]));
  if (is_tf()) {
    for (int l = 0; l <= c.n_layers; ++l) L.x.push_back(take(R * TD));
    if (c.token_norm) { L.x0raw = take(R * TD); L.xh0 = take(R * TD); L.rs0 = take(R); L.dx0raw = take(R * TD); }
    if (c.pytorch_encoder) { L.xfin = take(R * TD); L.xhF = take(R * TD); L.rsF = take(R); L.dxfin = take(R * TD); }
    for (int l = 0; l < c.n_layers; ++l) {
      LayerWs w;
      w.qkv = take(R * 3 * TD);
      w.P = take((int64_t)n * NTOK * NTOK);
      w.ctx = take(R * TD);
      w.xh1 = take(R * TD);
      w.rs1 = take(R);
      w.x1 = take(R * TD);
      w.f = take(R * c.ff_dim);
      w.xh2 = take(R * TD);
      w.rs2 = take(R);
      w.xin = take(R * TD);
      L.lw.push_back(w);
    }
    L.ytmp = take(R * TD);
    L.pooled = take((int64_t)n * 2 * TD);
  }
  for (int i = 0; i < c.n_head_hidden; ++i) L.hh.push_back(take((int64_t)n * c.head_hidden[i]));
  L.out = take((int64_t)n * OUT_LD);
  L.dout = take((int64_t)n * OUT_LD);
  // backward tensors
  for (int i = 0; i < c.n_head_hidden; ++i) L.dhh.push_back(take((int64_t)n * c.head_hidden[i]));
  for (int i = 0; i < c.n_enc_hidden; ++i) L.deh.push_back(take((int64_t)n * c.enc_hidden[i]));
  L.dhc = take((int64_t)n * maxw);
  if (is_tf()) {
    for (int l = 0; l <= c.n_layers; ++l) L.dxl.push_back(take(R * TD));
    for (int l = 0; l < c.n_layers; ++l) {
      LayerBw b;
      b.dz2 = take(R * TD); b.df = take(R * c.ff_dim); b.dx1 = take(R * TD); b.dz1 = take(R * TD);
      b.dctx = take(R * TD); b.dqkv = take(R * 3 * TD);
      L.lb.push_back(b);
    }
    L.dpool = take((int64_t)n * 2 * TD);
    if (!layers.empty() && layers[0].inproj.pkp >= 0) {
      for (int l = 0; l < c.n_layers; ++l) {  // sized for fp32 operands (parity mode); bf16 uses half
        L.wps_wg.push_back(take((int64_t)n * WPS_WG_STRIDE));
        L.wps_tk.push_back(take((int64_t)n * WPS_TK_ELEMS));
      }
    }
  }
  if (c.kind != V4L_NET_MLP) {
    L.dc3 = take((int64_t)n * 16 * 64);
    L.dc2 = take((int64_t)n * 36 * 64);
    L.dc1 = take((int64_t)n * 225 * 32);
  }
  L.slab = take(slab_floats(n));
  L.total = off;
  return L;
}

// ------------------------------------------------------------------------------------------ forward
// The weights of one TransformerEncoderLayer / of the pooled heads as the fused layer kernels take them (csrc/infer.h). frag: the
// k-permuted fragment-order packs of the wave-per-sample kernels (pkp), else the row-major packs of the block-cooperative ones.
// The caller adds xout and the saves of its launch.
template <typename T>
static InfLayer inf_layer(const v4l_net* N, const TLayer& t, bool frag, const float* xin) {
  const T* base = (const T*)N->packed;
  float* const* p = N->p.data();
  InfLayer d;
  memset(&d, 0, sizeof(d));
  d.win = base + (frag ? t.inproj.pkp : t.inproj.pk); d.wo = base + (frag ? t.outproj.pkp : t.outproj.pk);
  d.w1 = base + (frag ? t.ff1.pkp : t.ff1.pk); d.w2 = base + (frag ? t.ff2.pkp : t.ff2.pk);
  d.bin = p[t.inproj.b]; d.bo = p[t.outproj.b]; d.b1 = p[t.ff1.b]; d.b2 = p[t.ff2.b];
  d.g1 = p[t.ln1.g]; d.be1 = p[t.ln1.b]; d.g2 = p[t.ln2.g]; d.be2 = p[t.ln2.b];
  d.xin = xin;
  return d;
}
// pko: the vision-only net's first head layer, whose 64 real K entries sit in the pooled operand's second half
template <typename T>
static InfHead inf_head(const v4l_net* N, const Layout& L, float* ws, bool pko) {
  const T* base = (const T*)N->packed;
  float* const* p = N->p.data();
  const std::vector<Lin>& head = N->head;
  InfHead h;
  memset(&h, 0, sizeof(h));
  h.w0 = base + (pko ? head[0].pko : head[0].pk); h.w1 = base + head[1].pk; h.w2 = base + head[2].pk;
  h.b0 = p[head[0].b]; h.b1 = p[head[1].b]; h.b2 = p[head[2].b];
  h.out = ws + L.out; h.nout = N->cfg.out_dim; h.max_pool = N->cfg.max_pool;  // (pooling by max: the wave-per-sample kernels only)
  h.s_pooled = ws + L.pooled; h.s_h0 = ws + L.hh[0]; h.s_h1 = ws + L.hh[1];
  return h;
}

template <typename T>
int v4l_net::forward_t(const float* state, const T* image, const int* rowidx, int n, float* ws, hipStream_t s,
                       const float* enc_ws, int stage) {
  const Layout L = layout(n);
  const v4l_net_cfg& c = cfg;
  Ctx cx{this, s, nullptr, nullptr, 0, s};
  int rc;
  const int ne = c.n_enc_hidden, nh = c.n_head_hidden;
  const ADense sin = dense(state, Sp, n, Sp, rowidx);
  Act eacts[V4L_MAX_HIDDEN];
  for (int i = 0; i < ne; ++i) eacts[i] = Act{ws + L.eh[i], c.enc_hidden[i], c.enc_hidden[i]};
  ADense head_in;
  // the Transformer layers' route (and the switches it read): a forward that starts from another net's encoder output, or runs
  // one stage only, stays off the vision / option routes (their 17-row slots are laid out by the encoder pass of a whole forward)
  const LayerRoute r = layer_route(enc_ws == nullptr && stage == 0);
  // an encoder pass over this workspace rewrites its c1 / c2: whatever type they held is gone (train_enc marks it again)
  if (enc_ws == nullptr && stage != 2 && c.kind != V4L_NET_MLP && acts16_c1 == ws + L.c1) acts16_c1 = nullptr;
  // persistent 16-wave encoder blocks (csrc/infer.h train_encoder_kernel<MODE>): conv weights enter a CU once, not once per
  // sample; saves c1 / c2 / c3 (what the conv backward reads) and, with a proprio branch, the two MLP activations
  const bool mlp256 = ne == 2 && c.enc_hidden[0] == 256 && c.enc_hidden[1] == 256 && c.state_dim <= 128;
  const bool train_enc_ok = sizeof(T) == 2 && c.kind != V4L_NET_MLP && conv[0].pkf >= 0 &&
                            (vis_only() || (mlp256 && enc[0].Kp == 128 && enc[0].pkf >= 0));
  auto train_enc = [&](auto mode_tag, float* x0, float* s_h2, int ld_h2, bool proprio = true) -> int {
    constexpr int MODE = decltype(mode_tag)::value;
    typedef typename HalfOf<T>::type H;  // (train_enc_ok: 16-bit operand types only)
    V4L_HIP_CHECK(lds_limit<&train_encoder_kernel<H, MODE>>(TrainEncLds::bytes));
    const H* pb = (const H*)packed;
    const bool tok = MODE == ENC_TOK17 || MODE == ENC_TOK16, prop = proprio && (MODE == ENC_TOK17 || MODE == ENC_FUSE);
    InfEncFrag ef;
    memset(&ef, 0, sizeof(ef));
    ef.w1 = pb + conv[0].pkf; ef.w2 = pb + conv[1].pkf; ef.w3 = pb + conv[2].pkf; ef.wup = tok ? pb + upconv.pkf : ef.w3;
    ef.b1 = p[conv[0].b]; ef.b2 = p[conv[1].b]; ef.b3 = p[conv[2].b]; ef.bup = tok ? p[upconv.b] : ef.b3;
    if (prop) {
      ef.wf1 = pb + enc[0].pkf; ef.wf2 = pb + enc[1].pkf; ef.wpr = MODE == ENC_TOK17 ? pb + proj.pkf : ef.wf2;
      ef.bf1 = p[enc[0].b]; ef.bf2 = p[enc[1].b]; ef.bpr = MODE == ENC_TOK17 ? p[proj.b] : ef.bf2;
    }
    ef.S = c.state_dim; ef.Sp = Sp;
    TrainEnc te;
    te.image = (const void*)image; te.state = state; te.rowidx = rowidx;
    te.s_c1 = ws + L.c1; te.s_c2 = ws + L.c2; te.s_c3 = ws + L.c3;
    te.s_h1 = prop ? ws + L.eh[0] : nullptr; te.s_h2 = s_h2; te.ld_h2 = ld_h2;
    te.n = n; te.nmlp = prop ? cdiv(n, 32) : 0;
    // (V4L_ACTS_F32: keep c1 / c2 in fp32 — the cross-check of tests/test_gpu_parity.py::test_conv_acts_in_operand_type_same_bits)
    te.acts16 = want_acts16 && conv_bwd_fusable(this) && !r.taps && !sw_on("V4L_ACTS_F32");
    if (te.acts16) acts16_c1 = te.s_c1;
    constexpr int cus = 256;
    // the conv share never collapses: a very large minibatch (n >~ 8 K: nmlp -> cus) still gets half the CUs' worth of
    // persistent conv blocks (the MLP blocks are short; the two kinds then simply run in two waves over the chip)
    te.nconv = std::max(1, std::min(n, std::max(cus / 2, cus - te.nmlp)));
    g_op = "encoder";
    V4L_KLAUNCH("fused_encoder", 2.0 * n * 3784064.0, s, (train_encoder_kernel<H, MODE>), dim3(te.nmlp + te.nconv), dim3(1024),
                TrainEncLds::bytes, s, ef, te, x0);
    V4L_LAUNCH_CHECK();
    return 0;
  };
  // NatureCNN nets, whole forward: visual projector + head as ONE launch behind the encoder (csrc/dense_stack.h)
  const bool dense_stack = stage == 0 && (c.kind == V4L_NET_CNN_VIS || (c.kind == V4L_NET_CNN && enc_ws == nullptr)) &&
                           dense_stack_shape(this);
  if (c.kind == V4L_NET_MLP) {
    if (enc_ws != nullptr) eacts[ne - 1].p = const_cast<float*>(enc_ws) + L.eh[ne - 1];
    else if (stage != 2 && (rc = chain_fwd<T>(cx, enc.data(), ne, sin, eacts, true))) return rc;
    head_in = dense(eacts[ne - 1].p, eacts[ne - 1].ld, n, eacts[ne - 1].w);
  } else if (c.kind == V4L_NET_CNN && enc_ws != nullptr) {
    const int cw = c.visual_dim + c.enc_hidden[ne - 1];
    head_in = dense(enc_ws + L.vis, cw, n, cw);
  } else if (c.kind == V4L_NET_CNN) {
    const int cw = c.visual_dim + c.enc_hidden[ne - 1];
    if (stage != 2 && train_enc_ok) {
      // one launch: conv stack + proprio MLP (its last activation lands in the concat buffer's right half), then the
      // visual projector on the NHWC flatten of conv3 -> columns [0, visual_dim)
      if ((rc = train_enc(std::integral_constant<int, ENC_FUSE>(), nullptr, ws + L.vis + c.visual_dim, cw))) return rc;
      Epi ep = mk_epi(ws + L.vis, cw, c.visual_dim, nullptr, 1);
      if (!dense_stack && (rc = lin_fwd<T>(cx, proj, dense(ws + L.c3, 1024, n, 1024), ep))) return rc;
    } else if (stage != 2) {
      // proprio MLP on the aux stream next to the conv stack; both land in the concat buffer
      if ((rc = par_begin(cx))) return rc;
      Ctx cx2 = cx;
      cx2.s = cx.tn;
      eacts[ne - 1] = Act{ws + L.vis + c.visual_dim, cw, c.enc_hidden[ne - 1]};
      if ((rc = chain_fwd<T>(cx2, enc.data(), ne, sin, eacts, true))) return rc;
      if ((rc = conv_stack_fwd<T>(cx, image, rowidx, n, ws + L.c1, ws + L.c2, ws + L.c3))) return rc;
      // visual projector on the NHWC flatten of conv3 -> columns [0, visual_dim) of the concat buffer
      Epi ep = mk_epi(ws + L.vis, cw, c.visual_dim, nullptr, 1);
      if (!dense_stack && (rc = lin_fwd<T>(cx, proj, dense(ws + L.c3, 1024, n, 1024), ep))) return rc;
      if ((rc = par_end(cx))) return rc;
    }
    head_in = dense(ws + L.vis, cw, n, cw);
  } else if (c.kind == V4L_NET_CNN_VIS) {
    // NatureEncoderProjNet (nets.py:176-191): conv stack -> Flatten -> head; the flatten is conv3's NHWC rows, the
    // first head layer's pack carries the NCHW -> NHWC permutation
    if (enc_ws == nullptr && stage != 2) {
      if (train_enc_ok) rc = train_enc(std::integral_constant<int, ENC_FLAT>(), nullptr, nullptr, 0);
      else rc = conv_stack_fwd<T>(cx, image, rowidx, n, ws + L.c1, ws + L.c2, ws + L.c3);
      if (rc) return rc;
    }
    head_in = dense((enc_ws != nullptr ? enc_ws : ws) + L.c3, 1024, n, 1024);
  } else {
    // token_norm: the encoder's tokens go to x0raw (of the workspace the encoder ran in), x[0] of THIS net's workspace takes
    // their LayerNorm — token_ln belongs to the net, not to the (possibly shared) encoder — and the layers read x[0] as ever
    float* x0 = c.token_norm ? (enc_ws != nullptr ? const_cast<float*>(enc_ws) : ws) + L.x0raw
                             : (enc_ws != nullptr ? const_cast<float*>(enc_ws) + L.x[0] : ws + L.x[0]);
    const bool fused_enc = ne == 2 && c.enc_hidden[0] == 256 && c.enc_hidden[1] == 256 && c.state_dim <= 128;
    if (enc_ws == nullptr && stage != 2 && fused_enc) {
      // one launch for the whole encoder (csrc/infer.h): a block per sample runs conv1..3 + up-conv out of LDS, extra
      // blocks run the proprio MLP; the activations backward_t needs are saved on the way
      V4L_HIP_CHECK(lds_limit<&infer_encoder_kernel<T>>(InfEncLds<T>::bytes));
      const T* pk = (const T*)packed;
      InfEnc en;
      en.w1 = pk + conv[0].pk; en.w2 = pk + conv[1].pk; en.w3 = pk + conv[2].pk; en.wup = pk + upconv.pk;
      en.b1 = p[conv[0].b]; en.b2 = p[conv[1].b]; en.b3 = p[conv[2].b]; en.bup = p[upconv.b];
      en.wf1 = pk + enc[0].pk; en.wf2 = pk + enc[1].pk; en.wpr = pk + proj.pk;
      en.bf1 = p[enc[0].b]; en.bf2 = p[enc[1].b]; en.bpr = p[proj.b];
      en.S = c.state_dim; en.Sp = Sp; en.Kp1 = enc[0].Kp;
      InfEncTrain tr;
      tr.image = image; tr.state = state; tr.rowidx = rowidx;
      tr.s_c1 = ws + L.c1; tr.s_c2 = ws + L.c2; tr.s_c3 = ws + L.c3; tr.s_h1 = ws + L.eh[0]; tr.s_h2 = ws + L.eh[1];
      g_op = "encoder";
      if (train_enc_ok && c.kind == V4L_NET_LOCO) {
        if ((rc = train_enc(std::integral_constant<int, ENC_TOK17>(), x0, ws + L.eh[1], 256))) return rc;
      } else {
        V4L_KLAUNCH("fused_encoder", 2.0 * n * 3784064.0, s, infer_encoder_kernel<T>, dim3(n + cdiv(n, 32)), dim3(256),
                    InfEncLds<T>::bytes, s, (const ActCtl*)nullptr, (const float*)nullptr, n, en, (float*)nullptr, (T*)nullptr, x0,
                    tr);
      }
      V4L_LAUNCH_CHECK();
    } else if (enc_ws == nullptr && stage != 2 && c.kind == V4L_NET_LOCO_VIS) {
      // TransformerEncoder (base.py:388-494, depth only): conv stack -> 1x1 up-conv -> the 16 patch tokens, in order
      // wave-per-sample path: the 16 tokens go to rows 1..16 of a 17-row stride (row 0 = the dummy row, csrc/wps.h)
      if (train_enc_ok) {
        if (r.rows17) rc = train_enc(std::integral_constant<int, ENC_TOK17>(), x0, nullptr, 0, false);
        else rc = train_enc(std::integral_constant<int, ENC_TOK16>(), x0, nullptr, 0);
        if (rc) return rc;
      } else {
        if ((rc = conv_stack_fwd<T>(cx, image, rowidx, n, ws + L.c1, ws + L.c2, ws + L.c3))) return rc;
        Epi ep = mk_epi(x0, TD, TD);
        if (r.rows17) ep.rowmap = ROWMAP_TOK_DEPTH;
        if ((rc = lin_fwd<T>(cx, upconv, dense(ws + L.c3, 64, n * 16, 64), ep))) return rc;
      }
    } else if (enc_ws == nullptr && stage != 2) {
      // proprio branch (MLP + state_projector -> token 0) on the aux stream next to the conv branch (-> tokens 1..16)
      if ((rc = par_begin(cx))) return rc;
      Ctx cx2 = cx;
      cx2.s = cx.tn;
      if ((rc = chain_fwd<T>(cx2, enc.data(), ne, sin, eacts, true))) return rc;
      {  // state_projector + ReLU -> token 0   (base.py:611-615)
        Epi ep = mk_epi(x0, TD, TD, nullptr, 1);
        ep.rowmap = ROWMAP_TOK_STATE;
        if ((rc = lin_fwd<T>(cx2, proj, dense(eacts[ne - 1].p, eacts[ne - 1].ld, n, eacts[ne - 1].w), ep))) return rc;
      }
      if ((rc = conv_stack_fwd<T>(cx, image, rowidx, n, ws + L.c1, ws + L.c2, ws + L.c3))) return rc;
      {  // depth_up_conv (1x1, no activation) -> tokens 1..16   (base.py:581,602-608)
        Epi ep = mk_epi(x0, TD, TD);
        ep.rowmap = ROWMAP_TOK_DEPTH;
        if ((rc = lin_fwd<T>(cx, upconv, dense(ws + L.c3, 64, n * 16, 64), ep))) return rc;
      }
      if ((rc = par_end(cx))) return rc;
    }
    if (stage == 1) return 0;
    // (vision-only net with token_norm / use_pytorch_encoder on the wave-per-sample layers: 17-row slots, the dummy rows zeroed
    // wherever a LayerNorm launch walks over them)
    const bool vis_opt = r.family == LayerFamily::WPS_OPT_VIS;
    const int R = n * (vis_opt ? NTOK : ntok);
    auto zero_row0 = [&](float* rows) {
      return hipMemset2DAsync(rows, (size_t)NTOK * TD * sizeof(float), 0, (size_t)TD * sizeof(float), (size_t)n, s);
    };
    if (vis_opt && c.token_norm) V4L_HIP_CHECK(zero_row0(x0));
    if (c.token_norm) {  // out = token_ln(visual_out) (nets.py:879-880, 1007-1008): LayerNorm of (tokens + 0)
      V4L_HIP_CHECK(hipMemsetAsync(ws + L.ytmp, 0, (size_t)R * TD * sizeof(float), s));
      g_op = "token_ln";
      V4L_KLAUNCH("add_ln_fwd", 0, s, add_ln_fwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, (const float*)x0, (const float*)(ws + L.ytmp), R,
                  (const float*)p[tok_ln.g], (const float*)p[tok_ln.b], ws + L.x[0], ws + L.xh0, ws + L.rs0);
      V4L_LAUNCH_CHECK();
      x0 = ws + L.x[0];
    }
    InfHeadPair hd;  // (an option route without heads_in launches with the slots filled too; its kernel does not read them)
    memset(&hd, 0, sizeof(hd));
    if (r.wps() || r.heads_in) hd.n[0] = inf_head<T>(this, L, ws, r.rows17);
    g_op = "layer";
    if (r.wps()) {
      // wave-per-sample launch (csrc/wps.h): both layers + the pooled heads, 4 samples per block, weights resident in LDS
      InfLayerStack stk;
      memset(&stk, 0, sizeof(stk));
      stk.nl = 2;
      for (int k = 0; k < 2; ++k) {
        const LayerWs& w = L.lw[k];
        InfLayer& d = stk.l[k].n[0];
        d = inf_layer<T>(this, layers[k], true, k == 0 ? x0 : ws + L.x[k]);
        // production: the forward saves nothing but the layers' input rows (the backward recomputes, csrc/wps.h);
        // V4L_LAYER_TAPS=1 (tests): every intermediate goes out row-major, as the block-cooperative kernels save them
        // (max_pool: the backward finds the arg-max tokens again from the stack's output rows)
        // (use_pytorch_encoder: the final norm is a launch of its own behind this one)
        d.xout = (k + 1 < 2 || r.taps || c.max_pool || c.pytorch_encoder) ? ws + L.x[k + 1] : nullptr;
        if (r.taps) {
          d.s_qkv = ws + w.qkv; d.s_P = ws + w.P; d.s_ctx = ws + w.ctx; d.s_xh1 = ws + w.xh1; d.s_rs1 = ws + w.rs1;
          d.s_x1 = ws + w.x1; d.s_f = ws + w.f; d.s_xh2 = ws + w.xh2; d.s_rs2 = ws + w.rs2;
          d.s_xin = sizeof(T) == 2 ? ws + w.xin : nullptr;
        }
      }
#define V4L_WPS_FWD(HEAD_, TAPS_, VIS_)                                                                                   \
  do {                                                                                                                    \
    V4L_HIP_CHECK(lds_limit<&wps_layer_fwd_kernel<T, HEAD_, 2, TAPS_, VIS_>>(WpsFwdLds<T>::bytes));                       \
    if (HEAD_)                                                                                                            \
      V4L_KLAUNCH("wps_layer_stack_head", 2.0 * n * (2 * 872576.0 + 99840.0), s, (wps_layer_fwd_kernel<T, HEAD_, 2, TAPS_, VIS_>), \
                  dim3(cdiv(n, WPS_WPB)), dim3(256), (WpsFwdLds<T>::bytes), s, stk, hd, n);                               \
    else  /* layers only: final norm, pooling and heads follow below */                                                   \
      V4L_KLAUNCH("wps_layer_stack", 2.0 * n * (2 * 872576.0), s, (wps_layer_fwd_kernel<T, HEAD_, 2, TAPS_, VIS_>),        \
                  dim3(cdiv(n, WPS_WPB)), dim3(256), (WpsFwdLds<T>::bytes), s, stk, hd, n);                               \
  } while (0)
      switch (r.family) {
        case LayerFamily::WPS_OPT_VIS:
          if (r.heads_in) V4L_WPS_FWD(true, false, 2);
          else V4L_WPS_FWD(false, false, 2);
          break;
        case LayerFamily::WPS_OPT:
          if (r.heads_in) V4L_WPS_FWD(true, false, 0);
          else V4L_WPS_FWD(false, false, 0);
          break;
        case LayerFamily::WPS_VIS17:
          if (r.taps) V4L_WPS_FWD(true, true, 1);
          else V4L_WPS_FWD(true, false, 1);
          break;
        case LayerFamily::WPS_VIS:  // native 16-token instantiation: one token tile per sample (round 5)
          V4L_WPS_FWD(true, false, 2);
          break;
        default:  // WPS_PLAIN
          if (r.taps) V4L_WPS_FWD(true, true, 0);
          else V4L_WPS_FWD(true, false, 0);
      }
#undef V4L_WPS_FWD
      V4L_LAUNCH_CHECK();
    }
    // block-cooperative kernels (csrc/infer.h): both layers + the heads in ONE launch when the stack is the shipped two layers
    // (the token rows stay in LDS between the layers); otherwise one launch per TransformerEncoderLayer. 2 or 4 samples per
    // block, saving what backward_t reads.
    const bool stacked = r.family == LayerFamily::BLOCK_STACK;
    for (int l = 0; l < c.n_layers && r.block(); l += stacked ? 2 : 1) {
      // samples per block: 2 (48 MFMA rows, 2 blocks/CU: measured 20 % faster) or 4 (80 rows, 1 block/CU; not in fp32: 168 KB)
      static int spw = 2;
      InfLayerStack stk;
      memset(&stk, 0, sizeof(stk));
      stk.nl = stacked ? 2 : 1;
      for (int k = 0; k < stk.nl; ++k) {
        const LayerWs& w = L.lw[l + k];
        InfLayer& d = stk.l[k].n[0];
        d = inf_layer<T>(this, layers[l + k], false, l + k == 0 ? x0 : ws + L.x[l + k]);
        d.xout = ws + L.x[l + k + 1];
        d.s_qkv = ws + w.qkv; d.s_P = ws + w.P; d.s_ctx = ws + w.ctx; d.s_xh1 = ws + w.xh1; d.s_rs1 = ws + w.rs1;
        d.s_x1 = ws + w.x1; d.s_f = ws + w.f; d.s_xh2 = ws + w.xh2; d.s_rs2 = ws + w.rs2;
        d.s_xin = sizeof(T) == 2 ? ws + w.xin : nullptr;  // fp32 mode: the fp32 token tensor itself is the operand
      }
      const bool head_on = r.heads_in && l + stk.nl == c.n_layers;  // the last layer's blocks run the heads of their samples
      InfHeadPair none;
      memset(&none, 0, sizeof(none));
      const InfHeadPair& hp = head_on ? hd : none;
      InfFinish fin;
      memset(&fin, 0, sizeof(fin));
#define V4L_BLOCK_FWD(SPW_, HEAD_, NL_, LABEL_, FLOPS_)                                                                   \
  do {                                                                                                                    \
    V4L_HIP_CHECK(lds_limit<&infer_layer_kernel<T, SPW_, HEAD_, NL_>>(InfLayLds<T, SPW_>::bytes));                        \
    V4L_KLAUNCH(LABEL_, FLOPS_, s, (infer_layer_kernel<T, SPW_, HEAD_, NL_>), dim3(cdiv(n, SPW_), 1), dim3(256),          \
                (InfLayLds<T, SPW_>::bytes), s, stk, hp, fin, n, c.ff_dim);                                               \
  } while (0)
#define V4L_BLOCK_FWDS(SPW_)                                                                                              \
  do {                                                                                                                    \
    if (stacked) V4L_BLOCK_FWD(SPW_, true, 2, "fused_layer_stack_head", 2.0 * n * (2 * 872576.0 + 99840.0));              \
    else if (head_on) V4L_BLOCK_FWD(SPW_, true, 1, "fused_layer_head", 2.0 * n * (872576.0 + 99840.0));                   \
    else V4L_BLOCK_FWD(SPW_, false, 1, "fused_layer", 2.0 * n * 872576.0);                                                \
  } while (0)
      if (spw == 2) V4L_BLOCK_FWDS(2);
      else V4L_BLOCK_FWDS(4);
#undef V4L_BLOCK_FWDS
#undef V4L_BLOCK_FWD
      V4L_LAUNCH_CHECK();
    }
    if (r.heads_in) return 0;
    for (int l = 0; l < c.n_layers && r.family == LayerFamily::LAYER_BY_LAYER; ++l) {
      const TLayer& t = layers[l];
      const LayerWs& w = L.lw[l];
      float* xin = l == 0 ? x0 : ws + L.x[l];
      if ((rc = lin_fwd<T>(cx, t.inproj, dense(xin, TD, R, TD), mk_epi(ws + w.qkv, 3 * TD, 3 * TD)))) return rc;
      g_op = "attn";
      if (ntok == NTOK)
        V4L_KLAUNCH("attn_fwd", 4.0 * n * NTOK * NTOK * TD, s, attn_fwd_kernel<NTOK>, dim3(n), dim3(256), 0, s, ws + w.qkv, n, ws + w.P, ws + w.ctx, (int)ModeOf<T>::value);
      else
        V4L_KLAUNCH("attn_fwd", 4.0 * n * 16 * 16 * TD, s, attn_fwd_kernel<16>, dim3(n), dim3(256), 0, s, ws + w.qkv, n, ws + w.P, ws + w.ctx, (int)ModeOf<T>::value);
      V4L_LAUNCH_CHECK();
      if ((rc = lin_fwd<T>(cx, t.outproj, dense(ws + w.ctx, TD, R, TD), mk_epi(ws + L.ytmp, TD, TD)))) return rc;
      g_op = "ln1";
      V4L_KLAUNCH("add_ln_fwd", 0, s, add_ln_fwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, xin, ws + L.ytmp, R, p[t.ln1.g], p[t.ln1.b],
                         ws + w.x1, ws + w.xh1, ws + w.rs1);
      V4L_LAUNCH_CHECK();
      if ((rc = lin_fwd<T>(cx, t.ff1, dense(ws + w.x1, TD, R, TD), mk_epi(ws + w.f, c.ff_dim, c.ff_dim, nullptr, 1)))) return rc;
      if ((rc = lin_fwd<T>(cx, t.ff2, dense(ws + w.f, c.ff_dim, R, c.ff_dim), mk_epi(ws + L.ytmp, TD, TD)))) return rc;
      g_op = "ln2";
      V4L_KLAUNCH("add_ln_fwd", 0, s, add_ln_fwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, ws + w.x1, ws + L.ytmp, R, p[t.ln2.g],
                         p[t.ln2.b], ws + L.x[l + 1], ws + w.xh2, ws + w.rs2);
      V4L_LAUNCH_CHECK();
    }
    const float* xlast = ws + L.x[c.n_layers];
    if (vis_opt && c.pytorch_encoder) V4L_HIP_CHECK(zero_row0(ws + L.x[c.n_layers]));  // (the layers' launch wrote rows 1..16)
    if (c.pytorch_encoder) {  // nn.TransformerEncoder's final norm (nets.py:884-885, 1012-1013): LayerNorm of (rows + 0)
      V4L_HIP_CHECK(hipMemsetAsync(ws + L.ytmp, 0, (size_t)R * TD * sizeof(float), s));
      g_op = "final_ln";
      V4L_KLAUNCH("add_ln_fwd", 0, s, add_ln_fwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, xlast, (const float*)(ws + L.ytmp), R,
                  (const float*)p[fin_ln.g], (const float*)p[fin_ln.b], ws + L.xfin, ws + L.xhF, ws + L.rsF);
      V4L_LAUNCH_CHECK();
      xlast = ws + L.xfin;
    }
    g_op = "pool";
    if (c.kind == V4L_NET_LOCO_VIS) {
      V4L_KLAUNCH("pool_fwd", 0, s, pool_all_fwd_kernel, dim3(n), dim3(64), 0, s, xlast + (vis_opt ? TD : 0), n, ntok,
                  vis_opt ? NTOK : ntok, ws + L.pooled, c.max_pool);
      head_in = dense(ws + L.pooled, TD, n, TD);
    } else {
      V4L_KLAUNCH("pool_fwd", 0, s, pool_fwd_kernel, dim3(n), dim3(128), 0, s, xlast, n, ws + L.pooled, c.max_pool);
      head_in = dense(ws + L.pooled, 2 * TD, n, 2 * TD);
    }
    V4L_LAUNCH_CHECK();
  }
  if (stage == 1) return 0;
  if (dense_stack) {
    const bool fuse = c.kind == V4L_NET_CNN;
    const T* pb = (const T*)packed;
    DsFwd a;
    memset(&a, 0, sizeof(a));
    a.c3 = head_in.p;  // (vision-only net: the flatten is the head's input, possibly another net's workspace)
    if (fuse) { a.c3 = ws + L.c3; a.cat = ws + L.vis; a.wp = pb + proj.pkf; a.bp = p[proj.b]; }
    a.w0 = pb + head[0].pkf; a.w1 = pb + head[1].pkf; a.w2 = pb + head[2].pkf;
    a.b0 = p[head[0].b]; a.b1 = p[head[1].b]; a.b2 = p[head[2].b];
    a.h0 = ws + L.hh[0]; a.h1 = ws + L.hh[1]; a.out = ws + L.out;
    a.n = n; a.nout = c.out_dim;
    V4L_HIP_CHECK(lds_limit<&dense_stack_fwd_kernel<T, true>>(DsFwdLds<T>::bytes));
    V4L_HIP_CHECK(lds_limit<&dense_stack_fwd_kernel<T, false>>(DsFwdLds<T>::bytes));
    g_op = "dense.stack";
    const double fl = 2.0 * n * ((fuse ? 1024.0 * 256 + 512.0 * 256 : 1024.0 * 256) + 256.0 * 256 + 256.0 * c.out_dim);
    const dim3 grid(cdiv(n, 16 * DsCfg<T>::MT));
    if (fuse) V4L_KLAUNCH("dense_stack_fwd", fl, s, (dense_stack_fwd_kernel<T, true>), grid, dim3(256), DsFwdLds<T>::bytes, s, a);
    else V4L_KLAUNCH("dense_stack_fwd", fl, s, (dense_stack_fwd_kernel<T, false>), grid, dim3(256), DsFwdLds<T>::bytes, s, a);
    V4L_LAUNCH_CHECK();
    return 0;
  }
  Act hacts[V4L_MAX_HIDDEN + 1];
  for (int i = 0; i < nh; ++i) hacts[i] = Act{ws + L.hh[i], c.head_hidden[i], c.head_hidden[i]};
  hacts[nh] = Act{ws + L.out, OUT_LD, c.out_dim};
  // the last layer writes only out_dim columns: the padded row's other columns are zeros
  if (OUT_LD > head[nh].Np) V4L_HIP_CHECK(hipMemsetAsync(ws + L.out, 0, (size_t)n * OUT_LD * sizeof(float), s));
  return chain_fwd<T>(cx, head.data(), nh + 1, head_in, hacts, false, true);
}

// ------------------------------------------------------------------------------------------ backward
template <typename T>
int v4l_net::backward_t(const float* state, const T* image, const int* rowidx, int n, float* ws, float* grads,
                        hipStream_t s) {
  const Layout L = layout(n);
  const v4l_net_cfg& c = cfg;
  Ctx cx{this, s, grads, ws + L.slab, 0, s};
  const LayerRoute r = layer_route();  // the Transformer layers' route, as the forward of this pass took it, and the switches
  cx.taps = r.taps;
  red.clear();
  tnp.clear();
  tnp_flops = 0;
  wide.clear();
  wide_flops = 0;
  slab_cap = slab_floats(n);
  // (V4L_F16: the d(out) rows came scaled — by the rule, or by what the caller announced; wgrad_reduce multiplies it out)
  grad_unscale = 1.f / ((c.compute == V4L_F16 && grad_scale_next > 0.f) ? grad_scale_next : v4l_net_grad_scale(this, n));
  grad_scale_next = 0.f;
  int rc;
  const int ne = c.n_enc_hidden, nh = c.n_head_hidden;
  const ADense sin = dense(state, Sp, n, Sp, rowidx);
  Act eacts[V4L_MAX_HIDDEN];
  float* dehp[V4L_MAX_HIDDEN];
  for (int i = 0; i < ne; ++i) {
    eacts[i] = Act{ws + L.eh[i], c.enc_hidden[i], c.enc_hidden[i]};
    dehp[i] = ws + L.deh[i];
  }
  Act hacts[V4L_MAX_HIDDEN + 1];
  float* dhhp[V4L_MAX_HIDDEN];
  for (int i = 0; i < nh; ++i) {
    hacts[i] = Act{ws + L.hh[i], c.head_hidden[i], c.head_hidden[i]};
    dhhp[i] = ws + L.dhh[i];
  }
  hacts[nh] = Act{ws + L.out, OUT_LD, c.out_dim};
  const ADense dy = dense(ws + L.dout, OUT_LD, n, OUT_LD);

  auto conv_bwd_and_wgrads = [&]() -> int {
  int rc;
  // The three weight-grad launches (grouped dense, the layers' whole-output one, dW3) only depend on what the data-grad kernels
  // left behind. Measured in the update graph (ms per 48 updates): all serial 33.75; dense ones forked next to the conv-stack
  // data-grads 33.7 (bwd_conv_kernel holds every CU: nothing fits beside it); conv-stack data-grads FIRST, then dW3 on the
  // main stream next to the two dense launches on the auxiliary stream 32.8 (default); three branches 34.8.
  // V4L_PAR_WGRAD=0: serial, 1: the older fork.
  const int par_wgrad = r.par_wgrad;
  if (par_wgrad == 2 || par_wgrad == 3) {
    cx.defer_conv3 = true;
    if ((rc = conv_stack_bwd<T>(cx, image, rowidx, n, ws + L.c1, ws + L.c2, ws + L.dc3, ws + L.dc2, ws + L.dc1))) return rc;
    if ((rc = par_begin(cx, true))) return rc;  // a graph fork / join under capture
    // 3: the grouped dense weight-grads as a third branch beside wps_wgrad (auxiliary stream) and dW3 (main stream)
    const bool three = par_wgrad == 3 && aux2 != nullptr && cx.tn != cx.s && cx.wps_pending;
    if (three) {
      V4L_HIP_CHECK(hipEventRecord(ev_fork2, cx.s));
      V4L_HIP_CHECK(hipStreamWaitEvent(aux2, ev_fork2, 0));
    }
    // round 4: the reduction inside the forked section — the conv stack's partials (56 MB) right behind dW3 on the main
    // stream, the others behind the grouped weight-grads on the auxiliary stream — so that the join only gates clip_adam
    // (the update timeline showed 9 - 11 us of join latency in front of a 19 us reduce launch). V4L_SPLIT_REDUCE=0: one launch
    // behind the join. (Same descriptor order, hence the same bits, either way.)
    const bool split_red = !three && cx.tn != cx.s && sw_int("V4L_SPLIT_REDUCE", 1) != 0;
    int64_t rblocks[2] = {0, 0};
    if (split_red && (rc = wgrad_reduce_prepare(cx, rblocks))) return rc;
    if (split_red) {
      // (issue order matters to the graph's schedule: the auxiliary branch is the longer one and goes first)
      const size_t nred = cx.net->red.size();
      // (round 6: the fused launch's statistics block rides on the main stream in front of dW3 — the shorter branch;
      // wgrad_dense would put it at the head of the longer one. Launched AFTER the auxiliary branch's kernels were issued.)
      const bool fb_main = cx.fb_pending && cx.tn != cx.s;
      Ctx fbc = cx;
      if (fb_main) cx.fb_pending = false;
      if ((rc = wgrad_dense<T>(cx, cx.tn, nullptr))) return rc;
      if (fb_main && (rc = fb_finish(fbc, cx.s))) return rc;
      V4L_REQUIRE(cx.net->red.size() == nred, "internal: a weight-grad registered after the reduce table was prepared");
      if ((rc = conv3_wgrad_deferred<T>(cx, cx.s))) return rc;
      if ((rc = wgrad_reduce_launch(cx, 0, rblocks[0], cx.s))) return rc;
      if ((rc = wgrad_reduce_launch(cx, rblocks[0], rblocks[1], cx.tn))) return rc;
      return par_end(cx);
    }
    if ((rc = wgrad_dense<T>(cx, cx.tn, three ? aux2 : nullptr))) return rc;
    if ((rc = conv3_wgrad_deferred<T>(cx, cx.s))) return rc;
    if (three) {
      V4L_HIP_CHECK(hipEventRecord(ev_join2, aux2));
      V4L_HIP_CHECK(hipStreamWaitEvent(cx.s, ev_join2, 0));
    }
    if ((rc = par_end(cx))) return rc;
    return wgrad_reduce_all<T>(cx);
  }
  if (par_wgrad == 1 && (rc = par_begin(cx, true))) return rc;
  if ((rc = wgrad_dense<T>(cx, cx.tn))) return rc;
  if ((rc = conv_stack_bwd<T>(cx, image, rowidx, n, ws + L.c1, ws + L.c2, ws + L.dc3, ws + L.dc2, ws + L.dc1))) return rc;
  if ((rc = par_end(cx))) return rc;
  return wgrad_reduce_all<T>(cx);
  };

  if (c.kind == V4L_NET_MLP) {
    // head stack, then the base MLP; the grad w.r.t. the base output (through its activation: ReLU mask or 1 - a^2) is handed
    // over in `hand`
    const Act& last = eacts[ne - 1];
    float* hand = ws + L.dhc;
    Epi din = mk_epi(hand, last.w, last.w);
    din.mask = last.p;
    din.ldmask = last.ld;
    din.mask_mode = epi_mask_mode(this);
    if ((rc = chain_bwd<T>(cx, head.data(), nh + 1, dense(last.p, last.ld, n, last.w), hacts, dy, dhhp, &din))) return rc;
    if ((rc = chain_bwd<T>(cx, enc.data(), ne, sin, eacts, dense(hand, last.w, n, last.w), dehp, nullptr))) return rc;
    return wgrad_finish<T>(cx);
  }

  // NatureCNN nets: the dense stack's data-grads as ONE launch (csrc/dense_stack.h); the weight-grads are registered in the
  // order chain_bwd registers them (same grouped launch, same reduce table, same norm partials)
  if ((c.kind == V4L_NET_CNN || c.kind == V4L_NET_CNN_VIS) && dense_stack_shape(this)) {
    const bool fuse = c.kind == V4L_NET_CNN;
    const int cw = 512;
    float* hand = ws + L.dhc;
    const T* pb = (const T*)packed;
    DsBwd a;
    memset(&a, 0, sizeof(a));
    a.dout = ws + L.dout;
    a.w2t = pb + head[2].pkft; a.w1t = pb + head[1].pkft; a.w0t = pb + head[0].pkft;
    a.h1 = ws + L.hh[1]; a.h0 = ws + L.hh[0]; a.c3 = ws + L.c3;
    a.dh1 = dhhp[1]; a.dh0 = dhhp[0]; a.dc3 = ws + L.dc3;
    if (fuse) {
      a.wpt = pb + proj.pkft; a.wf2t = pb + enc[1].pkft;
      a.cat = ws + L.vis; a.e0 = ws + L.eh[0]; a.dcat = hand; a.de0 = dehp[0];
    }
    a.n = n;
    V4L_HIP_CHECK(lds_limit<&dense_stack_bwd_kernel<T, true>>(DsBwdLds<T>::bytes));
    V4L_HIP_CHECK(lds_limit<&dense_stack_bwd_kernel<T, false>>(DsBwdLds<T>::bytes));
    g_op = "dense.stack.bwd";
    const double fl = 2.0 * n * (256.0 * c.out_dim + 256.0 * 256 + (fuse ? 512.0 * 256 + 1024.0 * 256 + 256.0 * 256 : 1024.0 * 256));
    const dim3 grid(cdiv(n, 16 * DsCfg<T>::MT));
    if (fuse) V4L_KLAUNCH("dense_stack_bwd", fl, s, (dense_stack_bwd_kernel<T, true>), grid, dim3(256), DsBwdLds<T>::bytes, s, a);
    else V4L_KLAUNCH("dense_stack_bwd", fl, s, (dense_stack_bwd_kernel<T, false>), grid, dim3(256), DsBwdLds<T>::bytes, s, a);
    V4L_LAUNCH_CHECK();
    const ADense x_in = fuse ? dense(ws + L.vis, cw, n, cw) : dense(ws + L.c3, 1024, n, 1024);
    if ((rc = lin_wgrad<T>(cx, head[2], dy, dense(hacts[1].p, 256, n, 256), 256))) return rc;
    if ((rc = lin_wgrad<T>(cx, head[1], dense(dhhp[1], 256, n, 256), dense(hacts[0].p, 256, n, 256), 256))) return rc;
    if ((rc = lin_wgrad<T>(cx, head[0], dense(dhhp[0], 256, n, 256), x_in, x_in.K))) return rc;
    if (fuse) {
      ADense yv = dense(hand, cw, n, c.visual_dim, nullptr, 0, ws + L.vis);
      if ((rc = lin_wgrad<T>(cx, proj, yv, dense(ws + L.c3, 1024, n, 1024), 1024))) return rc;
      ADense ys = dense(hand + c.visual_dim, cw, n, 256, nullptr, 0, ws + L.vis + c.visual_dim);
      if ((rc = lin_wgrad<T>(cx, enc[1], ys, dense(ws + L.eh[0], 256, n, 256), 256))) return rc;
      if ((rc = lin_wgrad<T>(cx, enc[0], dense(dehp[0], 256, n, 256), sin, sin.K))) return rc;
    }
    return conv_bwd_and_wgrads();
  }

  if (c.kind == V4L_NET_CNN) {
    const int cw = c.visual_dim + c.enc_hidden[ne - 1];
    eacts[ne - 1] = Act{ws + L.vis + c.visual_dim, cw, c.enc_hidden[ne - 1]};
    float* hand = ws + L.dhc;  // grad w.r.t. the concat [visual_out | state_out], both post-ReLU
    Epi din = mk_epi(hand, cw, cw);
    if ((rc = chain_bwd<T>(cx, head.data(), nh + 1, dense(ws + L.vis, cw, n, cw), hacts, dy, dhhp, &din))) return rc;
    {  // visual branch: ReLU mask applied on load; data-grad lands in dc3 viewed as the NHWC flatten [n][1024]
      ADense yv = dense(hand, cw, n, c.visual_dim, nullptr, 0, ws + L.vis);
      if ((rc = lin_wgrad<T>(cx, proj, yv, dense(ws + L.c3, 1024, n, 1024), 1024))) return rc;
      Epi ep = mk_epi(ws + L.dc3, 1024, 1024);
      ep.mask = ws + L.c3;
      ep.ldmask = 1024;
      if ((rc = lin_dgrad<T>(cx, proj, yv, ep))) return rc;
    }
    {  // state branch
      ADense ys = dense(hand + c.visual_dim, cw, n, c.enc_hidden[ne - 1], nullptr, 0, ws + L.vis + c.visual_dim);
      if ((rc = chain_bwd<T>(cx, enc.data(), ne, sin, eacts, ys, dehp, nullptr))) return rc;
    }
    return conv_bwd_and_wgrads();  // (round 4: the forked weight-grad section of the LocoTransformer backward, dW3 next to the dense ones)
  }

  if (c.kind == V4L_NET_CNN_VIS) {
    // head stack; its data-grad lands in dc3 viewed as the NHWC flatten [n][1024], masked by conv3's ReLU
    Epi din = mk_epi(ws + L.dc3, 1024, 1024);
    din.mask = ws + L.c3;
    din.ldmask = 1024;
    if ((rc = chain_bwd<T>(cx, head.data(), nh + 1, dense(ws + L.c3, 1024, n, 1024), hacts, dy, dhhp, &din))) return rc;
    return conv_bwd_and_wgrads();
  }

  // ---- LocoTransformer / vision-only Transformer
  const bool vis = c.kind == V4L_NET_LOCO_VIS;
  const int pw = vis ? TD : 2 * TD;  // pooled width
  // (vision-only net with token_norm / use_pytorch_encoder around the wave-per-sample layers: 17-row slots — see forward_t)
  const bool vis_opt = r.family == LayerFamily::WPS_OPT_VIS;
  const int R = n * (vis_opt ? NTOK : ntok);
  auto zero_row0 = [&](float* rows) {
    return hipMemset2DAsync(rows, (size_t)NTOK * TD * sizeof(float), 0, (size_t)TD * sizeof(float), (size_t)n, s);
  };
  // heads_in: the last layer's launch starts from dout (heads + un-pool); tail_in: layer 0's continues into the encoder MLP /
  // up-conv. (An option route with the final norm: it, the pooling and the heads are the layer-by-layer launches below.)
  if (r.heads_in) {  // only the three weight-grads are registered here
    if ((rc = lin_wgrad<T>(cx, head[2], dy, dense(hacts[1].p, 256, n, 256), 256))) return rc;
    if ((rc = lin_wgrad<T>(cx, head[1], dense(dhhp[1], 256, n, 256), dense(hacts[0].p, 256, n, 256), 256))) return rc;
    if (r.rows17) rc = lin_wgrad<T>(cx, head[0], dense(dhhp[0], 256, n, 256), dense(ws + L.pooled + TD, 2 * TD, n, TD), TD);
    else rc = lin_wgrad<T>(cx, head[0], dense(dhhp[0], 256, n, 256), dense(ws + L.pooled, 2 * TD, n, 2 * TD), 2 * TD);
    if (rc) return rc;
  } else {
    Epi din = mk_epi(ws + L.dpool, pw, pw);
    if ((rc = chain_bwd<T>(cx, head.data(), nh + 1, dense(ws + L.pooled, pw, n, pw), hacts, dy, dhhp, &din)))
      return rc;
    g_op = "pool";
    // (pytorch_encoder: the pooled rows are the final LayerNorm's output; its backward then gives the grad w.r.t. the last layer's)
    float* dlast = c.pytorch_encoder ? ws + L.dxfin : ws + L.dxl[c.n_layers];
    const float* xlast = c.pytorch_encoder ? ws + L.xfin : ws + L.x[c.n_layers];
    if (vis_opt) V4L_HIP_CHECK(zero_row0(dlast));  // (the final norm's backward walks the 17-row slots)
    if (vis)
      V4L_KLAUNCH("pool_bwd", 0, s, pool_all_bwd_kernel, dim3(n), dim3(64), 0, s, ws + L.dpool, n, ntok, vis_opt ? NTOK : ntok,
                  dlast + (vis_opt ? TD : 0), xlast + (vis_opt ? TD : 0), c.max_pool);
    else
      V4L_KLAUNCH("pool_bwd", 0, s, pool_bwd_kernel, dim3(n), dim3(64), 0, s, ws + L.dpool, n, dlast, xlast, c.max_pool);
    V4L_LAUNCH_CHECK();
    if (c.pytorch_encoder) {
      g_op = "final_ln";
      if ((rc = ln_bwd_launch(cx, std::min(cdiv(R, 16), 128), dlast, ws + L.dxl[c.n_layers], ws + L.xhF, ws + L.rsF, fin_ln, R))) return rc;
    }
  }
  const int lnb = std::min(cdiv(R, 16), 128);
  // the fused layer kernels leave dgamma / dbeta of a layer's two norms as per-block partials: gp2 | bp2 | gp1 | bp1, [nblk][64] each
  auto reduce_ln_partials = [&](const TLayer& t, const float* part, int nblk) {
    const int lnp[4] = {t.ln2.g, t.ln2.b, t.ln1.g, t.ln1.b};
    for (int q = 0; q < 4; ++q) {
      RedDesc o;
      memset(&o, 0, sizeof(o));
      o.slab = part + (int64_t)q * nblk * TD;
      o.dW = grads + params[lnp[q]].goff;
      o.nsplit = nblk; o.N = 1; o.K = TD; o.Npad = 1; o.Kpad = TD; o.Ktorch = TD;
      red.push_back(o);
    }
  };
  // both layers (+ heads before, + encoder-side data-grads after) in ONE launch when the stack is the shipped two layers: the
  // upper layer's dx stays in LDS as the lower layer's dy; otherwise one launch per TransformerEncoderLayer (csrc/bwd.h).
  // Every data-grad of a layer has its intermediates in LDS; the four weight-grads are deferred to the grouped launch.
  const bool stacked = r.family == LayerFamily::BLOCK_STACK && r.tail_in;
  if (r.wps()) {
    // wave-per-sample launch (csrc/wps.h): heads -> per layer {recompute, backward} -> encoder-side data-grads; the four
    // weight-grads of each layer come from the fragment-order operand blocks it leaves, in one launch of their own
    const bool taps = r.taps, plain = r.family == LayerFamily::WPS_PLAIN;
    // round 4: the heads' and the proprio branch's data-grad chains outside this launch, 64 rows per block (csrc/wps.h
    // rows_chain): the heads ran beside the loss statistics when the trainer said so (heads_ext), the proprio chain rides in
    // the layers' weight-grad launch unless the grouped weight-grads (its consumer) go to a stream of their own
    const bool head_ext = plain && !taps && heads_ext_ws == ws && heads_ext_n == n;
    heads_ext_ws = nullptr;
    // (the option variants keep the proprio chain where the layer-0 gradient is: in the launch, or — token_norm — layer by layer
    // behind token_ln's backward)
    const bool tok0_ext = plain && !taps && r.par_wgrad != 3 && !r.tok0_in;
    const int nblk = cdiv(n, WPS_WPB);
    const T* base = (const T*)packed;
    WpsBwdStack d;
    memset(&d, 0, sizeof(d));
    for (int k = 0; k < 2; ++k) {  // d.l[0] = the upper layer
      const int li = 1 - k;
      const TLayer& t = layers[li];
      const LayerBw& b = L.lb[li];
      float* part = cx.slab + cx.slab_used;  // gp2 | bp2 | gp1 | bp1, [nblk][64] each
      cx.slab_used += 4 * (int64_t)nblk * TD;
      V4L_REQUIRE(cx.slab_used <= slab_cap, "internal: weight-grad slab arena overflow");
      WpsBwdLayer& e = d.l[k];
      e.w = base + t.inproj.pkp; e.wt = base + t.inproj.pkpt;
      e.bin = p[t.inproj.b]; e.bo = p[t.outproj.b]; e.b1 = p[t.ff1.b]; e.b2 = p[t.ff2.b];
      e.g1 = p[t.ln1.g]; e.be1 = p[t.ln1.b]; e.g2 = p[t.ln2.g]; e.be2 = p[t.ln2.b];
      e.xin = ws + L.x[li];
      e.wg = ws + L.wps_wg[li]; e.tk = ws + L.wps_tk[li];
      e.gp2 = part; e.bp2 = part + (int64_t)nblk * TD; e.gp1 = part + 2 * (int64_t)nblk * TD; e.bp1 = part + 3 * (int64_t)nblk * TD;
      e.o_dx = (li == 0 || taps) ? ws + L.dxl[li] : nullptr;  // layer 0's: operand of the projector / up-conv weight-grads
      if (taps) { e.t_dz2 = ws + b.dz2; e.t_df = ws + b.df; e.t_dz1 = ws + b.dz1; e.t_dqkv = ws + b.dqkv; }
      reduce_ln_partials(t, part, nblk);
    }
    BwdHead bh;
    memset(&bh, 0, sizeof(bh));
    bh.w2t = base + head[2].pkt; bh.w1t = base + head[1].pkt; bh.w0t = base + (r.rows17 ? head[0].pkto : head[0].pkt);
    bh.dout = ws + L.dout; bh.s_h1 = hacts[1].p; bh.s_h0 = hacts[0].p; bh.o_dh1 = dhhp[1]; bh.o_dh0 = dhhp[0];
    BwdTail bt;
    memset(&bt, 0, sizeof(bt));
    bt.wupt = base + upconv.pkt;
    bt.x0 = ws + L.x[0]; bt.s_c3 = ws + L.c3; bt.o_dc3 = ws + L.dc3;
    if (!vis && wps_tail_shape()) {  // the proprio branch's data-grads (token 0)
      bt.wpt = base + proj.pkt; bt.wf2t = base + enc[1].pkt;
      bt.s_e1 = eacts[1].p; bt.s_e0 = eacts[0].p; bt.o_dhc = ws + L.dhc; bt.o_de0 = dehp[0];
    }
    WpsTailExtra tx;
    tx.wupt_f = base + upconv.pkpt;
    tx.dpool = ws + L.dpool;
    tx.xlast = c.max_pool ? ws + L.x[c.n_layers] : nullptr;
    tx.dyrows = !r.heads_in ? ws + L.dxl[c.n_layers] : nullptr;  // (what the final norm's backward wrote)
    g_op = "layer";
    const double fl_heads = 2.0 * n * 2 * (16 * 256 + 256 * 256 + 256 * 128) / 2, fl_tok0 = 2.0 * n * (64 * 256 + 256 * 256);
    const double fl = 2 * 4.0 * n * 872576.0 + (head_ext ? 0.0 : 2 * fl_heads) + (tok0_ext ? 0.0 : fl_tok0) + 2.0 * n * 16 * 64 * 64;
#define V4L_WPS_BWD(TAPS_, VIS_, HIN_, TIN_, MODE_)                                                                       \
  do {                                                                                                                    \
    V4L_HIP_CHECK(lds_limit<&wps_layer_bwd_kernel<T, 2, TAPS_, VIS_, HIN_, TIN_, MODE_>>(WpsBwdLds<T>::bytes));            \
    V4L_KLAUNCH("wps_layer_bwd_stack", fl, s, (wps_layer_bwd_kernel<T, 2, TAPS_, VIS_, HIN_, TIN_, MODE_>), dim3(nblk), dim3(256), \
                (WpsBwdLds<T>::bytes), s, d, bh, bt, tx, n);                                                              \
  } while (0)
    // round 6: forward -> loss rows -> backward as ONE launch when the trainer handed the loss over (csrc/wps_fb.h)
    const FbLoss* fbl = fb_loss;
    fb_loss = nullptr;
    V4L_REQUIRE(fbl == nullptr || (r.fb_allowed && !head_ext),
                "internal: a fused forward-loss-backward pass was prepared for a net that does not take it");
    // MODE of the option routes: 1 = ends with the layer-0 input gradient rows, 2 = starts from the final norm's gradient rows, 3 = both
    const bool m_out = r.opt() && !r.tail_in, m_in = r.opt() && !r.heads_in;
    if (fbl != nullptr) {
      InfLayerStack fst;
      memset(&fst, 0, sizeof(fst));
      fst.nl = 2;
      for (int k = 0; k < 2; ++k)  // (layer 1's input rows stay in the wave's registers)
        fst.l[k].n[0] = inf_layer<T>(this, layers[k], true, k == 0 ? ws + L.x[0] : nullptr);
      InfHeadPair fhd;
      memset(&fhd, 0, sizeof(fhd));
      fhd.n[0] = inf_head<T>(this, L, ws, false);
      FbLoss lo = *fbl;
      lo.dout = ws + L.dout;
      cx.slab_used = (cx.slab_used + 1) & ~(int64_t)1;  // doubles
      lo.part = reinterpret_cast<double*>(cx.slab + cx.slab_used);
      V4L_REQUIRE((reinterpret_cast<uintptr_t>(lo.part) & 7) == 0, "internal: partial-statistics block not 8-byte aligned");
      cx.slab_used += 2 * (int64_t)nblk * FB_PART;
      V4L_REQUIRE(cx.slab_used <= slab_cap, "internal: weight-grad slab arena overflow");
      const double fl_fb = fl + 2.0 * n * (2 * 872576.0 + 99840.0);  // + the two layer forwards and the heads' forward
      V4L_HIP_CHECK(lds_limit<&wps_layer_fb_kernel<T, true>>(WpsFbLds<T>::bytes));
      V4L_HIP_CHECK(lds_limit<&wps_layer_fb_kernel<T, false>>(WpsFbLds<T>::bytes));
      if (tok0_ext)
        V4L_KLAUNCH("wps_layer_fb_stack", fl_fb, s, (wps_layer_fb_kernel<T, false>), dim3(nblk), dim3(256), (WpsFbLds<T>::bytes), s, fst,
                    fhd, d, bh, bt, tx, lo, n);
      else
        V4L_KLAUNCH("wps_layer_fb_stack", fl_fb, s, (wps_layer_fb_kernel<T, true>), dim3(nblk), dim3(256), (WpsFbLds<T>::bytes), s, fst,
                    fhd, d, bh, bt, tx, lo, n);
      cx.fb_pending = true;
      cx.fb_args = lo;
      cx.fb_blocks = nblk;
      cx.fb_n = n;
    } else
    switch (r.family) {
      case LayerFamily::WPS_OPT_VIS:
        if (m_out && m_in) V4L_WPS_BWD(false, 2, true, true, 3);
        else if (m_in) V4L_WPS_BWD(false, 2, true, true, 2);
        else V4L_WPS_BWD(false, 2, true, true, 1);
        break;
      case LayerFamily::WPS_OPT:
        if (m_out && m_in) V4L_WPS_BWD(false, false, true, true, 3);
        else if (m_in) V4L_WPS_BWD(false, false, true, true, 2);
        else V4L_WPS_BWD(false, false, true, true, 1);
        break;
      case LayerFamily::WPS_VIS17:
        if (taps) V4L_WPS_BWD(true, true, true, true, 0);
        else V4L_WPS_BWD(false, true, true, true, 0);
        break;
      case LayerFamily::WPS_VIS:  // native 16 tokens: no 17th-token side blocks (wa.l[].tk = null below)
        V4L_WPS_BWD(false, 2, true, true, 0);
        break;
      default:  // WPS_PLAIN
        if (taps) V4L_WPS_BWD(true, false, true, true, 0);
        else if (head_ext && tok0_ext) V4L_WPS_BWD(false, false, false, false, 0);
        else if (head_ext) V4L_WPS_BWD(false, false, false, true, 0);
        else if (tok0_ext) V4L_WPS_BWD(false, false, true, false, 0);
        else V4L_WPS_BWD(false, false, true, true, 0);
    }
#undef V4L_WPS_BWD
    V4L_LAUNCH_CHECK();
    // the layers' weight-grads: one partial slab set per run of WPS_SPLIT samples
    WpsWg wa;
    memset(&wa, 0, sizeof(wa));
    wa.n = n; wa.nsplit = cdiv(n, WPS_SPLIT); wa.nlayers = 2;
    for (int li = 0; li < 2; ++li) {
      const TLayer& t = layers[li];
      const Lin* ls[4] = {&t.inproj, &t.outproj, &t.ff1, &t.ff2};
      wa.l[li].wg = ws + L.wps_wg[li];
      wa.l[li].tk = (r.family == LayerFamily::WPS_VIS || vis_opt) ? nullptr : ws + L.wps_tk[li];
      for (int m = 0; m < 4; ++m) {
        const Lin& Lm = *ls[m];
        const int64_t sf = ((int64_t)wa.nsplit * Lm.N * Lm.K + 63) / 64 * 64, bf = ((int64_t)wa.nsplit * Lm.N + 63) / 64 * 64;
        float* sl = cx.slab + cx.slab_used;
        cx.slab_used += sf + bf;
        V4L_REQUIRE(cx.slab_used <= slab_cap, "internal: weight-grad slab arena overflow");
        wa.l[li].slab[m] = sl; wa.l[li].bslab[m] = sl + sf;
        RedDesc o;
        memset(&o, 0, sizeof(o));
        o.dW = grads + params[Lm.w].goff;
        o.db = grads + params[Lm.b].goff;
        o.N = Lm.N; o.K = Lm.K; o.Ktorch = Lm.K;
        o.slab = sl; o.bslab = sl + sf; o.nsplit = wa.nsplit; o.Npad = Lm.N; o.Kpad = Lm.K;
        red.push_back(o);
      }
    }
    if (tok0_ext) {  // the proprio chain as extra blocks of the layers' weight-grad launch (wgrad_dense)
      wa.chain_blocks = cdiv(n, RowsChainCfg<T>::MT_TOK0 * 16);
      wa.tl = bt;
      wa.dx0 = ws + L.dxl[0];
    }
    cx.wps_args = wa;
    cx.wps_pending = true;
    cx.wps_used = true;
  }
  for (int l = c.n_layers - 1; l >= 0 && r.block(); l -= stacked ? 2 : 1) {
    static int spw = 4;  // samples per block: 4 (80 MFMA rows, 1 block per CU) or 2 (48 rows, 2 blocks per CU): measured equal
    const int nblk = cdiv(n, spw);
    const int nl = stacked ? 2 : 1;
    const T* base = (const T*)packed;
    BwdLayerStack d;
    memset(&d, 0, sizeof(d));
    for (int k = 0; k < nl; ++k) {  // d.l[0] = layer l (the upper one), d.l[1] = layer l - 1
      const int li = l - k;
      const TLayer& t = layers[li];
      const LayerWs& w = L.lw[li];
      const LayerBw& b = L.lb[li];
      float* part = cx.slab + cx.slab_used;  // gp2 | bp2 | gp1 | bp1, [nblk][64] each
      cx.slab_used += 4 * (int64_t)nblk * TD;
      V4L_REQUIRE(cx.slab_used <= slab_cap, "internal: weight-grad slab arena overflow");
      BwdLayer& e = d.l[k];
      e.w2t = base + t.ff2.pkt; e.w1t = base + t.ff1.pkt; e.wot = base + t.outproj.pkt; e.wint = base + t.inproj.pkt;
      e.g1 = p[t.ln1.g]; e.g2 = p[t.ln2.g];
      e.dy = ws + L.dxl[li + 1];
      e.s_qkv = ws + w.qkv; e.s_P = ws + w.P; e.s_xh1 = ws + w.xh1; e.s_rs1 = ws + w.rs1; e.s_f = ws + w.f;
      e.s_xh2 = ws + w.xh2; e.s_rs2 = ws + w.rs2;
      e.o_dz2 = ws + b.dz2; e.o_df = ws + b.df; e.o_dz1 = ws + b.dz1; e.o_dqkv = ws + b.dqkv; e.o_dx = ws + L.dxl[li];
      e.gp2 = part; e.bp2 = part + (int64_t)nblk * TD; e.gp1 = part + 2 * (int64_t)nblk * TD; e.bp1 = part + 3 * (int64_t)nblk * TD;
    }
    const bool hd_on = r.heads_in && l == c.n_layers - 1, tl_on = r.tail_in && l - (nl - 1) == 0;
    BwdHead bh;
    memset(&bh, 0, sizeof(bh));
    if (hd_on) {
      bh.w2t = base + head[2].pkt; bh.w1t = base + head[1].pkt; bh.w0t = base + head[0].pkt;
      bh.dout = ws + L.dout; bh.s_h1 = hacts[1].p; bh.s_h0 = hacts[0].p; bh.o_dh1 = dhhp[1]; bh.o_dh0 = dhhp[0];
    }
    BwdTail bt;
    memset(&bt, 0, sizeof(bt));
    if (tl_on) {
      bt.wpt = base + proj.pkt; bt.wf2t = base + enc[1].pkt; bt.wupt = base + upconv.pkt;
      bt.x0 = ws + L.x[0]; bt.s_e1 = eacts[1].p; bt.s_e0 = eacts[0].p; bt.s_c3 = ws + L.c3;
      bt.o_dhc = ws + L.dhc; bt.o_de0 = dehp[0]; bt.o_dc3 = ws + L.dc3;
    }
    g_op = "layer";
    const double fl = nl * 4.0 * n * 872576.0 + (hd_on ? 2.0 * n * 2 * (16 * 256 + 256 * 256 + 256 * 128) : 0.0) +
                      (tl_on ? 2.0 * n * (64 * 256 + 256 * 256 + 16 * 64 * 64) : 0.0);
#define V4L_BWD_LAYER(SPW_, H_, TL_, NL_, LABEL_)                                                                         \
  do {                                                                                                                    \
    V4L_HIP_CHECK(lds_limit<&bwd_layer_kernel<T, SPW_, H_, TL_, NL_>>(BwdLayLds<T, SPW_>::bytes));                        \
    V4L_KLAUNCH(LABEL_, fl, s, (bwd_layer_kernel<T, SPW_, H_, TL_, NL_>), dim3(nblk), dim3(256), (BwdLayLds<T, SPW_>::bytes), s, d, bh, \
                bt, n);                                                                                                   \
  } while (0)
#define V4L_BWD_LAYERS(SPW_)                                                                                              \
  do {                                                                                                                    \
    if (stacked) V4L_BWD_LAYER(SPW_, true, true, 2, "fused_layer_bwd_stack");                                             \
    else if (hd_on && tl_on) V4L_BWD_LAYER(SPW_, true, true, 1, "fused_layer_bwd_head_tail");                             \
    else if (hd_on) V4L_BWD_LAYER(SPW_, true, false, 1, "fused_layer_bwd_head");                                          \
    else if (tl_on) V4L_BWD_LAYER(SPW_, false, true, 1, "fused_layer_bwd_tail");                                          \
    else V4L_BWD_LAYER(SPW_, false, false, 1, "fused_layer_bwd");                                                         \
  } while (0)
    if (spw == 2) V4L_BWD_LAYERS(2);
    else V4L_BWD_LAYERS(4);
#undef V4L_BWD_LAYERS
#undef V4L_BWD_LAYER
    V4L_LAUNCH_CHECK();
    for (int kk = 0; kk < nl; ++kk) {
      const int li = l - kk;
      const TLayer& t = layers[li];
      const LayerWs& w = L.lw[li];
      const LayerBw& b = L.lb[li];
      reduce_ln_partials(t, d.l[kk].gp2, nblk);
      const float* xin = sizeof(T) == 2 ? ws + w.xin : ws + L.x[li];
      if ((rc = lin_wgrad_wide(cx, t.ff2, ws + b.dz2, ws + w.f, R))) return rc;
      if ((rc = lin_wgrad_wide(cx, t.ff1, ws + b.df, ws + w.x1, R))) return rc;
      if ((rc = lin_wgrad_wide(cx, t.outproj, ws + b.dz1, ws + w.ctx, R))) return rc;
      if ((rc = lin_wgrad_wide(cx, t.inproj, ws + b.dqkv, xin, R))) return rc;
    }
  }
  for (int l = c.n_layers - 1; l >= 0 && r.family == LayerFamily::LAYER_BY_LAYER; --l) {
    const TLayer& t = layers[l];
    const LayerWs& w = L.lw[l];
    const LayerBw& b = L.lb[l];
    float* dx = ws + L.dxl[l + 1];  // grad w.r.t. this layer's output
    g_op = "ln2";
    if ((rc = ln_bwd_launch(cx, lnb, dx, ws + b.dz2, ws + w.xh2, ws + w.rs2, t.ln2, R))) return rc;
    {  // linear2 / linear1 (FFN), residual: d(x1) = dz2 + df W1
      ADense y = dense(ws + b.dz2, TD, R, TD);
      if ((rc = lin_wgrad<T>(cx, t.ff2, y, dense(ws + w.f, c.ff_dim, R, c.ff_dim), c.ff_dim))) return rc;
      Epi ep = mk_epi(ws + b.df, c.ff_dim, c.ff_dim);
      ep.mask = ws + w.f;
      ep.ldmask = c.ff_dim;
      if ((rc = lin_dgrad<T>(cx, t.ff2, y, ep))) return rc;
      ADense yf = dense(ws + b.df, c.ff_dim, R, c.ff_dim);
      if ((rc = lin_wgrad<T>(cx, t.ff1, yf, dense(ws + w.x1, TD, R, TD), TD))) return rc;
      Epi ea = mk_epi(ws + b.dx1, TD, TD);
      ea.addend = ws + b.dz2;
      if ((rc = lin_dgrad<T>(cx, t.ff1, yf, ea))) return rc;
    }
    g_op = "ln1";
    if ((rc = ln_bwd_launch(cx, lnb, ws + b.dx1, ws + b.dz1, ws + w.xh1, ws + w.rs1, t.ln1, R))) return rc;
    {  // self-attention block, residual: d(x_in) = dz1 + dqkv W_in
      ADense y = dense(ws + b.dz1, TD, R, TD);
      if ((rc = lin_wgrad<T>(cx, t.outproj, y, dense(ws + w.ctx, TD, R, TD), TD))) return rc;
      if ((rc = lin_dgrad<T>(cx, t.outproj, y, mk_epi(ws + b.dctx, TD, TD)))) return rc;
      g_op = "attn";
      if (ntok == NTOK)
        V4L_KLAUNCH("attn_bwd", 8.0 * n * NTOK * NTOK * TD, s, attn_bwd_kernel<NTOK>, dim3(n), dim3(256), 0, s, ws + w.qkv, ws + w.P,
                    ws + b.dctx, n, ws + b.dqkv, (int)ModeOf<T>::value);
      else
        V4L_KLAUNCH("attn_bwd", 8.0 * n * 16 * 16 * TD, s, attn_bwd_kernel<16>, dim3(n), dim3(256), 0, s, ws + w.qkv, ws + w.P,
                    ws + b.dctx, n, ws + b.dqkv, (int)ModeOf<T>::value);
      V4L_LAUNCH_CHECK();
      ADense yq = dense(ws + b.dqkv, 3 * TD, R, 3 * TD);
      if ((rc = lin_wgrad<T>(cx, t.inproj, yq, dense(ws + L.x[l], TD, R, TD), TD))) return rc;
      Epi ea = mk_epi(ws + L.dxl[l], TD, TD);
      ea.addend = ws + b.dz1;
      if ((rc = lin_dgrad<T>(cx, t.inproj, yq, ea))) return rc;
    }
  }
  float* dx = ws + L.dxl[0];
  const float* x0 = ws + L.x[0];
  if (c.token_norm) {  // through token_ln: grad w.r.t. the encoder's tokens; state_token_ln takes part in nothing (zero gradient)
    g_op = "token_ln";
    if (vis_opt) V4L_HIP_CHECK(zero_row0(dx));  // (the layers' launch wrote rows 1..16 of every slot)
    if ((rc = ln_bwd_launch(cx, lnb, dx, ws + L.dx0raw, ws + L.xh0, ws + L.rs0, tok_ln, R))) return rc;
    V4L_HIP_CHECK(hipMemsetAsync(grads + params[stok_ln.g].goff, 0, TD * sizeof(float), s));
    V4L_HIP_CHECK(hipMemsetAsync(grads + params[stok_ln.b].goff, 0, TD * sizeof(float), s));
    dx = ws + L.dx0raw;
    x0 = ws + L.x0raw;
  }
  if (r.tail_in && !vis) {  // data-grads done by layer 0's launch: register the four weight-grads
    const Act& last = eacts[ne - 1];
    if ((rc = lin_wgrad<T>(cx, proj, dense(dx, NTOK * TD, n, TD, nullptr, 0, x0), dense(last.p, last.ld, n, last.w), last.w)))
      return rc;
    if ((rc = lin_wgrad<T>(cx, enc[1], dense(ws + L.dhc, 256, n, 256), dense(eacts[0].p, 256, n, 256), 256))) return rc;
    if ((rc = lin_wgrad<T>(cx, enc[0], dense(dehp[0], 256, n, 256), sin, sin.K))) return rc;
    if ((rc = lin_wgrad<T>(cx, upconv, dense(dx, TD, n * 16, TD, nullptr, 1), dense(ws + L.c3, 64, n * 16, 64), 64))) return rc;
  }
  if (r.tail_in && vis) {  // the up-conv data-grad came out of the layer launch (dc3): its weight-grad reads rows 1..16 of the 17-row stride
    if ((rc = lin_wgrad<T>(cx, upconv, dense(dx, TD, n * 16, TD, nullptr, 1), dense(ws + L.c3, 64, n * 16, 64), 64))) return rc;
  }
  if (!r.tail_in && !vis) {  // token 0 -> state_projector -> encoder MLP
    const Act& last = eacts[ne - 1];
    ADense yp = dense(dx, NTOK * TD, n, TD, nullptr, 0, x0);
    if ((rc = lin_wgrad<T>(cx, proj, yp, dense(last.p, last.ld, n, last.w), last.w))) return rc;
    Epi ep = mk_epi(ws + L.dhc, last.w, last.w);
    ep.mask = last.p;
    ep.ldmask = last.ld;
    if ((rc = lin_dgrad<T>(cx, proj, yp, ep))) return rc;
    if ((rc = chain_bwd<T>(cx, enc.data(), ne, sin, eacts, dense(ws + L.dhc, last.w, n, last.w), dehp, nullptr))) return rc;
  }
  if (!r.tail_in) {  // tokens 1..16 (vision-only: all 16) -> depth_up_conv -> conv stack
    ADense yu = dense(dx, TD, n * 16, TD, nullptr, (vis && !vis_opt) ? 0 : 1);  // (1: rows 1..16 of 17-row slots)
    if ((rc = lin_wgrad<T>(cx, upconv, yu, dense(ws + L.c3, 64, n * 16, 64), 64))) return rc;
    Epi ep = mk_epi(ws + L.dc3, 64, 64);
    ep.mask = ws + L.c3;
    ep.ldmask = 64;
    if ((rc = lin_dgrad<T>(cx, upconv, yu, ep))) return rc;
  }
  return conv_bwd_and_wgrads();
}

// InfFinish::t_plus1 of a fused step: the host's step index + 1 for eager launches, 0 (= device cursor) under capture or when the
// host lost count (no v4l_actor_seek yet)
static inline long long actor_t_plus1(const v4l_actor* a, hipStream_t s) {
  return (a->t_host >= 0 && !capturing(s)) ? a->t_host + 1 : 0;
}
// The buffers of one rollout step (v4l_actor_step's arguments). img16 / ld_img16: v4l_actor_step_split's bf16 depth stacks
// [E][ld_img16] (null: the image is part of the fp32 observation rows).
struct StepIO {
  const float *obs, *eps;
  float* state_roll;
  void* image_roll;
  float *acts_roll, *values_roll, *logp_roll, *action, *mean, *stdv, *ent, *value;
  const void* img16;
  int64_t ld_img16;
};
// the epilogue of a fused step: sample the action, file action / value / log-prob, write the step's outputs
static InfFinish step_finish(const v4l_actor* a, const StepIO& io, hipStream_t s) {
  const v4l_net* pf = a->pf;
  InfFinish fin;
  memset(&fin, 0, sizeof(fin));
  fin.ctl = a->ctl; fin.logstd = pf->logstd >= 0 ? pf->p[pf->logstd] : nullptr;  // (null: a V4L_LOGSTD_HEAD policy, sigma from the head row)
  fin.eps = io.eps; fin.A = pf->act_dim(); fin.tanh_action = pf->cfg.tanh_action;
  fin.t_plus1 = actor_t_plus1(a, s);
  fin.acts_roll = io.acts_roll; fin.values_roll = io.values_roll; fin.logp_roll = io.logp_roll; fin.action = io.action;
  fin.mean = io.mean; fin.stdv = io.stdv; fin.ent = io.ent; fin.value = io.value;
  return fin;
}

// The kernels that run an actor's step, in the order step_route tries them
enum class StepRoute {
  MLP_ONE_BLOCK,   // state MLP, 16-bit: rollout_mlp2_kernel, one block per net for all E rows
  MLP_PER_SAMPLE,  // state MLP: rollout_mlp_kernel
  CNN_DENSE,       // NatureCNN, 16-bit: rollout_encoder2_kernel + rollout_dense_kernel (csrc/rollout_dense.h)
  CNN_PER_SAMPLE,  // NatureCNN: rollout_cnn_kernel
  STACK_TOK16,     // vision-only LocoTransformer, 16-bit: rollout_encoder2_kernel<ENC_TOK16> + rollout_stack_kernel
  STACK_TOK17,     // LocoTransformer, 16-bit: rollout_encoder2_kernel<ENC_TOK17> + rollout_stack_kernel
  STACK_F32ENC,    // LocoTransformer, fp32: rollout_encoder_kernel + rollout_stack_kernel
  GENERAL,         // layer by layer (forward_t of each net) + act_finish_kernel
};
static StepRoute step_route(const v4l_actor* a, int shared_encoder) {
  const v4l_net *pf = a->pf, *vf = a->vf;
  const v4l_net_cfg &p = pf->cfg, &v = vf->cfg;
  // (a categorical policy, v4l_net_set_categorical: always layer by layer + act_finish_cat_kernel — the fused state-MLP kernels'
  // epilogues are Gaussian — also where a shared trunk, REINFORCE's zero_critic, would pick one of them)
  if (!shared_encoder || pf->cat()) return StepRoute::GENERAL;
  auto both = [&](auto ok) { return ok(p) && ok(v); };
  auto frag_heads = [&] { return pf->head[0].pkf >= 0 && vf->head[0].pkf >= 0; };  // fragment-order packs of the heads
  // tanh_action policies (TanhNormal): the fused kernels' epilogues sample through tanh like act_finish_kernel (round 5), except
  // the one-block state-MLP and the dense NatureCNN kernels (rollout_dense.h) — such a policy takes the next family
  const bool tanh_pol = p.tanh_action != 0;
  if (both([](const v4l_net_cfg& c) { return c.kind == V4L_NET_MLP && mlp_256(c) && head_256(c); }) && pf->enc[0].Kp <= 128) {
    const bool one_block = is_half(p.compute) && a->E <= 64 && p.out_dim <= 16 && pf->enc[0].Kp == 128 && pf->enc[0].pkf >= 0 &&
                           frag_heads();
    // a V4L_LOGSTD_HEAD policy (sigma per row, from the head output) goes the same way: rollout_mlp2_kernel keeps one sigma per column
    return one_block && !tanh_pol && !pf->sd() ? StepRoute::MLP_ONE_BLOCK : StepRoute::MLP_PER_SAMPLE;
  }
  const bool dense_cnn = both([](const v4l_net_cfg& c) {
    if (!(head_256(c) && depth_64(c) && c.out_dim <= 16 && is_half(c.compute))) return false;
    return c.kind == V4L_NET_CNN_VIS || (c.kind == V4L_NET_CNN && mlp_256(c) && c.visual_dim == 256);
  }) && a->E <= 64 && pf->conv[0].pkf >= 0 && frag_heads() && (p.kind == V4L_NET_CNN_VIS || pf->enc[0].Kp == 128);
  if (dense_cnn && !tanh_pol) return StepRoute::CNN_DENSE;
  if (both([](const v4l_net_cfg& c) {
        return c.kind == V4L_NET_CNN && mlp_256(c) && head_256(c) && c.visual_dim == 256 && depth_64(c);
      }) && pf->enc[0].Kp <= 128)
    return StepRoute::CNN_PER_SAMPLE;
  // LocoTransformer, two layers (max_pool: a flag of rollout_stack_kernel's pooling — the stack itself is the same; token_norm /
  // use_pytorch_encoder: the same kernel with the extra norm in front of / behind the layers, one of the two, set alike on both nets)
  const bool stack = both([](const v4l_net_cfg& c) {
    const bool trunk = head_256(c) && c.ff_dim == 256 && c.n_layers == 2;
    if (c.kind == V4L_NET_LOCO_VIS) return trunk && is_half(c.compute);  // (16 tokens: 16-bit kernels only)
    return c.kind == V4L_NET_LOCO && mlp_256(c) && trunk;
  }) && p.token_norm == v.token_norm && p.pytorch_encoder == v.pytorch_encoder && !(p.token_norm && p.pytorch_encoder) &&
                     a->E <= 64 && pf->head.size() == 3 && frag_heads();
  if (!stack) return StepRoute::GENERAL;
  if (p.kind == V4L_NET_LOCO_VIS) return StepRoute::STACK_TOK16;
  if (is_half(p.compute) && pf->enc.size() == 2 && pf->enc[0].Kp == 128 && pf->conv[0].pkf >= 0) return StepRoute::STACK_TOK17;
  return StepRoute::STACK_F32ENC;  // (fp32 parity mode: fragments twice the size, weights streamed per wave)
}

// NatureCNN fuse nets of the shipped shape: one launch per env step (rollout_cnn_kernel)
template <typename T>
static int run_actor_fused_cnn(v4l_actor* a, const StepIO& io, hipStream_t s) {
  v4l_net *pf = a->pf, *vf = a->vf;
  const int E = a->E;
  V4L_HIP_CHECK(lds_limit<&rollout_cnn_kernel<T>>(RollCnnLds<T>::bytes));
  const T* pk = (const T*)pf->packed;
  const T* vk = (const T*)vf->packed;
  const Layout Lp = pf->layout(E), Lv = vf->layout(E);
  float* ws_pf = a->ws;
  float* ws_vf = a->ws + Lp.total;
  PhaseScope ps("rollout");
  InfCnn en;
  en.w1 = pk + pf->conv[0].pk; en.w2 = pk + pf->conv[1].pk; en.w3 = pk + pf->conv[2].pk;
  en.b1 = pf->p[pf->conv[0].b]; en.b2 = pf->p[pf->conv[1].b]; en.b3 = pf->p[pf->conv[2].b];
  en.wpr = pk + pf->proj.pk; en.wf1 = pk + pf->enc[0].pk; en.wf2 = pk + pf->enc[1].pk;
  en.bpr = pf->p[pf->proj.b]; en.bf1 = pf->p[pf->enc[0].b]; en.bf2 = pf->p[pf->enc[1].b];
  en.S = pf->cfg.state_dim; en.Sp = pf->Sp; en.Kp1 = pf->enc[0].Kp;
  InfCnnHeadPair hd;
  auto head = [&](InfCnnHead& h, v4l_net* net, const T* base, float* out) {
    h.w0 = base + net->head[0].pk; h.w1 = base + net->head[1].pk; h.w2 = base + net->head[2].pk;
    h.b0 = net->p[net->head[0].b]; h.b1 = net->p[net->head[1].b]; h.b2 = net->p[net->head[2].b];
    h.out = out; h.nout = net->cfg.out_dim;
  };
  head(hd.n[0], pf, pk, ws_pf + Lp.out);
  head(hd.n[1], vf, vk, ws_vf + Lv.out);
  const InfFinish fin = step_finish(a, io, s);
  g_op = "step";
  V4L_KLAUNCH("rollout_cnn", 2.0 * 2 * E * (3612672.0 + 1024 * 256 + 2 * 128 * 256 + 512 * 256 + 2 * 256 * 256), s, rollout_cnn_kernel<T>,
              dim3(E, 2), dim3(1024), RollCnnLds<T>::bytes, s, (const ActCtl*)a->ctl, io.obs, E, en, hd, fin, io.state_roll,
              (T*)io.image_roll);
  V4L_LAUNCH_CHECK();
  return 0;
}

// rollout_encoder2_kernel<MODE> on the step's observation: fp32 rows [E][S + C*H*W], or — v4l_actor_step_split — fp32 proprio
// rows [E][S] + bf16 depth stacks (io.img16)
template <typename H, int MODE, bool IMG16>
static int launch_encoder2_t(v4l_actor* a, const StepIO& io, hipStream_t s, double flops, dim3 grid, const InfEncFrag& ef, float* x0,
                             H* featv, H* featp) {
  V4L_HIP_CHECK(lds_limit<&rollout_encoder2_kernel<H, MODE, IMG16>>(RollEnc2Lds::bytes));
  const int img_elems = a->pf->cfg.in_channels * a->pf->cfg.img_hw * a->pf->cfg.img_hw;
  const int ld_obs = IMG16 ? ef.S : ef.S + img_elems;
  V4L_KLAUNCH("rollout_encoder", flops, s, (rollout_encoder2_kernel<H, MODE, IMG16>), grid, dim3(1024), RollEnc2Lds::bytes, s,
              (const ActCtl*)a->ctl, io.obs, ld_obs, (const H*)io.img16, io.ld_img16, a->E, ef, io.state_roll, (H*)io.image_roll, x0,
              featv, featp, actor_t_plus1(a, s));
  V4L_LAUNCH_CHECK();
  return 0;
}
template <typename H, int MODE>
static int launch_encoder2(v4l_actor* a, const StepIO& io, hipStream_t s, double flops, dim3 grid, const InfEncFrag& ef, float* x0,
                           H* featv, H* featp) {
  return io.img16 ? launch_encoder2_t<H, MODE, true>(a, io, s, flops, grid, ef, x0, featv, featp)
                  : launch_encoder2_t<H, MODE, false>(a, io, s, flops, grid, ef, x0, featv, featp);
}

// NatureCNN nets (fuse net and vision-only), bf16: the step as batched GEMMs over all E rows (csrc/rollout_dense.h)
template <typename H>
static int run_actor_dense_cnn(v4l_actor* a, const StepIO& io, hipStream_t s) {
  v4l_net *pf = a->pf, *vf = a->vf;
  const int E = a->E;
  const bool fuse = pf->cfg.kind == V4L_NET_CNN;
  const H* pk = (const H*)pf->packed;
  const H* vk = (const H*)vf->packed;
  const Layout Lp = pf->layout(E), Lv = vf->layout(E);
  float* ws_pf = a->ws;
  float* ws_vf = a->ws + Lp.total;
  // operand-type scratch in fragment order (act_frag_off), carved from the actor's weight-grad slab region (a rollout step
  // computes no gradients): conv3 flatten [R][1024], the concat [R][512], fc0 / fc1 outputs [R][256] per net, R = ceil16(E)
  const int64_t R16 = round_up(E, 16);
  V4L_REQUIRE(Lp.total - Lp.slab >= R16 * (512 + 256 + 4 * 128), "internal: rollout scratch does not fit the slab region");
  H* featv = reinterpret_cast<H*>(ws_pf + Lp.slab);
  H* cat = featv + R16 * 1024;
  H* h0p = cat + R16 * 512;
  H* h0v = h0p + R16 * 256;
  H* h1p = h0v + R16 * 256;
  H* h1v = h1p + R16 * 256;
  PhaseScope ps("rollout");
  InfEncFrag ef;
  memset(&ef, 0, sizeof(ef));
  ef.w1 = pk + pf->conv[0].pkf; ef.w2 = pk + pf->conv[1].pkf; ef.w3 = pk + pf->conv[2].pkf; ef.wup = ef.w3;
  ef.b1 = pf->p[pf->conv[0].b]; ef.b2 = pf->p[pf->conv[1].b]; ef.b3 = pf->p[pf->conv[2].b]; ef.bup = ef.b3;
  ef.S = pf->cfg.state_dim; ef.Sp = pf->Sp;
  g_op = "encoder";
  if (fuse) {
    ef.wf1 = pk + pf->enc[0].pkf; ef.wf2 = pk + pf->enc[1].pkf; ef.wpr = ef.wf2;
    ef.bf1 = pf->p[pf->enc[0].b]; ef.bf2 = pf->p[pf->enc[1].b]; ef.bpr = ef.bf2;
    if (int rc = launch_encoder2<H, ENC_FUSE>(a, io, s, 2.0 * E * (3612672.0 + 128 * 256 + 256 * 256), dim3(E + cdiv(E, 32)), ef,
                                           (float*)nullptr, featv, cat))
      return rc;
  } else {
    if (int rc = launch_encoder2<H, ENC_FLAT>(a, io, s, 2.0 * E * 3612672.0, dim3(E), ef, (float*)nullptr, featv, (H*)nullptr))
      return rc;
  }
  InfFinish fin = step_finish(a, io, s);
  g_op = "dense";
  if (!sw_on("V4L_ROLLOUT_DENSE_SPLIT")) {  // (read per call: tests switch it)
    // projector -> fc0 -> fc1 -> last linear -> epilogue as stages of one launch (device-side hand-overs)
    RollDense<H> d;
    memset(&d, 0, sizeof(d));
    if (fuse) { d.wpr = pk + pf->proj.pkf; d.bpr = pf->p[pf->proj.b]; }
    auto net_of = [&](int i, v4l_net* net, const H* base, H* h0, H* h1, float* out) {
      d.w0[i] = base + net->head[0].pkf; d.w1[i] = base + net->head[1].pkf; d.w2[i] = base + net->head[2].pkf;
      d.b0[i] = net->p[net->head[0].b]; d.b1[i] = net->p[net->head[1].b]; d.b2[i] = net->p[net->head[2].b];
      d.h0[i] = h0; d.h1[i] = h1; d.out[i] = out; d.nout[i] = net->cfg.out_dim;
    };
    net_of(0, pf, pk, h0p, h1p, ws_pf + Lp.out);
    net_of(1, vf, vk, h0v, h1v, ws_vf + Lv.out);
    d.featv = featv; d.cat = cat;
    const double fl = 2.0 * E * ((fuse ? 1024.0 * 256 : 0.0) + 2 * ((fuse ? 512.0 : 1024.0) * 256 + 256 * 256 + 256 * 16));
    if (capturing(s)) { fin.seq_plus1 = 0; a->dense_in_graph = true; }   // replays read (and advance) the device's count
    else fin.seq_plus1 = ++a->dense_seq;                                  // eager: this launch's number + 1, from the host
    if (fuse) V4L_KLAUNCH("rollout_dense", fl, s, (rollout_dense_kernel<H, true>), dim3(32), dim3(64), 0, s, d, fin, E);
    else V4L_KLAUNCH("rollout_dense", fl, s, (rollout_dense_kernel<H, false>), dim3(32), dim3(64), 0, s, d, fin, E);
    V4L_LAUNCH_CHECK();
    return 0;
  }
  RollLin<H> fc0;
  memset(&fc0, 0, sizeof(fc0));
  fc0.w[0] = pk + pf->head[0].pkf; fc0.w[1] = vk + vf->head[0].pkf;
  fc0.b[0] = pf->p[pf->head[0].b]; fc0.b[1] = vf->p[vf->head[0].b];
  fc0.y[0] = h0p; fc0.y[1] = h0v; fc0.ldy = 256;
  if (fuse) {
    RollLin<H> pr;
    memset(&pr, 0, sizeof(pr));
    pr.w[0] = pk + pf->proj.pkf; pr.b[0] = pf->p[pf->proj.b]; pr.x[0] = featv; pr.y[0] = cat; pr.ks_out = 16;
    V4L_KLAUNCH("rollout_linear", 2.0 * E * 1024 * 256, s, (rollout_linear_kernel<H, 32>), dim3(16, 1), dim3(64), 0, s, pr, E);
    V4L_LAUNCH_CHECK();
    fc0.x[0] = fc0.x[1] = cat;
    V4L_KLAUNCH("rollout_linear", 2.0 * 2 * E * 512 * 256, s, (rollout_linear_kernel<H, 16>), dim3(16, 2), dim3(64), 0, s, fc0, E);
  } else {
    fc0.x[0] = fc0.x[1] = featv;
    V4L_KLAUNCH("rollout_linear", 2.0 * 2 * E * 1024 * 256, s, (rollout_linear_kernel<H, 32>), dim3(16, 2), dim3(64), 0, s, fc0, E);
  }
  V4L_LAUNCH_CHECK();
  RollHead<H> hd;
  memset(&hd, 0, sizeof(hd));
  auto head = [&](int i, v4l_net* net, const H* base, const H* x, float* out) {
    hd.wb[i] = base + net->head[1].pkf; hd.wo[i] = base + net->head[2].pkf;
    hd.bb[i] = net->p[net->head[1].b]; hd.bo[i] = net->p[net->head[2].b];
    hd.x[i] = x; hd.out[i] = out; hd.nout[i] = net->cfg.out_dim;
  };
  head(0, pf, pk, h0p, ws_pf + Lp.out);
  head(1, vf, vk, h0v, ws_vf + Lv.out);
  V4L_HIP_CHECK(lds_limit<&rollout_head_kernel<H>>(RollHeadLds::bytes));
  g_op = "head";
  V4L_KLAUNCH("rollout_head", 2.0 * 2 * E * (256 * 256 + 256 * 16), s, rollout_head_kernel<H>, dim3(2), dim3(512), RollHeadLds::bytes,
              s, hd, fin, E);
  V4L_LAUNCH_CHECK();
  return 0;
}

// state-only MLP nets, bf16: one launch per env step, one block per net for ALL E rows (csrc/rollout_dense.h rollout_mlp2_kernel)
template <typename H, int ACT>
static int run_actor_mlp2(v4l_actor* a, const StepIO& io, hipStream_t s) {
  v4l_net *pf = a->pf, *vf = a->vf;
  const int E = a->E;
  V4L_HIP_CHECK((lds_limit<&rollout_mlp2_kernel<H, ACT>>(RollMlp2Lds::bytes)));
  const H* pk = (const H*)pf->packed;
  const H* vk = (const H*)vf->packed;
  const Layout Lp = pf->layout(E), Lv = vf->layout(E);
  PhaseScope ps("rollout");
  RollMlp2 m;
  memset(&m, 0, sizeof(m));
  m.wf1 = pk + pf->enc[0].pkf; m.wf2 = pk + pf->enc[1].pkf;
  m.bf1 = pf->p[pf->enc[0].b]; m.bf2 = pf->p[pf->enc[1].b];
  m.S = pf->cfg.state_dim; m.Sp = pf->Sp;
  auto head = [&](int i, v4l_net* net, const H* base, float* out) {
    m.w0[i] = base + net->head[0].pkf; m.w1[i] = base + net->head[1].pkf; m.w2[i] = base + net->head[2].pkf;
    m.b0[i] = net->p[net->head[0].b]; m.b1[i] = net->p[net->head[1].b]; m.b2[i] = net->p[net->head[2].b];
    m.out[i] = out; m.nout[i] = net->cfg.out_dim;
  };
  head(0, pf, pk, a->ws + Lp.out);
  head(1, vf, vk, a->ws + Lp.total + Lv.out);
  const InfFinish fin = step_finish(a, io, s);
  g_op = "step";
  V4L_KLAUNCH("rollout_mlp", 2.0 * 2 * E * (128.0 * 256 + 4 * 256 * 256), s, (rollout_mlp2_kernel<H, ACT>), dim3(2), dim3(1024),
              RollMlp2Lds::bytes, s, io.obs, E, m, fin, io.state_roll);
  V4L_LAUNCH_CHECK();
  return 0;
}

// state-only MLP nets of the shipped shape: one launch per env step (rollout_mlp_kernel)
template <typename T, int ACT, bool SD = false>
static int run_actor_fused_mlp(v4l_actor* a, const StepIO& io, hipStream_t s) {
  v4l_net *pf = a->pf, *vf = a->vf;
  const int E = a->E;
  const T* pk = (const T*)pf->packed;
  const T* vk = (const T*)vf->packed;
  const Layout Lp = pf->layout(E), Lv = vf->layout(E);
  float* ws_pf = a->ws;
  float* ws_vf = a->ws + Lp.total;
  PhaseScope ps("rollout");
  InfMlp en;
  en.wf1 = pk + pf->enc[0].pk; en.wf2 = pk + pf->enc[1].pk;
  en.bf1 = pf->p[pf->enc[0].b]; en.bf2 = pf->p[pf->enc[1].b];
  en.S = pf->cfg.state_dim; en.Sp = pf->Sp; en.Kp1 = pf->enc[0].Kp;
  InfCnnHeadPair hd;
  auto head = [&](InfCnnHead& h, v4l_net* net, const T* base, float* out) {
    h.w0 = base + net->head[0].pk; h.w1 = base + net->head[1].pk; h.w2 = base + net->head[2].pk;
    h.b0 = net->p[net->head[0].b]; h.b1 = net->p[net->head[1].b]; h.b2 = net->p[net->head[2].b];
    h.out = out; h.nout = net->cfg.out_dim;
  };
  head(hd.n[0], pf, pk, ws_pf + Lp.out);
  head(hd.n[1], vf, vk, ws_vf + Lv.out);
  const InfFinish fin = step_finish(a, io, s);
  g_op = "step";
  V4L_KLAUNCH("rollout_mlp", 2.0 * 2 * E * (128.0 * 256 + 4 * 256 * 256), s, (rollout_mlp_kernel<T, ACT, SD>), dim3(E, 2), dim3(1024), 0, s,
              (const ActCtl*)a->ctl, io.obs, E, en, hd, fin, io.state_roll);
  V4L_LAUNCH_CHECK();
  return 0;
}


// The fused LocoTransformer step after its encoder: one sample per block and net (2E blocks of 8 waves), ALL layers, the heads, the
// sampling of the action, the filing of action / value / log-prob at rollout slot t*E + i and the advance of the step cursor in
// one launch. warm = 0: L2 warm-up touches at kernel entry measured +-0 (round 2), compiled out of the launch. xcd = 1: one net
// per XCD half (see the kernel; the (E, 2) grid, where every XCD's L2 serves both nets, moved 6.1 MB of HBM traffic per launch
// instead of 3.65 — round 4's A/B).
template <typename T, int NT, int OPT>
static int launch_roll_stack(hipStream_t s, int E, const InfLayerStack& stk, const InfHeadPair& hd, const InfFinish& fin) {
  V4L_HIP_CHECK(lds_limit<&rollout_stack_kernel<T, 2, NT, OPT>>(RollStackLds<T>::bytes));
  V4L_KLAUNCH("rollout_layers_head", 2.0 * 2 * E * (stk.nl * 872576.0 + 99840.0), s, (rollout_stack_kernel<T, 2, NT, OPT>),
              dim3(2 * round_up(E, 4)), dim3(512), (RollStackLds<T>::bytes), s, stk, hd, fin, E, /*warm=*/0, /*xcd=*/1);
  V4L_LAUNCH_CHECK();
  return 0;
}
// Fused rollout step for the shipped LocoTransformer shape (csrc/infer.h): 2 launches instead of ~50. route: one of the STACK_*.
template <typename T>
static int run_actor_fused(v4l_actor* a, const StepIO& io, StepRoute route, hipStream_t s) {
  typedef typename HalfOf<T>::type H;  // the fragment-pack encoder kernels exist for the 16-bit operand types only
  v4l_net *pf = a->pf, *vf = a->vf;
  const int E = a->E;
  const T* pk = (const T*)pf->packed;
  const T* vk = (const T*)vf->packed;
  const Layout Lp = pf->layout(E), Lv = vf->layout(E);
  float* ws_pf = a->ws;
  float* ws_vf = a->ws + Lp.total;
  PhaseScope ps("rollout");
  float* x0 = ws_pf + Lp.x[0];
  g_op = "encoder";
  if (route == StepRoute::STACK_F32ENC) {
    InfEnc en;
    memset(&en, 0, sizeof(en));
    en.w1 = pk + pf->conv[0].pk; en.w2 = pk + pf->conv[1].pk; en.w3 = pk + pf->conv[2].pk; en.wup = pk + pf->upconv.pk;
    en.b1 = pf->p[pf->conv[0].b]; en.b2 = pf->p[pf->conv[1].b]; en.b3 = pf->p[pf->conv[2].b]; en.bup = pf->p[pf->upconv.b];
    en.wf1 = pk + pf->enc[0].pk; en.wf2 = pk + pf->enc[1].pk; en.wpr = pk + pf->proj.pk;
    en.bf1 = pf->p[pf->enc[0].b]; en.bf2 = pf->p[pf->enc[1].b]; en.bpr = pf->p[pf->proj.b];
    en.Kp1 = pf->enc[0].Kp;
    en.S = pf->cfg.state_dim; en.Sp = pf->Sp;
    V4L_HIP_CHECK(lds_limit<&rollout_encoder_kernel<T>>(InfEncLds<T>::bytes));
    V4L_KLAUNCH("rollout_encoder", 2.0 * E * 3678208.0, s, rollout_encoder_kernel<T>, dim3(E + cdiv(E, 32)), dim3(1024),
                InfEncLds<T>::bytes, s, (const ActCtl*)a->ctl, io.obs, E, en, io.state_roll, (T*)io.image_roll, x0);
  } else {
    const H* pb = (const H*)pf->packed;
    InfEncFrag ef;
    memset(&ef, 0, sizeof(ef));
    ef.w1 = pb + pf->conv[0].pkf; ef.w2 = pb + pf->conv[1].pkf; ef.w3 = pb + pf->conv[2].pkf; ef.wup = pb + pf->upconv.pkf;
    ef.b1 = pf->p[pf->conv[0].b]; ef.b2 = pf->p[pf->conv[1].b]; ef.b3 = pf->p[pf->conv[2].b]; ef.bup = pf->p[pf->upconv.b];
    ef.S = pf->cfg.state_dim; ef.Sp = pf->Sp;
    if (route == StepRoute::STACK_TOK16) {  // 16 depth tokens, no proprio blocks
      if (int rc = launch_encoder2<H, ENC_TOK16>(a, io, s, 2.0 * E * 3678208.0, dim3(E), ef, x0, (H*)nullptr, (H*)nullptr)) return rc;
    } else {
      ef.wf1 = pb + pf->enc[0].pkf; ef.wf2 = pb + pf->enc[1].pkf; ef.wpr = pb + pf->proj.pkf;
      ef.bf1 = pf->p[pf->enc[0].b]; ef.bf2 = pf->p[pf->enc[1].b]; ef.bpr = pf->p[pf->proj.b];
      if (int rc = launch_encoder2<H, ENC_TOK17>(a, io, s, 2.0 * E * 3678208.0, dim3(E + cdiv(E, 32)), ef, x0, (H*)nullptr,
                                              (H*)nullptr))
        return rc;
    }
  }
  V4L_LAUNCH_CHECK();
  const int nl = pf->cfg.n_layers;
  auto fill = [&](InfLayer& d, v4l_net* net, const T* base, const TLayer& t, const float* xin, float* xout) {
    d.win = base + t.inproj.pkf; d.wo = base + t.outproj.pkf; d.w1 = base + t.ff1.pkf; d.w2 = base + t.ff2.pkf;
    d.bin = net->p[t.inproj.b]; d.bo = net->p[t.outproj.b]; d.b1 = net->p[t.ff1.b]; d.b2 = net->p[t.ff2.b];
    d.g1 = net->p[t.ln1.g]; d.be1 = net->p[t.ln1.b]; d.g2 = net->p[t.ln2.g]; d.be2 = net->p[t.ln2.b];
    d.xin = xin; d.xout = xout;
  };
  InfLayerStack stk;
  memset(&stk, 0, sizeof(stk));
  stk.nl = nl;
  for (int l = 0; l < nl; ++l) {
    fill(stk.l[l].n[0], pf, pk, pf->layers[l], l == 0 ? x0 : ws_pf + Lp.x[l], ws_pf + Lp.x[l + 1]);
    fill(stk.l[l].n[1], vf, vk, vf->layers[l], l == 0 ? x0 : ws_vf + Lv.x[l], ws_vf + Lv.x[l + 1]);
  }
  InfHeadPair hd;
  memset(&hd, 0, sizeof(hd));
  auto head = [&](InfHead& h, v4l_net* net, const T* base, float* out) {
    h.w0 = base + net->head[0].pkf; h.w1 = base + net->head[1].pkf; h.w2 = base + net->head[2].pkf;
    h.b0 = net->p[net->head[0].b]; h.b1 = net->p[net->head[1].b]; h.b2 = net->p[net->head[2].b];
    h.out = out; h.nout = net->cfg.out_dim; h.max_pool = net->cfg.max_pool;
    if (net->cfg.token_norm) { h.tn_g = net->p[net->tok_ln.g]; h.tn_b = net->p[net->tok_ln.b]; }
    if (net->cfg.pytorch_encoder) { h.fn_g = net->p[net->fin_ln.g]; h.fn_b = net->p[net->fin_ln.b]; }
  };
  head(hd.n[0], pf, pk, ws_pf + Lp.out);
  head(hd.n[1], vf, vk, ws_vf + Lv.out);
  const InfFinish fin = step_finish(a, io, s);
  g_op = "layer";
  const int opt = (pf->cfg.token_norm ? 1 : 0) | (pf->cfg.pytorch_encoder ? 2 : 0);
  if (route == StepRoute::STACK_TOK16) {
    if (opt == 1) return launch_roll_stack<T, 16, 1>(s, E, stk, hd, fin);
    if (opt == 2) return launch_roll_stack<T, 16, 2>(s, E, stk, hd, fin);
    return launch_roll_stack<T, 16, 0>(s, E, stk, hd, fin);
  }
  if (opt == 1) return launch_roll_stack<T, NTOK, 1>(s, E, stk, hd, fin);
  if (opt == 2) return launch_roll_stack<T, NTOK, 2>(s, E, stk, hd, fin);
  return launch_roll_stack<T, NTOK, 0>(s, E, stk, hd, fin);
}


// the loss launch with the heads' chain beside the statistics: grid = 1 + row blocks, NW waves per block
template <typename T, int NW>
static int launch_critic_loss_heads(hipStream_t s, const float* values, const float* ret, const float* oldv, const int* rowidx, int n,
                                    float inv_n, int clipped, float clip, float* dvalues, float* st, const RowsChain& hc, float gscale) {
  // (the heads' data-grad chain: 85 KB of dynamic LDS in bf16, above the 64 KB default)
  V4L_HIP_CHECK(lds_limit<&critic_loss_heads_kernel<T, NW>>(RowsChainLds<T, RowsChainCfg<T>::MT>::bytes3));
  V4L_KLAUNCH("critic_loss", 2.0 * n * (16 * 256 + 256 * 256 + 256 * 128), s, (critic_loss_heads_kernel<T, NW>),
              dim3(1 + cdiv(n, RowsChainCfg<T>::MT * 16)), dim3(NW * 64), (RowsChainLds<T, RowsChainCfg<T>::MT>::bytes3), s, values, ret,
              oldv, rowidx, n, inv_n, clipped, clip, dvalues, st, hc, gscale);
  return 0;
}
template <typename T, int NW, int CAP>
static int launch_actor_loss_heads(hipStream_t s, const ActorArgs& aa, const RowsChain& hc) {
  V4L_HIP_CHECK(lds_limit<&actor_loss_heads_kernel<T, NW, CAP>>(RowsChainLds<T, RowsChainCfg<T>::MT>::bytes3));
  V4L_KLAUNCH("actor_loss", 2.0 * aa.n * (16 * 256 + 256 * 256 + 256 * 128), s, (actor_loss_heads_kernel<T, NW, CAP>),
              dim3(1 + cdiv(aa.n, RowsChainCfg<T>::MT * 16)), dim3(NW * 64), (RowsChainLds<T, RowsChainCfg<T>::MT>::bytes3), s, aa, hc);
  return 0;
}
// the statistics-only loss launch: one block
template <int CAP>
static int launch_actor_loss(hipStream_t s, const ActorArgs& aa, dim3 blk) {
  if (aa.tanh_action) V4L_KLAUNCH("actor_loss", 0, s, (actor_loss_kernel<true, CAP>), dim3(1), blk, 0, s, aa);
  else V4L_KLAUNCH("actor_loss", 0, s, (actor_loss_kernel<false, CAP>), dim3(1), blk, 0, s, aa);
  return 0;
}

// the same for a V4L_LOGSTD_HEAD policy (actor_loss_sd_kernel: sigma per row, d(raw log sigma) in the d(out) row)
static int launch_actor_loss_sd(hipStream_t s, const ActorArgs& aa, dim3 blk) {
  if (aa.tanh_action) V4L_KLAUNCH("actor_loss", 0, s, actor_loss_sd_kernel<true>, dim3(1), blk, 0, s, aa);
  else V4L_KLAUNCH("actor_loss", 0, s, actor_loss_sd_kernel<false>, dim3(1), blk, 0, s, aa);
  return 0;
}

// the same for a categorical policy (v4l_net_set_categorical; actor_loss_cat_kernel: logits rows, one action index per row)
static int launch_actor_loss_cat(hipStream_t s, const ActorArgs& aa, dim3 blk) {
  V4L_KLAUNCH("actor_loss", 0, s, actor_loss_cat_kernel, dim3(1), blk, 0, s, aa);
  return 0;
}

// V-MPO: the row selection and the single-block loss launch (csrc/elem.h)
static int launch_vmpo_select(hipStream_t s, const float* adv, const int* rowidx, int n, int* sel) {
  g_op = "select";
  V4L_KLAUNCH("vmpo_select", 0, s, vmpo_select_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, adv, rowidx, n, sel);
  V4L_LAUNCH_CHECK();
  return 0;
}
template <int CAP>
static int launch_vmpo_loss(hipStream_t s, const ActorArgs& aa, const VmpoArgs& va, dim3 blk) {
  if (aa.tanh_action) V4L_KLAUNCH("vmpo_loss", 0, s, (vmpo_loss_kernel<true, CAP>), dim3(1), blk, 0, s, aa, va);
  else V4L_KLAUNCH("vmpo_loss", 0, s, (vmpo_loss_kernel<false, CAP>), dim3(1), blk, 0, s, aa, va);
  V4L_LAUNCH_CHECK();
  return 0;
}

// A2C and REINFORCE: the policy's single-block loss launch (csrc/elem.h), 1024 threads from 512 rows on. Both kernel families
// have one signature; `family` holds a family's four instantiations: TANH is compiled in for TanhNormal policies, and the per-row
// code holds its per-dimension state per thread, so CAP is 8 for every A <= 8 and V4L_MAX_ACT above.
static inline dim3 loss_block(int n) { return dim3(n >= 512 ? 1024 : 256); }
typedef void (*RecLossKernel)(ActorArgs, const UpdCtl*, float*);
#define V4L_LOSS_FAMILY(kern) \
  { kern<false, ACT_CAP_NARROW>, kern<false, V4L_MAX_ACT>, kern<true, ACT_CAP_NARROW>, kern<true, V4L_MAX_ACT> }
static int launch_rec_loss(const char* label, const RecLossKernel (&family)[4], hipStream_t s, const ActorArgs& aa, const UpdCtl* ctl,
                           float* rec_all) {
  const RecLossKernel kern = family[(aa.tanh_action ? 2 : 0) + (act_cap(aa.A) != ACT_CAP_NARROW ? 1 : 0)];
  V4L_KLAUNCH(label, 0, s, kern, dim3(1), loss_block(aa.n), 0, s, aa, ctl, rec_all);
  V4L_LAUNCH_CHECK();
  return 0;
}
// the same launch for a categorical policy (v4l_net_set_categorical): one instantiation per learner
static int launch_cat_loss(const char* label, RecLossKernel kern, hipStream_t s, const ActorArgs& aa, const UpdCtl* ctl, float* rec_all) {
  V4L_KLAUNCH(label, 0, s, kern, dim3(1), loss_block(aa.n), 0, s, aa, ctl, rec_all);
  V4L_LAUNCH_CHECK();
  return 0;
}

// Captures what body() launches on s (thread-local mode) and instantiates it into *exec. A failed body ends the capture,
// destroys what was recorded and returns the body's rc; otherwise the end-capture error decides.
template <class Body>
static int capture_graph(hipStream_t s, const char* what, Body&& body, hipGraphExec_t* exec) {
  hipGraph_t graph = nullptr;
  V4L_TRACE("%s: begin capture", what);
  V4L_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  const int rc = body();
  V4L_TRACE("%s: end capture rc=%d", what, rc);
  const hipError_t e = hipStreamEndCapture(s, &graph);
  if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
  V4L_HIP_CHECK(e);
  V4L_TRACE("%s: instantiate", what);
  V4L_HIP_CHECK(hipGraphInstantiate(exec, graph, nullptr, nullptr, 0));
  V4L_HIP_CHECK(hipGraphDestroy(graph));
  V4L_TRACE("%s: instantiated", what);
  return 0;
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" {

const char* v4l_last_error(void) { return v4l::last_error(); }
// 113: v4l_net_cfg.has_logstd = V4L_LOGSTD_HEAD (GaussianContPolicy, continuous_policy.py:222-236: log sigma from the head's last layer, per row) —
// actor_loss_sd_kernel, the per-row sampling epilogues of rollout_mlp_kernel / act_finish_sd_kernel, v4l_gauss_head_sd
// 114: REINFORCE on every net kind the PPO update takes: v4l_trainer_reinforce_actor_grads / _update_next / _update_run / _graph_counts,
// V4L_REINFORCE_STATS (reinforce_loss_kernel; the opening launch packs the policy)
// 115: v4l_net_set_categorical (CategoricalDisPolicy, policies/discrete_policies.py:127-172: K = out_dim logits, one action index) — v4l_cat_head,
// v4l_cat_sample, a2c_cat_loss_kernel / reinforce_cat_loss_kernel behind the A2C and REINFORCE entry points, act_finish_cat_kernel on the GENERAL step
// 116: the opt-in KL early stop inside a run of PPO updates: v4l_trainer_kl_stop, v4l_trainer_kl_update_next / _update_run / _graph_counts (kl_stop_kernel, clip_adam_kernel<WD, true>)
// 117: the opt-in KL-adaptive learning rates of a run of PPO updates: v4l_trainer_kl_adapt, v4l_trainer_kl_adapt_update_next / _update_run / _graph_counts,
// v4l_trainer_lrs (kl_adapt_kernel)
// 118: the PPO update takes a categorical policy (PPODiscrete): actor_loss_cat_kernel behind v4l_trainer_actor_grads / _update_next / _update_run, log pi_old
// stored (act_finish_cat_kernel) or from the frozen target's logits rows; V-MPO, the KL early stop and the KL-adaptive rates keep refusing the flag
int v4l_version(void) { return 118; }  // 112: A2C on state-MLP nets: v4l_trainer_a2c_critic_grads / _actor_grads / _update_next / _update_run / _graph_counts, V4L_A2C_STATS; V-MPO updates as hipGraph replays: v4l_trainer_vmpo_update_next / _update_run / _graph_counts; V-MPO: v4l_vmpo_hyper, v4l_trainer_vmpo_* / v4l_vmpo_select; v4l_ppo_hyper.weight_decay / decoupled_weight_decay (Adam's L2 and AdamW); v4l_net_cfg.activation (V4L_ACT_TANH on V4L_NET_MLP); per-optimiser Adam step counts; v4l_trainer_begin_guarded (opt-in skip of non-finite steps) / v4l_trainer_steps
int v4l_abi_sizeof(int which) {
  return which == 0 ? (int)sizeof(v4l_net_cfg) : which == 1 ? (int)sizeof(v4l_ppo_hyper) : which == 2 ? (int)sizeof(v4l_rollout) :
         which == 4 ? (int)sizeof(v4l_vmpo_hyper) : -1;  // (3 stays unassigned)
}

int v4l_net_create(const v4l_net_cfg* cfg, v4l_net** out) {
  V4L_REQUIRE(cfg != nullptr && out != nullptr, "v4l_net_create: null argument");
  v4l_net* n = new v4l_net();
  n->cfg = *cfg;
  int rc = n->build();
  if (rc) { delete n; return rc; }
  *out = n;
  return 0;
}
int v4l_net_set_categorical(v4l_net* net, int on) {
  V4L_REQUIRE(net != nullptr, "v4l_net_set_categorical: null argument");
  V4L_REQUIRE(!net->bound, "v4l_net_set_categorical: the net is bound already (set the flag between v4l_net_create and v4l_net_bind)");
  V4L_REQUIRE(net->cfg.kind == V4L_NET_MLP, "v4l_net_set_categorical: a categorical policy is a state-MLP net (V4L_NET_MLP, the "
              "reference's networks.Net), got kind %d", net->cfg.kind);
  V4L_REQUIRE(net->cfg.has_logstd == V4L_LOGSTD_NONE, "v4l_net_set_categorical: has_logstd must be 0 (V4L_LOGSTD_NONE: a categorical "
              "policy has no log sigma), got %d", net->cfg.has_logstd);
  V4L_REQUIRE(net->cfg.out_dim >= 2 && net->cfg.out_dim <= V4L_OUT_LD, "v4l_net_set_categorical: 2 <= out_dim <= %d (V4L_OUT_LD: the "
              "logits of the K actions fill one padded head row) required, got %d", V4L_OUT_LD, net->cfg.out_dim);
  net->categorical = on != 0;
  return 0;
}
void v4l_net_destroy(v4l_net* net) {
  if (net && net->aux) {
    (void)hipStreamDestroy(net->aux);
    (void)hipEventDestroy(net->ev_fork);
    (void)hipEventDestroy(net->ev_join);
  }
  if (net && net->aux2) {
    (void)hipStreamDestroy(net->aux2);
    (void)hipEventDestroy(net->ev_fork2);
    (void)hipEventDestroy(net->ev_join2);
  }
  delete net;
}
int v4l_net_num_params(const v4l_net* net) { return net ? (int)net->params.size() : -1; }
int v4l_net_param_info(const v4l_net* net, int i, const char** name, int* ndim, int64_t shape[4], int64_t* numel,
                       int64_t* grad_offset) {
  V4L_REQUIRE(net && i >= 0 && i < (int)net->params.size(), "v4l_net_param_info: index out of range");
  const ParamInfo& pi = net->params[i];
  if (name) *name = pi.name.c_str();
  if (ndim) *ndim = pi.ndim;
  if (shape) for (int d = 0; d < 4; ++d) shape[d] = pi.shape[d];
  if (numel) *numel = pi.numel;
  if (grad_offset) *grad_offset = pi.goff;
  return 0;
}
int64_t v4l_net_total_params(const v4l_net* net) { return net ? net->total_params : -1; }
int64_t v4l_net_packed_bytes(const v4l_net* net) {
  return net ? net->packed_elems * (is_half(net->cfg.compute) ? 2 : 4) + 256 : -1;
}
int64_t v4l_net_table_bytes(const v4l_net* net) { return net ? net->table_bytes() : -1; }
int64_t v4l_net_ws_floats(const v4l_net* net, int n, int train) {
  (void)train;
  if (!net || n <= 0) return -1;
  return net->layout(n).total;
}
int v4l_net_state_ld(const v4l_net* net) { return net ? net->Sp : -1; }

int64_t v4l_net_ws_offset(const v4l_net* net, int n, const char* name) {
  if (!net || !name) return -1;
  const Layout L = net->layout(n);
  const std::string s(name);
  auto idx = [&](const std::string& pre, size_t cnt) -> int {
    if (s.compare(0, pre.size(), pre) != 0 || s.size() == pre.size()) return -1;
    for (size_t k = pre.size(); k < s.size(); ++k)
      if (s[k] < '0' || s[k] > '9') return -1;  // "x1" is a token tensor, "xin1" / "xh1_0" are not
    int i = atoi(s.c_str() + pre.size());
    return (i >= 0 && (size_t)i < cnt) ? i : -1;
  };
  if (s == "c1") return L.c1;
  if (s == "c2") return L.c2;
  if (s == "c3") return L.c3;
  if (s == "vis") return L.vis;
  if (s == "pooled") return L.pooled;
  if (s == "out") return L.out;
  if (s == "dout") return L.dout;
  if (s == "dhc") return L.dhc;
  if (s == "dc1") return L.dc1;
  if (s == "dc2") return L.dc2;
  if (s == "dc3") return L.dc3;
  int i;
  if ((i = idx("eh", L.eh.size())) >= 0) return L.eh[i];
  if ((i = idx("hh", L.hh.size())) >= 0) return L.hh[i];
  if ((i = idx("x", L.x.size())) >= 0) return L.x[i];
  if ((i = idx("qkv", L.lw.size())) >= 0) return L.lw[i].qkv;
  if ((i = idx("P", L.lw.size())) >= 0) return L.lw[i].P;
  if ((i = idx("ctx", L.lw.size())) >= 0) return L.lw[i].ctx;
  if ((i = idx("mid", L.lw.size())) >= 0) return L.lw[i].x1;
  if ((i = idx("ff", L.lw.size())) >= 0) return L.lw[i].f;
  if ((i = idx("xin", L.lw.size())) >= 0) return L.lw[i].xin;
  if ((i = idx("xh1_", L.lw.size())) >= 0) return L.lw[i].xh1;
  if ((i = idx("xh2_", L.lw.size())) >= 0) return L.lw[i].xh2;
  if ((i = idx("rs1_", L.lw.size())) >= 0) return L.lw[i].rs1;
  if ((i = idx("rs2_", L.lw.size())) >= 0) return L.lw[i].rs2;
  // backward tensors (valid after v4l_net_backward): gradients w.r.t. pre-activations / sub-layer outputs
  if ((i = idx("dz2_", L.lb.size())) >= 0) return L.lb[i].dz2;
  if ((i = idx("df", L.lb.size())) >= 0) return L.lb[i].df;
  if ((i = idx("dz1_", L.lb.size())) >= 0) return L.lb[i].dz1;
  if ((i = idx("dqkv", L.lb.size())) >= 0) return L.lb[i].dqkv;
  if ((i = idx("dx", L.dxl.size())) >= 0) return L.dxl[i];
  if ((i = idx("dhh", L.dhh.size())) >= 0) return L.dhh[i];
  if ((i = idx("deh", L.deh.size())) >= 0) return L.deh[i];
  if (s == "dpool") return L.dpool;
  return -1;
}

int v4l_net_bind(v4l_net* net, float* const* params_dev, void* packed_dev, void* table_dev, void* stream) {
  V4L_REQUIRE(net && params_dev && packed_dev && table_dev, "v4l_net_bind: null argument");
  hipStream_t s = (hipStream_t)stream;
  for (size_t i = 0; i < net->params.size(); ++i) {
    V4L_REQUIRE(params_dev[i] != nullptr, "v4l_net_bind: parameter %s has a null device pointer", net->params[i].name.c_str());
    net->p[i] = params_dev[i];
  }
  for (size_t i = 0; i < net->packs.size(); ++i) net->packs[i].src = net->p[net->pack_param[i]];
  std::vector<ParamSeg> segs(net->params.size());
  int64_t blk = 0;
  for (size_t i = 0; i < net->params.size(); ++i) {
    segs[i].p = net->p[i];
    segs[i].goff = net->params[i].goff;
    segs[i].n = net->params[i].numel;
    segs[i].blk0 = blk;
    blk += cdiv64(net->params[i].numel, 256);
  }
  if (net->aux == nullptr && sw_int("V4L_PAR", 1) != 0) {
    V4L_HIP_CHECK(hipStreamCreateWithFlags(&net->aux, hipStreamNonBlocking));
    V4L_HIP_CHECK(hipEventCreateWithFlags(&net->ev_fork, hipEventDisableTiming));
    V4L_HIP_CHECK(hipEventCreateWithFlags(&net->ev_join, hipEventDisableTiming));
    V4L_HIP_CHECK(hipStreamCreateWithFlags(&net->aux2, hipStreamNonBlocking));
    V4L_HIP_CHECK(hipEventCreateWithFlags(&net->ev_fork2, hipEventDisableTiming));
    V4L_HIP_CHECK(hipEventCreateWithFlags(&net->ev_join2, hipEventDisableTiming));
  }
  net->packed = packed_dev;
  net->d_packs = (PackDesc*)table_dev;
  net->d_segs = (ParamSeg*)((char*)table_dev + (net->packs.size() * sizeof(PackDesc) + 63) / 64 * 64);
  net->d_red = (RedDesc*)((char*)net->d_segs + (net->params.size() * sizeof(ParamSeg) + 63) / 64 * 64);
  net->red_cached.clear();
  net->d_tnp = (TnProb*)((char*)net->d_red + (v4l_net::MAX_RED * sizeof(RedDesc) + 63) / 64 * 64);
  net->d_wide = (TnWide*)((char*)net->d_tnp + (v4l_net::MAX_TNP * sizeof(TnProb) + 63) / 64 * 64);
  net->tnp_cached.clear();
  net->d_sq = (float*)((char*)net->d_wide + (v4l_net::MAX_WIDE * sizeof(TnWide) + 63) / 64 * 64);
  net->red_blocks = 0;
  // synchronous pageable copies: the host vectors die at return
  V4L_HIP_CHECK(hipStreamSynchronize(s));
  V4L_HIP_CHECK(hipMemcpy(net->d_packs, net->packs.data(), net->packs.size() * sizeof(PackDesc), hipMemcpyHostToDevice));
  V4L_HIP_CHECK(hipMemcpy(net->d_segs, segs.data(), segs.size() * sizeof(ParamSeg), hipMemcpyHostToDevice));
  net->bound = true;
  ++net->gen;  // graphs captured against the previous packed / table buffers must not be replayed
  return 0;
}

int v4l_net_pack(v4l_net* net, void* stream) {
  V4L_REQUIRE(net && net->bound, "v4l_net_pack: net is not bound");
  hipStream_t s = (hipStream_t)stream;
  return by_compute(net->cfg.compute, [&](auto tag) -> int {
    typedef typename decltype(tag)::type T;
    V4L_KLAUNCH("pack", 0, s, pack_kernel<T>, dim3((unsigned)net->pack_blocks), dim3(256), 0, s, net->d_packs,
                (int)net->packs.size(), (T*)net->packed);
    V4L_LAUNCH_CHECK();
    return 0;
  });
}

int v4l_ingest(const v4l_net* net, const float* obs_dev, int n, float* state_dev, void* image_dev, int64_t slot0,
               void* stream) {
  V4L_REQUIRE(net && obs_dev && state_dev && n > 0, "v4l_ingest: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int S = net->cfg.state_dim;
  const int img = net->cfg.kind == V4L_NET_MLP ? 0 : net->cfg.in_channels * net->cfg.img_hw * net->cfg.img_hw;
  V4L_REQUIRE(img == 0 || image_dev != nullptr, "v4l_ingest: image_dev is null for a visual net");
  return by_compute(net->cfg.compute, [&](auto tag) -> int {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL(ingest_kernel<T>, dim3(n), dim3(256), 0, s, obs_dev, n, S, net->Sp, img, state_dev, (T*)image_dev, slot0,
                       (const long long*)nullptr);
    V4L_LAUNCH_CHECK();
    return 0;
  });
}

int v4l_net_forward(v4l_net* net, const float* state_dev, const void* image_dev, const int* rowidx_dev, int n,
                    float* ws_dev, int train, void* stream) {
  V4L_REQUIRE(net && net->bound, "v4l_net_forward: net is not bound");
  V4L_REQUIRE(state_dev && ws_dev && n > 0, "v4l_net_forward: bad argument");
  V4L_REQUIRE(net->cfg.kind == V4L_NET_MLP || image_dev != nullptr, "v4l_net_forward: image_dev is null");
  // train: a v4l_net_backward over this workspace follows — the conv activations it reads may then be saved in the operand type
  net->want_acts16 = train != 0;
  const int rc = by_compute(net->cfg.compute, [&](auto tag) -> int {
    typedef typename decltype(tag)::type T;
    return net->forward_t<T>(state_dev, (const T*)image_dev, rowidx_dev, n, ws_dev, (hipStream_t)stream);
  });
  net->want_acts16 = false;
  return rc;
}
float* v4l_net_out_ptr(const v4l_net* net, float* ws_dev, int n, int train) {
  (void)train;
  return ws_dev + net->layout(n).out;
}
float* v4l_net_dout_ptr(const v4l_net* net, float* ws_dev, int n) { return ws_dev + net->layout(n).dout; }
int v4l_net_set_grad_scale(v4l_net* net, float scale) {
  V4L_REQUIRE(net != nullptr, "v4l_net_set_grad_scale: null net");
  int e = 0;
  V4L_REQUIRE(scale > 0.f && frexpf(scale, &e) == 0.5f, "v4l_net_set_grad_scale: %g is not a positive power of two", (double)scale);
  net->grad_scale_next = scale;
  return 0;
}
float v4l_net_grad_scale(const v4l_net* net, int n) {
  if (net == nullptr || net->cfg.compute != V4L_F16 || n < 1) return 1.f;
  int lg = 0;
  while ((1 << lg) < n && lg < 30) ++lg;  // ceil(log2 n)
  return ldexpf(1.f, V4L_F16_SCALE_LOG2 + lg);
}

int v4l_net_backward(v4l_net* net, const float* state_dev, const void* image_dev, const int* rowidx_dev, int n,
                     float* ws_dev, float* grads_dev, void* stream) {
  V4L_REQUIRE(net && net->bound, "v4l_net_backward: net is not bound");
  V4L_REQUIRE(state_dev && ws_dev && grads_dev && n > 0, "v4l_net_backward: bad argument");
  return by_compute(net->cfg.compute, [&](auto tag) -> int {
    typedef typename decltype(tag)::type T;
    return net->backward_t<T>(state_dev, (const T*)image_dev, rowidx_dev, n, ws_dev, grads_dev, (hipStream_t)stream);
  });
}

int v4l_gauss_head(const float* meanp_dev, const float* logstd_dev, const float* acts_dev, int n, int A,
                   float* mean_dev, float* std_dev, float* logstd_c_dev, float* ent_dev, float* logp_dev,
                   void* stream) {
  V4L_REQUIRE(meanp_dev && logstd_dev && mean_dev && std_dev && logstd_c_dev && ent_dev && n > 0,
              "v4l_gauss_head: bad argument");
  V4L_REQUIRE(A > 0 && A <= V4L_MAX_ACT, "v4l_gauss_head: 1<=A<=%d (V4L_MAX_ACT) required, got %d", V4L_MAX_ACT, A);
  V4L_REQUIRE(acts_dev == nullptr || logp_dev != nullptr, "v4l_gauss_head: logp_dev is null");
  hipLaunchKernelGGL(gauss_head_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, meanp_dev, logstd_dev,
                     acts_dev, n, A, mean_dev, std_dev, logstd_c_dev, ent_dev, logp_dev, 0, (const float*)nullptr);
  V4L_LAUNCH_CHECK();
  return 0;
}
int v4l_gauss_head_tanh(const float* meanp_dev, const float* logstd_dev, const float* acts_dev, const float* pre_tanh_dev, int n,
                        int A, float* mean_dev, float* std_dev, float* logstd_c_dev, float* ent_dev, float* logp_dev,
                        void* stream) {
  V4L_REQUIRE(meanp_dev && logstd_dev && mean_dev && std_dev && logstd_c_dev && ent_dev && n > 0,
              "v4l_gauss_head_tanh: bad argument");
  V4L_REQUIRE(A > 0 && A <= V4L_MAX_ACT, "v4l_gauss_head_tanh: 1<=A<=%d (V4L_MAX_ACT) required, got %d", V4L_MAX_ACT, A);
  V4L_REQUIRE(acts_dev == nullptr || logp_dev != nullptr, "v4l_gauss_head_tanh: logp_dev is null");
  hipLaunchKernelGGL(gauss_head_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, meanp_dev, logstd_dev,
                     acts_dev, n, A, mean_dev, std_dev, logstd_c_dev, ent_dev, logp_dev, 1, pre_tanh_dev);
  V4L_LAUNCH_CHECK();
  return 0;
}
int v4l_gauss_head_sd(const float* out_dev, const float* acts_dev, const float* pre_tanh_dev, int n, int A, int tanh_action,
                      float* mean_dev, float* std_dev, float* logstd_c_dev, float* ent_dev, float* logp_dev, void* stream) {
  V4L_REQUIRE(out_dev && mean_dev && std_dev && logstd_c_dev && ent_dev && n > 0, "v4l_gauss_head_sd: bad argument");
  V4L_REQUIRE(A > 0 && 2 * A <= OUT_LD, "v4l_gauss_head_sd: 1<=A<=%d (mean and log sigma share the %d-column head row) required, got %d",
              OUT_LD / 2, OUT_LD, A);
  V4L_REQUIRE(acts_dev == nullptr || logp_dev != nullptr, "v4l_gauss_head_sd: logp_dev is null");
  hipLaunchKernelGGL(gauss_head_sd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, out_dev, acts_dev, n, A, mean_dev,
                     std_dev, logstd_c_dev, ent_dev, logp_dev, tanh_action ? 1 : 0, pre_tanh_dev);
  V4L_LAUNCH_CHECK();
  return 0;
}
int v4l_cat_head(const float* logits_dev, const float* acts_dev, int n, int K, float* probs_dev, float* ent_dev, float* logp_dev,
                 void* stream) {
  V4L_REQUIRE(logits_dev && probs_dev && ent_dev && n > 0, "v4l_cat_head: bad argument");
  V4L_REQUIRE(K >= 2 && K <= V4L_OUT_LD, "v4l_cat_head: 2<=K<=%d (V4L_OUT_LD) required, got %d", V4L_OUT_LD, K);
  V4L_REQUIRE(acts_dev == nullptr || logp_dev != nullptr, "v4l_cat_head: logp_dev is null");
  hipLaunchKernelGGL(cat_head_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, logits_dev, acts_dev, n, K, probs_dev,
                     ent_dev, logp_dev);
  V4L_LAUNCH_CHECK();
  return 0;
}
int v4l_cat_sample(const float* probs_dev, const float* u_dev, int n, int K, int deterministic, int64_t* idx_dev, void* stream) {
  V4L_REQUIRE(probs_dev && idx_dev && n > 0, "v4l_cat_sample: bad argument");
  V4L_REQUIRE(deterministic || u_dev != nullptr, "v4l_cat_sample: u_dev is null");
  V4L_REQUIRE(K >= 2 && K <= V4L_OUT_LD, "v4l_cat_sample: 2<=K<=%d (V4L_OUT_LD) required, got %d", V4L_OUT_LD, K);
  hipLaunchKernelGGL(cat_sample_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, probs_dev, u_dev, n, K,
                     deterministic ? 1 : 0, (long long*)idx_dev);
  V4L_LAUNCH_CHECK();
  return 0;
}
int v4l_col0(const float* src_dev, int n, float* dst_dev, void* stream) {
  V4L_REQUIRE(src_dev && dst_dev && n > 0, "v4l_col0: bad argument");
  hipLaunchKernelGGL(col0_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, src_dev, n, dst_dev);
  V4L_LAUNCH_CHECK();
  return 0;
}

int v4l_gae(const double* rewards_dev, const double* values_dev, const double* terminals_dev,
            const double* time_limits_dev, int tl_per_env, const double* last_value_dev, int T, int E, double gamma,
            double tau, int use_time_limit, double* scratch_dev, double* advs_dev, double* rets_dev, float* advs32_dev,
            float* rets32_dev, void* stream) {
  V4L_REQUIRE(rewards_dev && values_dev && terminals_dev && last_value_dev && advs_dev && rets_dev && scratch_dev &&
                  T > 0 && E > 0, "v4l_gae: bad argument");
  V4L_REQUIRE(!use_time_limit || time_limits_dev != nullptr, "v4l_gae: time_limits_dev is null");
  V4L_REQUIRE((advs32_dev == nullptr) == (rets32_dev == nullptr), "v4l_gae: advs32/rets32 must both be set or null");
  hipStream_t s = (hipStream_t)stream;
  const int64_t te = (int64_t)T * E;
  double *delta = scratch_dev, *coef = scratch_dev + te, *tlm = scratch_dev + 2 * te;
  g_op = "gae";
  V4L_KLAUNCH("gae_prep", 0, s, gae_prep_kernel, dim3((unsigned)cdiv64(te, 256)), dim3(256), 0, s, rewards_dev, values_dev,
              terminals_dev, time_limits_dev, tl_per_env, last_value_dev, T, E, gamma, tau, use_time_limit, delta, coef, tlm);
  V4L_LAUNCH_CHECK();
  V4L_KLAUNCH("gae_scan", 0, s, gae_scan_kernel, dim3(cdiv(E, 64)), dim3(64), 0, s, delta, coef, tlm, values_dev, T, E,
              use_time_limit, advs_dev, rets_dev, advs32_dev, rets32_dev);
  V4L_LAUNCH_CHECK();
  return 0;
}

int v4l_discount_reward(const double* rewards_dev, const double* values_dev, const double* terminals_dev,
                        const double* time_limits_dev, int tl_per_env, const double* last_value_dev, int T, int E, double gamma,
                        int use_time_limit, double* advs_dev, double* rets_dev, float* advs32_dev, float* rets32_dev,
                        void* stream) {
  V4L_REQUIRE(rewards_dev && values_dev && terminals_dev && last_value_dev && advs_dev && rets_dev && T > 0 && E > 0,
              "v4l_discount_reward: bad argument");
  V4L_REQUIRE(!use_time_limit || time_limits_dev != nullptr, "v4l_discount_reward: time_limits_dev is null");
  V4L_REQUIRE((advs32_dev == nullptr) == (rets32_dev == nullptr), "v4l_discount_reward: advs32/rets32 must both be set or null");
  hipStream_t s = (hipStream_t)stream;
  g_op = "gae";
  V4L_KLAUNCH("discount_scan", 0, s, discount_scan_kernel, dim3(cdiv(E, 64)), dim3(64), 0, s, rewards_dev, values_dev,
              terminals_dev, time_limits_dev, tl_per_env, last_value_dev, T, E, gamma, use_time_limit, advs_dev, rets_dev,
              advs32_dev, rets32_dev);
  V4L_LAUNCH_CHECK();
  return 0;
}

int v4l_obs_norm(const double* raw_dev, int64_t ld_raw, int E, int S, double* mean_dev, double* var_dev, double* count_dev,
                 double clip, int update, float* out32_dev, int64_t ld_out32, double* out64_dev, int64_t ld_out64,
                 const void* image_dev, int image_f64, int64_t ld_image, int64_t image_elems, float* image_out_dev,
                 int64_t ld_image_out, void* stream) {
  V4L_REQUIRE(raw_dev && mean_dev && var_dev && count_dev && E > 0 && S > 0 && ld_raw >= S, "v4l_obs_norm: bad argument");
  V4L_REQUIRE(out32_dev || out64_dev, "v4l_obs_norm: no output buffer");
  V4L_REQUIRE((!out32_dev || ld_out32 >= S) && (!out64_dev || ld_out64 >= S), "v4l_obs_norm: output row stride < S");
  V4L_REQUIRE(!image_dev || (image_out_dev && image_elems > 0 && ld_image >= image_elems && ld_image_out >= image_elems),
              "v4l_obs_norm: bad image arguments");
  ObsNorm p;
  p.raw = raw_dev; p.ld_raw = ld_raw;
  p.mean = mean_dev; p.var = var_dev; p.count = count_dev;
  p.clip = clip; p.E = E; p.S = S; p.update = update != 0;
  p.out32 = out32_dev; p.ld32 = ld_out32;
  p.out64 = out64_dev; p.ld64 = ld_out64;
  p.img = image_dev; p.img_f64 = image_f64 != 0; p.ld_img = ld_image; p.img_elems = image_dev ? image_elems : 0;
  p.img_out = image_out_dev; p.ld_img_out = ld_image_out;
  const int64_t img_blocks = image_dev ? std::min<int64_t>(cdiv64((int64_t)E * image_elems, 1024), 1024) : 0;
  g_op = "obs_norm";
  V4L_KLAUNCH("obs_norm", 0, (hipStream_t)stream, obs_norm_kernel, dim3((unsigned)(1 + img_blocks)), dim3(256), 0,
              (hipStream_t)stream, p);
  V4L_LAUNCH_CHECK();
  return 0;
}

#ifdef V4L_INFER_TIMING
int v4l_debug_stamps(long long* out32) {
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  return hipMemcpyFromSymbol(out32, HIP_SYMBOL(v4l::g_inf_stamps), 128 * sizeof(long long)) == hipSuccess ? 0 : -2;
}
int v4l_debug_block_log(long long* out5120) {
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  return hipMemcpyFromSymbol(out5120, HIP_SYMBOL(v4l::g_blk_log), 1024 * 5 * sizeof(long long)) == hipSuccess ? 0 : -2;
}
#endif
int v4l_prof_enable(int on) {
  g_prof = on != 0;
  return 0;
}
/* Writes one line per (phase|op|kernel): "label\tcalls\ttotal_us\tflops\n", clears the records. Synchronises. */
int64_t v4l_prof_collect(char* buf, int64_t cap) {
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  struct Agg { int64_t calls = 0; double us = 0, flops = 0; };
  std::vector<std::pair<std::string, Agg>> agg;
  for (ProfRec& r : g_recs) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
    size_t i = 0;
    for (; i < agg.size(); ++i) if (agg[i].first == r.label) break;
    if (i == agg.size()) agg.push_back({r.label, Agg()});
    agg[i].second.calls += 1;
    agg[i].second.us += ms * 1000.0;
    agg[i].second.flops += r.flops;
  }
  g_recs.clear();
  std::string out;
  char line[512];
  for (auto& kv : agg) {
    snprintf(line, sizeof(line), "%s\t%lld\t%.3f\t%.6e\n", kv.first.c_str(), (long long)kv.second.calls, kv.second.us,
             kv.second.flops);
    out += line;
  }
  if (buf && cap > 0) {
    const int64_t n = std::min<int64_t>(cap - 1, (int64_t)out.size());
    memcpy(buf, out.data(), n);
    buf[n] = 0;
  }
  return (int64_t)out.size();
}


// ------------------------------------------------------------------------------------------ actor (rollout step)
int v4l_actor_create(v4l_net* pf, v4l_net* vf, int E, v4l_actor** out) {
  V4L_REQUIRE(pf && vf && out && E > 0, "v4l_actor_create: bad argument");
  // (a policy: Gaussian, or a net flagged by v4l_net_set_categorical)
  V4L_REQUIRE(pf->is_policy() && !vf->is_policy() && vf->cfg.out_dim == 1 && pf->cfg.kind == vf->cfg.kind &&
                  pf->cfg.compute == vf->cfg.compute && pf->cfg.state_dim == vf->cfg.state_dim &&
                  pf->cfg.n_enc_hidden == vf->cfg.n_enc_hidden && pf->cfg.activation == vf->cfg.activation,
              "v4l_actor_create: pf must be a Gaussian policy and vf a value net of the same kind/compute/shape/activation");
  v4l_actor* a = new v4l_actor();
  a->pf = pf; a->vf = vf; a->E = E;
  *out = a;
  return 0;
}
void v4l_actor_destroy(v4l_actor* a) {
  if (a && a->gexec) (void)hipGraphExecDestroy(a->gexec);
  if (a && a->aux) {
    (void)hipStreamDestroy(a->aux);
    (void)hipEventDestroy(a->ev_fork);
    (void)hipEventDestroy(a->ev_join);
  }
  delete a;
}
int64_t v4l_actor_ws_floats(const v4l_actor* a) {
  if (!a) return -1;
  return a->pf->layout(a->E).total + a->vf->layout(a->E).total;
}
int64_t v4l_actor_ctl_bytes(const v4l_actor* a) { return a ? 256 + (int64_t)round_up(a->E, 64) * sizeof(int) : -1; }
int v4l_actor_bind(v4l_actor* a, float* ws_dev, void* ctl_dev, void* stream) {
  (void)stream;
  V4L_REQUIRE(a && ws_dev && ctl_dev, "v4l_actor_bind: null argument");
  V4L_REQUIRE(a->pf->bound && a->vf->bound, "v4l_actor_bind: bind pf and vf first");
  if (a->gexec) { (void)hipGraphExecDestroy(a->gexec); a->gexec = nullptr; }
  a->warm = false;
  if (a->aux == nullptr && a->pf->aux != nullptr) {
    V4L_HIP_CHECK(hipStreamCreateWithFlags(&a->aux, hipStreamNonBlocking));
    V4L_HIP_CHECK(hipEventCreateWithFlags(&a->ev_fork, hipEventDisableTiming));
    V4L_HIP_CHECK(hipEventCreateWithFlags(&a->ev_join, hipEventDisableTiming));
  }
  a->ws = ws_dev;
  a->ctl = (ActCtl*)ctl_dev;
  a->rowidx = (int*)((char*)ctl_dev + 256);
  // step cursor, launch sequence number, hand-over counters and the error flag start from zero, together with their host mirrors
  V4L_HIP_CHECK(hipMemsetAsync(ctl_dev, 0, sizeof(ActCtl), (hipStream_t)stream));
  a->dense_seq = 0; a->dense_in_graph = false; a->t_host = -1;
  a->bound = true;
  return 0;
}
// Health of the rollout step's device-side hand-overs (csrc/rollout_dense.h): *err_out = 0, or 1 + the index of the stage
// counter a block gave up waiting for since the last check. Synchronises the stream and clears the flag. A step that ran with
// the flag set has already filed NaN actions (the collector's non-finite-action check stops the epoch); this call is how a host
// finds out about a lost hand-over on the value side as well — the collector calls it once per epoch.
int v4l_actor_check(v4l_actor* a, int* err_out, void* stream) {
  V4L_REQUIRE(a && a->bound && err_out, "v4l_actor_check: bad argument");
  hipStream_t s = (hipStream_t)stream;
  unsigned err = 0;
  V4L_HIP_CHECK(hipMemcpyAsync(&err, &a->ctl->err, sizeof(err), hipMemcpyDeviceToHost, s));
  V4L_HIP_CHECK(hipStreamSynchronize(s));
  if (err != 0) V4L_HIP_CHECK(hipMemsetAsync(&a->ctl->err, 0, sizeof(err), s));
  *err_out = (int)err;
  return 0;
}
int v4l_actor_seek(v4l_actor* a, int64_t t, void* stream) {
  V4L_REQUIRE(a && a->bound && t >= 0, "v4l_actor_seek: bad argument");
  a->t_host = t;
  hipLaunchKernelGGL(act_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, a->ctl, (long long)t);
  V4L_LAUNCH_CHECK();
  return 0;
}

static bool actor_same_encoder_layout(const v4l_actor* a) {
  const v4l_net_cfg &p = a->pf->cfg, &v = a->vf->cfg;
  bool same = p.token_norm == v.token_norm && p.pytorch_encoder == v.pytorch_encoder && p.n_layers == v.n_layers &&
              p.n_enc_hidden == v.n_enc_hidden && p.token_dim == v.token_dim && p.visual_dim == v.visual_dim &&
              p.ff_dim == v.ff_dim && p.in_channels == v.in_channels && p.img_hw == v.img_hw && p.max_pool == v.max_pool;
  for (int i = 0; same && i < p.n_enc_hidden; ++i) same = p.enc_hidden[i] == v.enc_hidden[i];
  return same;
}

static int run_actor_step(v4l_actor* a, const StepIO& io, int shared_encoder, hipStream_t s) {
  v4l_net *pf = a->pf, *vf = a->vf;
  const int E = a->E;
  int rc;
  V4L_REQUIRE(pf->bound && vf->bound, "v4l_actor_step: nets are not bound");
  const int compute = pf->cfg.compute;
  switch (const StepRoute route = step_route(a, shared_encoder)) {
    // (the state-MLP kernels carry the hidden activation as a template argument; v4l_actor_create saw pf's and vf's agree)
    case StepRoute::MLP_ONE_BLOCK:
      return by_half(compute, [&](auto tag) -> int {
        typedef typename decltype(tag)::type H;
        return pf->cfg.activation == V4L_ACT_TANH ? run_actor_mlp2<H, V4L_ACT_TANH>(a, io, s) : run_actor_mlp2<H, V4L_ACT_RELU>(a, io, s);
      });
    case StepRoute::MLP_PER_SAMPLE:
      return by_compute(compute, [&](auto tag) -> int {
        typedef typename decltype(tag)::type T;
        if (pf->sd())  // (sigma from the head row: instantiations of their own, the others are the code they were)
          return pf->cfg.activation == V4L_ACT_TANH ? run_actor_fused_mlp<T, V4L_ACT_TANH, true>(a, io, s)
                                                    : run_actor_fused_mlp<T, V4L_ACT_RELU, true>(a, io, s);
        return pf->cfg.activation == V4L_ACT_TANH ? run_actor_fused_mlp<T, V4L_ACT_TANH>(a, io, s)
                                                  : run_actor_fused_mlp<T, V4L_ACT_RELU>(a, io, s);
      });
    case StepRoute::CNN_DENSE:
      return by_half(compute, [&](auto tag) -> int { return run_actor_dense_cnn<typename decltype(tag)::type>(a, io, s); });
    case StepRoute::CNN_PER_SAMPLE:
      return by_compute(compute, [&](auto tag) -> int { return run_actor_fused_cnn<typename decltype(tag)::type>(a, io, s); });
    case StepRoute::STACK_TOK16:
    case StepRoute::STACK_TOK17:
    case StepRoute::STACK_F32ENC:
      return by_compute(compute, [&](auto tag) -> int { return run_actor_fused<typename decltype(tag)::type>(a, io, route, s); });
    case StepRoute::GENERAL:
      break;
  }
  // General step. The value net may continue from the POLICY's encoder output (stage 2 reads enc_ws + its OWN layout's offset of
  // the token tensor) only if both nets lay their workspaces out identically up to that tensor: token_norm, use_pytorch_encoder
  // and the layer count belong to each net in the reference (nets.py:797-820, 948-963) and may differ between pf and vf — then
  // each net runs its own encoder pass over the shared parameters (same values, one more encoder launch), never a read of a
  // region the policy did not write.
  if (shared_encoder && !actor_same_encoder_layout(a)) shared_encoder = 0;
  PhaseScope ps("rollout");
  g_op = "ctl";
  V4L_KLAUNCH("act_begin", 0, s, act_begin_kernel, dim3(1), dim3(256), 0, s, a->ctl, E, a->rowidx);
  V4L_LAUNCH_CHECK();
  const int S = pf->cfg.state_dim;
  const int img = pf->cfg.kind == V4L_NET_MLP ? 0 : pf->cfg.in_channels * pf->cfg.img_hw * pf->cfg.img_hw;
  g_op = "ingest";
  if ((rc = by_compute(pf->cfg.compute, [&](auto tag) -> int {
        typedef typename decltype(tag)::type T;
        V4L_KLAUNCH("ingest", 0, s, ingest_kernel<T>, dim3(E), dim3(256), 0, s, io.obs, E, S, pf->Sp, img, io.state_roll, (T*)io.image_roll,
                    (int64_t)0, (const long long*)&a->ctl->t);
        V4L_LAUNCH_CHECK();
        return 0;
      })))
    return rc;
  float* ws_pf = a->ws;
  float* ws_vf = a->ws + pf->layout(E).total;
  // policy encoder, then the two trunks side by side: the value net shares the encoder with the policy
  // (starter/ppo_locotransformer.py:79-100) and continues from the policy's token tensor on the aux stream
  auto fwd = [&](v4l_net* net, float* ws, hipStream_t st, const float* enc, int stage) {
    return by_compute(pf->cfg.compute, [&](auto tag) -> int {
      typedef typename decltype(tag)::type T;
      return net->forward_t<T>(io.state_roll, (const T*)io.image_roll, a->rowidx, E, ws, st, enc, stage);
    });
  };
  const bool par = shared_encoder && a->aux != nullptr && !capturing(s);
  if (shared_encoder) {
    if ((rc = fwd(pf, ws_pf, s, nullptr, 1))) return rc;
    hipStream_t sv = s;
    if (par) {
      V4L_HIP_CHECK(hipEventRecord(a->ev_fork, s));
      V4L_HIP_CHECK(hipStreamWaitEvent(a->aux, a->ev_fork, 0));
      sv = a->aux;
    }
    if ((rc = fwd(vf, ws_vf, sv, ws_pf, 2))) return rc;
    if ((rc = fwd(pf, ws_pf, s, nullptr, 2))) return rc;
    if (par) {
      V4L_HIP_CHECK(hipEventRecord(a->ev_join, a->aux));
      V4L_HIP_CHECK(hipStreamWaitEvent(s, a->ev_join, 0));
    }
  } else {
    if ((rc = fwd(pf, ws_pf, s, nullptr, 0))) return rc;
    if ((rc = fwd(vf, ws_vf, s, nullptr, 0))) return rc;
  }
  g_op = "sample";
  if (pf->cat())  // io.eps: [E] uniforms (negative: argmax); io.mean / io.stdv are not written
    V4L_KLAUNCH("act_finish", 0, s, act_finish_cat_kernel, dim3(1), dim3(256), 0, s, a->ctl, ws_pf + pf->layout(E).out,
                ws_vf + vf->layout(E).out, io.eps, E, pf->cfg.out_dim, io.acts_roll, io.values_roll, io.logp_roll, io.action, io.ent,
                io.value);
  else if (pf->sd())
    V4L_KLAUNCH("act_finish", 0, s, act_finish_sd_kernel, dim3(1), dim3(256), 0, s, a->ctl, ws_pf + pf->layout(E).out,
                ws_vf + vf->layout(E).out, io.eps, E, pf->act_dim(), io.acts_roll, io.values_roll, io.logp_roll, io.action, io.mean,
                io.stdv, io.ent, io.value, pf->cfg.tanh_action);
  else
  V4L_KLAUNCH("act_finish", 0, s, act_finish_kernel, dim3(1), dim3(256), 0, s, a->ctl, ws_pf + pf->layout(E).out,
              pf->p[pf->logstd], ws_vf + vf->layout(E).out, io.eps, E, pf->cfg.out_dim, io.acts_roll, io.values_roll, io.logp_roll,
              io.action, io.mean, io.stdv, io.ent, io.value, pf->cfg.tanh_action);
  V4L_LAUNCH_CHECK();
  return 0;
}

static int actor_step_impl(v4l_actor* a, const StepIO& io, int shared_encoder, int use_graph, hipStream_t s) {
  V4L_REQUIRE(a && a->bound, "v4l_actor_step: actor is not bound");
  V4L_REQUIRE(io.obs && io.eps && io.state_roll && io.action && io.mean && io.stdv && io.ent && io.value,
              "v4l_actor_step: null argument");
  V4L_REQUIRE(a->pf->cfg.kind == V4L_NET_MLP || io.image_roll, "v4l_actor_step: image rollout array missing");
  auto run = [&]() { return run_actor_step(a, io, shared_encoder, s); };
  if (!use_graph || g_prof || s == nullptr) return run();
  // (a captured step reads fp32 rows: img16 is null here)
  const void* key[16] = {io.obs, io.eps, io.state_roll, io.image_roll, io.acts_roll, io.values_roll, io.logp_roll, io.action,
                         io.mean, io.stdv, io.ent, io.value, io.img16, (const void*)(intptr_t)(shared_encoder + 1),
                         (const void*)(intptr_t)a->pf->gen, (const void*)(intptr_t)a->vf->gen};
  static_assert(sizeof(key) == sizeof(a->key), "graph key size");
  if (memcmp(key, a->key, sizeof(key)) != 0) {
    if (a->gexec) { (void)hipGraphExecDestroy(a->gexec); a->gexec = nullptr; }
    a->warm = false;
    a->dense_in_graph = false;
    memcpy(a->key, key, sizeof(key));
  }
  if (!a->warm) { a->warm = true; return run(); }
  if (a->gexec == nullptr)
    if (int rc = capture_graph(s, "actor", run, &a->gexec)) return rc;
  V4L_HIP_CHECK(hipGraphLaunch(a->gexec, s));
  if (a->dense_in_graph) ++a->dense_seq;  // the replayed rollout_dense_kernel advanced ctl->seq
  V4L_TRACE("actor: launched");
  return 0;
}
static int actor_step(v4l_actor* a, const StepIO& io, int shared_encoder, int use_graph, void* stream) {
  const int rc = actor_step_impl(a, io, shared_encoder, use_graph, (hipStream_t)stream);
  if (rc == 0 && a->t_host >= 0) ++a->t_host;  // one env step, whichever way it was launched (the device cursor moved too)
  return rc;
}
int v4l_actor_step(v4l_actor* a, const float* obs_dev, const float* eps_dev, float* state_roll_dev, void* image_roll_dev,
                   float* acts_roll_dev, float* values_roll_dev, float* logp_roll_dev, float* action_dev, float* mean_dev,
                   float* std_dev, float* ent_dev, float* value_dev, int shared_encoder, int use_graph, void* stream) {
  const StepIO io = {obs_dev, eps_dev, state_roll_dev, image_roll_dev, acts_roll_dev, values_roll_dev, logp_roll_dev, action_dev,
                     mean_dev, std_dev, ent_dev, value_dev, nullptr, 0};
  return actor_step(a, io, shared_encoder, use_graph, stream);
}

// Which actors' steps take the observation split: the routes on rollout_encoder2_kernel (they imply a shared encoder, 16-bit
// compute and an image net). A TanhNormal policy keeps the fp32 rows, even on a LocoTransformer route that could read the split.
static bool actor_takes_split(const v4l_actor* a, int shared_encoder) {
  if (a->pf->cfg.tanh_action) return false;
  const StepRoute r = step_route(a, shared_encoder);
  return r == StepRoute::CNN_DENSE || r == StepRoute::STACK_TOK16 || r == StepRoute::STACK_TOK17;
}
// introspection for tests: the name of the route step_route picks for this actor (the state-MLP kernels share one profiler label)
const char* v4l_actor_route(const v4l_actor* a, int shared_encoder) {
  if (a == nullptr) return "";
  switch (step_route(a, shared_encoder)) {
    case StepRoute::MLP_ONE_BLOCK: return "MLP_ONE_BLOCK";
    case StepRoute::MLP_PER_SAMPLE: return "MLP_PER_SAMPLE";
    case StepRoute::CNN_DENSE: return "CNN_DENSE";
    case StepRoute::CNN_PER_SAMPLE: return "CNN_PER_SAMPLE";
    case StepRoute::STACK_TOK16: return "STACK_TOK16";
    case StepRoute::STACK_TOK17: return "STACK_TOK17";
    case StepRoute::STACK_F32ENC: return "STACK_F32ENC";
    case StepRoute::GENERAL: return "GENERAL";
  }
  return "";
}
int v4l_actor_split_supported(const v4l_actor* a, int shared_encoder) {
  return (a && a->bound && actor_takes_split(a, shared_encoder)) ? 1 : 0;
}
int v4l_actor_step_split(v4l_actor* a, const float* proprio_dev, const void* image16_dev, const float* eps_dev,
                         float* state_roll_dev, void* image_roll_dev, float* acts_roll_dev, float* values_roll_dev,
                         float* logp_roll_dev, float* action_dev, float* mean_dev, float* std_dev, float* ent_dev,
                         float* value_dev, int shared_encoder, void* stream) {
  V4L_REQUIRE(a && a->bound && image16_dev, "v4l_actor_step_split: bad argument");
  V4L_REQUIRE(actor_takes_split(a, shared_encoder),
              "v4l_actor_step_split: this actor's step does not run on the split-observation kernels (bf16 compute, an image "
              "net on the fused rollout step); use v4l_actor_step with fp32 observation rows");
  V4L_REQUIRE(proprio_dev != nullptr || a->pf->cfg.state_dim == 0, "v4l_actor_step_split: proprio rows missing");
  // (vision-only nets, S = 0: no kernel reads the row pointer; the argument check of the step wants it non-null)
  const float* rows = proprio_dev != nullptr ? proprio_dev : reinterpret_cast<const float*>(image16_dev);
  const StepIO io = {rows, eps_dev, state_roll_dev, image_roll_dev, acts_roll_dev, values_roll_dev, logp_roll_dev, action_dev,
                     mean_dev, std_dev, ent_dev, value_dev, image16_dev,
                     (int64_t)a->pf->cfg.in_channels * a->pf->cfg.img_hw * a->pf->cfg.img_hw};
  return actor_step(a, io, shared_encoder, /*use_graph=*/0, stream);
}

// ---- the collector's env step as one host call (csrc/host_step.h)
int v4l_host_cast_rows(const double* rows_host, int64_t ld, int E, int S, int64_t img_elems, float* proprio_out, void* image_out,
                       int compute, int threads) {
  V4L_REQUIRE(rows_host && image_out && E > 0 && S >= 0 && img_elems > 0 && ld >= S + img_elems, "v4l_host_cast_rows: bad argument");
  V4L_REQUIRE(S == 0 || proprio_out != nullptr, "v4l_host_cast_rows: proprio rows have nowhere to go");
  V4L_REQUIRE(compute == V4L_F32 || compute == V4L_BF16 || compute == V4L_F16, "v4l_host_cast_rows: unknown compute mode %d", compute);
  V4L_REQUIRE(threads >= 1 && threads <= 256, "v4l_host_cast_rows: threads must be in [1, 256]");
  const int kind = compute == V4L_BF16 ? host::CAST_BF16 : compute == V4L_F16 ? host::CAST_F16 : 0;
  return host::cast_rows(rows_host, ld, E, S, img_elems, proprio_out, image_out, kind, threads);
}
int v4l_host_cast_simd(void) { return host::have_avx512() ? 1 : 0; }
int v4l_actor_step_rows(v4l_actor* a, const double* rows_host, int64_t ld, float* proprio_pinned, void* image16_pinned,
                        const float* eps_dev, float* state_roll_dev, void* image_roll_dev, float* acts_roll_dev,
                        float* values_roll_dev, float* logp_roll_dev, float* action_pinned, float* mean_dev, float* std_dev,
                        float* ent_dev, float* value_pinned, int shared_encoder, int threads, double poll_seconds, void* stream) {
  V4L_REQUIRE(a && a->bound && rows_host && image16_pinned && action_pinned && value_pinned, "v4l_actor_step_rows: bad argument");
  V4L_REQUIRE(actor_takes_split(a, shared_encoder), "v4l_actor_step_rows: this actor's step does not take the split observation "
              "(16-bit compute, an image net on the fused rollout step)");
  const v4l_net_cfg& c = a->pf->cfg;
  const int64_t img = (int64_t)c.in_channels * c.img_hw * c.img_hw;
  int rc = v4l_host_cast_rows(rows_host, ld, a->E, c.state_dim, img, proprio_pinned, image16_pinned, c.compute, threads);
  if (rc) return rc;
  const int na = a->E * a->pf->act_dim(), nv = a->E;
  const bool poll = poll_seconds > 0.0;
  if (poll) {  // armed: a number in every slot means every (env, net) block has written its output, i.e. finished reading the rows
    const float nan = __builtin_nanf("");
    for (int i = 0; i < na; ++i) action_pinned[i] = nan;
    for (int i = 0; i < nv; ++i) value_pinned[i] = nan;
    std::atomic_thread_fence(std::memory_order_seq_cst);
  }
  rc = v4l_actor_step_split(a, c.state_dim ? proprio_pinned : nullptr, image16_pinned, eps_dev, state_roll_dev, image_roll_dev,
                            acts_roll_dev, values_roll_dev, logp_roll_dev, action_pinned, mean_dev, std_dev, ent_dev, value_pinned,
                            shared_encoder, stream);
  if (rc) return rc;
  if (!poll) return 1;
  const auto t_end = std::chrono::steady_clock::now() + std::chrono::nanoseconds((int64_t)(poll_seconds * 1e9));
  for (unsigned it = 0;; ++it) {
    if (host::arrived(action_pinned, na) && host::arrived(value_pinned, nv)) return 0;
    host::cpu_relax();
    if ((it & 63) == 63 && std::chrono::steady_clock::now() > t_end) return 1;  // the caller synchronises (a policy that emits NaN ends here)
  }
}

// ------------------------------------------------------------------------------------------ trainer
int v4l_trainer_create(v4l_net* pf, v4l_net* vf, v4l_net* target_pf, v4l_trainer** out) {
  V4L_REQUIRE(pf && vf && target_pf && out, "v4l_trainer_create: null argument");
  // (a policy / target pair with a logstd parameter each, or V4L_LOGSTD_HEAD each: GaussianContPolicy, continuous_policy.py:222-236)
  // or flagged by v4l_net_set_categorical each (CategoricalDisPolicy, policies/discrete_policies.py:127-172)
  V4L_REQUIRE(pf->is_policy() && pf->cfg.has_logstd == target_pf->cfg.has_logstd && pf->cat() == target_pf->cat() &&
                  !vf->is_policy() && vf->cfg.out_dim == 1,
              "v4l_trainer_create: pf/target_pf must be Gaussian policies of one kind (a logstd parameter each, or "
              "V4L_LOGSTD_HEAD each) and vf a scalar value net");
  V4L_REQUIRE(pf->cfg.out_dim == target_pf->cfg.out_dim, "v4l_trainer_create: pf and target_pf disagree on out_dim");
  V4L_REQUIRE(pf->cfg.compute == vf->cfg.compute && pf->cfg.compute == target_pf->cfg.compute &&
                  pf->cfg.kind == vf->cfg.kind && pf->cfg.kind == target_pf->cfg.kind &&
                  pf->cfg.state_dim == vf->cfg.state_dim && pf->total_params == target_pf->total_params &&
                  pf->cfg.activation == vf->cfg.activation && pf->cfg.activation == target_pf->cfg.activation,
              "v4l_trainer_create: pf, vf and target_pf disagree on kind/compute/shape/activation");
  v4l_trainer* t = new v4l_trainer();
  t->pf = pf; t->vf = vf; t->tpf = target_pf;
  *out = t;
  return 0;
}
static void drop_ppo_graph(v4l_trainer* tr) {
  if (tr->gexec) { (void)hipGraphExecDestroy(tr->gexec); tr->gexec = nullptr; }
  if (tr->gexec_run) { (void)hipGraphExecDestroy(tr->gexec_run); tr->gexec_run = nullptr; }
  tr->gexec_run_count = 0;
  tr->warm = false;
}
static void drop_vmpo_graph(v4l_trainer* tr) {
  if (tr->vexec) { (void)hipGraphExecDestroy(tr->vexec); tr->vexec = nullptr; }
  if (tr->vexec_run) { (void)hipGraphExecDestroy(tr->vexec_run); tr->vexec_run = nullptr; }
  tr->vexec_run_count = 0;
  tr->vwarm = false;
}
// (PPO's graphs and V-MPO's: both bake the same addresses in, so whatever invalidates one invalidates the other)
static void drop_a2c_graph(v4l_trainer* tr) {
  if (tr->aexec) { (void)hipGraphExecDestroy(tr->aexec); tr->aexec = nullptr; }
  if (tr->aexec_run) { (void)hipGraphExecDestroy(tr->aexec_run); tr->aexec_run = nullptr; }
  tr->aexec_run_count = 0;
  tr->awarm = false;
}
static void drop_reinforce_graph(v4l_trainer* tr) {
  if (tr->rexec) { (void)hipGraphExecDestroy(tr->rexec); tr->rexec = nullptr; }
  if (tr->rexec_run) { (void)hipGraphExecDestroy(tr->rexec_run); tr->rexec_run = nullptr; }
  tr->rexec_run_count = 0;
  tr->rwarm = false;
}
static void drop_kl_graph(v4l_trainer* tr) {
  if (tr->kexec) { (void)hipGraphExecDestroy(tr->kexec); tr->kexec = nullptr; }
  if (tr->kexec_run) { (void)hipGraphExecDestroy(tr->kexec_run); tr->kexec_run = nullptr; }
  tr->kexec_run_count = 0;
  tr->kwarm = false;
}
static void drop_kl_adapt_graph(v4l_trainer* tr) {
  if (tr->dexec) { (void)hipGraphExecDestroy(tr->dexec); tr->dexec = nullptr; }
  if (tr->dexec_run) { (void)hipGraphExecDestroy(tr->dexec_run); tr->dexec_run = nullptr; }
  tr->dexec_run_count = 0;
  tr->dwarm = false;
}
static void drop_graph(v4l_trainer* tr) {
  drop_kl_adapt_graph(tr);
  drop_kl_graph(tr);
  drop_ppo_graph(tr);
  drop_vmpo_graph(tr);
  drop_a2c_graph(tr);
  drop_reinforce_graph(tr);
}
void v4l_trainer_destroy(v4l_trainer* tr) {
  if (tr) drop_graph(tr);
  if (tr && tr->comm && g_rccl.CommDestroy) { (void)g_rccl.CommDestroy(tr->comm); tr->comm = nullptr; }
  if (tr && tr->aux) {
    (void)hipStreamDestroy(tr->aux);
    (void)hipEventDestroy(tr->ev_fork);
    (void)hipEventDestroy(tr->ev_join);
  }
  delete tr;
}
int64_t v4l_trainer_ws_floats(const v4l_trainer* tr, int n) {
  if (!tr || n <= 0) return -1;
  return std::max(tr->pf->layout(n).total, tr->vf->layout(n).total) + tr->tpf->layout(n).total;
}
int64_t v4l_trainer_ctl_bytes(const v4l_trainer* tr, int n) {
  if (!tr || n <= 0) return -1;
  return 256 + 256 + 2 * GRAD_NORM_PARTS * sizeof(float) + (int64_t)round_up(n, 64) * sizeof(int);
}
int v4l_trainer_bind(v4l_trainer* tr, float* g_pf_dev, float* m_pf_dev, float* v_pf_dev, float* g_vf_dev,
                     float* m_vf_dev, float* v_vf_dev, float* ws_dev, int64_t ws_floats, void* ctl_dev, int n_max,
                     void* stream) {
  (void)stream;
  V4L_REQUIRE(tr && g_pf_dev && m_pf_dev && v_pf_dev && g_vf_dev && m_vf_dev && v_vf_dev && ws_dev && ctl_dev && n_max > 1,
              "v4l_trainer_bind: bad argument");
  V4L_REQUIRE(tr->pf->bound && tr->vf->bound && tr->tpf->bound, "v4l_trainer_bind: bind the three nets first");
  drop_graph(tr);
  tr->g_pf = g_pf_dev; tr->m_pf = m_pf_dev; tr->v_pf = v_pf_dev;
  tr->g_vf = g_vf_dev; tr->m_vf = m_vf_dev; tr->v_vf = v_vf_dev;
  tr->ws = ws_dev; tr->ws_floats = ws_floats;
  if (tr->aux == nullptr && tr->pf->aux != nullptr) {
    V4L_HIP_CHECK(hipStreamCreateWithFlags(&tr->aux, hipStreamNonBlocking));
    V4L_HIP_CHECK(hipEventCreateWithFlags(&tr->ev_fork, hipEventDisableTiming));
    V4L_HIP_CHECK(hipEventCreateWithFlags(&tr->ev_join, hipEventDisableTiming));
  }
  tr->ctl = (UpdCtl*)ctl_dev;
  tr->stats_cur = (float*)((char*)ctl_dev + 256);
  tr->norm_part = (float*)((char*)ctl_dev + 512);  // [2][GRAD_NORM_PARTS] squared-norm partials (vf, pf)
  tr->rowidx_cur = (int*)((char*)ctl_dev + 512 + 2 * GRAD_NORM_PARTS * sizeof(float));
  tr->n_max = n_max;
  tr->bound = true;
  return 0;
}

// The optimiser fields every entry point that takes a v4l_ppo_hyper checks (they are fixed for the life of a trainer: the
// opening launch copies them into UpdCtl and the captured graphs bake the kernel variant in).
static int check_hyper(const v4l_ppo_hyper* hp) {
  V4L_REQUIRE(hp->weight_decay >= 0.0 && hp->weight_decay <= 3.0e38,
              "v4l_ppo_hyper.weight_decay must be finite and >= 0 (got %g)", hp->weight_decay);
  return 0;
}

int v4l_trainer_begin_guarded(v4l_trainer* tr, const int* rowidx_all_dev, float* stats_all_dev, int* skip_all_dev, double lr_pf,
                              double lr_vf, int64_t step_pf, int64_t step_vf, const v4l_ppo_hyper* hp, void* stream) {
  V4L_REQUIRE(tr && tr->bound && hp && step_pf >= 0 && step_vf >= 0, "v4l_trainer_begin: bad argument");
  if (int rc = check_hyper(hp)) return rc;
  // baked into the graph (the flag pointer also decides whether the guard is on)
  if (rowidx_all_dev != tr->rowidx_all || stats_all_dev != tr->stats_all || skip_all_dev != tr->skip_all) drop_graph(tr);
  tr->rowidx_all = rowidx_all_dev;
  tr->stats_all = stats_all_dev;
  tr->skip_all = skip_all_dev;
  hipLaunchKernelGGL(ctl_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, tr->ctl, 0, (long long)step_pf, (long long)step_vf,
                     lr_pf, lr_vf, hp->beta1, hp->beta2, hp->weight_decay, hp->decoupled_weight_decay != 0 ? 1 : 0);
  V4L_LAUNCH_CHECK();
  return 0;
}
int v4l_trainer_begin(v4l_trainer* tr, const int* rowidx_all_dev, float* stats_all_dev, double lr_pf, double lr_vf,
                      int64_t steps_done, const v4l_ppo_hyper* hp, void* stream) {
  return v4l_trainer_begin_guarded(tr, rowidx_all_dev, stats_all_dev, nullptr, lr_pf, lr_vf, steps_done, steps_done, hp, stream);
}
int v4l_trainer_steps(v4l_trainer* tr, int64_t* step_pf_out, int64_t* step_vf_out, void* stream) {
  V4L_REQUIRE(tr && tr->bound && step_pf_out && step_vf_out, "v4l_trainer_steps: bad argument");
  hipStream_t s = (hipStream_t)stream;
  long long st[2] = {0, 0};
  V4L_HIP_CHECK(hipMemcpyAsync(st, tr->ctl->step, sizeof(st), hipMemcpyDeviceToHost, s));
  V4L_HIP_CHECK(hipStreamSynchronize(s));
  *step_pf_out = st[0];
  *step_vf_out = st[1];
  return 0;
}

// The encoder half of a training forward (forward_t stage 1: up to the token tensor) for a pass whose layers, heads and loss
// rows run inside the fused launch of the backward that follows (csrc/wps_fb.h)
static int net_forward_encoder(v4l_net* net, const float* state_dev, const void* image_dev, const int* rowidx_dev, int n, float* ws_dev,
                               void* stream) {
  V4L_REQUIRE(net && net->bound, "v4l_net_forward: net is not bound");
  net->want_acts16 = true;
  const int rc = by_compute(net->cfg.compute, [&](auto tag) -> int {
    typedef typename decltype(tag)::type T;
    return net->forward_t<T>(state_dev, (const T*)image_dev, rowidx_dev, n, ws_dev, (hipStream_t)stream, nullptr, 1);
  });
  net->want_acts16 = false;
  return rc;
}

static int check_update_args(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp) {
  V4L_REQUIRE(tr && tr->bound, "v4l_trainer: not bound");
  V4L_REQUIRE(ro && hp && n > 1 && n <= tr->n_max, "v4l_trainer: bad argument (need 1 < n <= n_max)");
  V4L_REQUIRE(ro->state_dev && ro->acts_dev && ro->advs_dev && ro->rets_dev, "v4l_trainer: rollout arrays missing");
  V4L_REQUIRE(tr->pf->cfg.kind == V4L_NET_MLP || ro->image_dev, "v4l_trainer: rollout image array missing");
  V4L_REQUIRE(!hp->clipped_value_loss || ro->values_dev, "v4l_trainer: clipped_value_loss needs values_dev");
  V4L_REQUIRE(hp->world_size >= 1, "v4l_trainer: world_size must be >= 1");
  V4L_REQUIRE(!tr->pf->sd() || (hp->world_size == 1 && tr->comm == nullptr),
              "v4l_trainer: a V4L_LOGSTD_HEAD policy (GaussianContPolicy) runs in a single process");
  V4L_REQUIRE(!tr->pf->cat() || (hp->world_size == 1 && tr->comm == nullptr),
              "v4l_trainer: a categorical policy (v4l_net_set_categorical) runs in a single process");
  if (int rc = check_hyper(hp)) return rc;
  V4L_REQUIRE(tr->comm == nullptr || hp->world_size == tr->comm_world,
              "v4l_trainer: hyper.world_size (%d) differs from the communicator's (%d)", hp->world_size, tr->comm_world);
  V4L_REQUIRE(v4l_trainer_ws_floats(tr, n) <= tr->ws_floats, "v4l_trainer: workspace too small for n=%d", n);
  return 0;
}

// ---- the pieces the A2C and REINFORCE stages are put together from (the PPO and V-MPO stages below spell theirs out: DESIGN.md 7)
// An update's opening launch, as in v4l_trainer_critic_grads: selects the rows of this update, clears the statistics record, advances Adam's step,
// advantage statistics (block 0) and refreshes `net`'s packed weights (the other blocks): the critic's, or the policy's where no
// critic runs.
static int launch_begin_pack(v4l_trainer* tr, v4l_net* net, const v4l_rollout* ro, int n, hipStream_t s) {
  g_op = "ctl";
  return by_compute(net->cfg.compute, [&](auto tag) -> int {
    typedef typename decltype(tag)::type T;
    V4L_KLAUNCH("begin_pack", 0, s, begin_pack_kernel<T>, dim3((unsigned)net->pack_blocks + 1), dim3(256), 0, s, tr->ctl, tr->rowidx_all, n,
                tr->rowidx_cur, tr->stats_cur, ro->advs_dev, net->d_packs, (int)net->packs.size(), (T*)net->packed);
    V4L_LAUNCH_CHECK();
    return 0;
  });
}
// The loss launch's arguments for `rows` rows of the policy's forward read through rowidx, a log sigma per action column and no
// target policy (tmean, tlogstd, logp_old, clip stay zero); the stage sets ent_coef.
static ActorArgs actor_args(const v4l_trainer* tr, const v4l_rollout* ro, int rows, const int* rowidx) {
  v4l_net* pf = tr->pf;
  const Layout Lp = pf->layout(rows);
  ActorArgs aa;
  memset(&aa, 0, sizeof(aa));
  // (a categorical policy: mean = the logits rows, A = K, no log sigma)
  aa.mean = tr->ws + Lp.out; aa.logstd = pf->cat() ? nullptr : pf->p[pf->logstd];
  aa.acts = ro->acts_dev; aa.adv = ro->advs_dev; aa.rowidx = rowidx;
  aa.n = rows; aa.A = pf->cfg.out_dim; aa.inv_n = 1.f / (float)rows;
  aa.dmean = tr->ws + Lp.dout; aa.dlogstd = pf->cat() ? nullptr : tr->g_pf + pf->params[pf->logstd].goff; aa.st = tr->stats_cur;
  aa.tanh_action = pf->cfg.tanh_action;
  aa.gscale = v4l_net_grad_scale(pf, rows);
  return aa;
}

int v4l_trainer_critic_grads(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, void* stream) {
  int rc = check_update_args(tr, ro, n, hp);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  v4l_net* vf = tr->vf;
  float* st = tr->stats_cur;
  const int* rowidx = tr->rowidx_cur;
  g_op = "ctl";
  // selects the rows of this update, clears the statistics record, advances Adam's step, advantage statistics (block 0) and
  // refreshes the critic's packed weights (the other blocks) in one launch
  // (no clearing of g_vf / g_pf: v4l_net_backward writes every element of the flat gradient — tests/test_gpu_parity.py
  // test_backward starts from a NaN-filled buffer)
  V4L_REQUIRE(vf->bound, "v4l_trainer_critic_grads: the critic net is not bound");
  if ((rc = by_compute(vf->cfg.compute, [&](auto tag) -> int {
        typedef typename decltype(tag)::type T;
        V4L_KLAUNCH("begin_pack", 0, s, begin_pack_kernel<T>, dim3((unsigned)vf->pack_blocks + 1), dim3(256), 0, s, tr->ctl, tr->rowidx_all, n,
                    tr->rowidx_cur, st, ro->advs_dev, vf->d_packs, (int)vf->packs.size(), (T*)vf->packed);
        V4L_LAUNCH_CHECK();
        return 0;
      })))
    return rc;
  const float inv_n = 1.f / ((float)n * (float)hp->world_size);
  const float gscale = v4l_net_grad_scale(vf, n);
  if (vf->layer_route().fb_allowed) {
    // round 6: encoder forward, then ONE launch for layers + heads forward, the loss rows and the backward (csrc/wps_fb.h)
    { PhaseScope ps("vf.fwd");
    if ((rc = net_forward_encoder(vf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, stream))) return rc; }
    FbLoss lo;
    memset(&lo, 0, sizeof(lo));
    lo.actor = 0;
    lo.ret = ro->rets_dev; lo.oldv = ro->values_dev; lo.clipped = hp->clipped_value_loss; lo.clip = hp->clip_para;
    lo.rowidx = rowidx; lo.inv_n = inv_n; lo.gscale = gscale; lo.st = st;
    vf->fb_loss = &lo;
    PhaseScope ps("vf.bwd");
    rc = v4l_net_backward(vf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, tr->g_vf, stream);
    vf->fb_loss = nullptr;
    return rc;
  }
  { PhaseScope ps("vf.fwd");
  if ((rc = v4l_net_forward(vf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, 1, stream))) return rc; }
  const Layout L = vf->layout(n);
  g_op = "loss";
  {
    // The heads' data-grad chain as extra blocks of the loss launch (when the backward that follows is the wave-per-sample
    // one) pays for the POLICY: its statistics block takes 17 us on its own, so the 21 us chain rides along almost for free
    // and wps_layer_bwd_kernel loses its 10 us heads phase. The critic's statistics take 6.7 us: there the chain would cost
    // more (21 us launch) than it saves — measured with tools/update_timeline.py, profiles/r4_update_timeline.txt — so the
    // critic keeps the in-kernel heads unless V4L_WPS_HEAD_EXT_CRITIC=1.
    RowsChain hc;
    const bool ext = vf->heads_ext(tr->ws, n, &hc, true) != 0;
    const dim3 blk(n >= 512 ? 1024 : 256);
    if (ext) {
      const bool big = n >= 512;
#define V4L_CL(T_, NW_) launch_critic_loss_heads<T_, NW_>(s, tr->ws + L.out, ro->rets_dev, ro->values_dev, rowidx, n, inv_n, \
                                                          hp->clipped_value_loss, hp->clip_para, tr->ws + L.dout, st, hc, gscale)
      rc = by_compute(vf->cfg.compute, [&](auto tag) -> int {
        typedef typename decltype(tag)::type T;
        return big ? V4L_CL(T, 16) : V4L_CL(T, 4);
      });
#undef V4L_CL
      if (rc) return rc;
    } else {
      V4L_KLAUNCH("critic_loss", 0, s, critic_loss_kernel, dim3(1), blk, 0, s, tr->ws + L.out, ro->rets_dev, ro->values_dev,
                  rowidx, n, inv_n, hp->clipped_value_loss, hp->clip_para, tr->ws + L.dout, st, gscale);
    }
  }
  V4L_LAUNCH_CHECK();
  PhaseScope ps("vf.bwd");
  return v4l_net_backward(vf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, tr->g_vf, stream);
}

static int adam_step(v4l_trainer* tr, v4l_net* net, float* g, float* m, float* v, const v4l_ppo_hyper* hp, int which,
                     float* norm_out, hipStream_t s, bool close_update = false) {
  int gb = (int)std::min<int64_t>(GRAD_NORM_PARTS, cdiv64(net->total_params, 1024));
  const float* part = tr->norm_part + which * GRAD_NORM_PARTS;
  const float* extra = nullptr;
  int nextra = 0;
  if (int rc = check_hyper(hp)) return rc;
  g_op = "optim";
  // The gradient's sum of squares: on one GPU the backward's wgrad_reduce launch already left it, one partial per block
  // (plus log sigma's gradient, which the loss kernel writes itself); after an all-reduce the buffer is summed again.
  constexpr bool sq_from_reduce = true;
  // (only for the buffer the last backward pass of this net wrote, and only once: a host that drives the phases itself and
  // runs another v4l_net_backward — or hands over another buffer — between grads and step gets the summed-again norm)
  if (sq_from_reduce && tr->comm == nullptr && hp->world_size == 1 && net->red_blocks > 0 && net->red_blocks <= ADAM_MAX_PARTS &&
      net->red_grads == g) {
    part = net->d_sq;
    gb = net->red_blocks;
    net->red_blocks = 0;  // consumed
    if (net->logstd >= 0) { extra = g + net->params[net->logstd].goff; nextra = (int)net->params[net->logstd].numel; }
    V4L_REQUIRE(nextra <= 64, "internal: log sigma wider than a wave");
  } else {
    V4L_KLAUNCH("grad_sumsq", 0, s, grad_sumsq_kernel, dim3(gb), dim3(256), 0, s, g, net->total_params, tr->norm_part + which * GRAD_NORM_PARTS);
    V4L_LAUNCH_CHECK();
  }
  // (a 1-dimensional policy logs log_std/std = NaN, as the reference's log_std.std() does: not a non-finite update)
  const unsigned nf_exempt = tr->pf->cfg.out_dim == 1 ? 1u << ST_LS_STD : 0u;
  // weight_decay == 0 (with either class) is the kernel without decay: today's arithmetic, bit for bit
#define V4L_CLIP_ADAM(WD_)                                                                                                     \
  V4L_KLAUNCH("clip_adam", 0, s, clip_adam_kernel<WD_>, dim3((unsigned)net->seg_blocks), dim3(256), 0, s, net->d_segs,         \
              (int)net->params.size(), g, m, v, part, gb, extra, nextra, hp->max_grad_norm, hp->eps, tr->ctl, which, norm_out, \
              close_update ? tr->ctl : (UpdCtl*)nullptr, (const float*)tr->stats_cur, tr->stats_all, tr->skip_all, nf_exempt)
  if (!(hp->weight_decay > 0.0)) V4L_CLIP_ADAM(WD_NONE);
  else if (hp->decoupled_weight_decay) V4L_CLIP_ADAM(WD_DECOUPLED);
  else V4L_CLIP_ADAM(WD_COUPLED);
#undef V4L_CLIP_ADAM
  V4L_LAUNCH_CHECK();
  return 0;
}

int v4l_trainer_critic_step(v4l_trainer* tr, const v4l_ppo_hyper* hp, void* stream) {
  V4L_REQUIRE(tr && tr->bound && hp, "v4l_trainer_critic_step: bad argument");
  float* st = tr->stats_cur;
  return adam_step(tr, tr->vf, tr->g_vf, tr->m_vf, tr->v_vf, hp, 1, st + ST_GN_VF, (hipStream_t)stream);
}

int v4l_trainer_actor_grads(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, void* stream) {
  int rc = check_update_args(tr, ro, n, hp);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  v4l_net *pf = tr->pf, *tp = tr->tpf;
  float* st = tr->stats_cur;
  const int* rowidx = tr->rowidx_cur;
  if (hp->world_size > 1 || tr->comm != nullptr) {
    hipLaunchKernelGGL(adv_stats_finalize_kernel, dim3(1), dim3(1), 0, s, st);
    V4L_LAUNCH_CHECK();
  }
  const Layout Lp = pf->layout(n), Lt = tp->layout(n);
  float* ws_t = tr->ws + std::max(Lp.total, tr->vf->layout(n).total);
  // frozen target policy (packed once per epoch by v4l_trainer_sync_target) on the trainer's aux stream, next to the
  // live policy's repack + forward: the two passes are independent until the loss. Skipped entirely when the rollout
  // carries log pi_old recorded at action time.
  const bool stored = ro->logp_old_dev != nullptr;
  hipStream_t s_tgt = s;
  const bool par_tgt = !stored && tr->aux != nullptr && !capturing(s);
  if (par_tgt) {
    V4L_HIP_CHECK(hipEventRecord(tr->ev_fork, s));
    V4L_HIP_CHECK(hipStreamWaitEvent(tr->aux, tr->ev_fork, 0));
    s_tgt = tr->aux;
  }
  if (!stored) {
    PhaseScope ps("tpf.fwd");
    if ((rc = v4l_net_forward(tp, ro->state_dev, ro->image_dev, rowidx, n, ws_t, 0, (void*)s_tgt))) return rc;
  }
  if ((rc = v4l_net_pack(pf, stream))) return rc;  // the critic step moved the shared encoder
  // round 6: with log pi_old stored at action time the policy's pass is encoder forward + ONE fused launch (csrc/wps_fb.h)
  const bool fb = stored && !pf->cfg.tanh_action && pf->layer_route().fb_allowed;
  { PhaseScope ps("pf.fwd");
  if (fb) rc = net_forward_encoder(pf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, stream);
  else rc = v4l_net_forward(pf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, 1, stream);
  if (rc) return rc; }
  if (par_tgt) {
    V4L_HIP_CHECK(hipEventRecord(tr->ev_join, tr->aux));
    V4L_HIP_CHECK(hipStreamWaitEvent(s, tr->ev_join, 0));
  }
  const float inv_n = 1.f / ((float)n * (float)hp->world_size);
  g_op = "loss";
  {
    ActorArgs aa;
    const bool sd = pf->sd();  // log sigma from the head row: no logstd parameter, its gradient leaves in the d(out) row
    if (pf->cat()) {  // logits rows, A = K, one action index per row: actor_args' conventions plus the target's rows and the clip
      aa = actor_args(tr, ro, n, rowidx);
      aa.tmean = stored ? nullptr : ws_t + Lt.out;
      aa.logp_old = ro->logp_old_dev; aa.inv_n = inv_n; aa.clip = hp->clip_para; aa.ent_coef = hp->entropy_coeff;
      // (V4L_NET_MLP: neither the fused forward-loss-backward launch nor the heads' chain beside the statistics)
      if ((rc = launch_actor_loss_cat(s, aa, loss_block(n)))) return rc;
      V4L_LAUNCH_CHECK();
      PhaseScope ps("pf.bwd");
      return v4l_net_backward(pf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, tr->g_pf, stream);
    }
    aa.mean = tr->ws + Lp.out; aa.logstd = sd ? nullptr : pf->p[pf->logstd];
    aa.tmean = stored ? nullptr : ws_t + Lt.out; aa.tlogstd = stored || sd ? nullptr : tp->p[tp->logstd];
    aa.logp_old = ro->logp_old_dev; aa.acts = ro->acts_dev; aa.adv = ro->advs_dev; aa.rowidx = rowidx;
    aa.n = n; aa.A = pf->act_dim(); aa.inv_n = inv_n; aa.clip = hp->clip_para; aa.ent_coef = hp->entropy_coeff;
    aa.dmean = tr->ws + Lp.dout; aa.dlogstd = sd ? nullptr : tr->g_pf + pf->params[pf->logstd].goff; aa.st = st;
    aa.tanh_action = pf->cfg.tanh_action;
    aa.gscale = v4l_net_grad_scale(pf, n);
    if (sd) {  // (V4L_NET_MLP: neither the fused forward-loss-backward launch nor the heads' chain beside the statistics)
      const dim3 blk(n >= 512 ? 1024 : 256);
      if ((rc = launch_actor_loss_sd(s, aa, blk))) return rc;
      V4L_LAUNCH_CHECK();
      PhaseScope ps("pf.bwd");
      return v4l_net_backward(pf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, tr->g_pf, stream);
    }
    if (fb) {
      FbLoss lo;
      memset(&lo, 0, sizeof(lo));
      lo.actor = 1;
      lo.aa = aa;
      lo.rowidx = rowidx; lo.inv_n = inv_n; lo.gscale = aa.gscale; lo.st = st;
      pf->fb_loss = &lo;
      PhaseScope ps("pf.bwd");
      rc = v4l_net_backward(pf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, tr->g_pf, stream);
      pf->fb_loss = nullptr;
      return rc;
    }
    RowsChain hc;
    const bool ext = !pf->cfg.tanh_action && pf->heads_ext(tr->ws, n, &hc) != 0;
    const dim3 blk(n >= 512 ? 1024 : 256);
    // the per-row code holds its per-dimension state per thread: capacity 8 for every A <= 8, V4L_MAX_ACT above (csrc/elem.h)
    const bool wide = act_cap(aa.A) != ACT_CAP_NARROW;
    if (ext) {
      const bool big = n >= 512;
      rc = by_compute(pf->cfg.compute, [&](auto tag) -> int {
        typedef typename decltype(tag)::type T;
        if (wide) return big ? launch_actor_loss_heads<T, 16, V4L_MAX_ACT>(s, aa, hc) : launch_actor_loss_heads<T, 4, V4L_MAX_ACT>(s, aa, hc);
        return big ? launch_actor_loss_heads<T, 16, ACT_CAP_NARROW>(s, aa, hc) : launch_actor_loss_heads<T, 4, ACT_CAP_NARROW>(s, aa, hc);
      });
    } else {
      rc = wide ? launch_actor_loss<V4L_MAX_ACT>(s, aa, blk) : launch_actor_loss<ACT_CAP_NARROW>(s, aa, blk);
    }
    if (rc) return rc;
  }
  V4L_LAUNCH_CHECK();
  PhaseScope ps("pf.bwd");
  return v4l_net_backward(pf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, tr->g_pf, stream);
}

int v4l_trainer_actor_step(v4l_trainer* tr, const v4l_ppo_hyper* hp, void* stream) {
  V4L_REQUIRE(tr && tr->bound && hp, "v4l_trainer_actor_step: bad argument");
  hipStream_t s = (hipStream_t)stream;
  float* st = tr->stats_cur;
  // the policy's Adam launch also closes the update (statistics record out, minibatch index + 1)
  return adam_step(tr, tr->pf, tr->g_pf, tr->m_pf, tr->v_pf, hp, 0, st + ST_GN_PF, s, true);
}

// ---- V-MPO (torchrl/algo/on_policy/v_mpo.py): the actor stage of an update whose other phases are PPO's
int v4l_vmpo_select(const float* adv_dev, const int* rowidx_dev, int n, int* sel_dev, void* stream) {
  V4L_REQUIRE(adv_dev && sel_dev && n >= 1, "v4l_vmpo_select: bad argument");
  return launch_vmpo_select((hipStream_t)stream, adv_dev, rowidx_dev, n, sel_dev);
}
int64_t v4l_trainer_vmpo_bytes(const v4l_trainer* tr, int n_max) {
  if (!tr || n_max <= 0) return -1;
  static_assert(sizeof(VmpoState) <= 128 && VST_SIZE * sizeof(float) <= 128, "V-MPO block layout [VmpoState | record | rows]");
  return 256 + (int64_t)round_up((n_max + 1) / 2, 64) * sizeof(int);
}
static int vmpo_write_state(v4l_trainer* tr, const double* v, hipStream_t s) {
  hipLaunchKernelGGL(vmpo_state_set_kernel, dim3(1), dim3(1), 0, s, tr->vmpo, v[0], v[1], v[2], v[3], v[4], v[5], (long long)v[6]);
  V4L_LAUNCH_CHECK();
  return 0;
}
int v4l_trainer_vmpo_init(v4l_trainer* tr, const v4l_vmpo_hyper* vhp, void* block_dev, int n_max, void* stream) {
  V4L_REQUIRE(tr && vhp && block_dev && n_max > 1, "v4l_trainer_vmpo_init: bad argument");
  V4L_REQUIRE(((uintptr_t)block_dev & 255) == 0, "v4l_trainer_vmpo_init: the block must be 256-byte aligned");
  V4L_REQUIRE(vhp->eta0 > 0.0 && vhp->alpha0 > 0.0 && vhp->eta0 <= 3.0e38 && vhp->alpha0 <= 3.0e38,
              "v4l_vmpo_hyper: eta0 and alpha0 must be finite and > 0 (got %g, %g)", vhp->eta0, vhp->alpha0);
  V4L_REQUIRE(vhp->eta_eps == vhp->eta_eps && vhp->alpha_eps == vhp->alpha_eps && (vhp->lr_scale == 0.0 || vhp->lr_scale == 1.0),
              "v4l_vmpo_hyper: eta_eps / alpha_eps must be numbers and lr_scale 0 or 1");
  tr->vmpo = (VmpoState*)block_dev;
  tr->vmpo_stats_cur = (float*)((char*)block_dev + 128);
  tr->vmpo_sel = (int*)((char*)block_dev + 256);
  tr->vmpo_n_max = n_max;
  tr->vmpo_hp = *vhp;
  const double fresh[V4L_VMPO_STATE] = {(double)(float)vhp->eta0, (double)(float)vhp->alpha0, 0.0, 0.0, 0.0, 0.0, 0.0};
  return vmpo_write_state(tr, fresh, (hipStream_t)stream);
}
int v4l_trainer_vmpo_state(v4l_trainer* tr, double* out, void* stream) {
  V4L_REQUIRE(tr && tr->vmpo && out, "v4l_trainer_vmpo_state: no V-MPO state (v4l_trainer_vmpo_init)");
  hipStream_t s = (hipStream_t)stream;
  VmpoState h;
  V4L_HIP_CHECK(hipMemcpyAsync(&h, tr->vmpo, sizeof(h), hipMemcpyDeviceToHost, s));
  V4L_HIP_CHECK(hipStreamSynchronize(s));
  out[0] = h.eta; out[1] = h.alpha; out[2] = h.m[0]; out[3] = h.m[1]; out[4] = h.v[0]; out[5] = h.v[1]; out[6] = (double)h.step;
  return 0;
}
int v4l_trainer_vmpo_set_state(v4l_trainer* tr, const double* in, void* stream) {
  V4L_REQUIRE(tr && tr->vmpo && in, "v4l_trainer_vmpo_set_state: no V-MPO state (v4l_trainer_vmpo_init)");
  V4L_REQUIRE(in[0] > 0.0 && in[1] > 0.0 && in[4] >= 0.0 && in[5] >= 0.0 && in[6] >= 0.0,
              "v4l_trainer_vmpo_set_state: eta, alpha must be > 0, the second moments and the step count >= 0");
  return vmpo_write_state(tr, in, (hipStream_t)stream);
}
static int check_vmpo_args(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp) {
  int rc = check_update_args(tr, ro, n, hp);
  if (rc) return rc;
  V4L_REQUIRE(!tr->pf->sd(), "v4l_trainer_vmpo: a V4L_LOGSTD_HEAD policy (GaussianContPolicy) runs under the PPO update only: the V-MPO "
              "loss kernel takes one log sigma per action column");
  V4L_REQUIRE(!tr->pf->cat(), "v4l_trainer_vmpo: a categorical policy (v4l_net_set_categorical) runs under the A2C and REINFORCE updates "
              "only: the V-MPO loss kernel and its KL are Gaussian");
  V4L_REQUIRE(tr->kl_all == nullptr, "v4l_trainer_vmpo: no KL early stop (v4l_trainer_kl_stop) in a V-MPO run");
  V4L_REQUIRE(tr->ad_all == nullptr, "v4l_trainer_vmpo: no KL-adaptive learning rates (v4l_trainer_kl_adapt) in a V-MPO run");
  V4L_REQUIRE(tr->vmpo != nullptr, "v4l_trainer_vmpo_actor_grads: no V-MPO state (v4l_trainer_vmpo_init)");
  V4L_REQUIRE(n <= tr->vmpo_n_max, "v4l_trainer_vmpo_actor_grads: n = %d is over the V-MPO block's n_max = %d", n, tr->vmpo_n_max);
  V4L_REQUIRE(hp->world_size == 1 && tr->comm == nullptr, "v4l_trainer_vmpo_actor_grads: V-MPO runs in a single process");
  return 0;
}
// The actor stage itself, eagerly or under THIS library's capture (v4l_trainer_vmpo_update_next / _update_run). Under capture the
// target forward stays on the capturing stream, as in v4l_trainer_actor_grads: its launch sequence holds memset nodes
// (hipMemsetAsync / hipMemset2DAsync of the forward's row buffers), and a capture with those on a forked side stream is the
// pattern that crashes inside the runtime (see capturing() above; the captured weight-grad forks hold kernels only).
static int vmpo_actor_stage(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* vstats_all_dev,
                            void* stream) {
  int rc;
  hipStream_t s = (hipStream_t)stream;
  v4l_net *pf = tr->pf, *tp = tr->tpf;
  const int m = (n + 1) / 2;  // idx.chunk(2)[0], v_mpo.py:67
  const int* sel = tr->vmpo_sel;
  // 1. the better half of the minibatch, on the device (nothing below waits for the host)
  if ((rc = launch_vmpo_select(s, ro->advs_dev, tr->rowidx_cur, n, tr->vmpo_sel))) return rc;
  const Layout Lp = pf->layout(m), Lt = tp->layout(m);
  float* ws_t = tr->ws + std::max(pf->layout(n).total, tr->vf->layout(n).total);
  // 2. the frozen target policy on those rows, next to the live policy's repack + forward (v4l_trainer_actor_grads' fork)
  hipStream_t s_tgt = s;
  const bool par_tgt = tr->aux != nullptr && !capturing(s);
  if (par_tgt) {
    V4L_HIP_CHECK(hipEventRecord(tr->ev_fork, s));
    V4L_HIP_CHECK(hipStreamWaitEvent(tr->aux, tr->ev_fork, 0));
    s_tgt = tr->aux;
  }
  { PhaseScope ps("tpf.fwd");
  if ((rc = v4l_net_forward(tp, ro->state_dev, ro->image_dev, sel, m, ws_t, 0, (void*)s_tgt))) return rc; }
  if ((rc = v4l_net_pack(pf, stream))) return rc;  // 3. the critic step moved the shared encoder
  { PhaseScope ps("pf.fwd");  // 4. forward, loss and backward as launches of their own (the fused launch's loss is PPO's)
  if ((rc = v4l_net_forward(pf, ro->state_dev, ro->image_dev, sel, m, tr->ws, 1, stream))) return rc; }
  if (par_tgt) {
    V4L_HIP_CHECK(hipEventRecord(tr->ev_join, tr->aux));
    V4L_HIP_CHECK(hipStreamWaitEvent(s, tr->ev_join, 0));
  }
  g_op = "loss";
  {
    ActorArgs aa;
    memset(&aa, 0, sizeof(aa));
    aa.mean = tr->ws + Lp.out; aa.logstd = pf->p[pf->logstd];
    aa.tmean = ws_t + Lt.out; aa.tlogstd = tp->p[tp->logstd];
    aa.logp_old = nullptr; aa.acts = ro->acts_dev; aa.adv = ro->advs_dev; aa.rowidx = sel;
    aa.n = m; aa.A = pf->cfg.out_dim; aa.inv_n = 1.f / (float)m; aa.clip = 0.f; aa.ent_coef = 0.f;  // entropy_coeff: accepted, unused (v_mpo.py)
    aa.dmean = tr->ws + Lp.dout; aa.dlogstd = tr->g_pf + pf->params[pf->logstd].goff; aa.st = tr->stats_cur;
    aa.tanh_action = pf->cfg.tanh_action;
    aa.gscale = v4l_net_grad_scale(pf, m);
    VmpoArgs va;
    memset(&va, 0, sizeof(va));
    va.vs = tr->vmpo; va.vst_cur = tr->vmpo_stats_cur; va.vst_all = vstats_all_dev; va.ctl = tr->ctl;
    va.eta_eps = tr->vmpo_hp.eta_eps; va.alpha_eps = tr->vmpo_hp.alpha_eps; va.lr_scale = tr->vmpo_hp.lr_scale; va.adam_eps = hp->eps;
    const dim3 blk(m >= 512 ? 1024 : 256);
    rc = act_cap(aa.A) != ACT_CAP_NARROW ? launch_vmpo_loss<V4L_MAX_ACT>(s, aa, va, blk) : launch_vmpo_loss<ACT_CAP_NARROW>(s, aa, va, blk);  // 5.
    if (rc) return rc;
  }
  PhaseScope ps("pf.bwd");  // 6.
  return v4l_net_backward(pf, ro->state_dev, ro->image_dev, sel, m, tr->ws, tr->g_pf, stream);
}
int v4l_trainer_vmpo_actor_grads(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* vstats_all_dev,
                                 void* stream) {
  int rc = check_vmpo_args(tr, ro, n, hp);
  if (rc) return rc;
  // (a caller's capture is refused: the captured V-MPO update is v4l_trainer_vmpo_update_next's, which keys and owns its graph)
  V4L_REQUIRE(!capturing((hipStream_t)stream),
              "v4l_trainer_vmpo_actor_grads: a V-MPO update is a sequence of eager launches (no stream capture)");
  return vmpo_actor_stage(tr, ro, n, hp, vstats_all_dev, stream);
}


int v4l_comm_available(void) { return rccl_load(); }
int v4l_trainer_comm_info(const v4l_trainer* tr, int* rank_out, int* world_out) {
  V4L_REQUIRE(tr != nullptr, "v4l_trainer_comm_info: null argument");
  int rank = 0, world = 1;
  if (tr->comm != nullptr) {  // as the communicator itself reports them, not as the caller passed them in
    V4L_RCCL_CHECK(g_rccl.CommCount(tr->comm, &world));
    V4L_RCCL_CHECK(g_rccl.CommUserRank(tr->comm, &rank));
  }
  if (rank_out) *rank_out = rank;
  if (world_out) *world_out = world;
  return 0;
}
int v4l_comm_unique_id(char* id_out) {
  V4L_REQUIRE(id_out != nullptr, "v4l_comm_unique_id: null argument");
  int rc = rccl_load();
  if (rc) return rc;
  RcclUid id;
  V4L_RCCL_CHECK(g_rccl.GetUniqueId(&id));
  memcpy(id_out, id.internal, sizeof(id.internal));
  return 0;
}
int v4l_trainer_comm_init(v4l_trainer* tr, const char* id, int rank, int world) {
  V4L_REQUIRE(tr && id && world >= 1 && rank >= 0 && rank < world, "v4l_trainer_comm_init: bad argument");
  V4L_REQUIRE(tr->comm == nullptr, "v4l_trainer_comm_init: the trainer already has a communicator");
  int rc = rccl_load();
  if (rc) return rc;
  RcclUid uid;
  memcpy(uid.internal, id, sizeof(uid.internal));
  void* comm = nullptr;
  V4L_RCCL_CHECK(g_rccl.CommInitRank(&comm, world, uid, rank));
  drop_graph(tr);
  tr->comm = comm; tr->comm_rank = rank; tr->comm_world = world;
  return 0;
}
int v4l_trainer_comm_destroy(v4l_trainer* tr) {
  V4L_REQUIRE(tr != nullptr, "v4l_trainer_comm_destroy: null argument");
  if (tr->comm == nullptr) return 0;
  drop_graph(tr);
  void* comm = tr->comm;
  tr->comm = nullptr; tr->comm_world = 1; tr->comm_rank = 0;
  V4L_RCCL_CHECK(g_rccl.CommDestroy(comm));
  return 0;
}
// The scalars of a bucket's tail, for hosts that run the collective themselves (pack = 1 before it, 0 after it)
int v4l_trainer_bucket_tail(v4l_trainer* tr, int which, int pack, int world, void* stream) {
  V4L_REQUIRE(tr && tr->bound && (which == 0 || which == 1) && world >= 1, "v4l_trainer_bucket_tail: bad argument");
  v4l_net* net = which ? tr->vf : tr->pf;
  float* tail = (which ? tr->g_vf : tr->g_pf) + net->total_params;
  hipLaunchKernelGGL(bucket_tail_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tr->stats_cur, tail, which, pack ? 1 : 0,
                     1.f / (float)world);
  V4L_LAUNCH_CHECK();
  return 0;
}
// One in-place sum all-reduce of a gradient bucket: [gradients | V4L_BUCKET_TAIL scalars] (which: 1 = critic, 0 = policy)
int v4l_sync_grads(v4l_trainer* tr, int which, void* stream) {
  V4L_REQUIRE(tr && tr->bound && (which == 0 || which == 1), "v4l_sync_grads: bad argument");
  V4L_REQUIRE(tr->comm != nullptr, "v4l_sync_grads: no communicator (v4l_trainer_comm_init)");
  hipStream_t s = (hipStream_t)stream;
  v4l_net* net = which ? tr->vf : tr->pf;
  float* g = which ? tr->g_vf : tr->g_pf;
  float* tail = g + net->total_params;
  float* st = tr->stats_cur;
  g_op = "allreduce";
  hipLaunchKernelGGL(bucket_tail_kernel, dim3(1), dim3(64), 0, s, st, tail, which, 1, 1.f / (float)tr->comm_world);
  V4L_LAUNCH_CHECK();
  {
    // (HIP events around the collective on its own stream when the built-in profiler is on: bench.py reports the measured time of
    // one all-reduce next to DESIGN.md section 6's cost model)
    v4l::ProfGuard pg(which ? "allreduce_vf" : "allreduce_pf", 0.0, s);
    V4L_RCCL_CHECK(g_rccl.AllReduce(g, g, (size_t)net->total_params + V4L_BUCKET_TAIL, /*ncclFloat32*/ 7, /*ncclSum*/ 0, tr->comm, s));
  }
  hipLaunchKernelGGL(bucket_tail_kernel, dim3(1), dim3(64), 0, s, st, tail, which, 0, 1.f);
  V4L_LAUNCH_CHECK();
  return 0;
}

// Self-test of the attached communicator through the very calls an update makes: both buckets get a rank-dependent integer
// pattern (bucket + the record fields the tail carries), v4l_sync_grads all-reduces them — eagerly, then (use_graph) as a
// captured hipGraph replayed twice, the way v4l_trainer_update_next runs it — and every element is compared on the device with
// the sum each rank can compute alone. *mismatches_out = elements that differ on THIS rank (0 = pass). Synchronises the stream.
// Overwrites the gradient buckets and the current statistics record: call it between updates (PPO.__init__ does).
int v4l_trainer_comm_selftest(v4l_trainer* tr, int use_graph, int64_t* mismatches_out, void* stream) {
  V4L_REQUIRE(tr && tr->bound && mismatches_out, "v4l_trainer_comm_selftest: bad argument");
  V4L_REQUIRE(tr->comm != nullptr, "v4l_trainer_comm_selftest: no communicator (v4l_trainer_comm_init)");
  hipStream_t s = (hipStream_t)stream;
  V4L_REQUIRE(!use_graph || s != nullptr, "v4l_trainer_comm_selftest: graph capture needs a non-default stream");
  int* bad = (int*)tr->norm_part;  // scratch between updates
  V4L_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), s));
  auto fill_and_reduce = [&](void) -> int {
    for (int which = 1; which >= 0; --which) {
      v4l_net* net = which ? tr->vf : tr->pf;
      float* g = which ? tr->g_vf : tr->g_pf;
      hipLaunchKernelGGL(comm_pattern_kernel, dim3(256), dim3(256), 0, s, g, net->total_params, tr->comm_rank, tr->stats_cur, which);
      V4L_LAUNCH_CHECK();
      int rc = v4l_sync_grads(tr, which, stream);
      if (rc) return rc;
    }
    return 0;
  };
  auto check = [&](void) -> int {
    for (int which = 1; which >= 0; --which) {
      v4l_net* net = which ? tr->vf : tr->pf;
      hipLaunchKernelGGL(comm_check_kernel, dim3(256), dim3(256), 0, s, which ? tr->g_vf : tr->g_pf, net->total_params,
                         tr->comm_world, tr->stats_cur, which, bad);
      V4L_LAUNCH_CHECK();
    }
    return 0;
  };
  int rc;
  if ((rc = fill_and_reduce()) || (rc = check())) return rc;
  hipGraphExec_t exec = nullptr;
  if (use_graph) {
    if ((rc = capture_graph(s, "comm selftest", fill_and_reduce, &exec))) return rc;
    hipError_t el = hipSuccess;
    for (int rep = 0; rep < 2 && !rc && el == hipSuccess; ++rep) {
      el = hipGraphLaunch(exec, s);
      if (el == hipSuccess) rc = check();
    }
    if (rc || el != hipSuccess) {
      (void)hipStreamSynchronize(s);
      (void)hipGraphExecDestroy(exec);
      if (rc) return rc;
      V4L_HIP_CHECK(el);
    }
  }
  int host_bad = 0;
  const hipError_t ec = hipMemcpyAsync(&host_bad, bad, sizeof(int), hipMemcpyDeviceToHost, s);
  const hipError_t es = hipStreamSynchronize(s);
  if (exec) (void)hipGraphExecDestroy(exec);  // only once nothing of it is in flight
  V4L_HIP_CHECK(ec);
  V4L_HIP_CHECK(es);
  V4L_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), s));
  *mismatches_out = host_bad;
  return 0;
}

static int run_update(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, void* stream) {
  int rc;
  const bool dp = tr->comm != nullptr;  // a 1-rank communicator runs the same sequence (how one GPU exercises it)
  if ((rc = v4l_trainer_critic_grads(tr, ro, n, hp, stream))) return rc;
  if (dp && (rc = v4l_sync_grads(tr, 1, stream))) return rc;  // critic gradients + advantage moments + vf_loss share
  if ((rc = v4l_trainer_critic_step(tr, hp, stream))) return rc;
  if ((rc = v4l_trainer_actor_grads(tr, ro, n, hp, stream))) return rc;
  if (dp && (rc = v4l_sync_grads(tr, 0, stream))) return rc;
  return v4l_trainer_actor_step(tr, hp, stream);
}

int v4l_trainer_update_next(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, int use_graph,
                            void* stream) {
  int rc = check_update_args(tr, ro, n, hp);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  drop_vmpo_graph(tr);  // (a PPO update on a V-MPO trainer runs the policy's pass over n rows: other descriptor tables)
  drop_a2c_graph(tr);
  drop_reinforce_graph(tr);
  if (!use_graph || g_prof || s == nullptr) return run_update(tr, ro, n, hp, stream);
  // the captured launch sequence is specific to (rollout pointers, n, hyper-parameters)
  GraphKey key;
  memset(&key, 0, sizeof(key));
  key.ro = *ro; memcpy(&key.hp, hp, sizeof(*hp)); key.n = n;  // (bytewise: v4l_ppo_hyper ends in padding)
  key.gen[0] = tr->pf->gen; key.gen[1] = tr->vf->gen; key.gen[2] = tr->tpf->gen;
  if (memcmp(&key, &tr->gkey, sizeof(key)) != 0) { drop_graph(tr); tr->gkey = key; }
  if (!tr->warm) {  // first update of a configuration runs eagerly: it uploads the descriptor tables
    tr->warm = true;
    return run_update(tr, ro, n, hp, stream);
  }
  if (tr->gexec == nullptr &&
      (rc = capture_graph(s, "update", [&]() { return run_update(tr, ro, n, hp, stream); }, &tr->gexec)))
    return rc;
  V4L_HIP_CHECK(hipGraphLaunch(tr->gexec, s));
  V4L_TRACE("update: launched");
  return 0;
}

int v4l_trainer_update_run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, int count, int use_graph,
                           void* stream) {
  int rc = check_update_args(tr, ro, n, hp);
  if (rc) return rc;
  V4L_REQUIRE(count >= 1, "v4l_trainer_update_run: count must be >= 1");
  hipStream_t s = (hipStream_t)stream;
  GraphKey key;
  memset(&key, 0, sizeof(key));
  key.ro = *ro; memcpy(&key.hp, hp, sizeof(*hp)); key.n = n;  // (bytewise: v4l_ppo_hyper ends in padding)
  key.gen[0] = tr->pf->gen; key.gen[1] = tr->vf->gen; key.gen[2] = tr->tpf->gen;
  const bool same = memcmp(&key, &tr->gkey, sizeof(key)) == 0;
  if (!use_graph || g_prof || s == nullptr || !same || !tr->warm) {
    // no graph, or a configuration this trainer has not run yet: update by update (the first one eagerly — it uploads the
    // descriptor tables —, then single-update replays); the next call captures the whole run
    for (int u = 0; u < count; ++u)
      if ((rc = v4l_trainer_update_next(tr, ro, n, hp, use_graph, stream))) return rc;
    return 0;
  }
  if (tr->gexec_run != nullptr && tr->gexec_run_count != count) {
    (void)hipGraphExecDestroy(tr->gexec_run);
    tr->gexec_run = nullptr;
  }
  if (tr->gexec_run == nullptr) {
    V4L_TRACE("update run: %d updates", count);
    auto run = [&]() {
      int rb = 0;
      for (int u = 0; u < count && !rb; ++u) rb = run_update(tr, ro, n, hp, stream);
      return rb;
    };
    if ((rc = capture_graph(s, "update run", run, &tr->gexec_run))) return rc;
    tr->gexec_run_count = count;
  }
  V4L_HIP_CHECK(hipGraphLaunch(tr->gexec_run, s));
  return 0;
}

// ---- V-MPO updates: v4l_trainer_update_next / _update_run's rules with the V-MPO actor stage, graphs and key of their own
static int run_vmpo_update(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* vstats_all_dev,
                           void* stream) {
  int rc;  // v_mpo.py:181-182: update_critic, then update_actor
  if ((rc = v4l_trainer_critic_grads(tr, ro, n, hp, stream))) return rc;
  if ((rc = v4l_trainer_critic_step(tr, hp, stream))) return rc;
  if ((rc = vmpo_actor_stage(tr, ro, n, hp, vstats_all_dev, stream))) return rc;
  return v4l_trainer_actor_step(tr, hp, stream);
}
static void vmpo_graph_key(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, const float* vstats_all_dev,
                           VmpoGraphKey* key) {
  memset(key, 0, sizeof(*key));
  key->base.ro = *ro; memcpy(&key->base.hp, hp, sizeof(*hp)); key->base.n = n;  // (bytewise: v4l_ppo_hyper ends in padding)
  key->base.gen[0] = tr->pf->gen; key->base.gen[1] = tr->vf->gen; key->base.gen[2] = tr->tpf->gen;
  key->block = tr->vmpo; key->vstats_all = vstats_all_dev;
  memcpy(&key->vhp, &tr->vmpo_hp, sizeof(tr->vmpo_hp));
}
// Captures `count` V-MPO updates on s into *exec
static int capture_vmpo(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* vstats_all_dev, int count,
                        hipStream_t s, hipGraphExec_t* exec) {
  hipGraph_t graph = nullptr;
  int rc = 0;
  V4L_TRACE("vmpo update: begin capture of %d update(s)", count);
  V4L_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  for (int u = 0; u < count && !rc; ++u) rc = run_vmpo_update(tr, ro, n, hp, vstats_all_dev, (void*)s);
  const hipError_t e = hipStreamEndCapture(s, &graph);
  if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
  V4L_HIP_CHECK(e);
  V4L_HIP_CHECK(hipGraphInstantiate(exec, graph, nullptr, nullptr, 0));
  V4L_HIP_CHECK(hipGraphDestroy(graph));
  ++tr->vmpo_captures;
  V4L_TRACE("vmpo update: instantiated");
  return 0;
}
int v4l_trainer_vmpo_update_next(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* vstats_all_dev,
                                 int use_graph, void* stream) {
  int rc = check_vmpo_args(tr, ro, n, hp);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  V4L_REQUIRE(!capturing(s), "v4l_trainer_vmpo_update_next: called under a caller's stream capture (use_graph = 1 captures itself)");
  drop_ppo_graph(tr);  // (the policy's pass runs over ceil(n / 2) rows here: other descriptor tables than a PPO update's)
  drop_a2c_graph(tr);
  drop_reinforce_graph(tr);
  if (!use_graph || g_prof || s == nullptr) return run_vmpo_update(tr, ro, n, hp, vstats_all_dev, stream);
  VmpoGraphKey key;
  vmpo_graph_key(tr, ro, n, hp, vstats_all_dev, &key);
  if (memcmp(&key, &tr->vkey, sizeof(key)) != 0) { drop_vmpo_graph(tr); tr->vkey = key; }
  if (!tr->vwarm) {  // first update of a configuration runs eagerly: it uploads the descriptor tables (the m-row passes' too)
    tr->vwarm = true;
    return run_vmpo_update(tr, ro, n, hp, vstats_all_dev, stream);
  }
  if (tr->vexec == nullptr && (rc = capture_vmpo(tr, ro, n, hp, vstats_all_dev, 1, s, &tr->vexec))) return rc;
  V4L_HIP_CHECK(hipGraphLaunch(tr->vexec, s));
  ++tr->vmpo_replays;
  return 0;
}
int v4l_trainer_vmpo_update_run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* vstats_all_dev,
                                int count, int use_graph, void* stream) {
  int rc = check_vmpo_args(tr, ro, n, hp);
  if (rc) return rc;
  V4L_REQUIRE(count >= 1, "v4l_trainer_vmpo_update_run: count must be >= 1");
  hipStream_t s = (hipStream_t)stream;
  V4L_REQUIRE(!capturing(s), "v4l_trainer_vmpo_update_run: called under a caller's stream capture (use_graph = 1 captures itself)");
  VmpoGraphKey key;
  vmpo_graph_key(tr, ro, n, hp, vstats_all_dev, &key);
  const bool same = memcmp(&key, &tr->vkey, sizeof(key)) == 0;
  if (!use_graph || g_prof || s == nullptr || !same || !tr->vwarm) {
    // no graph, or a configuration this trainer has not run yet: update by update (the first one eagerly, then single-update
    // replays); the next call captures the whole run
    for (int u = 0; u < count; ++u)
      if ((rc = v4l_trainer_vmpo_update_next(tr, ro, n, hp, vstats_all_dev, use_graph, stream))) return rc;
    return 0;
  }
  if (tr->vexec_run != nullptr && tr->vexec_run_count != count) {
    (void)hipGraphExecDestroy(tr->vexec_run);
    tr->vexec_run = nullptr;
  }
  if (tr->vexec_run == nullptr) {
    if ((rc = capture_vmpo(tr, ro, n, hp, vstats_all_dev, count, s, &tr->vexec_run))) return rc;
    tr->vexec_run_count = count;
  }
  V4L_HIP_CHECK(hipGraphLaunch(tr->vexec_run, s));
  ++tr->vmpo_replays;
  return 0;
}
int v4l_trainer_vmpo_graph_counts(const v4l_trainer* tr, int64_t* captures, int64_t* replays) {
  V4L_REQUIRE(tr && captures && replays, "v4l_trainer_vmpo_graph_counts: null argument");
  *captures = tr->vmpo_captures;
  *replays = tr->vmpo_replays;
  return 0;
}

// ---- A2C (torchrl/algo/on_policy/a2c.py:46-107) on state-MLP nets: the PPO update's opening launch, forwards, backwards and
// clip + Adam launches around two loss launches of its own
static int check_a2c_args(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, const float* astats_all_dev) {
  int rc = check_update_args(tr, ro, n, hp);
  if (rc) return rc;
  V4L_REQUIRE(astats_all_dev != nullptr, "v4l_trainer_a2c: the A2C record array is missing");
  V4L_REQUIRE(!tr->pf->sd(), "v4l_trainer_a2c: a V4L_LOGSTD_HEAD policy (GaussianContPolicy) runs under the PPO update only: the A2C loss "
              "kernel takes one log sigma per action column");
  V4L_REQUIRE(tr->pf->cfg.kind == V4L_NET_MLP && tr->vf->cfg.kind == V4L_NET_MLP,
              "v4l_trainer_a2c: A2C runs state-MLP nets (V4L_NET_MLP) only: the reference's A2C raises on a shared encoder");
  V4L_REQUIRE(hp->world_size == 1 && tr->comm == nullptr, "v4l_trainer_a2c: A2C runs in a single process");
  V4L_REQUIRE(tr->skip_all == nullptr, "v4l_trainer_a2c: no skipping of non-finite steps (v4l_trainer_begin_guarded) in an A2C run");
  V4L_REQUIRE(tr->kl_all == nullptr, "v4l_trainer_a2c: no KL early stop (v4l_trainer_kl_stop) in an A2C run");
  V4L_REQUIRE(tr->ad_all == nullptr, "v4l_trainer_a2c: no KL-adaptive learning rates (v4l_trainer_kl_adapt) in an A2C run");
  return 0;
}
// a2c.py:76-77, 84-85 (values = vf(obs), vf_loss, vf_loss.backward()): v4l_trainer_critic_grads' launches for a state-MLP net with
// the A2C critic loss in critic_loss_kernel's place
static int a2c_critic_stage(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* astats_all_dev, void* stream) {
  int rc;
  hipStream_t s = (hipStream_t)stream;
  v4l_net* vf = tr->vf;
  float* st = tr->stats_cur;
  const int* rowidx = tr->rowidx_cur;
  if ((rc = launch_begin_pack(tr, vf, ro, n, s))) return rc;
  { PhaseScope ps("vf.fwd");
  if ((rc = v4l_net_forward(vf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, 1, stream))) return rc; }
  const Layout L = vf->layout(n);
  g_op = "loss";
  V4L_KLAUNCH("a2c_critic_loss", 0, s, a2c_critic_loss_kernel, dim3(1), loss_block(n), 0, s, tr->ws + L.out, ro->rets_dev, rowidx, n, 1.f / (float)n,
              tr->ws + L.dout, st, v4l_net_grad_scale(vf, n), (const UpdCtl*)tr->ctl, astats_all_dev);
  V4L_LAUNCH_CHECK();
  PhaseScope ps("vf.bwd");
  return v4l_net_backward(vf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, tr->g_vf, stream);
}
// a2c.py:61-74, 79-80 (pf.update(obs, acts), policy_loss, policy_loss.backward())
static int a2c_actor_stage(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* astats_all_dev, void* stream) {
  int rc;
  hipStream_t s = (hipStream_t)stream;
  v4l_net* pf = tr->pf;
  const int* rowidx = tr->rowidx_cur;
  if ((rc = v4l_net_pack(pf, stream))) return rc;  // the previous update's policy step moved the weights
  { PhaseScope ps("pf.fwd");
  if ((rc = v4l_net_forward(pf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, 1, stream))) return rc; }
  g_op = "loss";
  ActorArgs aa = actor_args(tr, ro, n, rowidx);
  aa.ent_coef = hp->entropy_coeff;
  if (pf->cat()) {
    if ((rc = launch_cat_loss("a2c_loss", a2c_cat_loss_kernel, s, aa, tr->ctl, astats_all_dev))) return rc;
  } else if ((rc = launch_rec_loss("a2c_loss", V4L_LOSS_FAMILY(a2c_loss_kernel), s, aa, tr->ctl, astats_all_dev))) return rc;
  PhaseScope ps("pf.bwd");
  return v4l_net_backward(pf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, tr->g_pf, stream);
}
int v4l_trainer_a2c_critic_grads(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* astats_all_dev,
                                 void* stream) {
  int rc = check_a2c_args(tr, ro, n, hp, astats_all_dev);
  if (rc) return rc;
  V4L_REQUIRE(!capturing((hipStream_t)stream), "v4l_trainer_a2c_critic_grads: called under a caller's stream capture");
  return a2c_critic_stage(tr, ro, n, hp, astats_all_dev, stream);
}
int v4l_trainer_a2c_actor_grads(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* astats_all_dev,
                                void* stream) {
  int rc = check_a2c_args(tr, ro, n, hp, astats_all_dev);
  if (rc) return rc;
  V4L_REQUIRE(!capturing((hipStream_t)stream), "v4l_trainer_a2c_actor_grads: called under a caller's stream capture");
  return a2c_actor_stage(tr, ro, n, hp, astats_all_dev, stream);
}
static int run_a2c_update(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* astats_all_dev, void* stream) {
  int rc;  // (critic first, as the PPO update: with disjoint parameter sets the two steps of a2c.py:79-87 are independent)
  if ((rc = a2c_critic_stage(tr, ro, n, hp, astats_all_dev, stream))) return rc;
  if ((rc = v4l_trainer_critic_step(tr, hp, stream))) return rc;
  if ((rc = a2c_actor_stage(tr, ro, n, hp, astats_all_dev, stream))) return rc;
  return v4l_trainer_actor_step(tr, hp, stream);
}
// ---- the graphed driver of the learners whose captured update is keyed on GraphKey + one record array (A2C, REINFORCE). A
// learner L names its entry points, checks the arguments (L::check), launches one update (L::run), owns its graph state in the
// trainer (L::state) and drops the graphs of the other kinds (L::drop_others); the rules are v4l_trainer_update_next's.
extern "C++" {  // (templates: this file's C ABI block is open here)
struct RecGraphState {
  A2cGraphKey* key; hipGraphExec_t* exec; hipGraphExec_t* exec_run; int* run_count; bool* warm; int64_t* captures; int64_t* replays;
};
static void rec_graph_key(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, const float* rec_all_dev,
                          A2cGraphKey* key) {
  memset(key, 0, sizeof(*key));
  key->base.ro = *ro; memcpy(&key->base.hp, hp, sizeof(*hp)); key->base.n = n;  // (bytewise: v4l_ppo_hyper ends in padding)
  key->base.gen[0] = tr->pf->gen; key->base.gen[1] = tr->vf->gen; key->base.gen[2] = tr->tpf->gen;
  key->astats_all = rec_all_dev;
}
// Captures `count` updates of learner L on s into *exec
template <class L>
static int rec_capture(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* rec_all_dev, int count,
                       hipStream_t s, hipGraphExec_t* exec) {
  V4L_TRACE("%s: %d update(s)", L::what, count);
  auto run = [&]() {
    int rb = 0;
    for (int u = 0; u < count && !rb; ++u) rb = L::run(tr, ro, n, hp, rec_all_dev, (void*)s);
    return rb;
  };
  if (int rc = capture_graph(s, L::what, run, exec)) return rc;
  ++*L::state(tr).captures;
  return 0;
}
template <class L>
static int rec_update_next(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* rec_all_dev, int use_graph,
                           void* stream) {
  int rc = L::check(tr, ro, n, hp, rec_all_dev);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  V4L_REQUIRE(!capturing(s), "%s: called under a caller's stream capture (use_graph = 1 captures itself)", L::next_name);
  L::drop_others(tr);
  if (!use_graph || g_prof || s == nullptr) return L::run(tr, ro, n, hp, rec_all_dev, stream);
  const RecGraphState g = L::state(tr);
  A2cGraphKey key;
  rec_graph_key(tr, ro, n, hp, rec_all_dev, &key);
  if (memcmp(&key, g.key, sizeof(key)) != 0) { L::drop(tr); *g.key = key; }
  if (!*g.warm) {  // first update of a configuration runs eagerly: it uploads the descriptor tables
    *g.warm = true;
    return L::run(tr, ro, n, hp, rec_all_dev, stream);
  }
  if (*g.exec == nullptr && (rc = rec_capture<L>(tr, ro, n, hp, rec_all_dev, 1, s, g.exec))) return rc;
  V4L_HIP_CHECK(hipGraphLaunch(*g.exec, s));
  ++*g.replays;
  return 0;
}
template <class L>
static int rec_update_run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* rec_all_dev, int count,
                          int use_graph, void* stream) {
  int rc = L::check(tr, ro, n, hp, rec_all_dev);
  if (rc) return rc;
  V4L_REQUIRE(count >= 1, "%s: count must be >= 1", L::run_name);
  hipStream_t s = (hipStream_t)stream;
  V4L_REQUIRE(!capturing(s), "%s: called under a caller's stream capture (use_graph = 1 captures itself)", L::run_name);
  const RecGraphState g = L::state(tr);
  A2cGraphKey key;
  rec_graph_key(tr, ro, n, hp, rec_all_dev, &key);
  const bool same = memcmp(&key, g.key, sizeof(key)) == 0;
  if (!use_graph || g_prof || s == nullptr || !same || !*g.warm) {
    // no graph, or a configuration this trainer has not run yet: update by update (the first one eagerly, then single-update
    // replays); the next call captures the whole run
    for (int u = 0; u < count; ++u)
      if ((rc = rec_update_next<L>(tr, ro, n, hp, rec_all_dev, use_graph, stream))) return rc;
    return 0;
  }
  if (*g.exec_run != nullptr && *g.run_count != count) {
    (void)hipGraphExecDestroy(*g.exec_run);
    *g.exec_run = nullptr;
  }
  if (*g.exec_run == nullptr) {
    if ((rc = rec_capture<L>(tr, ro, n, hp, rec_all_dev, count, s, g.exec_run))) return rc;
    *g.run_count = count;
  }
  V4L_HIP_CHECK(hipGraphLaunch(*g.exec_run, s));
  ++*g.replays;
  return 0;
}
}  // extern "C++"
struct A2cLearner {
  static constexpr const char* what = "a2c update";
  static constexpr const char* next_name = "v4l_trainer_a2c_update_next";
  static constexpr const char* run_name = "v4l_trainer_a2c_update_run";
  static int check(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, const float* rec) {
    return check_a2c_args(tr, ro, n, hp, rec);
  }
  static int run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* rec, void* stream) {
    return run_a2c_update(tr, ro, n, hp, rec, stream);
  }
  static RecGraphState state(v4l_trainer* tr) {
    return {&tr->akey, &tr->aexec, &tr->aexec_run, &tr->aexec_run_count, &tr->awarm, &tr->a2c_captures, &tr->a2c_replays};
  }
  static void drop(v4l_trainer* tr) { drop_a2c_graph(tr); }
  static void drop_others(v4l_trainer* tr) { drop_ppo_graph(tr); drop_vmpo_graph(tr); drop_reinforce_graph(tr); }
};
int v4l_trainer_a2c_update_next(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* astats_all_dev,
                                int use_graph, void* stream) {
  return rec_update_next<A2cLearner>(tr, ro, n, hp, astats_all_dev, use_graph, stream);
}
int v4l_trainer_a2c_update_run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* astats_all_dev,
                               int count, int use_graph, void* stream) {
  return rec_update_run<A2cLearner>(tr, ro, n, hp, astats_all_dev, count, use_graph, stream);
}
int v4l_trainer_a2c_graph_counts(const v4l_trainer* tr, int64_t* captures, int64_t* replays) {
  V4L_REQUIRE(tr && captures && replays, "v4l_trainer_a2c_graph_counts: null argument");
  *captures = tr->a2c_captures;
  *replays = tr->a2c_replays;
  return 0;
}

// ---- REINFORCE (torchrl/algo/on_policy/reinforce.py:34-76) on every net kind: the opening launch on the POLICY's packs, its
// forward, one loss launch of its own, its backward, clip + Adam. No critic launch of any kind.
static int check_reinforce_args(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, const float* rstats_all_dev) {
  int rc = check_update_args(tr, ro, n, hp);
  if (rc) return rc;
  V4L_REQUIRE(rstats_all_dev != nullptr, "v4l_trainer_reinforce: the REINFORCE record array is missing");
  V4L_REQUIRE(!tr->pf->sd(), "v4l_trainer_reinforce: a V4L_LOGSTD_HEAD policy (GaussianContPolicy) runs under the PPO update only: the "
              "REINFORCE loss kernel takes one log sigma per action column");
  V4L_REQUIRE(hp->world_size == 1 && tr->comm == nullptr, "v4l_trainer_reinforce: REINFORCE runs in a single process");
  V4L_REQUIRE(tr->skip_all == nullptr,
              "v4l_trainer_reinforce: no skipping of non-finite steps (v4l_trainer_begin_guarded) in a REINFORCE run");
  V4L_REQUIRE(tr->kl_all == nullptr, "v4l_trainer_reinforce: no KL early stop (v4l_trainer_kl_stop) in a REINFORCE run");
  V4L_REQUIRE(tr->ad_all == nullptr,
              "v4l_trainer_reinforce: no KL-adaptive learning rates (v4l_trainer_kl_adapt) in a REINFORCE run");
  return 0;
}
// reinforce.py:52-63 (pf.update(obs, acts), policy_loss, policy_loss.backward())
static int reinforce_actor_stage(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* rstats_all_dev,
                                 void* stream) {
  int rc;
  hipStream_t s = (hipStream_t)stream;
  v4l_net* pf = tr->pf;
  const int* rowidx = tr->rowidx_cur;
  // the opening launch with the policy's packs in the critic's place: the weight copies the previous policy step outdated
  if ((rc = launch_begin_pack(tr, pf, ro, n, s))) return rc;
  { PhaseScope ps("pf.fwd");
  if ((rc = v4l_net_forward(pf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, 1, stream))) return rc; }
  g_op = "loss";
  ActorArgs aa = actor_args(tr, ro, n, rowidx);
  aa.ent_coef = hp->entropy_coeff;
  if (pf->cat()) {
    if ((rc = launch_cat_loss("reinforce_loss", reinforce_cat_loss_kernel, s, aa, tr->ctl, rstats_all_dev))) return rc;
  } else if ((rc = launch_rec_loss("reinforce_loss", V4L_LOSS_FAMILY(reinforce_loss_kernel), s, aa, tr->ctl, rstats_all_dev))) return rc;
  PhaseScope ps("pf.bwd");
  return v4l_net_backward(pf, ro->state_dev, ro->image_dev, rowidx, n, tr->ws, tr->g_pf, stream);
}
int v4l_trainer_reinforce_actor_grads(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* rstats_all_dev,
                                      void* stream) {
  int rc = check_reinforce_args(tr, ro, n, hp, rstats_all_dev);
  if (rc) return rc;
  V4L_REQUIRE(!capturing((hipStream_t)stream), "v4l_trainer_reinforce_actor_grads: called under a caller's stream capture");
  return reinforce_actor_stage(tr, ro, n, hp, rstats_all_dev, stream);
}
static int run_reinforce_update(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* rstats_all_dev,
                                void* stream) {
  if (int rc = reinforce_actor_stage(tr, ro, n, hp, rstats_all_dev, stream)) return rc;
  return v4l_trainer_actor_step(tr, hp, stream);
}
struct ReinforceLearner {
  static constexpr const char* what = "reinforce update";
  static constexpr const char* next_name = "v4l_trainer_reinforce_update_next";
  static constexpr const char* run_name = "v4l_trainer_reinforce_update_run";
  static int check(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, const float* rec) {
    return check_reinforce_args(tr, ro, n, hp, rec);
  }
  static int run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* rec, void* stream) {
    return run_reinforce_update(tr, ro, n, hp, rec, stream);
  }
  static RecGraphState state(v4l_trainer* tr) {
    return {&tr->rkey, &tr->rexec, &tr->rexec_run, &tr->rexec_run_count, &tr->rwarm, &tr->reinforce_captures, &tr->reinforce_replays};
  }
  static void drop(v4l_trainer* tr) { drop_reinforce_graph(tr); }
  static void drop_others(v4l_trainer* tr) { drop_ppo_graph(tr); drop_vmpo_graph(tr); drop_a2c_graph(tr); }
};
int v4l_trainer_reinforce_update_next(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* rstats_all_dev,
                                      int use_graph, void* stream) {
  return rec_update_next<ReinforceLearner>(tr, ro, n, hp, rstats_all_dev, use_graph, stream);
}
int v4l_trainer_reinforce_update_run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float* rstats_all_dev,
                                     int count, int use_graph, void* stream) {
  return rec_update_run<ReinforceLearner>(tr, ro, n, hp, rstats_all_dev, count, use_graph, stream);
}
int v4l_trainer_reinforce_graph_counts(const v4l_trainer* tr, int64_t* captures, int64_t* replays) {
  V4L_REQUIRE(tr && captures && replays, "v4l_trainer_reinforce_graph_counts: null argument");
  *captures = tr->reinforce_captures;
  *replays = tr->reinforce_replays;
  return 0;
}

// ---- the opt-in KL early stop of a run of PPO updates (PPO(target_kl=...)). An armed update is PPO's update with
// one more launch (kl_stop_kernel behind the policy's backward) and the clip_adam_kernel<WD, true> instantiation, which honours
// the latch. It runs through entry points, a graph key and graph handles of its own, on the graphed driver of the learners with
// one record array (the KL array takes the record array's place): v4l_trainer_update_next / _update_run, the stages they call
// and their graphs are not touched.
int v4l_trainer_kl_stop(v4l_trainer* tr, double target_kl, float* kl_all_dev, void* stream) {
  V4L_REQUIRE(tr && tr->bound, "v4l_trainer_kl_stop: the trainer is not bound");
  if (kl_all_dev == nullptr) {  // disarm
    tr->kl_all = nullptr; tr->kl_thresh = 0.0;
    return 0;
  }
  V4L_REQUIRE(target_kl > 0.0 && target_kl <= 3.0e38, "v4l_trainer_kl_stop: target_kl must be a positive finite number (got %g)", target_kl);
  V4L_REQUIRE(tr->comm == nullptr, "v4l_trainer_kl_stop: the KL early stop runs in a single process (each rank would decide on its own shard)");
  V4L_REQUIRE(!tr->pf->cat(), "v4l_trainer_kl_stop: the KL early stop belongs to the PPO update, which takes Gaussian policies");
  V4L_REQUIRE(tr->ad_all == nullptr, "v4l_trainer_kl_stop: the trainer is armed with the KL-adaptive learning rates (v4l_trainer_kl_adapt): "
              "one run takes one of the two");
  if (tr->kl_thresh != 1.5 * target_kl) drop_kl_graph(tr);  // (baked into the captured kl_stop launches; the array is in the key)
  tr->kl_all = kl_all_dev;
  tr->kl_thresh = 1.5 * target_kl;  // the factor of Spinning Up and Stable-Baselines3
  hipLaunchKernelGGL(kl_arm_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, tr->ctl);  // the run opens with a cleared latch
  V4L_LAUNCH_CHECK();
  return 0;
}
static int check_kl_args(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, const float* kl_all_dev) {
  int rc = check_update_args(tr, ro, n, hp);
  if (rc) return rc;
  V4L_REQUIRE(kl_all_dev != nullptr && kl_all_dev == tr->kl_all, "v4l_trainer_kl_update: arm the run first (v4l_trainer_kl_stop, after v4l_trainer_begin)");
  V4L_REQUIRE(!tr->pf->cat(), "v4l_trainer_kl_update: the PPO loss kernels are Gaussian");
  V4L_REQUIRE(hp->world_size == 1 && tr->comm == nullptr, "v4l_trainer_kl_update: the KL early stop runs in a single process");
  return 0;
}
// adam_step's launch for an armed run: the same arguments, the instantiation that reads the latch (the norm partials as adam_step
// takes them from the backward's reduce launch, or summed again)
static int adam_step_kl(v4l_trainer* tr, v4l_net* net, float* g, float* m, float* v, const v4l_ppo_hyper* hp, int which,
                        float* norm_out, hipStream_t s, bool close_update) {
  int gb = (int)std::min<int64_t>(GRAD_NORM_PARTS, cdiv64(net->total_params, 1024));
  const float* part = tr->norm_part + which * GRAD_NORM_PARTS;
  const float* extra = nullptr;
  int nextra = 0;
  if (int rc = check_hyper(hp)) return rc;
  g_op = "optim";
  if (net->red_blocks > 0 && net->red_blocks <= ADAM_MAX_PARTS && net->red_grads == g) {
    part = net->d_sq;
    gb = net->red_blocks;
    net->red_blocks = 0;  // consumed
    if (net->logstd >= 0) { extra = g + net->params[net->logstd].goff; nextra = (int)net->params[net->logstd].numel; }
    V4L_REQUIRE(nextra <= 64, "internal: log sigma wider than a wave");
  } else {
    V4L_KLAUNCH("grad_sumsq", 0, s, grad_sumsq_kernel, dim3(gb), dim3(256), 0, s, g, net->total_params, tr->norm_part + which * GRAD_NORM_PARTS);
    V4L_LAUNCH_CHECK();
  }
  const unsigned nf_exempt = tr->pf->cfg.out_dim == 1 ? 1u << ST_LS_STD : 0u;
#define V4L_CLIP_ADAM_KL(WD_)                                                                                                       \
  V4L_KLAUNCH("clip_adam", 0, s, (clip_adam_kernel<WD_, true>), dim3((unsigned)net->seg_blocks), dim3(256), 0, s, net->d_segs,      \
              (int)net->params.size(), g, m, v, part, gb, extra, nextra, hp->max_grad_norm, hp->eps, tr->ctl, which, norm_out,      \
              close_update ? tr->ctl : (UpdCtl*)nullptr, (const float*)tr->stats_cur, tr->stats_all, tr->skip_all, nf_exempt)
  if (!(hp->weight_decay > 0.0)) V4L_CLIP_ADAM_KL(WD_NONE);
  else if (hp->decoupled_weight_decay) V4L_CLIP_ADAM_KL(WD_DECOUPLED);
  else V4L_CLIP_ADAM_KL(WD_COUPLED);
#undef V4L_CLIP_ADAM_KL
  V4L_LAUNCH_CHECK();
  return 0;
}
// kl_stop_kernel behind the policy's backward, on the trainer's stream: by then every loss route has completed the record (the
// fused route's fb_loss_finish_kernel runs inside the weight-grad fork, which is joined before the backward returns), and the
// target's head rows and the stored actions are where the loss launch read them.
static int launch_kl_stop(v4l_trainer* tr, const v4l_rollout* ro, int n, hipStream_t s) {
  v4l_net *pf = tr->pf, *tp = tr->tpf;
  const bool stored = ro->logp_old_dev != nullptr, sd = pf->sd();
  float* ws_t = tr->ws + std::max(pf->layout(n).total, tr->vf->layout(n).total);
  KlArgs q;
  memset(&q, 0, sizeof(q));
  q.tmean = stored ? nullptr : ws_t + tp->layout(n).out;
  q.tlogstd = stored || sd ? nullptr : tp->p[tp->logstd];
  q.logp_old = ro->logp_old_dev; q.acts = ro->acts_dev; q.rowidx = tr->rowidx_cur;
  q.n = n; q.A = pf->act_dim(); q.sd = sd ? 1 : 0;
  q.st = tr->stats_cur; q.upd_index = &tr->ctl->upd_index; q.latch = &tr->ctl->kl_stop;
  q.kl_all = tr->kl_all; q.thresh = tr->kl_thresh;
  g_op = "kl_stop";
  if (pf->cfg.tanh_action) V4L_KLAUNCH("kl_stop", 0, s, kl_stop_kernel<true>, dim3(1), loss_block(n), 0, s, q);
  else V4L_KLAUNCH("kl_stop", 0, s, kl_stop_kernel<false>, dim3(1), loss_block(n), 0, s, q);
  V4L_LAUNCH_CHECK();
  return 0;
}
static int run_kl_update(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, void* stream) {
  int rc;
  hipStream_t s = (hipStream_t)stream;
  float* st = tr->stats_cur;
  if ((rc = v4l_trainer_critic_grads(tr, ro, n, hp, stream))) return rc;
  if ((rc = adam_step_kl(tr, tr->vf, tr->g_vf, tr->m_vf, tr->v_vf, hp, 1, st + ST_GN_VF, s, false))) return rc;
  if ((rc = v4l_trainer_actor_grads(tr, ro, n, hp, stream))) return rc;
  if ((rc = launch_kl_stop(tr, ro, n, s))) return rc;
  return adam_step_kl(tr, tr->pf, tr->g_pf, tr->m_pf, tr->v_pf, hp, 0, st + ST_GN_PF, s, true);
}
struct KlLearner {
  static constexpr const char* what = "kl-stop update";
  static constexpr const char* next_name = "v4l_trainer_kl_update_next";
  static constexpr const char* run_name = "v4l_trainer_kl_update_run";
  static int check(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, const float* rec) {
    return check_kl_args(tr, ro, n, hp, rec);
  }
  static int run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float*, void* stream) {
    return run_kl_update(tr, ro, n, hp, stream);
  }
  static RecGraphState state(v4l_trainer* tr) {
    return {&tr->kkey, &tr->kexec, &tr->kexec_run, &tr->kexec_run_count, &tr->kwarm, &tr->kl_captures, &tr->kl_replays};
  }
  static void drop(v4l_trainer* tr) { drop_kl_graph(tr); }
  // (V-MPO's, A2C's and REINFORCE's graphs bake other descriptor tables in; PPO's bake the same ones and stay)
  static void drop_others(v4l_trainer* tr) { drop_vmpo_graph(tr); drop_a2c_graph(tr); drop_reinforce_graph(tr); }
};
int v4l_trainer_kl_update_next(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, int use_graph, void* stream) {
  V4L_REQUIRE(tr != nullptr, "v4l_trainer_kl_update_next: null argument");
  return rec_update_next<KlLearner>(tr, ro, n, hp, tr->kl_all, use_graph, stream);
}
int v4l_trainer_kl_update_run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, int count, int use_graph,
                              void* stream) {
  V4L_REQUIRE(tr != nullptr, "v4l_trainer_kl_update_run: null argument");
  return rec_update_run<KlLearner>(tr, ro, n, hp, tr->kl_all, count, use_graph, stream);
}
int v4l_trainer_kl_graph_counts(const v4l_trainer* tr, int64_t* captures, int64_t* replays) {
  V4L_REQUIRE(tr && captures && replays, "v4l_trainer_kl_graph_counts: null argument");
  *captures = tr->kl_captures;
  *replays = tr->kl_replays;
  return 0;
}

// ---- the opt-in KL-adaptive learning rates of a run of PPO updates (PPO(desired_kl=...)). An armed update is
// PPO's update with one more launch (kl_adapt_kernel behind the policy's backward, where an early-stop run has kl_stop_kernel);
// both clip + Adam launches are the plain ones (no step is ever skipped by this option). Entry points, graph key and graph
// handles of its own on the record-array driver, like the early stop's: v4l_trainer_update_next / _update_run, the
// v4l_trainer_kl_update_* calls, the stages they call and their graphs are not touched.
int v4l_trainer_kl_adapt(v4l_trainer* tr, double desired_kl, double factor, double lr_min, double lr_max, float* rec_all_dev,
                         void* stream) {
  (void)stream;  // (nothing to clear on the device: the rates of the run are those v4l_trainer_begin wrote)
  V4L_REQUIRE(tr && tr->bound, "v4l_trainer_kl_adapt: the trainer is not bound");
  if (rec_all_dev == nullptr) {  // disarm
    tr->ad_all = nullptr;
    return 0;
  }
  const double big = 1.0e300;
  V4L_REQUIRE(desired_kl > 0.0 && desired_kl <= big, "v4l_trainer_kl_adapt: desired_kl must be a positive finite number (got %g)", desired_kl);
  V4L_REQUIRE(factor > 1.0 && factor <= big, "v4l_trainer_kl_adapt: factor must be a finite number > 1 (got %g)", factor);
  V4L_REQUIRE(lr_min > 0.0 && lr_min <= big && lr_max > 0.0 && lr_max <= big && lr_min <= lr_max,
              "v4l_trainer_kl_adapt: lr_min and lr_max must be positive finite numbers with lr_min <= lr_max (got %g, %g)", lr_min, lr_max);
  V4L_REQUIRE(tr->comm == nullptr, "v4l_trainer_kl_adapt: the adaptive rates run in a single process (each rank would decide on its own shard)");
  V4L_REQUIRE(!tr->pf->cat(), "v4l_trainer_kl_adapt: the adaptive rates belong to the PPO update, which takes Gaussian policies");
  V4L_REQUIRE(tr->kl_all == nullptr, "v4l_trainer_kl_adapt: the trainer is armed with the KL early stop (v4l_trainer_kl_stop): one run "
              "takes one of the two");
  const double num[4] = {desired_kl, factor, lr_min, lr_max};
  if (memcmp(num, tr->ad_num, sizeof(num)) != 0) drop_kl_adapt_graph(tr);  // (baked into the captured kl_adapt launches; the array is in the key)
  memcpy(tr->ad_num, num, sizeof(num));
  tr->ad_all = rec_all_dev;
  return 0;
}
static int check_kl_adapt_args(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, const float* rec_all_dev) {
  int rc = check_update_args(tr, ro, n, hp);
  if (rc) return rc;
  V4L_REQUIRE(rec_all_dev != nullptr && rec_all_dev == tr->ad_all, "v4l_trainer_kl_adapt_update: arm the run first (v4l_trainer_kl_adapt, after v4l_trainer_begin)");
  V4L_REQUIRE(tr->kl_all == nullptr, "v4l_trainer_kl_adapt_update: the trainer is armed with the KL early stop as well (v4l_trainer_kl_stop)");
  V4L_REQUIRE(!tr->pf->cat(), "v4l_trainer_kl_adapt_update: the PPO loss kernels are Gaussian");
  V4L_REQUIRE(hp->world_size == 1 && tr->comm == nullptr, "v4l_trainer_kl_adapt_update: the adaptive rates run in a single process");
  return 0;
}
// kl_adapt_kernel behind the policy's backward, on the trainer's stream (launch_kl_stop's place and operands: the record is
// complete, the target's head rows and the stored actions are where the loss launch read them)
static int launch_kl_adapt(v4l_trainer* tr, const v4l_rollout* ro, int n, hipStream_t s) {
  v4l_net *pf = tr->pf, *tp = tr->tpf;
  const bool stored = ro->logp_old_dev != nullptr, sd = pf->sd();
  float* ws_t = tr->ws + std::max(pf->layout(n).total, tr->vf->layout(n).total);
  KlAdaptArgs q;
  memset(&q, 0, sizeof(q));
  q.tmean = stored ? nullptr : ws_t + tp->layout(n).out;
  q.tlogstd = stored || sd ? nullptr : tp->p[tp->logstd];
  q.logp_old = ro->logp_old_dev; q.acts = ro->acts_dev; q.rowidx = tr->rowidx_cur;
  q.n = n; q.A = pf->act_dim(); q.sd = sd ? 1 : 0;
  q.st = tr->stats_cur; q.upd_index = &tr->ctl->upd_index; q.lr_pf = &tr->ctl->lr_pf; q.lr_vf = &tr->ctl->lr_vf;
  q.rec = tr->ad_all;
  q.lo = 0.5 * tr->ad_num[0]; q.hi = 2.0 * tr->ad_num[0];  // rsl_rl's thresholds (exact in double)
  q.factor = tr->ad_num[1]; q.lr_min = tr->ad_num[2]; q.lr_max = tr->ad_num[3];
  g_op = "kl_adapt";
  if (pf->cfg.tanh_action) V4L_KLAUNCH("kl_adapt", 0, s, kl_adapt_kernel<true>, dim3(1), loss_block(n), 0, s, q);
  else V4L_KLAUNCH("kl_adapt", 0, s, kl_adapt_kernel<false>, dim3(1), loss_block(n), 0, s, q);
  V4L_LAUNCH_CHECK();
  return 0;
}
static int run_kl_adapt_update(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, void* stream) {
  int rc;
  if ((rc = v4l_trainer_critic_grads(tr, ro, n, hp, stream))) return rc;
  if ((rc = v4l_trainer_critic_step(tr, hp, stream))) return rc;
  if ((rc = v4l_trainer_actor_grads(tr, ro, n, hp, stream))) return rc;
  if ((rc = launch_kl_adapt(tr, ro, n, (hipStream_t)stream))) return rc;
  return v4l_trainer_actor_step(tr, hp, stream);
}
struct KlAdaptLearner {
  static constexpr const char* what = "kl-adapt update";
  static constexpr const char* next_name = "v4l_trainer_kl_adapt_update_next";
  static constexpr const char* run_name = "v4l_trainer_kl_adapt_update_run";
  static int check(const v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, const float* rec) {
    return check_kl_adapt_args(tr, ro, n, hp, rec);
  }
  static int run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, float*, void* stream) {
    return run_kl_adapt_update(tr, ro, n, hp, stream);
  }
  static RecGraphState state(v4l_trainer* tr) {
    return {&tr->dkey, &tr->dexec, &tr->dexec_run, &tr->dexec_run_count, &tr->dwarm, &tr->ad_captures, &tr->ad_replays};
  }
  static void drop(v4l_trainer* tr) { drop_kl_adapt_graph(tr); }
  // (as KlLearner: PPO's graphs, and the early stop's, bake the same descriptor tables in and stay)
  static void drop_others(v4l_trainer* tr) { drop_vmpo_graph(tr); drop_a2c_graph(tr); drop_reinforce_graph(tr); }
};
int v4l_trainer_kl_adapt_update_next(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, int use_graph,
                                     void* stream) {
  V4L_REQUIRE(tr != nullptr, "v4l_trainer_kl_adapt_update_next: null argument");
  return rec_update_next<KlAdaptLearner>(tr, ro, n, hp, tr->ad_all, use_graph, stream);
}
int v4l_trainer_kl_adapt_update_run(v4l_trainer* tr, const v4l_rollout* ro, int n, const v4l_ppo_hyper* hp, int count, int use_graph,
                                    void* stream) {
  V4L_REQUIRE(tr != nullptr, "v4l_trainer_kl_adapt_update_run: null argument");
  return rec_update_run<KlAdaptLearner>(tr, ro, n, hp, tr->ad_all, count, use_graph, stream);
}
int v4l_trainer_kl_adapt_graph_counts(const v4l_trainer* tr, int64_t* captures, int64_t* replays) {
  V4L_REQUIRE(tr && captures && replays, "v4l_trainer_kl_adapt_graph_counts: null argument");
  *captures = tr->ad_captures;
  *replays = tr->ad_replays;
  return 0;
}
// The two learning rates of the control block as doubles ({lr_pf, lr_vf}: what v4l_trainer_begin wrote, or what the last
// kl_adapt launch left: the rates the next update of the run would use). Synchronises the stream.
int v4l_trainer_lrs(v4l_trainer* tr, double* out, void* stream) {
  V4L_REQUIRE(tr && tr->bound && tr->ctl && out, "v4l_trainer_lrs: the trainer is not bound");
  hipStream_t s = (hipStream_t)stream;
  double h[2] = {0.0, 0.0};
  static_assert(offsetof(UpdCtl, lr_vf) == offsetof(UpdCtl, lr_pf) + sizeof(double), "lr_pf and lr_vf are read with one copy");
  V4L_HIP_CHECK(hipMemcpyAsync(h, (const char*)tr->ctl + offsetof(UpdCtl, lr_pf), sizeof(h), hipMemcpyDeviceToHost, s));
  V4L_HIP_CHECK(hipStreamSynchronize(s));
  out[0] = h[0]; out[1] = h[1];
  return 0;
}

int v4l_trainer_update(v4l_trainer* tr, const v4l_rollout* ro, const int* rowidx_dev, int n, const v4l_ppo_hyper* hp,
                       double lr_pf, double lr_vf, int64_t step, float* stats_dev, void* stream) {
  V4L_REQUIRE(step >= 1, "v4l_trainer_update: Adam step count starts at 1");
  int rc = v4l_trainer_begin(tr, rowidx_dev, stats_dev, lr_pf, lr_vf, step - 1, hp, stream);
  if (rc) return rc;
  return v4l_trainer_update_next(tr, ro, n, hp, 0, stream);
}

float* v4l_trainer_stats_cur(const v4l_trainer* tr) { return tr ? tr->stats_cur : nullptr; }

int v4l_trainer_sync_target(v4l_trainer* tr, void* stream) {
  V4L_REQUIRE(tr && tr->pf->bound && tr->tpf->bound, "v4l_trainer_sync_target: nets are not bound");
  hipStream_t s = (hipStream_t)stream;
  for (size_t i = 0; i < tr->pf->params.size(); ++i)
    V4L_HIP_CHECK(hipMemcpyAsync(tr->tpf->p[i], tr->pf->p[i], (size_t)tr->pf->params[i].numel * sizeof(float),
                                 hipMemcpyDeviceToDevice, s));
  return v4l_net_pack(tr->tpf, stream);
}

}  // extern "C"
