// Host side of one env step of the collector (torchrl/collector/on_policy.py:90-100: `torch.Tensor(self.current_ob).to(device)`,
// pf.explore, vf, `.cpu().numpy()`), as ONE C call with no interpreter in the loop (round 6):
//
//   float64 rows [E][S + C*H*W] (what the env wrappers hand over)
//     -> cast_rows: fp32 proprio block | 16-bit depth block in pinned memory, on a persistent pool of worker threads (AVX-512:
//        vcvtpd2ps, then vcvtps2ph for half / an integer round-to-nearest-even for bfloat16 — the same two-step rounding
//        torch's float64 -> float16 / bfloat16 copy performs, i.e. torch.Tensor(ob) followed by the kernels' ingest cast)
//     -> the step's two launches, reading the pinned rows in place (v4l_actor_step_split)
//     -> wait until the [E][A] action AND the [E] value have arrived in pinned memory (both armed with NaN before the launch;
//        every block writes its output last, so the observation buffers are free when the call returns)
//
// The pool: workers spin on a generation word for SPIN_NS after their last job, then block on a condition variable — a
// simulator that steps for milliseconds gets its cores back, a fast one never pays a wake-up.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include "../../include/v4l_hip.h"

namespace v4l {
namespace host {

enum { CAST_BF16 = 1, CAST_F16 = 2 };

static inline void cpu_relax() {
#if defined(__x86_64__)
  _mm_pause();
#endif
}

// ---- scalar reference of the two-step rounding (also the tail / non-AVX-512 path)
static inline uint16_t f32_to_bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);  // NaN stays NaN (quiet)
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline uint16_t f32_to_f16_rne(float f) {
  const _Float16 h = (_Float16)f;  // IEEE round-to-nearest-even, subnormals kept, overflow -> inf
  uint16_t b;
  memcpy(&b, &h, 2);
  return b;
}
static void cast_span_scalar(const double* src, uint16_t* dst, int64_t n, int kind) {
  if (kind == CAST_BF16) for (int64_t i = 0; i < n; ++i) dst[i] = f32_to_bf16_rne((float)src[i]);
  else for (int64_t i = 0; i < n; ++i) dst[i] = f32_to_f16_rne((float)src[i]);
}
static void cast_span_f32_scalar(const double* src, float* dst, int64_t n) {
  for (int64_t i = 0; i < n; ++i) dst[i] = (float)src[i];
}

#if defined(__x86_64__)
__attribute__((target("avx512f,avx512vl,avx512bw,f16c"))) static void cast_span_avx512(const double* src, uint16_t* dst, int64_t n,
                                                                                       int kind) {
  int64_t i = 0;
  if (kind == CAST_F16) {
    for (; i + 16 <= n; i += 16) {
      const __m256 a = _mm512_cvtpd_ps(_mm512_loadu_pd(src + i)), b = _mm512_cvtpd_ps(_mm512_loadu_pd(src + i + 8));
      _mm_storeu_si128(reinterpret_cast<__m128i*>(dst + i), _mm256_cvtps_ph(a, _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC));
      _mm_storeu_si128(reinterpret_cast<__m128i*>(dst + i + 8), _mm256_cvtps_ph(b, _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC));
    }
  } else {
    const __m256i bias = _mm256_set1_epi32(0x7fff), one = _mm256_set1_epi32(1), absm = _mm256_set1_epi32(0x7fffffff),
                  inf = _mm256_set1_epi32(0x7f800000), quiet = _mm256_set1_epi32(0x0040);
    for (; i + 8 <= n; i += 8) {
      const __m256i u = _mm256_castps_si256(_mm512_cvtpd_ps(_mm512_loadu_pd(src + i)));
      const __m256i hi = _mm256_srli_epi32(u, 16);
      const __m256i r = _mm256_srli_epi32(_mm256_add_epi32(u, _mm256_add_epi32(bias, _mm256_and_si256(hi, one))), 16);
      const __mmask8 nan = _mm256_cmpgt_epi32_mask(_mm256_and_si256(u, absm), inf);
      const __m256i out = _mm256_mask_blend_epi32(nan, r, _mm256_or_si256(hi, quiet));
      _mm_storeu_si128(reinterpret_cast<__m128i*>(dst + i), _mm256_cvtepi32_epi16(out));
    }
  }
  if (i < n) cast_span_scalar(src + i, dst + i, n - i, kind);
}
__attribute__((target("avx512f"))) static void cast_span_f32_avx512(const double* src, float* dst, int64_t n) {
  int64_t i = 0;
  for (; i + 8 <= n; i += 8) _mm256_storeu_ps(dst + i, _mm512_cvtpd_ps(_mm512_loadu_pd(src + i)));
  if (i < n) cast_span_f32_scalar(src + i, dst + i, n - i);
}
static bool have_avx512() {
  static const bool ok = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512vl") && __builtin_cpu_supports("avx512bw") &&
                         __builtin_cpu_supports("f16c");
  return ok;
}
#else
static bool have_avx512() { return false; }
#endif

static inline void cast_span(const double* src, uint16_t* dst, int64_t n, int kind, bool simd) {
#if defined(__x86_64__)
  if (simd) return cast_span_avx512(src, dst, n, kind);
#endif
  cast_span_scalar(src, dst, n, kind);
}
static inline void cast_span_f32(const double* src, float* dst, int64_t n, bool simd) {
#if defined(__x86_64__)
  if (simd) return cast_span_f32_avx512(src, dst, n);
#endif
  cast_span_f32_scalar(src, dst, n);
}

// ---- one cast job: rows [E][ld] float64 -> prop [E][S] fp32 (S may be 0) | img [E][img] 16-bit (or fp32 when kind == 0)
// Split into `parts` contiguous runs of (row, 2048-column chunk) units, one per participant (static: no shared counter is touched
// per unit — a first version with a shared "next unit" word scaled to 3.3 x on 8 threads and got SLOWER beyond 16); a participant
// that finishes early walks the other parts and takes any that nobody has claimed yet (a worker that was asleep).
constexpr int64_t CAST_CHUNK = 2048;
constexpr int CAST_MAX_PARTS = V4L_CAST_MAX_THREADS;
struct CastParams {
  const double* rows; int64_t ld; int E, S; int64_t img;
  float* prop; void* img_out; int kind; bool simd;
  int units, parts;
};
struct alignas(64) CastClaim { std::atomic<int> taken{0}; };
struct CastJob {
  CastParams p;
  CastClaim claim[CAST_MAX_PARTS];
  alignas(64) std::atomic<int> done{0};  // parts finished
};
static inline void cast_unit(const CastParams& j, int u) {
  const int64_t per_row = (j.img + CAST_CHUNK - 1) / CAST_CHUNK;
  const int e = (int)(u / per_row);
  const int64_t c0 = (u - (int64_t)e * per_row) * CAST_CHUNK, c1 = c0 + CAST_CHUNK < j.img ? c0 + CAST_CHUNK : j.img;
  const double* src = j.rows + (int64_t)e * j.ld;
  if (c0 == 0 && j.S > 0) cast_span_f32(src, j.prop + (int64_t)e * j.S, j.S, j.simd);
  if (j.kind == 0) cast_span_f32(src + j.S + c0, reinterpret_cast<float*>(j.img_out) + (int64_t)e * j.img + c0, c1 - c0, j.simd);
  else cast_span(src + j.S + c0, reinterpret_cast<uint16_t*>(j.img_out) + (int64_t)e * j.img + c0, c1 - c0, j.kind, j.simd);
}
// participant `id` (0 = the caller, 1 .. parts - 1 = workers): its own part first, then whatever is still unclaimed
static inline void cast_drain(CastJob& j, int id) {
  const int parts = j.p.parts, units = j.p.units;
  for (int k = 0; k < parts; ++k) {
    const int p = (id + k) % parts;
    if (j.claim[p].taken.load(std::memory_order_relaxed) != 0 || j.claim[p].taken.exchange(1, std::memory_order_acq_rel) != 0) continue;
    const int u0 = (int)((int64_t)units * p / parts), u1 = (int)((int64_t)units * (p + 1) / parts);
    for (int u = u0; u < u1; ++u) cast_unit(j.p, u);
    j.done.fetch_add(1, std::memory_order_release);
  }
}

// The pool lives as long as the process: it only ever gains workers, they are detached and keep `this`, so the one instance
// is never destroyed and no other can be made.
class CastPool {
 public:
  static constexpr int64_t SPIN_NS = 300000;  // a worker keeps spinning this long after its last job, then sleeps
  static CastPool& instance() { static CastPool* pool = new CastPool; return *pool; }
  int workers() const { return workers_; }    // threads started so far
  // (call between jobs) starts workers until there are `workers` of them; the ones already running stay
  void grow(int workers) {
    for (; workers_ < workers; ++workers_)
      std::thread([this, id = workers_ + 1, seen = state_.load(std::memory_order_relaxed) >> 1] { loop(id, seen); }).detach();
  }
  // runs the job on the workers 1 .. p.parts - 1 + the calling thread; returns when every unit is done and no worker is inside
  void run(const CastParams& p) {
    job_.p = p;
    for (int i = 0; i < p.parts; ++i) job_.claim[i].taken.store(0, std::memory_order_relaxed);
    job_.done.store(0, std::memory_order_relaxed);
    const uint64_t gen = (state_.load(std::memory_order_relaxed) >> 1) + 1;
    state_.store(gen << 1 | 1, std::memory_order_seq_cst);  // open: the next generation and its job in one write
    if (sleepers_.load(std::memory_order_seq_cst) > 0) {
      std::lock_guard<std::mutex> g(mu_);
      cv_.notify_all();
    }
    cast_drain(job_, 0);
    while (job_.done.load(std::memory_order_acquire) < p.parts) cpu_relax();
    state_.store(gen << 1, std::memory_order_seq_cst);  // close
    while (busy_.load(std::memory_order_seq_cst) > 0) cpu_relax();
  }

 private:
  CastPool() = default;
  void loop(int id, uint64_t seen) {
    uint64_t spins = 0;
#ifdef V4L_CAST_POOL_TEST_STALL
    uint64_t lcg = 0x9e3779b97f4a7c15ull * (uint64_t)id;
#endif
    auto last = std::chrono::steady_clock::now();
    for (;;) {
      const uint64_t g = state_.load(std::memory_order_acquire) >> 1;
      if (g != seen) {
        seen = g;
#ifdef V4L_CAST_POOL_TEST_STALL  // (tools/host/cast_pool_check.cpp only) a late worker on nearly every job: 0 - 200 us before it registers
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        std::this_thread::sleep_for(std::chrono::microseconds((lcg >> 33) % 201));
#endif
        busy_.fetch_add(1, std::memory_order_seq_cst);
        const uint64_t s = state_.load(std::memory_order_seq_cst);
        seen = s >> 1;  // (a late worker may find a LATER job open: that is the generation it has now dealt with)
        if ((s & 1) != 0 && id < job_.p.parts) cast_drain(job_, id);
        busy_.fetch_sub(1, std::memory_order_acq_rel);
        last = std::chrono::steady_clock::now();
        continue;
      }
      cpu_relax();
      if ((++spins & 1023) == 0 &&
          std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - last).count() > SPIN_NS) {
        std::unique_lock<std::mutex> lk(mu_);
        sleepers_.fetch_add(1, std::memory_order_seq_cst);
        cv_.wait(lk, [&] { return state_.load(std::memory_order_seq_cst) >> 1 != seen; });
        sleepers_.fetch_sub(1, std::memory_order_acq_rel);
      }
    }
  }
  // The one job slot (jobs are strictly sequential: pool_mutex()) and its state word: generation << 1 | open. A job is open
  // from run()'s first store of state_ to its second. Invariant: a worker reads or claims anything in job_ only between its busy_
  // increment and decrement AND after it has read the open bit set in between; run() writes job_'s plain fields only while the
  // bit is clear and after it has read busy_ == 0 since clearing it. Close -> read busy_ on the caller's side and register ->
  // read state_ on the worker's side are store-then-load pairs, so all four are seq_cst: in their single total order either the
  // caller sees the worker and waits for it, or the worker sees the job closed and leaves (or sees a LATER job open — whose
  // store it then acquires, fields and all, and whose run() finds it in busy_; it takes that reading's generation as seen, so it
  // does not register for the same job twice). Open -> read sleepers_ against count myself -> read state_ (a worker going to
  // sleep) is the same pattern and seq_cst for the same reason.
  // A cache line each for what the idle workers spin on (state_) and what every participant increments and decrements per job
  // (busy_): on one line, each of those 14 writes per job took the line from every spinner, and on a two-socket host a process
  // ran 6.6 - 7.5 or 9 - 11 us per job depending on where its threads had landed (profiles/cast_pool_timing.txt).
  CastJob job_;
  alignas(64) std::atomic<uint64_t> state_{0};
  alignas(64) std::atomic<int> busy_{0};
  alignas(64) std::atomic<int> sleepers_{0};
  std::mutex mu_;
  std::condition_variable cv_;
  int workers_ = 0;
};

// process-wide pool (threads - 1 workers: the caller works too), grown to the largest count asked for so far and never shrunk:
// a job with fewer parts leaves the workers beyond them idle. One job at a time: the library's contract is one HANDLE per host
// thread at a time, but the pool is shared by all handles of the process — two collectors in two threads take turns here
// (uncontended: one atomic exchange).
static std::mutex& pool_mutex() { static std::mutex mu; return mu; }

static int cast_rows(const double* rows, int64_t ld, int E, int S, int64_t img, float* prop, void* img_out, int kind, int threads) {
  CastParams p = {rows, ld, E, S, img, prop, img_out, kind, have_avx512(), E * (int)((img + CAST_CHUNK - 1) / CAST_CHUNK), 1};
  if (threads > CAST_MAX_PARTS) threads = CAST_MAX_PARTS;
  if (threads > p.units) threads = p.units;
  if (threads <= 1) {
    for (int u = 0; u < p.units; ++u) cast_unit(p, u);
    return 0;
  }
  p.parts = threads;
  std::lock_guard<std::mutex> g(pool_mutex());
  CastPool::instance().grow(p.parts - 1);
  CastPool::instance().run(p);
  return 0;
}

// all of `n` floats are numbers (the buffers were armed with NaN)?
static inline bool arrived(const volatile float* p, int n) {
  for (int i = 0; i < n; ++i) { const float x = p[i]; if (x != x) return false; }
  return true;
}

}  // namespace host
}  // namespace v4l
