// Sanitizer harness for csrc/host_step.h (the collector's host-side cast pool): two callers that share the pool with different
// thread counts, many casts with changing thread counts from frames of changing stack depth, pauses longer than the workers'
// spin window (sleep / wake path), a pool that grows and never shrinks, ragged sizes; every result compared with the scalar
// two-step rounding. Built with -fsanitize=thread and -fsanitize=address, each with and without -DV4L_CAST_POOL_TEST_STALL (a
// worker sleeps 0 - 200 us between noticing a job and registering for it: late workers on nearly every job), by
// tools/host_step_sanitize.sh (no GPU, no HIP).
//   cast_pool_check [iterations]   verify
//   cast_pool_check --time         no verification, for an -O2 build without sanitizers: us per job of the shipped shape
// (--time uses cast_rows alone, so the same file times an older host_step.h placed at the same relative path)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../vision4leg_amd/csrc/host_step.h"

using namespace v4l::host;

// cast_rows from a frame `depth` calls further down the stack: back-to-back jobs start from different stack addresses
__attribute__((noinline)) static int cast_at_depth(int depth, const double* rows, int64_t ld, int E, int S, int64_t img, float* prop,
                                                   void* dst, int kind, int threads) {
  volatile char pad[192];
  pad[0] = (char)depth;
  const int rc = depth > 0 ? cast_at_depth(depth - 1, rows, ld, E, S, img, prop, dst, kind, threads)
                           : cast_rows(rows, ld, E, S, img, prop, dst, kind, threads);
  return rc + (pad[0] != (char)depth);
}

static int time_jobs() {
  const int S = 93, threads = 8, jobs = 2000;
  const int64_t img = 16384, ld = S + img;
  for (int E : {32, 64}) {
    std::mt19937_64 rng(3);
    std::normal_distribution<double> nd(0.0, 1.0);
    std::vector<double> rows((size_t)E * ld);
    for (double& x : rows) x = nd(rng);
    std::vector<float> prop((size_t)E * S);
    std::vector<uint16_t> out((size_t)E * img);
    std::vector<double> us(jobs);
    for (int it = -200; it < jobs; ++it) {  // (200 jobs of warm-up)
      const auto t0 = std::chrono::steady_clock::now();
      if (cast_rows(rows.data(), ld, E, S, img, prop.data(), out.data(), CAST_F16, threads) != 0) return 2;
      const auto t1 = std::chrono::steady_clock::now();
      if (it >= 0) us[it] = std::chrono::duration<double, std::micro>(t1 - t0).count();
    }
    std::sort(us.begin(), us.end());
    std::printf("cast pool time: E %d S %d img %lld f16 %d threads, %d jobs: median %.2f us, p99 %.2f us per job\n", E, S, (long long)img,
                threads, jobs, us[jobs / 2], us[jobs * 99 / 100]);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--time") == 0) return time_jobs();
  const int iters = argc > 1 ? std::atoi(argv[1]) : 240;
  // two host threads (two collectors) share the process-wide pool and ask for different thread counts: they must take turns
  {
    std::atomic<int> bad{0};
    auto caller = [&](int seed, int threads, int jobs) {
      std::mt19937_64 r2(seed);
      std::normal_distribution<double> n2(0.0, 1.0);
      const int E = 8, S = 5; const int64_t img = 4099, ld = S + img;
      std::vector<double> rows((size_t)E * ld);
      std::vector<float> prop((size_t)E * S);
      std::vector<uint16_t> out((size_t)E * img);
      for (int it = 0; it < jobs; ++it) {
        for (double& x : rows) x = n2(r2);
        if (cast_rows(rows.data(), ld, E, S, img, prop.data(), out.data(), CAST_F16, threads) != 0) { bad++; return; }
        for (int e = 0; e < E; ++e)
          for (int64_t c = 0; c < img; ++c)
            if (out[(size_t)e * img + c] != f32_to_f16_rne((float)rows[(size_t)e * ld + S + c])) { bad++; return; }
      }
    };
    std::thread a(caller, 11, 4, 25), b(caller, 12, 7, 25);
    a.join(); b.join();
    if (bad.load() != 0) { std::printf("concurrent callers: mismatch\n"); return 1; }
    for (int it = 0; it < 12; ++it) caller(13 + it, it % 2 ? 7 : 4, 1);  // and one caller that alternates: 4, 7, 4, 7, ...
    if (bad.load() != 0) { std::printf("alternating caller: mismatch\n"); return 1; }
#ifdef V4L_CAST_MAX_THREADS  // (a host_step.h with the grow-only pool) 4 and 7 threads, however often they alternate: 6 workers, started once
    if (CastPool::instance().workers() != 6) { std::printf("4 / 7 threads started %d workers, not 6\n", CastPool::instance().workers()); return 1; }
#endif
  }
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd(0.0, 1.0);
  long long checked = 0;
  const int shapes[][3] = {{32, 93, 16384}, {5, 0, 4099}, {3, 7, 2048 * 3 + 5}, {64, 93, 1000}};
  for (int it = 0; it < iters; ++it) {
    const int* sh = shapes[it % 4];
    const int E = sh[0], S = sh[1];
    const int64_t img = sh[2], ld = S + img;
    std::vector<double> rows((size_t)E * ld);
    for (double& x : rows) x = nd(rng) * (it % 7 == 0 ? 1e-6 : 1.0);
    rows[S] = 65520.0; rows[S + 1] = 1.0 + std::ldexp(1.0, -11) + std::ldexp(1.0, -30); rows[S + 2] = NAN; rows[S + 3] = 6e-8;
    const int kind = it % 3;  // 0: fp32 image, 1: bf16, 2: f16
    const int threads = 1 + (it * 5) % 13;
    std::vector<float> prop((size_t)E * (S > 0 ? S : 1), -7.f);
    std::vector<uint16_t> out16((size_t)E * img);
    std::vector<float> out32((size_t)E * img);
    void* dst = kind == 0 ? (void*)out32.data() : (void*)out16.data();
    if (cast_at_depth((it * 3) % 7, rows.data(), ld, E, S, img, S ? prop.data() : nullptr, dst, kind, threads) != 0) return 2;
    for (int e = 0; e < E; ++e) {
      for (int s = 0; s < S; ++s)
        if (prop[(size_t)e * S + s] != (float)rows[(size_t)e * ld + s]) { std::printf("proprio mismatch it %d\n", it); return 1; }
      for (int64_t c = 0; c < img; ++c) {
        const float f = (float)rows[(size_t)e * ld + S + c];
        if (kind == 0) {
          const float g = out32[(size_t)e * img + c];
          if (!(g == f || (f != f && g != g))) { std::printf("fp32 mismatch it %d\n", it); return 1; }
        } else {
          const uint16_t want = kind == CAST_BF16 ? f32_to_bf16_rne(f) : f32_to_f16_rne(f), got = out16[(size_t)e * img + c];
          const bool nan = f != f;
          if (!nan && want != got) { std::printf("16-bit mismatch it %d kind %d e %d c %lld: %04x vs %04x\n", it, kind, e, (long long)c, got, want); return 1; }
        }
        ++checked;
      }
    }
    if (it % 40 == 39) std::this_thread::sleep_for(std::chrono::milliseconds(2));  // longer than SPIN_NS: the workers go to sleep
  }
#ifdef V4L_CAST_MAX_THREADS
  if (iters >= 6 && CastPool::instance().workers() != 12) { std::printf("1..13 threads started %d workers, not 12\n", CastPool::instance().workers()); return 1; }
#endif
  std::printf("cast pool check: %lld elements over %d jobs (1..13 threads, pool grown, sleep / wake), simd %d: OK\n", checked, iters, (int)have_avx512());
  return 0;
}
