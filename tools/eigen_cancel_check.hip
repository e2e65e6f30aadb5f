// eigen_cancel_check.hip — cancellation of a speculative rank <= 64 decomposition (k_posterior_eigen_rr), stand-alone.
// build: see tools/Makefile.  usage: eigen_cancel_check [rank ...]   (default: 5 32 33 50 51 64); exit status 0: every check held,
// 1: a check failed, 3: a launch did not end within 2 s (nothing more is started then).
// run by tests/test_gpu_speculation_cancel.py
//
// Per rank: matrices as in eigen_bench.hip (the femur model's spectrum), the second a 3 % perturbation of the first, given as 13
// split-K partials and warm-started from the first one's basis — the form the merged chain step launches.  The reference is that
// decomposition, not cancelled, on a fresh zeroed work area.
//   cancelled before the start   the word is set when the launch is enqueued, `ready` null / raised / raised 50 µs later: the launch
//                                ends, V, Vt and S keep their sentinel bytes, the pinned status is not "done" (0);
//   cancelled while it runs      the launch waits for `ready`; the host raises it and writes the word d µs later, d = 0, 5, …, 100:
//                                the launch ends, and the outputs are either untouched or bit-equal to the reference;
//   after every one of these     the same decomposition, not cancelled, on the SAME work area: V, Vt, S and the sweep count bit-equal
//                                to the reference.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../icp-proposal_amd/csrc/icp_kernels.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("error: %s at line %d\n", hipGetErrorString(e_), __LINE__); fflush(stdout); _Exit(2); } } while (0)

namespace {
using clk = std::chrono::steady_clock;
void spin_us(double us) {
  const auto t0 = clk::now();
  while (std::chrono::duration<double, std::micro>(clk::now() - t0).count() < us) {}
}
// the stream's work has ended (true), or 2 s have passed (the program stops: a launch that does not end is the finding)
void wait_done(hipStream_t st, const char* what, int r) {
  const auto t0 = clk::now();
  for (;;) {
    const hipError_t e = hipStreamQuery(st);
    if (e == hipSuccess) return;
    if (e != hipErrorNotReady) { printf("rank %d, %s: %s\n", r, what, hipGetErrorString(e)); fflush(stdout); _Exit(2); }
    if (clk::now() - t0 > std::chrono::seconds(2)) { printf("rank %d, %s: the launch did not end within 2 s\n", r, what); fflush(stdout); _Exit(3); }
  }
}
struct Out { std::vector<double> V, Vt, S; int sweeps, status; };
bool same(const Out& a, const Out& b) {
  return a.sweeps == b.sweeps && a.status == b.status && std::memcmp(a.V.data(), b.V.data(), 8 * a.V.size()) == 0 &&
         std::memcmp(a.Vt.data(), b.Vt.data(), 8 * a.Vt.size()) == 0 && std::memcmp(a.S.data(), b.S.data(), 8 * a.S.size()) == 0;
}
bool all_bytes(const std::vector<double>& v, unsigned char b) {
  const unsigned char* p = (const unsigned char*)v.data();
  for (size_t i = 0; i < 8 * v.size(); ++i) if (p[i] != b) return false;
  return true;
}

int check_rank(int r) {
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd;
  auto make_M = [&](const std::vector<double>& B, int K) {  // M = I + 0.02·Bᵀ B
    std::vector<double> M((size_t)r * r, 0.0);
    for (int i = 0; i < r; ++i) M[(size_t)i * r + i] = 1.0;
    for (int k = 0; k < K; ++k)
      for (int i = 0; i < r; ++i)
        for (int j = 0; j < r; ++j) M[(size_t)i * r + j] += 0.02 * B[(size_t)k * r + i] * B[(size_t)k * r + j];
    return M;
  };
  const int K = 6 * r, n = r + 1, S = 13;
  std::vector<double> sl(r), B((size_t)K * r);
  for (int j = 0; j < r; ++j) sl[j] = std::sqrt(28.0 * std::pow(0.182 / 28.0, (double)j / (r - 1)));
  for (auto& b : B) b = nd(rng);
  for (int k = 0; k < K; ++k) for (int j = 0; j < r; ++j) B[(size_t)k * r + j] *= sl[j];
  const std::vector<double> M0 = make_M(B, K);
  std::vector<double> B2 = B;
  for (auto& b : B2) b *= 1.0 + 0.03 * nd(rng);
  const std::vector<double> M1 = make_M(B2, K);
  std::vector<double> Mp((size_t)S * n * n, 0.0);  // M1 − I as split-K partials (lower triangles of (r+1)² matrices)
  for (int sp = 0; sp < S; ++sp)
    for (int i = 0; i < r; ++i) for (int j = 0; j <= i; ++j) Mp[(size_t)sp * n * n + (size_t)i * n + j] = (M1[(size_t)i * r + j] - (i == j ? 1.0 : 0.0)) / S;

  const size_t rr = (size_t)r * r, wb = 8 * icp::eigen_work_doubles(r);
  double *dM0, *dMp, *dsl, *dV0, *dV, *dVt, *dS, *dwork, *dfresh; int* dstat;
  CK(hipMalloc(&dM0, 8 * rr)); CK(hipMalloc(&dMp, 8 * Mp.size())); CK(hipMalloc(&dsl, 8 * r)); CK(hipMalloc(&dV0, 8 * rr));
  CK(hipMalloc(&dV, 8 * rr)); CK(hipMalloc(&dVt, 8 * rr)); CK(hipMalloc(&dS, 8 * r)); CK(hipMalloc(&dwork, wb)); CK(hipMalloc(&dfresh, wb));
  CK(hipMalloc(&dstat, 64));
  CK(hipMemset(dwork, 0, wb)); CK(hipMemset(dfresh, 0, wb));
  CK(hipMemcpy(dM0, M0.data(), 8 * rr, hipMemcpyHostToDevice)); CK(hipMemcpy(dMp, Mp.data(), 8 * Mp.size(), hipMemcpyHostToDevice));
  CK(hipMemcpy(dsl, sl.data(), 8 * r, hipMemcpyHostToDevice));
  int* pinned;  // [0] cancel word, [16] ready word, [32] status of the decomposition
  CK(hipHostMalloc((void**)&pinned, 256, hipHostMallocDefault));
  volatile int* hcancel = pinned; volatile int* hready = pinned + 16; volatile int* hstat = pinned + 32;
  *hcancel = 0; *hready = 0; *hstat = -1;
  hipStream_t st; CK(hipStreamCreate(&st));

  // the neighbour's basis (cold, the ordinary way), on a work area of its own
  icp::launch_posterior_eigen(st, r, dM0, dsl, nullptr, dV0, dVt, dS, dfresh, dstat + 1);
  wait_done(st, "neighbour's basis", r);
  CK(hipMemset(dfresh, 0, wb));

  int seq = 100;
  // one speculative launch: ready_mode 0: no ready word, 1: raised already, 2: not raised yet
  auto launch = [&](double* work, int ready_mode) {
    ++seq;
    CK(hipMemset(dV, 0xA5, 8 * rr)); CK(hipMemset(dVt, 0xA5, 8 * rr)); CK(hipMemset(dS, 0xA5, 8 * r)); CK(hipMemset(dstat, 0xA5, 64));
    *hstat = -1;
    *hready = ready_mode == 2 ? 0 : 1;
    const icp::EigenSpec spec{S, (const int*)pinned, seq, ready_mode == 0 ? nullptr : (const int*)(pinned + 16), 1};
    const icp::EigenRequest rq{dMp, dV0, dV, dVt, dS, work, dstat + 1, &spec, (int*)(pinned + 32), nullptr, 0};
    if (!icp::launch_posterior_eigen_pair(st, r, dsl, 1, &rq)) { printf("rank %d: no kernel\n", r); fflush(stdout); _Exit(2); }
  };
  auto fetch = [&]() {
    Out o{std::vector<double>(rr), std::vector<double>(rr), std::vector<double>(r), 0, 0};
    int stat[2];
    CK(hipMemcpy(o.V.data(), dV, 8 * rr, hipMemcpyDeviceToHost)); CK(hipMemcpy(o.Vt.data(), dVt, 8 * rr, hipMemcpyDeviceToHost));
    CK(hipMemcpy(o.S.data(), dS, 8 * r, hipMemcpyDeviceToHost)); CK(hipMemcpy(stat, dstat, 8, hipMemcpyDeviceToHost));
    o.sweeps = stat[0]; o.status = stat[1];
    return o;
  };
  auto untouched = [&](const Out& o) { return all_bytes(o.V, 0xA5) && all_bytes(o.Vt, 0xA5) && all_bytes(o.S, 0xA5); };

  launch(dfresh, 1);
  wait_done(st, "reference", r);
  const Out ref = fetch();
  int bad = 0;
  if (ref.status != 0 || *hstat != 0 || untouched(ref)) { printf("rank %d: the reference decomposition failed (status %d, pinned %d)\n", r, ref.status, *hstat); ++bad; }
  auto follow_up = [&](const char* what) {  // not cancelled, on the work area the cancelled launch left behind
    launch(dwork, 1);
    wait_done(st, "decomposition after a cancelled one", r);
    const Out o = fetch();
    if (!same(o, ref) || *hstat != 0) {
      printf("rank %d, after %s: the next decomposition differs from the reference (sweeps %d vs %d, status %d, pinned %d)\n", r, what, o.sweeps,
             ref.sweeps, o.status, *hstat);
      ++bad;
    }
  };
  follow_up("nothing");

  // ---- cancelled before the start
  const char* names[3] = {"cancel before the start, no ready word", "cancel before the start, ready raised", "cancel before the start, ready raised later"};
  for (int mode = 0; mode < 3; ++mode) {
    *hcancel = seq + 1;  // (the launch below takes this number)
    launch(dwork, mode);
    if (mode == 2) { spin_us(50.0); *hready = 1; }
    wait_done(st, names[mode], r);
    const Out o = fetch();
    if (!untouched(o) || *hstat == 0) { printf("rank %d, %s: outputs %s, pinned status %d\n", r, names[mode], untouched(o) ? "untouched" : "WRITTEN", *hstat); ++bad; }
    follow_up(names[mode]);
  }
  // ---- cancelled while it runs
  std::string dropped, finished;
  for (int d = 0; d <= 100; d += 5) {
    launch(dwork, 2);
    spin_us(200.0);  // (the launch is resident and waits for its input)
    const int my = seq;
    *hready = 1;
    spin_us((double)d);
    *hcancel = my;
    char what[64];
    std::snprintf(what, sizeof what, "cancel %d us after the input", d);
    wait_done(st, what, r);
    const Out o = fetch();
    const bool un = untouched(o), eq = same(o, ref);
    if (!(un && *hstat != 0) && !(eq && *hstat == 0)) {
      printf("rank %d, %s: outputs neither untouched nor the reference's (untouched %d, equal %d, pinned status %d)\n", r, what, (int)un, (int)eq, *hstat);
      ++bad;
    }
    (un ? dropped : finished) += " " + std::to_string(d);
    follow_up(what);
  }
  printf("rank %d: reference %d sweeps; dropped when cancelled at [%s ] us, complete at [%s ] us; %s\n", r, ref.sweeps, dropped.c_str(), finished.c_str(),
         bad ? "FAILED" : "ok");
  fflush(stdout);
  CK(hipStreamDestroy(st)); CK(hipHostFree(pinned));
  for (void* p : {(void*)dM0, (void*)dMp, (void*)dsl, (void*)dV0, (void*)dV, (void*)dVt, (void*)dS, (void*)dwork, (void*)dfresh, (void*)dstat}) CK(hipFree(p));
  return bad;
}
}  // namespace

int main(int argc, char** argv) {
  std::vector<int> ranks;
  for (int i = 1; i < argc; ++i) ranks.push_back(std::atoi(argv[i]));
  if (ranks.empty()) ranks = {5, 32, 33, 50, 51, 64};
  int bad = 0;
  for (int r : ranks) bad += check_rank(r);
  printf("%s\n", bad ? "eigen_cancel_check: FAILED" : "eigen_cancel_check: ok");
  return bad ? 1 : 0;
}
