// atc_evaluator.hip — the evaluator of atc_header_test.cc: a kernel of the test's own (no library code), one thread per
// LISTED row.  Chained Rosenbrock at n = 5 in the operation order of the library's functor at eight lanes per problem
// (csrc/objectives.hpp; built with -ffp-contract=off as the library is), so that the loop can be held against the
// persistent kernel bit for bit:
//   t2_j = x_{j+1} - x_j x_j,  term_j = (1 - x_j)^2 + (100 t2_j) t2_j  for j < 4
//   f = ((term_0 + term_1) + (term_2 + term_3)) + 0      the butterfly over eight lanes, the upper four all zero
//   g_j = [-2 (1 - x_j) + (200 t2_j) (-2 x_j)]_{j < 4} + [200 t2_{j-1}]_{j > 0}
// It also counts, per PROBLEM (through ids), how often the problem was evaluated.
#include <hip/hip_runtime.h>

namespace {

constexpr int kN = 5;

__global__ void rosenbrock5(const double* x, double* f, double* g, long long rows, const long long* ids,
                            unsigned* evaluations) {
  const long long s = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (s >= rows) return;
  const double* const xs = x + s * kN;
  double t2[kN - 1], term[kN - 1];
  for (int j = 0; j < kN - 1; ++j) {
    const double t1 = 1.0 - xs[j];
    t2[j] = xs[j + 1] - xs[j] * xs[j];
    term[j] = t1 * t1 + (100.0 * t2[j]) * t2[j];
  }
  f[s] = ((term[0] + term[1]) + (term[2] + term[3])) + 0.0;
  for (int j = 0; j < kN; ++j) {
    const double a = (j < kN - 1) ? -2.0 * (1.0 - xs[j]) + (200.0 * t2[j]) * (-2.0 * xs[j]) : 0.0;
    const double b = (j > 0) ? 200.0 * t2[j - 1] : 0.0;
    g[s * kN + j] = (j == 0) ? a : ((j == kN - 1) ? b : a + b);
  }
  evaluations[ids[s]] += 1;  // (a problem is listed once: no two threads share a counter)
}

}  // namespace

// rows listed problems: x [rows][5] -> f [rows], g [rows][5]; evaluations [B] by problem.  Returns the HIP error code.
extern "C" int atc_rosenbrock5(const double* x, double* f, double* g, long long rows, const long long* ids,
                               unsigned* evaluations, void* stream) {
  if (rows <= 0) return 0;
  const unsigned blocks = static_cast<unsigned>((rows + 63) / 64);
  hipLaunchKernelGGL(rosenbrock5, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), x, f, g, rows, ids,
                     evaluations);
  return static_cast<int>(hipGetLastError());
}
