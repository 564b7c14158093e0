// ask_tell_compact_kernel.hpp — the compaction of an ask/tell handle's list (mi355_ask_tell_compact_*): of the problems
// listed now, those whose phase is not "finished" are listed next, in the same (ascending) order, and their rows of the
// evaluation buffer move with them, so that the caller evaluates the live problems only.  An order-preserving stream
// compaction over the CURRENT list, in three launches and without any waiting between workgroups:
//   count_kernel    one wavefront per group of 64 list entries: the keep count of the group (ballot + popcount)
//   scan_kernel     ONE workgroup: the counts become their exclusive scan in place; the total follows the last group
//   scatter_kernel  one wavefront per group: ids_next[offset + rank] = id, and the group's kept rows, one after the
//                   other (or several side by side when n is small), with the lanes across the n coordinates
// No atomic decides a destination: the output is a function of the phase words alone.  Rows move from `rows` to
// `rows_next`, never in place (the host copies the packed rows back: ask_tell_host.hpp).  Every loop is bounded by the
// list length, 64 or n.  One file for every path: the kernels are templates over the path's Scalars type and its
// "finished" phase word.
#pragma once
#include <hip/hip_runtime.h>

#include "ask_tell_host.hpp"

namespace mi355 {
namespace ask_tell_compact {

constexpr int kScanThreads = 1024;

// Is list entry s kept?  `prob`: the problem it names (ids == nullptr: the identity list of a handle that has not been
// compacted yet).
template <class Scalar, class Scalars, int kFinished>
__device__ __forceinline__ bool keeps(const Args<Scalar, Scalars>& a, long long s, long long& prob) {
  prob = 0;
  if (s >= a.listed) return false;
  prob = (a.ids != nullptr) ? a.ids[s] : s;
  return a.scalars[prob].phase != kFinished;
}

template <class Scalar, class Scalars, int kFinished>
__global__ __launch_bounds__(kGroup) void count_kernel(const Args<Scalar, Scalars> a) {
  const long long group = blockIdx.x;
  long long prob;
  const bool keep = keeps<Scalar, Scalars, kFinished>(a, group * kGroup + threadIdx.x, prob);
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
  if (threadIdx.x == 0) a.counts[group] = __builtin_popcountll(mask);
}

// counts[0 .. groups) -> their exclusive scan, counts[groups] = the total.  Thread t owns the groups
// [t per, (t + 1) per): it sums them, the workgroup scans the kScanThreads sums in LDS, the thread writes its offsets.
// (A template so that every unit that launches a compaction may hold it: dispatch_ask_tell_compact.hip for the three
// wavefront paths, dispatch_lbfgs_ask_tell_wide_listed.hip for the path above n = 256.)
template <int kThreads = kScanThreads>
__global__ __launch_bounds__(kScanThreads) void scan_kernel(long long* counts, long long groups) {
  static_assert(kThreads == kScanThreads, "one scan width");
  __shared__ long long sums[kScanThreads];
  const int t = threadIdx.x;
  const long long per = (groups + kScanThreads - 1) / kScanThreads;
  const long long first = t * per;
  const long long last = (first + per < groups) ? first + per : groups;
  long long own = 0;
  for (long long i = first; i < last; ++i) own += counts[i];
  sums[t] = own;
  __syncthreads();
  for (int step = 1; step < kScanThreads; step <<= 1) {  // inclusive scan, ten rounds
    const long long below = (t >= step) ? sums[t - step] : 0;
    __syncthreads();
    sums[t] += below;
    __syncthreads();
  }
  long long running = sums[t] - own;
  for (long long i = first; i < last; ++i) {
    const long long c = counts[i];
    counts[i] = running;
    running += c;
  }
  if (t == kScanThreads - 1) counts[groups] = sums[t];
}

// lanes_per_row: a power of two, min(n rounded up, 64): 64 / lanes_per_row rows move side by side
template <class Scalar, class Scalars, int kFinished>
__global__ __launch_bounds__(kGroup) void scatter_kernel(const Args<Scalar, Scalars> a, int lanes_per_row) {
  __shared__ int kept_lane[kGroup];  // the lanes of the set bits of the ballot, in order
  const long long group = blockIdx.x;
  const int lane = threadIdx.x;
  long long prob;
  const bool keep = keeps<Scalar, Scalars, kFinished>(a, group * kGroup + lane, prob);
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
  const int count = __builtin_popcountll(mask);
  const int rank = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
  const long long offset = a.counts[group];
  if (keep) {
    a.ids_next[offset + rank] = prob;
    kept_lane[rank] = lane;
  }
  __syncthreads();
  const int side_by_side = kGroup / lanes_per_row;
  const int j0 = lane % lanes_per_row;
  for (int k = lane / lanes_per_row; k < count; k += side_by_side) {
    const Scalar* const from = a.rows + (group * kGroup + kept_lane[k]) * a.n;
    Scalar* const to = a.rows_next + (offset + k) * a.n;
    for (int j = j0; j < a.n; j += lanes_per_row) to[j] = from[j];
  }
}

template <class Scalar, class Scalars, int kFinished>
int launch(const Args<Scalar, Scalars>& a, hipStream_t stream) {
  if (a.listed <= 0) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: compaction of an empty list");
  const long long groups = (a.listed + kGroup - 1) / kGroup;
  int lanes_per_row = 1;
  while (lanes_per_row < a.n && lanes_per_row < kGroup) lanes_per_row <<= 1;
  const dim3 grid(static_cast<unsigned>(groups));
  hipLaunchKernelGGL((count_kernel<Scalar, Scalars, kFinished>), grid, dim3(kGroup), 0, stream, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(scan_kernel<kScanThreads>, dim3(1), dim3(kScanThreads), 0, stream, a.counts, groups);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL((scatter_kernel<Scalar, Scalars, kFinished>), grid, dim3(kGroup), 0, stream, a, lanes_per_row);
  HIP_TRY(hipGetLastError());
  return MI355_OK;
}

}  // namespace ask_tell_compact
}  // namespace mi355
