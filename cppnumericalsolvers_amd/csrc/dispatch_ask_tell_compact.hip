// dispatch_ask_tell_compact.hip — the compaction kernels (ask_tell_compact_kernel.hpp) for the three ask/tell paths:
// Lbfgs in double, Lbfgs in float and Lbfgsb, each with its Scalars type and its "finished" phase word.
#define MI355_DISPATCH_TU 1
#include "ask_tell_compact_kernel.hpp"
#include "lbfgs_ask_tell_config.hpp"
#include "lbfgs_ask_tell_f32_config.hpp"
#include "lbfgsb_ask_tell_config.hpp"

namespace mi355 {

template <class Scalar, class Scalars, int kFinished>
int dispatch_ask_tell_compact(const ask_tell_compact::Args<Scalar, Scalars>& args, hipStream_t stream) {
  return ask_tell_compact::launch<Scalar, Scalars, kFinished>(args, stream);
}

template int dispatch_ask_tell_compact<double, ask_tell::Scalars, ask_tell::kPhaseFinished>(
    const ask_tell_compact::Args<double, ask_tell::Scalars>&, hipStream_t);
template int dispatch_ask_tell_compact<float, ask_tell_f32::Scalars, ask_tell_f32::kPhaseFinished>(
    const ask_tell_compact::Args<float, ask_tell_f32::Scalars>&, hipStream_t);
template int dispatch_ask_tell_compact<double, ask_tell_box::Scalars, ask_tell_box::kPhaseFinished>(
    const ask_tell_compact::Args<double, ask_tell_box::Scalars>&, hipStream_t);

}  // namespace mi355
