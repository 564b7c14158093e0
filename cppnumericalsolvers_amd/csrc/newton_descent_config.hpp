// newton_descent_config.hpp — the constants of the reference's NewtonDescent and of its Armijo<F, 2> search as the
// Newton-descent kernel reads them (newton_descent_kernel.hpp), apart from the kernel so that the declarations of
// engine_internal.hpp need no kernel code.
#pragma once

namespace mi355 {

struct NewtonDescentDeviceConfig {
  double safe_guard;   // added to the diagonal of H before the LU      (newton_descent.h:69, :74)
  double armijo_c;     // c of the sufficient-decrease test              (linesearch/armijo.h:85)
  double armijo_rho;   // the factor alpha shrinks by per rejected trial (:86)
};

}  // namespace mi355
