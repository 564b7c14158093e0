// nelder_mead_config.hpp — the coefficients of the reference's NelderMead (solver/nelder_mead.h:58-64) as the
// Nelder-Mead kernel reads them (nelder_mead_kernel.hpp), apart from the kernel so that the declarations of
// engine_internal.hpp need no kernel code.
#pragma once

namespace mi355 {

struct NelderMeadDeviceConfig {
  double rho, xi, gamma, sigma, degenerate_tol;
  int first_mode;  // 0: value mode (DifferentiabilityMode::None), 1: first mode (value and gradient at the returned vertex)
};

}  // namespace mi355
