// trust_region_config.hpp — the reference's TrustRegionNewtonConfig as the trust-region kernel reads it
// (trust_region_kernel.hpp), apart from the kernel so that the declarations of engine_internal.hpp need no kernel code.
#pragma once

namespace mi355 {

// radius scalars as given; the CG and retry caps pre-clamped by the entry point
struct TrustRegionDeviceConfig {
  double initial_radius, max_radius, acceptance_threshold, shrink_factor, expand_factor, rho_low, rho_high,
      cg_forcing_coefficient, min_radius;
  int cg_extra_iterations;   // max(cg_max_iterations_floor, 0): the CG cap (trust_region_newton.h:357-358, see the kernel)
  int rejection_retry_limit; // min(max(rejection_retry_limit, 0), 1000)                (:244-247)
};

}  // namespace mi355
