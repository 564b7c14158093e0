// first_order_config.hpp — the constants of the reference's Armijo<F, 1> search as the first-order kernel reads them
// (first_order_kernel.hpp), apart from the kernel so that the declarations of engine_internal.hpp need no kernel code.
#pragma once

namespace mi355 {

enum FirstOrderMethod : int {
  kGradientDescent = 0,            // solver/gradient_descent.h, More-Thuente search
  kConjugatedGradientDescent = 1,  // solver/conjugated_gradient_descent.h, Armijo<F, 1> search
};

struct FirstOrderDeviceConfig {
  double armijo_c;          // c of the sufficient-decrease test              (linesearch/armijo.h:49)
  double armijo_rho;        // the factor alpha shrinks by per rejected trial (:50)
  double armijo_alpha_min;  // the search ends when alpha <= alpha_min        (:56)
  int eval_trials;          // 1 = the Armijo trials run eval (value and gradient) and the last gradient is kept;
                            // 0 = they run the functor's value() and one eval follows at the accepted point
};

}  // namespace mi355
