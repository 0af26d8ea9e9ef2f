// g2o's Levenberg-Marquardt damping rule (OptimizationAlgorithmLevenberg::solve), shared by every LM kernel:
// snapshot, fusion, window, chain, chain3, tree, tree_wave, wave3, wave6 and arrow3.  The constants and the accepted-step update live
// here once; each kernel keeps its own control flow (its acceptance test, the reject step lambda *= nu, nu *= 2, the reset nu = 2).
// fusion, window, wave6 and arrow3 write lm_lambda_accepted out with these constants: called, it perturbs the compiler's instruction
// order and register assignment in those kernels (wave6: three more SGPR spills), so their machine code would no longer be the same.
// Internal to the including translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace locamd {
namespace {

constexpr double lm_tau = 1e-5;            // computeLambdaInit: lambda = tau * max_j |H_jj|
constexpr double lm_good_lo = 1.0 / 3.0;   // the clamp of an accepted step's factor (goodStepLowerScale, goodStepUpperScale)
constexpr double lm_good_hi = 2.0 / 3.0;
constexpr int lm_max_trials = 10;          // maxTrialsAfterFailure
constexpr double lm_scale_eps = 1e-3;      // what computeScale adds to sum_j dx_j (lambda dx_j + b_j): the scale is never zero

// lambda after an accepted step: lambda * max(1/3, min(1 - (2 rho - 1)^3, 2/3)), in g2o's operation order
__device__ __forceinline__ double lm_lambda_accepted(double lambda, double rho) {
    const double r21 = 2.0 * rho - 1.0;
    double alpha = 1.0 - r21 * r21 * r21;
    alpha = fmin(alpha, lm_good_hi);
    return lambda * fmax(lm_good_lo, alpha);
}

}  // namespace
}  // namespace locamd
