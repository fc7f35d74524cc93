// The RbfController's solve beta_k = (K_k + noise_k I)^-1 Y_k and its adjoint, the routine the host reverse sweep of
// pilco_rollout_grad_rbf ends with (grad.hip: RbfSolve), for a caller that accumulated the cotangents itself.
#pragma once
// Xbar (bf,E): direct part of the centres' cotangent, lsbar (U,E): of the lengthscales', betabar (U,bf): beta's
// -> dX (bf,E), dY (bf,U), dls (U,E).  false: K + noise I is singular.  betabar == nullptr: only that answer.
bool rbf_solve_adjoint(int bf, int E, int U, const double* Xp, const double* Yp, const double* lsp, const double* noisep,
                       const double* Xbar, const double* lsbar, const double* betabar, double* dX, double* dY, double* dls);
