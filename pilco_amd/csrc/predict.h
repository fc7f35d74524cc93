// GP posterior at deterministic inputs, shared by predict.hip (pilco_gp_predict_points) and particles.hip
// (pilco_rollout_particles): the per-slot work buffers, the operands of one model and the device-to-device routine.
#pragma once
#include "ctx.h"

constexpr size_t PP_KS_BUDGET = size_t(1) << 24;   // doubles of cross-covariance per chunk (128 MB)

// the per-call buffers of the predictions, and the FITC operands of per-output inducing inputs (a slot of its own whose
// data, targets and hyper-parameters are views of the parent slot's).  Who reserves what for the particle entry points
// (particle_frame.hip, docs/particle_frame.md):
//   ParticleFrame::open       pt_x, pt_eps, pt_part, pt_stats, pt_par, pt_ev_* (the events' integers -- first hits, block
//                             counts, counts -- in buffers of doubles)
//   ParticleGradFrame::open   pt_x, pt_eps, pt_rew, pt_par, pg_*
//   the marginal drivers      Xt, Ks, out, pt_rew (forward); Xt, Ks, out, jac, jacW (gradient)
//   fn_setup                  fn_* (features, weights, residuals, V); the function drivers: Xt, pt_rew (forward)
//   the conditioned driver    Ks, out, pc2_*
//   pilco_debug_particle_actions   pt_x, Xt, pt_par
struct PredictWork {
    DevBuf raw, Xt, Ks, out, jac, jacW;
    Slot fitc;
    DevBuf pt_x, pt_eps, pt_rew, pt_part, pt_stats, pt_par;
    DevBuf pt_ev_first, pt_ev_part, pt_ev_counts;
    DevBuf pg_A, pg_lam, pg_ds, pg_part, pg_rew, pg_out;
    DevBuf fn_om, fn_ph, fn_Wt, fn_phix, fn_R, fn_V, fn_xi, fn_raw;   // the function-sample rollout (particles_fn.hip)
    // the full posterior covariance and the joint samples (predict_cov.hip): [Eu][Ntpad][Ntpad] covariance, its copy with
    // the jitter (factored in place), the inverses of the factor's diagonal blocks; [Eu][Ntpad][Spad] normals and C z;
    // [S][Nt][Eu] normals and samples in the caller's layout
    DevBuf pc_cov, pc_fac, pc_linv, pc_z, pc_f, pc_zraw, pc_smp;
    // the path-conditioned particle rollout (particles_cond.hip): the histories of W rows [H][nops][E][G][npad] and of points
    // [H][D][G], the packed factor and path covariance [G][E][H (H + 1) / 2], the observation draws [H][P][E], the rewards
    // [H][P], the pivot words [G][E] (int)
    DevBuf pc2_Wh, pc2_Xh, pc2_lam, pc2_cov, pc2_zeta, pc2_rew, pc2_info;
};

// The operator blocks and the points of the cross-covariance of Eu outputs of one model (device pointers).
struct PredictModel {
    const double* Pt;      // [D][npad] training / inducing points, transposed
    long sP;               // doubles between the outputs' point sets (0: one set shared by every output)
    const double *ls, *sf2, *sn2;   // [Eu][D], [Eu], [Eu]
    const double *L, *iAt, *beta;   // [Eu][npad][npad] L^{-1}, FITC: Am^{-1} Luu^{-1} (nullptr: exact GP), [Eu][npad]
    int n, npad, D, Eu;
};
PredictModel predict_model_of(const Slot& s, int e0, int Eu);   // the slot's own factorisation, outputs e0 .. e0 + Eu - 1
// test points per chunk: the cross-covariance of a chunk is at most PP_KS_BUDGET doubles (a multiple of 64)
inline int predict_chunk_cap(int Eu, int npad) { return std::max(64, (int)(PP_KS_BUDGET / ((size_t)Eu * npad)) / 64 * 64); }
// One chunk, device to device: Xt [D][ldt] holds ntc test points (transposed, ldt a multiple of 64); Ks is scratch of
// Eu * ldt * npad doubles; out_mean, out_var [Eu][ldt].  Two launches (the cross-covariances, the walk over the operator)
// on ctx->st; does not wait for the stream.
int predict_points_device(pilco_ctx* ctx, const PredictModel& m, const double* Xt, int ntc, int ldt, double* Ks, double* out_mean,
                          double* out_var);
// The same chunk's input Jacobians, after predict_points_device has left its cross-covariances in Ks (predict_jac.hip):
// dmean, dvar [Eu][ldt][D] = d mean / d x, d var / d x of the ntc test points; W is scratch of predict_jac_nops(m) * Eu * ldt *
// npad doubles (the products L^{-1} K*, iAt K*).  Two launches on ctx->st; does not wait.
inline int predict_jac_nops(const PredictModel& m) { return m.iAt ? 2 : 1; }
int predict_points_jac_device(pilco_ctx* ctx, const PredictModel& m, const double* Xt, int ntc, int ldt, const double* Ks,
                              double* W, double* dmean, double* dvar);
// W alone, in the covariance's scaling (predict_cov.hip): W[0] = L^{-1} K*, FITC W[1] = sqrt(sn2) iAt K* -- the same walk
// and the same product tiles as above, another factor on the second operator.  One launch; does not wait.
int predict_points_w_device(pilco_ctx* ctx, const PredictModel& m, int ntc, int ldt, const double* Ks, double* W);
// FITC operands of outputs e0 .. e0 + Eu - 1 on their own inducing inputs Z_all (host (E, M, D)), in pw.fitc
int factorize_own_z(pilco_ctx* ctx, Slot& s, PredictWork& pw, const double* Z_all, int e0, int Eu);
