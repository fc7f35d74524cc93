// Policy gradients through function-sample particle rollouts: pilco_rollout_particles_fn_grad / _grad_rbf.
// docs/particle_fn_gradients.md.  With the draws fixed, particle p follows ONE function f_p (particles_fn.hip), so its return is
// a plain deterministic function of the controller parameters: no clamp, no variance derivative.  The step matrix is
//   A_t[e][d] = [e == d] + d f_pe / d z_d,
//   d f_pe / d z_d = -A_e sum_l w_pel sin(omega_el . z + b_el) omega_eld - var_e sum_i k_i v_pei (z_d - X_id) / l_ed^2
// and the reverse sweep is that of particles_grad.hip (k_pg_reverse, k_pg_param_partials, k_pg_finish), unchanged: both
// gradients run it through ParticleGradFrame::sweep (particle_frame.hip).
//
// SET-UP, once per call: that of pilco_rollout_particles_fn (fn_setup).
// FORWARD, per group and step t: k_particle_head over the group; t < H - 1: k_particle_fn_step_jac -- the value step and row e
// of the step matrix in one walk of the data, stored [t][e][d][particle of the group] --; t = H - 1: k_particle_fn_step (its
// matrix meets lam_H = 0); k_pg_reward_partials.
// k_particle_fn_step_jac is fn_step_body<DM, true> (particles_fn.h): the value arithmetic is the statement k_particle_fn_step
// compiles, so states and rewards have its bits.  ORDER OF THE JACOBIAN SUMS, per particle, output e and input d: wave w takes
// the indices 8 w .. 8 w + 7 of every tile, tiles and indices ascending -- the order of the value sums -- with
//   JK_w[d] = fma(g_i, z_d - X_id, JK_w[d]),  g_i = exp(-r2_i / 2) * v_i      (the exp of the value sum; one product)
//   JF_w[d] = fma(c_l, omega_ld, JF_w[d]),    c_l = w_l * sin(arg_l)          (the argument of the value's cosine)
// then JK[d] = (((JK_0 + JK_1) + JK_2) + ..) + JK_7 and JF[d] likewise (by wave d mod 8, through LDS, 8 inputs a round), then
//   A[e][d] = [e == d] + fma(-(var_e * (il_d * il_d)), JK[d], -(A_e * JF[d])),   il_d = 1 / l_ed,  A_e = sqrt(2 var_e / L).
// No floating-point atomics, no cross-lane arithmetic.  ONE array of D sums per lane serves the kernel phase, is combined,
// and serves the feature phase; 1 / l_ed lives in LDS (it is uniform over the workgroup).
// GROUPS: as particles_grad.hip (PILCO_PARTICLE_GRAD_BUDGET, multiples of PT_BLOCK = 128); a group runs its forward and its
// reverse over its own columns of V and Wt; the set-up runs once.  No output bit depends on the grouping.
#include "particles_fn.h"

namespace pilco {

struct ParticleFnJacArgs {
    ParticleFnArgs f;
    ParticleFnJac j;
};

// grid (columns of the group / 64, E), FN_WAVES waves
template <int DM>
__global__ __launch_bounds__(64 * FN_WAVES) void k_particle_fn_step_jac(ParticleFnJacArgs a) {
    __shared__ FnStepLds<DM, true> sh;
    fn_step_body<DM, true>(a.f, a.j, sh);
}

}  // namespace pilco

using namespace pilco;

namespace {

void launch_fn_step_jac(hipStream_t st, const ParticleFnJacArgs& a, int count) {
    const dim3 grid(round_up(count, 64) / 64, a.f.E), block(64 * FN_WAVES);
    const int D = a.f.D;
    if (D <= 4) hipLaunchKernelGGL(k_particle_fn_step_jac<4>, grid, block, 0, st, a);
    else if (D <= 8) hipLaunchKernelGGL(k_particle_fn_step_jac<8>, grid, block, 0, st, a);
    else if (D <= 12) hipLaunchKernelGGL(k_particle_fn_step_jac<12>, grid, block, 0, st, a);
    else if (D <= 16) hipLaunchKernelGGL(k_particle_fn_step_jac<16>, grid, block, 0, st, a);
    else if (D <= 24) hipLaunchKernelGGL(k_particle_fn_step_jac<24>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_particle_fn_step_jac<MAX_D>, grid, block, 0, st, a);
}

// Both entry points, after their refusals.  par: as rollout_particles_grad (particles_grad.hip), on the same frame
int rollout_particles_fn_grad(pilco_ctx* ctx, const FnPlan& pl, const pilco_policy* policy, const pilco_reward_term* rewards,
                              int n_rewards, const double* x0, int P, int H, const double* eps, unsigned long long seed,
                              int observation_noise, const pilco_function_draws* draws, const pilco_function_draws_out* draws_out,
                              double* reward, double* reward_steps, std::vector<double>& par, double* dreturn_dx0) {
    FnDrawsStage stage;   // (before the frame, which drains the stream when it leaves)
    ParticleGradFrame g(ctx, policy, rewards, n_rewards, x0, P, H, dreturn_dx0, par);
    const int E = g.E, D = g.D;
    const size_t PE = g.PE;
    if (int r = g.attach()) return r;
    hipStream_t st = g.st;
    if (H == 0) {   // no step: the draws are still the call's
        if (draws_out) {
            if (int r = fn_setup(ctx, pl, draws, draws_out, seed)) return r;
            if (int r = fn_draws_download(ctx, pl, draws_out, stage)) return r;
            HIPCHK(hipStreamSynchronize(st));
            fn_draws_finish(pl, draws, draws_out, stage);
        }
        *reward = 0.0;
        if (dreturn_dx0) std::fill(dreturn_dx0, dreturn_dx0 + PE, 0.0);
        return PILCO_OK;
    }
    const bool noisy = observation_noise != 0;
    ParticleFnJacArgs ja{};
    ParticleFnArgs& fa = ja.f;
    if (int r = g.open((noisy && eps) ? (size_t)H * PE : 0, fa.rw)) return r;
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    PredictWork& pw = *g.work;
    const int ldg = g.pl.ldg;
    ENSURE(pw.Xt, (size_t)D * ldg);
    if (int r = g.upload((noisy && eps) ? eps : nullptr)) return r;
    if (int r = fn_setup(ctx, pl, draws, draws_out, seed)) return r;

    ParticleHeadArgs& ha = g.ha;
    fa.n_rewards = n_rewards;
    fa.E = E; fa.D = D; fa.N = pl.N; fa.npad = pl.npad; fa.L = pl.L; fa.Lpad = pl.Lpad; fa.P = P; fa.Ppad = pl.Ppad; fa.seed = seed;
    fa.Xq = pw.Xt.p; fa.ldq = ldg; fa.Xt = s.Xt.p; fa.ls = s.ls.p; fa.sf2 = s.var.p;
    fa.noise = noisy ? s.noise.p : nullptr;
    fa.om = pw.fn_om.p; fa.ph = pw.fn_ph.p; fa.Wt = pw.fn_Wt.p; fa.V = pw.fn_V.p;
    fa.rew = pw.pt_rew.p;
    ja.j.ldg = ldg;
    ha.Xt = pw.Xt.p; ha.ldt = ldg;
    auto step = [&](int g0, int ng, int t) {
        ha.p0 = fa.p0 = g0; ha.ntc = ng;
        ha.x = fa.x = g.slab(t);
        fa.xn = g.slab(t + 1);
        fa.t = t;
        fa.eps_in = (noisy && eps) ? pw.pt_eps.p + (size_t)t * PE : nullptr;
        fa.eps_out = nullptr;
        launch_particle_head(st, ha);
        if (t < H - 1) {
            ja.j.A = pw.pg_A.p + (size_t)t * E * D * ldg;
            launch_fn_step_jac(st, ja, ng);
        } else {
            launch_fn_step(st, fa, ng);
        }
        return (int)PILCO_OK;
    };
    if (int r = g.sweep(step)) return r;
    if (int r = g.finish_enqueue()) return r;
    if (int r = fn_draws_download(ctx, pl, draws_out, stage)) return r;
    HIPCHK(hipStreamSynchronize(st));
    fn_draws_finish(pl, draws, draws_out, stage);
    g.finish(reward, reward_steps, par);
    return PILCO_OK;
}

// the refusals of both entry points, before any launch or upload: those of the marginal gradient, then those of the
// function-sample rollout about the slot, the draws and the budget
int check_fn_grad_call(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards, const double* x0, int P,
                       int H, const double* reward, int entry, const pilco_function_draws* draws, FnPlan& pl) {
    if (int r = check_particle_grad_call(ctx, "rollout_particles_fn_grad", policy, rewards, n_rewards, x0, P, H, reward, entry)) return r;
    return fn_plan(ctx, "rollout_particles_fn_grad", draws, P, pl);
}

}  // namespace

extern "C" int pilco_rollout_particles_fn_grad(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                               const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                               int observation_noise, const pilco_function_draws* draws,
                                               const pilco_function_draws_out* draws_out, double* reward, double* reward_steps,
                                               double* dW, double* db, double* dreturn_dx0) {
    if (!ctx) return PILCO_E_SHAPE;
    FnPlan pl{};
    if (int r = check_fn_grad_call(ctx, policy, rewards, n_rewards, x0, P, H, reward, PILCO_POLICY_LINEAR, draws, pl)) return r;
    return pg_linear_entry(ctx, "rollout_particles_fn_grad", policy, dW, db, [&](std::vector<double>& par) {
        return rollout_particles_fn_grad(ctx, pl, policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, draws, draws_out,
                                         reward, reward_steps, par, dreturn_dx0);
    });
}

extern "C" int pilco_rollout_particles_fn_grad_rbf(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards,
                                                   int n_rewards, const double* x0, int P, int H, const double* eps,
                                                   unsigned long long seed, int observation_noise, const pilco_function_draws* draws,
                                                   const pilco_function_draws_out* draws_out, const double* Xp, const double* Yp,
                                                   const double* lsp, const double* noisep, int bf, double* reward,
                                                   double* reward_steps, double* dX, double* dY, double* dls, double* dreturn_dx0) {
    if (!ctx) return PILCO_E_SHAPE;
    FnPlan pl{};
    if (int r = check_fn_grad_call(ctx, policy, rewards, n_rewards, x0, P, H, reward, PILCO_POLICY_RBF, draws, pl)) return r;
    return pg_rbf_entry(ctx, "rollout_particles_fn_grad", policy, Xp, Yp, lsp, noisep, bf, dX, dY, dls, [&](std::vector<double>& par) {
        return rollout_particles_fn_grad(ctx, pl, policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, draws, draws_out,
                                         reward, reward_steps, par, dreturn_dx0);
    });
}

extern "C" int pilco_rollout_particles_fn_grad_mlp(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards,
                                                   int n_rewards, const double* x0, int P, int H, const double* eps,
                                                   unsigned long long seed, int observation_noise, const pilco_function_draws* draws,
                                                   const pilco_function_draws_out* draws_out, double* reward, double* reward_steps,
                                                   double* dW1, double* db1, double* dW2, double* db2, double* dreturn_dx0) {
    if (!ctx) return PILCO_E_SHAPE;
    FnPlan pl{};
    if (int r = check_fn_grad_call(ctx, policy, rewards, n_rewards, x0, P, H, reward, PILCO_POLICY_MLP, draws, pl)) return r;
    return pg_mlp_entry(ctx, "rollout_particles_fn_grad", policy, dW1, db1, dW2, db2, [&](std::vector<double>& par) {
        return rollout_particles_fn_grad(ctx, pl, policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, draws, draws_out,
                                         reward, reward_steps, par, dreturn_dx0);
    });
}
