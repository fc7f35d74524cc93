// Policy gradients through function-sample particle rollouts: pilco_rollout_particles_fn_grad / _grad_rbf.
// docs/particle_fn_gradients.md.  With the draws fixed, particle p follows ONE function f_p (particles_fn.hip), so its return is
// a plain deterministic function of the controller parameters: no clamp, no variance derivative.  The step matrix is
//   A_t[e][d] = [e == d] + d f_pe / d z_d,
//   d f_pe / d z_d = -A_e sum_l w_pel sin(omega_el . z + b_el) omega_eld - var_e sum_i k_i v_pei (z_d - X_id) / l_ed^2
// and the reverse sweep is that of particles_grad.hip (k_pg_reverse, k_pg_param_partials, k_pg_finish), unchanged.
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
#include "rbf_solve_adj.h"

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

// Both entry points, after their refusals.  par: as rollout_particles_grad (particles_grad.hip)
int rollout_particles_fn_grad(pilco_ctx* ctx, const FnPlan& pl, const pilco_policy* policy, const pilco_reward_term* rewards,
                              int n_rewards, const double* x0, int P, int H, const double* eps, unsigned long long seed,
                              int observation_noise, const pilco_function_draws* draws, const pilco_function_draws_out* draws_out,
                              double* reward, double* reward_steps, std::vector<double>& par, double* dreturn_dx0) {
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    const int E = pl.E, D = pl.D, U = D - E, Ppad = pl.Ppad;
    const int bf = policy->kind == PILCO_POLICY_RBF ? ctx->slot[PILCO_SLOT_POLICY].N : 0;
    const int Q = U > 0 ? pg_quantities(policy->kind, E, U, bf) : 0;
    par.assign((size_t)Q, 0.0);
    const size_t PE = (size_t)P * E;
    HIPCHK(hipSetDevice(ctx->device));
    if (!s.factor_valid)
        if (int r = pilco_gp_factorize(ctx, PILCO_SLOT_DYNAMICS)) return r;
    if (!s.pred) s.pred = new PredictWork();
    PredictWork& pw = *s.pred;
    hipStream_t st = ctx->st;
    StreamDrain drain{st};
    FnDrawsStage stage;
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
    const int nblk = (P + PT_BLOCK - 1) / PT_BLOCK;
    // the groups: a multiple of PT_BLOCK particles whose matrices fit the budget (at least one block)
    const size_t per_particle = (size_t)(H - 1) * E * D;
    int Pg = P;
    if (per_particle * (size_t)P > pg_group_budget())
        Pg = (int)std::min<size_t>((size_t)round_up(P, PT_BLOCK), std::max<size_t>(1, pg_group_budget() / per_particle / PT_BLOCK) * PT_BLOCK);
    const int ldg = round_up(std::min(Pg, P), 64);
    std::vector<double> hp(particle_par_doubles(E, U), 0.0);
    std::vector<double> hout((size_t)H + Q), hlam(dreturn_dx0 ? (size_t)E * ldg : 0);
    ENSURE(pw.Xt, (size_t)D * ldg);
    if (H > 1) ENSURE(pw.pg_A, per_particle * ldg);
    ENSURE(pw.pt_x, (size_t)(H + 1) * PE);
    if (noisy && eps) ENSURE(pw.pt_eps, (size_t)H * PE);
    ENSURE(pw.pt_rew, (size_t)P);
    ENSURE(pw.pt_par, hp.size());
    ENSURE(pw.pg_lam, (size_t)2 * E * ldg);
    ENSURE(pw.pg_ds, (size_t)std::max(U, 1) * ldg);
    ENSURE(pw.pg_part, (size_t)nblk * std::max(Q, 1));
    ENSURE(pw.pg_rew, (size_t)H * nblk);
    ENSURE(pw.pg_out, hout.size());

    PgReverseArgs ra{};
    ParticleFnJacArgs ja{};
    ParticleFnArgs& fa = ja.f;
    size_t off = 0;
    stage_policy(ctx, policy, hp, off, pw.pt_par.p, ra.pol);
    fa.n_rewards = ra.n_rewards = n_rewards;
    stage_rewards(rewards, n_rewards, E, hp, off, pw.pt_par.p, fa.rw);
    for (int i = 0; i < n_rewards; ++i) ra.rw[i] = fa.rw[i];
    ParticleHeadArgs ha = ra.pol;
    // one upload: parameters, initial particles, the caller's draws
    HIPCHK(hipMemcpyAsync(pw.pt_par.p, hp.data(), sizeof(double) * hp.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pw.pt_x.p, x0, sizeof(double) * PE, hipMemcpyHostToDevice, st));
    if (noisy && eps) HIPCHK(hipMemcpyAsync(pw.pt_eps.p, eps, sizeof(double) * H * PE, hipMemcpyHostToDevice, st));
    if (Q > 0) HIPCHK(hipMemsetAsync(pw.pg_part.p, 0, sizeof(double) * nblk * Q, st));
    if (int r = fn_setup(ctx, pl, draws, draws_out, seed)) return r;

    fa.E = E; fa.D = D; fa.N = pl.N; fa.npad = pl.npad; fa.L = pl.L; fa.Lpad = pl.Lpad; fa.P = P; fa.Ppad = Ppad; fa.seed = seed;
    fa.Xq = pw.Xt.p; fa.ldq = ldg; fa.Xt = s.Xt.p; fa.ls = s.ls.p; fa.sf2 = s.var.p;
    fa.noise = noisy ? s.noise.p : nullptr;
    fa.om = pw.fn_om.p; fa.ph = pw.fn_ph.p; fa.Wt = pw.fn_Wt.p; fa.V = pw.fn_V.p;
    fa.rew = pw.pt_rew.p;
    ja.j.ldg = ldg;
    PgParamArgs pa{};
    pa.ds = ra.ds = pw.pg_ds.p; pa.part = pw.pg_part.p; pa.ldg = ra.ldg = ldg; pa.Q = Q;
    auto slab = [&](int t) { return pw.pt_x.p + (size_t)t * PE; };
    ha.Xt = pw.Xt.p; ha.ldt = ldg;
    for (int g0 = 0; g0 < P; g0 += Pg) {
        const int ng = std::min(Pg, P - g0), nbg = (ng + PT_BLOCK - 1) / PT_BLOCK;
        ha.p0 = fa.p0 = g0; ha.ntc = ng;
        for (int t = 0; t < H; ++t) {
            ha.x = fa.x = slab(t);
            fa.xn = slab(t + 1);
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
            launch_pg_reward_partials(st, pw.pt_rew.p, pw.pg_rew.p, P, g0 / PT_BLOCK, nbg, t, H);
        }
        ra.pol.p0 = g0; ra.pol.ntc = ng;
        for (int t = H - 1; t >= 0; --t) {
            const int in = (H - 1 - t) & 1;
            ra.pol.x = slab(t);
            ra.A = t < H - 1 ? pw.pg_A.p + (size_t)t * E * D * ldg : nullptr;
            ra.lam_in = pw.pg_lam.p + (size_t)in * E * ldg;
            ra.lam_out = pw.pg_lam.p + (size_t)(in ^ 1) * E * ldg;
            launch_pg_reverse(st, ra);
            if (Q > 0 && t < H - 1) {
                pa.pol = ra.pol;
                launch_pg_param_partials(st, pa);
            }
        }
        HIPCHK(hipGetLastError());
        if (dreturn_dx0) {   // lam_0, [E][ldg]: the group's download and synchronisation
            const double* lam0 = pw.pg_lam.p + (size_t)(H & 1) * E * ldg;
            HIPCHK(hipMemcpyAsync(hlam.data(), lam0, sizeof(double) * E * ldg, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (int l = 0; l < ng; ++l)
                for (int e = 0; e < E; ++e) dreturn_dx0[(size_t)(g0 + l) * E + e] = hlam[(size_t)e * ldg + l];
        }
    }
    // the steps' rewards in the block order of pilco_rollout_particles_fn's statistics, and the parameter sums: one download
    launch_pg_finish(st, pw.pg_rew.p, pw.pg_out.p, nblk, H, P);
    if (Q > 0) launch_pg_finish(st, pw.pg_part.p, pw.pg_out.p + H, nblk, Q, P);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hout.data(), pw.pg_out.p, sizeof(double) * hout.size(), hipMemcpyDeviceToHost, st));
    if (int r = fn_draws_download(ctx, pl, draws_out, stage)) return r;
    HIPCHK(hipStreamSynchronize(st));
    fn_draws_finish(pl, draws, draws_out, stage);
    double total = 0.0;
    for (int t = 0; t < H; ++t) total += hout[t];   // J: the steps' rewards added in step order
    *reward = total;
    if (reward_steps) memcpy(reward_steps, hout.data(), sizeof(double) * H);
    std::copy(hout.begin() + H, hout.end(), par.begin());
    return PILCO_OK;
}

// the refusals of both entry points, before any launch or upload: those of the marginal gradient, then those of the
// function-sample rollout about the slot, the draws and the budget
int check_fn_grad_call(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards, const double* x0, int P,
                       int H, const double* reward, bool rbf, const pilco_function_draws* draws, FnPlan& pl) {
    if (int r = check_particle_grad_call(ctx, "rollout_particles_fn_grad", policy, rewards, n_rewards, x0, P, H, reward, rbf)) return r;
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
    if (int r = check_fn_grad_call(ctx, policy, rewards, n_rewards, x0, P, H, reward, false, draws, pl)) return r;
    if (policy->kind == PILCO_POLICY_LINEAR && (!dW || !db)) return fail(ctx, PILCO_E_SHAPE, "rollout_particles_fn_grad: null dW or db");
    std::vector<double> par;
    if (int r = rollout_particles_fn_grad(ctx, pl, policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, draws, draws_out,
                                          reward, reward_steps, par, dreturn_dx0))
        return r;
    if (policy->kind == PILCO_POLICY_LINEAR) {
        const size_t UE = (size_t)policy->control_dim * policy->state_dim;
        memcpy(dW, par.data(), sizeof(double) * UE);
        memcpy(db, par.data() + UE, sizeof(double) * policy->control_dim);
    }
    return PILCO_OK;
}

extern "C" int pilco_rollout_particles_fn_grad_rbf(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards,
                                                   int n_rewards, const double* x0, int P, int H, const double* eps,
                                                   unsigned long long seed, int observation_noise, const pilco_function_draws* draws,
                                                   const pilco_function_draws_out* draws_out, const double* Xp, const double* Yp,
                                                   const double* lsp, const double* noisep, int bf, double* reward,
                                                   double* reward_steps, double* dX, double* dY, double* dls, double* dreturn_dx0) {
    if (!ctx) return PILCO_E_SHAPE;
    FnPlan pl{};
    if (int r = check_fn_grad_call(ctx, policy, rewards, n_rewards, x0, P, H, reward, true, draws, pl)) return r;
    if (!Xp || !Yp || !lsp || !noisep || !dX || !dY || !dls)
        return fail(ctx, PILCO_E_SHAPE, "rollout_particles_fn_grad_rbf: null policy parameters or null dX, dY or dls");
    if (bf != ctx->slot[PILCO_SLOT_POLICY].N)
        return fail(ctx, PILCO_E_SHAPE, "rollout_particles_fn_grad_rbf: bf is not the number of points of the policy slot");
    const int E = policy->state_dim, U = policy->control_dim;
    if (!rbf_solve_adjoint(bf, E, U, Xp, Yp, lsp, noisep, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return fail(ctx, PILCO_E_NOT_PD, "rollout_particles_fn_grad_rbf: K + noise I of the policy is singular");
    std::vector<double> par;
    if (int r = rollout_particles_fn_grad(ctx, pl, policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, draws, draws_out,
                                          reward, reward_steps, par, dreturn_dx0))
        return r;
    // dbeta (U,bf) | dC (bf,E) | dl (U,E): dbeta through beta_k = (K_k + noise_k I)^-1 Y_k into dY, dX and dls
    const double *dbeta = par.data(), *dC = dbeta + (size_t)U * bf, *dl = dC + (size_t)bf * E;
    rbf_solve_adjoint(bf, E, U, Xp, Yp, lsp, noisep, dC, dl, dbeta, dX, dY, dls);
    return PILCO_OK;
}
