// Particle rollouts on posterior function samples: pilco_rollout_particles_fn.  docs/particle_functions.md.
// pilco_rollout_particles moves a particle by an independent marginal draw per step; here particle p draws ONE dynamics
// function f_p from the GP posterior -- pathwise conditioning (Matheron's rule) on a random-Fourier-feature prior, exact GP
// only -- and rolls it out deterministically.  With xt = [x, u] in R^D, output e, L features, N training points:
//   phi_el(xt) = A_e cos(omega_el . xt + b_el),  A_e = sqrt(2 var_e / L),  omega_eld = z_eld / lengthscale_ed,  b_el = 2 pi u
//   r_pe = y_e - Phi_e(X) w_pe - sqrt(noise_e) xi_pe,      v_pe = iK_e r_pe
//   f_pe(xt) = sum_l w_pel phi_el(xt) + sum_i k_e(xt, X_i) v_pei,      x'_e = x_e + f_pe(xt) [+ sqrt(noise_e) eps[t][p][e]]
// SET-UP, once per call (particles along the fast axis everywhere, Ppad / Lpad / npad = P / L / N rounded up to 64):
//   k_fn_features   omega [E][L][D], phase [E][L] from the stream (philox_normal.h, domains 1 and 2) -- or the caller's, uploaded
//   k_fn_weights    Wt [E][Lpad][Ppad]: generated (domain 3) or the caller's w transposed; zero past L and past P
//   k_fn_phix       Phi(X) [E][npad][Lpad] over the slot's Xt; zero past N and past L
//   launch_gemm     R = Phi(X) Wt                      [E][npad][Ppad]   (full K: column p depends on column p of Wt only)
//   k_fn_resid      R = (Y - R) - sqrt(noise) xi, xi generated in place (domain 4) or the caller's; zero past N and past P
//   launch_gemm     V = iK R                           [E][npad][Ppad]
// STEP, once per step:
//   k_particle_head (particles.hip)  the actions and the transposed block [x, u] of ALL particles (ldt = Ppad)
//   k_particle_fn_step               f, the update, the optional noise draw, the reward of the pre-step state
//   the statistics and event launches of every forward rollout (ParticleFrame::state, particle_frame.hip)
// k_particle_fn_step: a workgroup of FN_WAVES = 8 waves owns 64 particles (one per lane) and ONE output e.  The training points, then
// the features, are walked in tiles of FN_TILE = 64 staged through LDS (points [i][D], frequencies [l][D], phases [l]: every
// lane of a wave reads the same word, a broadcast); V and Wt are read straight from memory, 64 consecutive particles of one
// row per wave, each word once.  ORDER OF THE SUMS: wave w takes the indices 8 w .. 8 w + 7 of every tile, tiles in
// ascending order, indices in ascending order, one fused multiply-add per term into the wave's two sums
//   sK_w = sum_i exp(-1/2 sum_d ((xt_d - X_id) / l_d)^2) v_i,        sF_w = sum_l w_l cos(b_l + sum_d omega_ld xt_d)
// (d ascending inside either); then K = (((sK_0 + sK_1) + sK_2) + ..) + sK_7, F likewise, f = fma(A, F, var K).  No cross-covariance
// goes to memory, no floating-point atomics; nothing of a particle's arithmetic looks at another lane.
#include "particle_events.h"
#include "particles_fn.h"

#include <cstdlib>

namespace pilco {

constexpr size_t FN_BUDGET = size_t(1) << 29;   // doubles of weights, residuals and V

struct FnSetupArgs {
    double *om, *ph;          // [E][L][D], [E][L]
    double* Wt;               // [E][Lpad][Ppad]
    double* PhiX;             // [E][npad][Lpad]
    double* R;                // [E][npad][Ppad]
    double* xi_out;           // [E][npad][Ppad] the noise draws used, or nullptr
    const double *w_in, *xi_in;   // the caller's [P][E][L], [P][E][N], or nullptr: generated
    const double *Xt, *Yt;    // slot: [D][npad], [E][npad]
    const double *ls, *sf2, *noise;   // [E][D], [E], [E]
    unsigned long long seed;
    int E, D, N, npad, L, Lpad, P, Ppad;
};

__global__ __launch_bounds__(256) void k_fn_features(FnSetupArgs a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.E * a.L) return;
    const int e = idx / a.L, l = idx - e * a.L, D = a.D;
    for (int j = 0; 2 * j < D; ++j) {
        double z[2];
        philox_domain_normal_pair(a.seed, (uint32_t)l, (uint32_t)e, (uint32_t)j, PHILOX_FN_FREQ, &z[0], &z[1]);
        for (int h = 0; h < 2 && 2 * j + h < D; ++h) a.om[(long)idx * D + 2 * j + h] = z[h] / a.ls[e * D + 2 * j + h];
    }
    a.ph[idx] = philox_fn_phase(a.seed, (uint32_t)l, (uint32_t)e);
}

// grid (Ppad / 256 rounded up, Lpad): thread p of row l writes Wt[e][l][p] of every output
__global__ __launch_bounds__(256) void k_fn_weights(FnSetupArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y, E = a.E;
    if (p >= a.Ppad) return;
    const bool live = p < a.P && l < a.L;
    for (int j = 0; 2 * j < E; ++j) {
        double z[2] = {0.0, 0.0};
        if (live && !a.w_in) philox_domain_normal_pair(a.seed, (uint32_t)p, (uint32_t)l, (uint32_t)j, PHILOX_FN_WEIGHT, &z[0], &z[1]);
        for (int h = 0; h < 2 && 2 * j + h < E; ++h) {
            const int e = 2 * j + h;
            if (live && a.w_in) z[h] = a.w_in[((long)p * E + e) * a.L + l];
            a.Wt[((long)e * a.Lpad + l) * a.Ppad + p] = z[h];
        }
    }
}

// grid (npad * Lpad / 256, E): Phi(X)[e][i][l] = A_e cos(b_el + sum_d omega_eld X_id)
__global__ __launch_bounds__(256) void k_fn_phix(FnSetupArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int e = blockIdx.y, i = (int)(idx / a.Lpad), l = (int)(idx - (long)i * a.Lpad);
    if (i >= a.npad) return;
    double v = 0.0;
    if (i < a.N && l < a.L) {
        const double* om = a.om + ((long)e * a.L + l) * a.D;
        double arg = a.ph[e * a.L + l];
        for (int d = 0; d < a.D; ++d) arg = fma(om[d], a.Xt[(long)d * a.npad + i], arg);
        v = sqrt(2.0 * a.sf2[e] / (double)a.L) * cos(arg);
    }
    a.PhiX[((long)e * a.npad + i) * a.Lpad + l] = v;
}

// grid (Ppad / 256 rounded up, npad): thread p of row i: R[e][i][p] = (y_ei - R[e][i][p]) - sqrt(noise_e) xi_pei
__global__ __launch_bounds__(256) void k_fn_resid(FnSetupArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, E = a.E;
    if (p >= a.Ppad) return;
    const bool live = p < a.P && i < a.N;
    for (int j = 0; 2 * j < E; ++j) {
        double z[2] = {0.0, 0.0};
        if (live && !a.xi_in) philox_domain_normal_pair(a.seed, (uint32_t)p, (uint32_t)i, (uint32_t)j, PHILOX_FN_XI, &z[0], &z[1]);
        for (int h = 0; h < 2 && 2 * j + h < E; ++h) {
            const int e = 2 * j + h;
            const long at = ((long)e * a.npad + i) * a.Ppad + p;
            if (live && a.xi_in) z[h] = a.xi_in[((long)p * E + e) * a.N + i];
            a.R[at] = live ? (a.Yt[(long)e * a.npad + i] - a.R[at]) - sqrt(a.noise[e]) * z[h] : 0.0;
            if (a.xi_out) a.xi_out[at] = z[h];
        }
    }
}

// grid (columns / 64, E), FN_WAVES waves: see the head of this file; the body is fn_step_body (particles_fn.h), shared with
// k_particle_fn_step_jac.  DM: the register build, D <= DM
template <int DM>
__global__ __launch_bounds__(64 * FN_WAVES) void k_particle_fn_step(ParticleFnArgs a) {
    __shared__ FnStepLds<DM, false> sh;
    fn_step_body<DM, false>(a, ParticleFnJac{}, sh);
}

}  // namespace pilco

using namespace pilco;

namespace {

size_t fn_budget() {
    if (const char* v = getenv("PILCO_PARTICLE_FN_BUDGET")) {
        const long long n = atoll(v);
        if (n > 0) return (size_t)n;
    }
    return FN_BUDGET;
}

// [E][rows_pad][Ppad] on the device's side -> the caller's [P][E][rows]
void fn_untranspose(const std::vector<double>& dev, double* out, int E, int rows, int rows_pad, int P, int Ppad) {
    for (int p = 0; p < P; ++p)
        for (int e = 0; e < E; ++e)
            for (int i = 0; i < rows; ++i) out[((size_t)p * E + e) * rows + i] = dev[((size_t)e * rows_pad + i) * Ppad + p];
}

}  // namespace

void launch_fn_step(hipStream_t st, const ParticleFnArgs& a, int count) {
    const dim3 grid(round_up(count, 64) / 64, a.E), block(64 * FN_WAVES);
    if (a.D <= 4) hipLaunchKernelGGL(k_particle_fn_step<4>, grid, block, 0, st, a);
    else if (a.D <= 8) hipLaunchKernelGGL(k_particle_fn_step<8>, grid, block, 0, st, a);
    else if (a.D <= 12) hipLaunchKernelGGL(k_particle_fn_step<12>, grid, block, 0, st, a);
    else if (a.D <= 16) hipLaunchKernelGGL(k_particle_fn_step<16>, grid, block, 0, st, a);
    else if (a.D <= 24) hipLaunchKernelGGL(k_particle_fn_step<24>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_particle_fn_step<MAX_D>, grid, block, 0, st, a);
}

int fn_plan(pilco_ctx* ctx, const char* who, const pilco_function_draws* draws, int P, FnPlan& pl) {
    const Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    const std::string pre = std::string(who) + ": ";
    if (s.M > 0) return fail(ctx, PILCO_E_STATE, pre + "the slot is sparse (FITC, M > 0); function samples need an exact GP");
    if (!draws) return fail(ctx, PILCO_E_SHAPE, pre + "null draws");
    const int L = draws->L;
    if (L < 1 || L > PILCO_MAX_FN_FEATURES) return fail(ctx, PILCO_E_SHAPE, pre + "L must be in 1..4096");
    const int given = (draws->omega != nullptr) + (draws->phase != nullptr) + (draws->w != nullptr) + (draws->xi != nullptr);
    if (given != 0 && given != 4) return fail(ctx, PILCO_E_SHAPE, pre + "omega, phase, w and xi are given together or not at all");
    pl.own = given == 4;
    pl.E = s.E; pl.D = s.D; pl.N = s.N; pl.npad = s.Npad; pl.L = L; pl.Lpad = round_up(L, 64); pl.P = P; pl.Ppad = round_up(P, 64);
    const size_t per_p = (size_t)pl.E * ((size_t)pl.Lpad + 2 * (size_t)pl.npad), budget = fn_budget();
    if (per_p * pl.Ppad > budget) {
        const long long fit = (long long)(budget / per_p / 64 * 64);
        return fail(ctx, PILCO_E_SHAPE, pre + "E Ppad (Lpad + 2 npad) = " + std::to_string(per_p * pl.Ppad) +
                                            " doubles exceed the budget of " + std::to_string(budget) +
                                            " (PILCO_PARTICLE_FN_BUDGET); the largest P that fits is " + std::to_string(fit));
    }
    pl.n_om = (size_t)pl.E * L * pl.D; pl.n_ph = (size_t)pl.E * L;
    pl.n_w = (size_t)P * pl.E * L; pl.n_xi = (size_t)P * pl.E * pl.N;
    pl.n_Wt = (size_t)pl.E * pl.Lpad * pl.Ppad; pl.n_V = (size_t)pl.E * pl.npad * pl.Ppad;
    return PILCO_OK;
}

int fn_setup(pilco_ctx* ctx, const FnPlan& pl, const pilco_function_draws* draws, const pilco_function_draws_out* draws_out,
             unsigned long long seed) {
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    PredictWork& pw = *s.pred;
    hipStream_t st = ctx->st;
    const int E = pl.E, D = pl.D, N = pl.N, npad = pl.npad, L = pl.L, Lpad = pl.Lpad, P = pl.P, Ppad = pl.Ppad;
    const bool own = pl.own, want_xi = draws_out && draws_out->xi && !own;
    ENSURE(pw.fn_om, pl.n_om);
    ENSURE(pw.fn_ph, pl.n_ph);
    ENSURE(pw.fn_Wt, pl.n_Wt);
    ENSURE(pw.fn_phix, (size_t)E * npad * Lpad);
    ENSURE(pw.fn_R, pl.n_V);
    ENSURE(pw.fn_V, pl.n_V);
    if (want_xi) ENSURE(pw.fn_xi, pl.n_V);
    if (own) {
        ENSURE(pw.fn_raw, pl.n_w + pl.n_xi);
        HIPCHK(hipMemcpyAsync(pw.fn_om.p, draws->omega, sizeof(double) * pl.n_om, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(pw.fn_ph.p, draws->phase, sizeof(double) * pl.n_ph, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(pw.fn_raw.p, draws->w, sizeof(double) * pl.n_w, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(pw.fn_raw.p + pl.n_w, draws->xi, sizeof(double) * pl.n_xi, hipMemcpyHostToDevice, st));
    }
    // set-up: features, weights, residuals, V
    FnSetupArgs ua{};
    ua.om = pw.fn_om.p; ua.ph = pw.fn_ph.p; ua.Wt = pw.fn_Wt.p; ua.PhiX = pw.fn_phix.p; ua.R = pw.fn_R.p;
    ua.xi_out = want_xi ? pw.fn_xi.p : nullptr;
    ua.w_in = own ? pw.fn_raw.p : nullptr;
    ua.xi_in = own ? pw.fn_raw.p + pl.n_w : nullptr;
    ua.Xt = s.Xt.p; ua.Yt = s.Yt.p; ua.ls = s.ls.p; ua.sf2 = s.var.p; ua.noise = s.noise.p;
    ua.seed = seed; ua.E = E; ua.D = D; ua.N = N; ua.npad = npad; ua.L = L; ua.Lpad = Lpad; ua.P = P; ua.Ppad = Ppad;
    if (!own) hipLaunchKernelGGL(k_fn_features, dim3((E * L + 255) / 256), dim3(256), 0, st, ua);
    hipLaunchKernelGGL(k_fn_weights, dim3((Ppad + 255) / 256, Lpad), dim3(256), 0, st, ua);
    hipLaunchKernelGGL(k_fn_phix, dim3((unsigned)(((long)npad * Lpad + 255) / 256), E), dim3(256), 0, st, ua);
    GemmDesc g{};
    g.alpha = 1.0; g.beta = 0.0;
    g.A = pw.fn_phix.p; g.lda = Lpad; g.sA = (long)npad * Lpad;
    g.B = pw.fn_Wt.p; g.ldb = Ppad; g.sB = (long)Lpad * Ppad;
    g.C = pw.fn_R.p; g.ldc = Ppad; g.sC = (long)npad * Ppad;
    g.M = npad; g.N = Ppad; g.K = Lpad;
    launch_gemm(st, g, false, false, E);
    hipLaunchKernelGGL(k_fn_resid, dim3((Ppad + 255) / 256, npad), dim3(256), 0, st, ua);
    g.A = s.iK.p; g.lda = npad; g.sA = (long)npad * npad;
    g.B = pw.fn_R.p; g.ldb = Ppad; g.sB = (long)npad * Ppad;
    g.C = pw.fn_V.p;
    g.K = npad;
    launch_gemm(st, g, false, false, E);
    return PILCO_OK;
}

int fn_draws_download(pilco_ctx* ctx, const FnPlan& pl, const pilco_function_draws_out* draws_out, FnDrawsStage& stage) {
    if (!draws_out) return PILCO_OK;
    PredictWork& pw = *ctx->slot[PILCO_SLOT_DYNAMICS].pred;
    hipStream_t st = ctx->st;
    if (draws_out->omega) HIPCHK(hipMemcpyAsync(draws_out->omega, pw.fn_om.p, sizeof(double) * pl.n_om, hipMemcpyDeviceToHost, st));
    if (draws_out->phase) HIPCHK(hipMemcpyAsync(draws_out->phase, pw.fn_ph.p, sizeof(double) * pl.n_ph, hipMemcpyDeviceToHost, st));
    if (draws_out->w && !pl.own) {
        stage.w.resize(pl.n_Wt);
        HIPCHK(hipMemcpyAsync(stage.w.data(), pw.fn_Wt.p, sizeof(double) * pl.n_Wt, hipMemcpyDeviceToHost, st));
    }
    if (draws_out->xi && !pl.own) {
        stage.xi.resize(pl.n_V);
        HIPCHK(hipMemcpyAsync(stage.xi.data(), pw.fn_xi.p, sizeof(double) * pl.n_V, hipMemcpyDeviceToHost, st));
    }
    if (draws_out->v) {
        stage.v.resize(pl.n_V);
        HIPCHK(hipMemcpyAsync(stage.v.data(), pw.fn_V.p, sizeof(double) * pl.n_V, hipMemcpyDeviceToHost, st));
    }
    return PILCO_OK;
}

void fn_draws_finish(const FnPlan& pl, const pilco_function_draws* draws, const pilco_function_draws_out* draws_out,
                     const FnDrawsStage& stage) {
    if (!draws_out) return;
    if (draws_out->w) {
        if (pl.own) memcpy(draws_out->w, draws->w, sizeof(double) * pl.n_w);
        else fn_untranspose(stage.w, draws_out->w, pl.E, pl.L, pl.Lpad, pl.P, pl.Ppad);
    }
    if (draws_out->xi) {
        if (pl.own) memcpy(draws_out->xi, draws->xi, sizeof(double) * pl.n_xi);
        else fn_untranspose(stage.xi, draws_out->xi, pl.E, pl.N, pl.npad, pl.P, pl.Ppad);
    }
    if (draws_out->v) fn_untranspose(stage.v, draws_out->v, pl.E, pl.N, pl.npad, pl.P, pl.Ppad);
}

extern "C" int pilco_rollout_particles_fn(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                          const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                          int observation_noise, double* mean, double* cov, double* reward_steps, double* particles,
                                          double* eps_out, const pilco_event* events, int n_events, long long* counts,
                                          int* first_hit, const pilco_function_draws* draws, const pilco_function_draws_out* draws_out) {
    const bool noisy = observation_noise != 0;
    FnDrawsStage stage;   // (before the frame, which drains the stream when it leaves)
    ParticleFrame f{ctx, {policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, mean, cov, reward_steps, particles, eps_out,
                          events, n_events, counts, first_hit}};
    if (int r = f.check("rollout_particles_fn")) return r;
    FnPlan pl{};
    if (int r = fn_plan(ctx, "rollout_particles_fn", draws, P, pl)) return r;
    const int E = f.E, D = f.D, Ppad = pl.Ppad;
    const size_t PE = f.PE;
    const bool keep_eps = noisy && H > 0 && (eps || eps_out);
    ParticleFnArgs fa{};
    if (int r = f.open(particles ? H + 1 : 2, keep_eps ? (size_t)H * PE : 0, fa.rw)) return r;
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    PredictWork& pw = *f.work;
    hipStream_t st = f.st;
    ENSURE(pw.Xt, (size_t)D * Ppad);
    ENSURE(pw.pt_rew, (size_t)P);
    if (int r = f.upload()) return r;
    if (int r = fn_setup(ctx, pl, draws, draws_out, seed)) return r;

    ParticleHeadArgs& ha = f.ha;
    fa.n_rewards = n_rewards;
    fa.E = E; fa.D = D; fa.N = pl.N; fa.npad = pl.npad; fa.L = pl.L; fa.Lpad = pl.Lpad; fa.P = P; fa.Ppad = Ppad; fa.seed = seed;
    fa.Xq = pw.Xt.p; fa.ldq = Ppad; fa.Xt = s.Xt.p; fa.ls = s.ls.p; fa.sf2 = s.var.p;
    fa.noise = noisy ? s.noise.p : nullptr;
    fa.om = pw.fn_om.p; fa.ph = pw.fn_ph.p; fa.Wt = pw.fn_Wt.p; fa.V = pw.fn_V.p;
    fa.rew = pw.pt_rew.p;
    if (int r = f.state(0, nullptr)) return r;
    ha.Xt = pw.Xt.p; ha.p0 = 0; ha.ntc = P; ha.ldt = Ppad;
    for (int t = 0; t < H; ++t) {
        ha.x = fa.x = f.slab(t);
        fa.xn = f.slab(t + 1);
        fa.t = t;
        fa.eps_in = (noisy && eps) ? pw.pt_eps.p + (size_t)t * PE : nullptr;
        fa.eps_out = (noisy && !eps && eps_out) ? pw.pt_eps.p + (size_t)t * PE : nullptr;
        launch_particle_head(st, ha);
        launch_fn_step(st, fa, P);
        if (int r = f.state(t + 1, pw.pt_rew.p)) return r;
    }
    // one download, one synchronisation
    if (int r = f.download(particles, (noisy && !eps) ? eps_out : nullptr)) return r;
    if (int r = f.download_events(counts, first_hit)) return r;
    if (int r = fn_draws_download(ctx, pl, draws_out, stage)) return r;
    HIPCHK(hipStreamSynchronize(st));
    if (noisy && eps_out && eps && H > 0) memcpy(eps_out, eps, sizeof(double) * H * PE);
    fn_draws_finish(pl, draws, draws_out, stage);
    f.finish();
    return PILCO_OK;
}
