// The host frames of the particle entry points (particles.h; docs/particle_frame.md): the checks and the staging of policy
// and rewards, ParticleFrame under pilco_rollout_particles[_events], _fn and _cond, ParticleGradFrame under
// pilco_rollout_particles_grad[_rbf] and _fn_grad[_rbf].  Host code only: no kernel lives here.
#include "particle_events.h"
#include "particles.h"
#include "rbf_solve_adj.h"

using namespace pilco;

// the policy against the dynamics slot (and, RbfController, the policy slot)
int check_policy(pilco_ctx* ctx, const pilco_policy* policy) {
    const Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    if (!policy) return fail(ctx, PILCO_E_SHAPE, "rollout_particles: null policy");
    const int E = s.E, D = s.D, U = D - E;
    if (policy->state_dim != E || policy->control_dim != U || U < 0 || D > MAX_D)
        return fail(ctx, PILCO_E_SHAPE, "rollout_particles: policy dims do not match the model (state_dim must be E, control_dim D-E)");
    if (policy->kind < 0 || policy->kind > PILCO_POLICY_MLP) return fail(ctx, PILCO_E_SHAPE, "rollout_particles: unknown policy kind");
    if (policy->kind == PILCO_POLICY_NONE && U != 0) return fail(ctx, PILCO_E_SHAPE, "rollout_particles: policy NONE needs D == E");
    if (policy->kind != PILCO_POLICY_NONE && U == 0) return fail(ctx, PILCO_E_SHAPE, "rollout_particles: a policy needs control_dim > 0");
    if (policy->kind == PILCO_POLICY_LINEAR && (!policy->W || !policy->b))
        return fail(ctx, PILCO_E_SHAPE, "rollout_particles: linear policy needs W and b");
    if (policy->kind == PILCO_POLICY_RBF) {
        const Slot& ps = ctx->slot[PILCO_SLOT_POLICY];
        if (!ps.factor_valid || ps.M > 0) return fail(ctx, PILCO_E_STATE, "rollout_particles: RBF policy slot has no current (exact) factorisation");
        if (ps.D != E || ps.E != U) return fail(ctx, PILCO_E_SHAPE, "rollout_particles: RBF policy GP must map state_dim -> control_dim");
    }
    if (policy->kind == PILCO_POLICY_MLP) {
        if (ctx->mlp.Hn == 0) return fail(ctx, PILCO_E_STATE, "rollout_particles: MLP policy needs pilco_set_policy_mlp first");
        if (ctx->mlp.E != E || ctx->mlp.U != U) return fail(ctx, PILCO_E_SHAPE, "rollout_particles: the MLP policy must map state_dim -> control_dim");
    }
    return PILCO_OK;
}

// the policy's parameters into the staging vector hp (W[U*E] b[U] maxact[U]; MLP policy: W1 b1 W2 b2 maxact[U]) and the action
// kernel's arguments; dev: where hp goes
void stage_policy(pilco_ctx* ctx, const pilco_policy* policy, std::vector<double>& hp, size_t& off, const double* dev,
                  ParticleHeadArgs& ha) {
    const Slot &s = ctx->slot[PILCO_SLOT_DYNAMICS], &ps = ctx->slot[PILCO_SLOT_POLICY];
    const int E = s.E, U = s.D - s.E;
    ha.E = E; ha.U = U; ha.kind = policy->kind; ha.squash = policy->squash;
    if (policy->kind == PILCO_POLICY_LINEAR) {
        memcpy(&hp[off], policy->W, sizeof(double) * U * E);
        ha.W = dev + off; off += (size_t)U * E;
        memcpy(&hp[off], policy->b, sizeof(double) * U);
        ha.b = dev + off; off += U;
    }
    if (policy->kind == PILCO_POLICY_MLP) {
        const int Hn = ctx->mlp.Hn;
        std::copy(ctx->mlp.par.begin(), ctx->mlp.par.end(), hp.begin() + off);
        ha.Hn = Hn;
        ha.W1 = dev + off; ha.b1 = ha.W1 + (size_t)Hn * E; ha.W2 = ha.b1 + Hn; ha.b2 = ha.W2 + (size_t)U * Hn;
        off += ctx->mlp.par.size();
    }
    for (int u = 0; u < U; ++u) hp[off + u] = policy->max_action ? policy->max_action[u] : 1.0;
    ha.maxact = dev + off; off += U;
    if (policy->kind == PILCO_POLICY_RBF) {
        ha.pc = ps.Xt.p; ha.pls = ps.ls.p; ha.pvar = ps.var.p; ha.pbeta = ps.beta.p;
        ha.pn = ps.N; ha.pnpad = ps.Npad;
    }
}

// what pilco_rollout_particles refuses about the slot, the context, P and H
int check_particle_state(pilco_ctx* ctx, int P, int H) {
    if (int r = check_slot(ctx, PILCO_SLOT_DYNAMICS)) return r;
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    if (ctx->nranks != 1 || ctx->comm || s.shW > 1) return fail(ctx, PILCO_E_STATE, "rollout_particles: single rank only");
    if (!s.has_data || !s.has_hyp) return fail(ctx, PILCO_E_STATE, "rollout_particles needs set_data and set_hyp first");
    if (s.user_factors)
        return fail(ctx, PILCO_E_STATE, "rollout_particles: the slot holds factors set by pilco_gp_set_factors, not its own factorisation");
    if (P <= 0 || H < 0) return fail(ctx, PILCO_E_SHAPE, "rollout_particles: P must be positive and H non-negative");
    return PILCO_OK;
}

// ... and about the policy and the reward terms
int check_particle_terms(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards) {
    if (int r = check_policy(ctx, policy)) return r;
    if (n_rewards < 0 || n_rewards > MAX_REWARD_TERMS || (n_rewards > 0 && !rewards))
        return fail(ctx, PILCO_E_SHAPE, "rollout_particles: 0..4 reward terms supported");
    for (int i = 0; i < n_rewards; ++i) {
        if (rewards[i].kind != PILCO_REWARD_EXPONENTIAL && rewards[i].kind != PILCO_REWARD_LINEAR)
            return fail(ctx, PILCO_E_SHAPE, "reward: unknown kind");
        if (!rewards[i].W) return fail(ctx, PILCO_E_SHAPE, "reward: W is required");
    }
    return PILCO_OK;
}

// the reward terms into the staging vector hp and the draw kernel's arguments; dev: where hp goes
void stage_rewards(const pilco_reward_term* rewards, int n_rewards, int E, std::vector<double>& hp, size_t& off, const double* dev,
                   ParticleReward* rw) {
    for (int i = 0; i < n_rewards; ++i) {
        ParticleReward& r = rw[i];
        r.kind = rewards[i].kind;
        r.coef = rewards[i].coef;
        if (r.kind == PILCO_REWARD_EXPONENTIAL) {
            memcpy(&hp[off], rewards[i].W, sizeof(double) * E * E);
            r.W = dev + off; off += (size_t)E * E;
            if (rewards[i].t) memcpy(&hp[off], rewards[i].t, sizeof(double) * E);   // (NULL: the zeros hp holds)
            r.t = dev + off; off += E;
        } else {
            memcpy(&hp[off], rewards[i].W, sizeof(double) * E);
            r.W = dev + off; off += E;
            r.t = r.W;
        }
    }
}

int particle_work(pilco_ctx* ctx, PredictWork*& work) {
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    HIPCHK(hipSetDevice(ctx->device));
    if (!s.factor_valid)
        if (int r = pilco_gp_factorize(ctx, PILCO_SLOT_DYNAMICS)) return r;
    if (!s.pred) s.pred = new PredictWork();
    work = s.pred;
    return PILCO_OK;
}

// ---- the forward frame

int ParticleFrame::check(const char* who) {
    if (int r = check_particle_state(ctx, c.P, c.H)) return r;
    if (!c.x0 || !c.mean || !c.cov) return fail(ctx, PILCO_E_SHAPE, std::string(who) + ": null x0, mean or cov");
    if (int r = check_particle_terms(ctx, c.policy, c.rewards, c.n_rewards)) return r;
    const Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    E = s.E; D = s.D; U = D - E;
    if (const char* why = event_table_refusal(c.events, c.n_events, c.counts, E))
        return fail(ctx, PILCO_E_SHAPE, std::string(who) + ": " + why);
    K = c.n_events; Q = E + E * E + 1; nblk = (c.P + PT_BLOCK - 1) / PT_BLOCK;
    PE = (size_t)c.P * E; fh_bytes = sizeof(int) * (size_t)c.P * K;
    return PILCO_OK;
}

int ParticleFrame::open(int nslab_, size_t eps_doubles_, ParticleReward* rw) {
    st = ctx->st; nslab = nslab_; eps_doubles = eps_doubles_;
    if (int r = particle_work(ctx, work)) return r;
    PredictWork& pw = *work;
    const int P = c.P, H = c.H;
    hp.assign(particle_par_doubles(E, U, policy_mlp_hidden(ctx, c.policy)), 0.0);
    hstats.resize((size_t)(H + 1) * Q);
    ENSURE(pw.pt_x, (size_t)nslab * PE);
    if (eps_doubles) ENSURE(pw.pt_eps, eps_doubles);
    ENSURE(pw.pt_part, (size_t)nblk * Q);
    ENSURE(pw.pt_stats, hstats.size());
    ENSURE(pw.pt_par, hp.size());
    size_t off = 0;
    stage_policy(ctx, c.policy, hp, off, pw.pt_par.p, ha);
    stage_rewards(c.rewards, c.n_rewards, E, hp, off, pw.pt_par.p, rw);
    sa.P = P; sa.E = E; sa.nblk = nblk; sa.part = pw.pt_part.p;
    if (K == 0) return PILCO_OK;
    // the events' integers live in buffers of doubles: first hits [P][K] int, the blocks' counts [nblk][K] int, counts [H+1][K] long long
    if (c.first_hit) ENSURE(pw.pt_ev_first, (fh_bytes + 7) / 8);
    ENSURE(pw.pt_ev_part, (sizeof(int) * (size_t)nblk * K + 7) / 8);
    ENSURE(pw.pt_ev_counts, (size_t)(H + 1) * K);
    ea.P = P; ea.E = E; ea.K = K; ea.nblk = nblk;
    ea.first_hit = c.first_hit ? reinterpret_cast<int*>(pw.pt_ev_first.p) : nullptr;
    ea.part = reinterpret_cast<int*>(pw.pt_ev_part.p);
    for (int k = 0; k < K; ++k) ea.ev[k] = c.events[k];
    return PILCO_OK;
}

int ParticleFrame::upload() {
    PredictWork& pw = *work;
    HIPCHK(hipMemcpyAsync(pw.pt_par.p, hp.data(), sizeof(double) * hp.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pw.pt_x.p, c.x0, sizeof(double) * PE, hipMemcpyHostToDevice, st));
    if (c.eps && c.H > 0 && eps_doubles) HIPCHK(hipMemcpyAsync(pw.pt_eps.p, c.eps, sizeof(double) * c.H * PE, hipMemcpyHostToDevice, st));
    return PILCO_OK;
}

int ParticleFrame::state(int t, const double* rew) {
    if (t == 0 && ea.first_hit) HIPCHK(hipMemsetAsync(ea.first_hit, 0xFF, fh_bytes, st));   // every entry -1
    sa.x = ea.x = slab(t);
    sa.rew = rew;   // (the reward word of state t: the mean reward of the pre-step states of step t - 1)
    sa.out = work->pt_stats.p + (size_t)t * Q;
    launch_particle_stats(st, sa);
    if (K == 0) return PILCO_OK;
    ea.t = t;
    ea.counts = reinterpret_cast<long long*>(work->pt_ev_counts.p) + (size_t)t * K;
    launch_particle_events(st, ea);
    return PILCO_OK;
}

int ParticleFrame::download(double* particles, double* eps_out) {
    PredictWork& pw = *work;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hstats.data(), pw.pt_stats.p, sizeof(double) * hstats.size(), hipMemcpyDeviceToHost, st));
    if (particles) HIPCHK(hipMemcpyAsync(particles, pw.pt_x.p, sizeof(double) * (c.H + 1) * PE, hipMemcpyDeviceToHost, st));
    if (eps_out && c.H > 0) HIPCHK(hipMemcpyAsync(eps_out, pw.pt_eps.p, sizeof(double) * c.H * PE, hipMemcpyDeviceToHost, st));
    return PILCO_OK;
}

int ParticleFrame::download_events(long long* counts, int* first_hit) {
    if (K == 0) return PILCO_OK;
    HIPCHK(hipMemcpyAsync(counts, work->pt_ev_counts.p, sizeof(long long) * (c.H + 1) * K, hipMemcpyDeviceToHost, st));
    if (ea.first_hit) HIPCHK(hipMemcpyAsync(first_hit, ea.first_hit, fh_bytes, hipMemcpyDeviceToHost, st));
    return PILCO_OK;
}

void ParticleFrame::finish() {
    for (int t = 0; t <= c.H; ++t) {
        const double* row = &hstats[(size_t)t * Q];
        memcpy(c.mean + (size_t)t * E, row, sizeof(double) * E);
        memcpy(c.cov + (size_t)t * E * E, row + E, sizeof(double) * E * E);
        if (t > 0 && c.reward_steps) c.reward_steps[t - 1] = row[Q - 1];
    }
}

// ---- the gradient frame

// a multiple of PT_BLOCK particles whose matrices fit the budget (at least one block)
PgPlan pg_plan(int P, int H, int E, int D, size_t budget) {
    PgPlan pl{};
    pl.per_particle = (size_t)(H - 1) * E * D;
    pl.Pg = P;
    if (pl.per_particle * (size_t)P > budget)
        pl.Pg = (int)std::min<size_t>((size_t)round_up(P, PT_BLOCK), std::max<size_t>(1, budget / pl.per_particle / PT_BLOCK) * PT_BLOCK);
    pl.ldg = round_up(std::min(pl.Pg, P), 64);
    pl.nblk = (P + PT_BLOCK - 1) / PT_BLOCK;
    return pl;
}

ParticleGradFrame::ParticleGradFrame(pilco_ctx* ctx_, const pilco_policy* policy_, const pilco_reward_term* rewards_, int n_rewards_,
                                     const double* x0_, int P_, int H_, double* dreturn_dx0_, std::vector<double>& par)
    : ctx(ctx_), policy(policy_), rewards(rewards_), n_rewards(n_rewards_), x0(x0_), P(P_), H(H_), dreturn_dx0(dreturn_dx0_) {
    const Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    E = s.E; D = s.D; U = D - E;
    const int bf = policy->kind == PILCO_POLICY_RBF ? ctx->slot[PILCO_SLOT_POLICY].N : policy_mlp_hidden(ctx, policy);
    Q = U > 0 ? pg_quantities(policy->kind, E, U, bf) : 0;
    PE = (size_t)P * E;
    par.assign((size_t)Q, 0.0);
}

int ParticleGradFrame::open(size_t eps_doubles, ParticleReward* rw) {
    if (!work)
        if (int r = attach()) return r;
    PredictWork& pw = *work;
    pl = pg_plan(P, H, E, D, pg_group_budget());
    const int ldg = pl.ldg, nblk = pl.nblk;
    hp.assign(particle_par_doubles(E, U, policy_mlp_hidden(ctx, policy)), 0.0);
    hout.resize((size_t)H + Q);
    hlam.resize(dreturn_dx0 ? (size_t)E * ldg : 0);
    if (H > 1) ENSURE(pw.pg_A, pl.per_particle * ldg);
    ENSURE(pw.pt_x, (size_t)(H + 1) * PE);
    if (eps_doubles) ENSURE(pw.pt_eps, eps_doubles);
    ENSURE(pw.pt_rew, (size_t)P);
    ENSURE(pw.pt_par, hp.size());
    ENSURE(pw.pg_lam, (size_t)2 * E * ldg);
    ENSURE(pw.pg_ds, (size_t)std::max(U, 1) * ldg);
    ENSURE(pw.pg_part, (size_t)nblk * std::max(Q, 1));
    ENSURE(pw.pg_rew, (size_t)H * nblk);
    ENSURE(pw.pg_out, hout.size());
    size_t off = 0;
    stage_policy(ctx, policy, hp, off, pw.pt_par.p, ra.pol);
    ra.n_rewards = n_rewards;
    stage_rewards(rewards, n_rewards, E, hp, off, pw.pt_par.p, rw);
    for (int i = 0; i < n_rewards; ++i) ra.rw[i] = rw[i];
    ha = ra.pol;
    pa.ds = ra.ds = pw.pg_ds.p; pa.part = pw.pg_part.p; pa.ldg = ra.ldg = ldg; pa.Q = Q;
    return PILCO_OK;
}

int ParticleGradFrame::upload(const double* eps) {
    PredictWork& pw = *work;
    HIPCHK(hipMemcpyAsync(pw.pt_par.p, hp.data(), sizeof(double) * hp.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pw.pt_x.p, x0, sizeof(double) * PE, hipMemcpyHostToDevice, st));
    if (eps) HIPCHK(hipMemcpyAsync(pw.pt_eps.p, eps, sizeof(double) * H * PE, hipMemcpyHostToDevice, st));
    if (Q > 0) HIPCHK(hipMemsetAsync(pw.pg_part.p, 0, sizeof(double) * pl.nblk * Q, st));
    return PILCO_OK;
}

int ParticleGradFrame::sweep(const std::function<int(int, int, int)>& step) {
    PredictWork& pw = *work;
    const int ldg = pl.ldg;
    for (int g0 = 0; g0 < P; g0 += pl.Pg) {
        const int ng = std::min(pl.Pg, P - g0), nbg = (ng + PT_BLOCK - 1) / PT_BLOCK;
        for (int t = 0; t < H; ++t) {
            if (int r = step(g0, ng, t)) return r;
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
    return PILCO_OK;
}

// the rewards of the steps in the block order of the forward rollouts' statistics (k_particle_finish), and the parameter sums
int ParticleGradFrame::finish_enqueue() {
    PredictWork& pw = *work;
    launch_pg_finish(st, pw.pg_rew.p, pw.pg_out.p, pl.nblk, H, P);
    if (Q > 0) launch_pg_finish(st, pw.pg_part.p, pw.pg_out.p + H, pl.nblk, Q, P);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hout.data(), pw.pg_out.p, sizeof(double) * hout.size(), hipMemcpyDeviceToHost, st));
    return PILCO_OK;
}

void ParticleGradFrame::finish(double* reward, double* reward_steps, std::vector<double>& par) {
    double total = 0.0;
    for (int t = 0; t < H; ++t) total += hout[t];   // J: the steps' rewards added in step order
    *reward = total;
    if (reward_steps) memcpy(reward_steps, hout.data(), sizeof(double) * H);
    std::copy(hout.begin() + H, hout.end(), par.begin());
}

int pg_linear_entry(pilco_ctx* ctx, const char* who, const pilco_policy* policy, double* dW, double* db, const PgRollout& rollout) {
    const bool linear = policy->kind == PILCO_POLICY_LINEAR;
    if (linear && (!dW || !db)) return fail(ctx, PILCO_E_SHAPE, std::string(who) + ": null dW or db");
    std::vector<double> par;
    if (int r = rollout(par)) return r;
    if (linear) {
        const size_t UE = (size_t)policy->control_dim * policy->state_dim;
        memcpy(dW, par.data(), sizeof(double) * UE);
        memcpy(db, par.data() + UE, sizeof(double) * policy->control_dim);
    }
    return PILCO_OK;
}

int pg_mlp_entry(pilco_ctx* ctx, const char* who, const pilco_policy* policy, double* dW1, double* db1, double* dW2, double* db2,
                 const PgRollout& rollout) {
    if (!dW1 || !db1 || !dW2 || !db2) return fail(ctx, PILCO_E_SHAPE, std::string(who) + "_mlp: null dW1, db1, dW2 or db2");
    std::vector<double> par;
    if (int r = rollout(par)) return r;
    // dW1 (Hn,E) | db1 (Hn) | dW2 (U,Hn) | db2 (U)
    const size_t Hn = (size_t)ctx->mlp.Hn, E = (size_t)policy->state_dim, U = (size_t)policy->control_dim;
    const double* q = par.data();
    memcpy(dW1, q, sizeof(double) * Hn * E); q += Hn * E;
    memcpy(db1, q, sizeof(double) * Hn); q += Hn;
    memcpy(dW2, q, sizeof(double) * U * Hn); q += U * Hn;
    memcpy(db2, q, sizeof(double) * U);
    return PILCO_OK;
}

// the network of PILCO_POLICY_MLP: a host copy, staged into every call's parameter upload by stage_policy
extern "C" int pilco_set_policy_mlp(pilco_ctx* ctx, int state_dim, int control_dim, int hidden, const double* W1, const double* b1,
                                    const double* W2, const double* b2) {
    if (!ctx) return PILCO_E_SHAPE;
    if (hidden < 1 || hidden > PILCO_MAX_MLP_HIDDEN) return fail(ctx, PILCO_E_SHAPE, "set_policy_mlp: hidden must be 1..256");
    if (state_dim < 1 || control_dim < 1 || state_dim + control_dim > MAX_D)
        return fail(ctx, PILCO_E_SHAPE, "set_policy_mlp: state_dim and control_dim must be positive, their sum at most 32");
    if (!W1 || !b1 || !W2 || !b2) return fail(ctx, PILCO_E_SHAPE, "set_policy_mlp: null W1, b1, W2 or b2");
    const size_t E = (size_t)state_dim, U = (size_t)control_dim, Hn = (size_t)hidden;
    std::vector<double> par(Hn * (E + 1) + U * (Hn + 1));
    double* q = par.data();
    memcpy(q, W1, sizeof(double) * Hn * E); q += Hn * E;
    memcpy(q, b1, sizeof(double) * Hn); q += Hn;
    memcpy(q, W2, sizeof(double) * U * Hn); q += U * Hn;
    memcpy(q, b2, sizeof(double) * U);
    ctx->mlp.par.swap(par);
    ctx->mlp.E = state_dim; ctx->mlp.U = control_dim; ctx->mlp.Hn = hidden;
    return PILCO_OK;
}

int pg_rbf_entry(pilco_ctx* ctx, const char* who, const pilco_policy* policy, const double* Xp, const double* Yp, const double* lsp,
                 const double* noisep, int bf, double* dX, double* dY, double* dls, const PgRollout& rollout) {
    const std::string pre = std::string(who) + "_rbf: ";
    if (!Xp || !Yp || !lsp || !noisep || !dX || !dY || !dls) return fail(ctx, PILCO_E_SHAPE, pre + "null policy parameters or null dX, dY or dls");
    if (bf != ctx->slot[PILCO_SLOT_POLICY].N) return fail(ctx, PILCO_E_SHAPE, pre + "bf is not the number of points of the policy slot");
    const int E = policy->state_dim, U = policy->control_dim;
    if (!rbf_solve_adjoint(bf, E, U, Xp, Yp, lsp, noisep, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return fail(ctx, PILCO_E_NOT_PD, pre + "K + noise I of the policy is singular");
    std::vector<double> par;
    if (int r = rollout(par)) return r;
    // dbeta (U,bf) | dC (bf,E) | dl (U,E): dbeta through beta_k = (K_k + noise_k I)^-1 Y_k into dY, dX and dls
    const double *dbeta = par.data(), *dC = dbeta + (size_t)U * bf, *dl = dC + (size_t)bf * E;
    rbf_solve_adjoint(bf, E, U, Xp, Yp, lsp, noisep, dC, dl, dbeta, dX, dY, dls);
    return PILCO_OK;
}
