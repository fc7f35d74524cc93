// What the particle entry points share.  Device side: the arguments of the action, draw, statistics and event kernels
// (kernels in particles.hip), the reward terms at a point, and the arguments of the gradient's reverse sweep (kernels in
// particles_grad.hip; the function-sample gradient runs it on its own step matrices), each with its launch.  Host side
// (particle_frame.hip, docs/particle_frame.md): the checks and the staging of policy and rewards, ParticleFrame -- what the
// three forward rollouts do around their step loops -- and ParticleGradFrame -- what the two gradients do around their
// forward passes.
#pragma once
#include "predict.h"

#include <functional>

namespace pilco {

constexpr int PT_BLOCK = 128;

struct ParticleHeadArgs {
    const double* x;   // [P][E] the step's states
    double* Xt;        // [D][ldt] the chunk's test points [x, u], transposed; zero past ntc
    int p0, ntc, ldt, E, U, kind, squash;
    const double *W, *b, *maxact;             // LinearController [U][E], [U]; scale of the squash [U]
    const double *pc, *pls, *pvar, *pbeta;    // RbfController (policy slot): centres [E][pnpad], lengthscales [U][E], variances [U], beta [U][pnpad]
    int pn, pnpad;
    const double *W1, *b1, *W2, *b2;          // MLP policy (pilco_set_policy_mlp): [Hn][E], [Hn], [U][Hn], [U]
    int Hn;
};

constexpr int HEAD_BLOCK = 256;   // particles (threads) per workgroup of k_particle_head
// doubles of an MLP policy's parameters W1 [Hn][E] | b1 [Hn] | W2 [U][Hn] | b2 [U]: contiguous in the parameter upload from W1 on
inline int mlp_par_doubles(int E, int U, int Hn) { return Hn * (E + 1) + U * (Hn + 1); }
// dynamic LDS of k_particle_head: MLP policy [U][HEAD_BLOCK] the pre-squash sums, [E][HEAD_BLOCK] the states (a column per
// thread), then the workgroup's copy of the parameters; none otherwise
inline int particle_head_lds_doubles(int kind, int E, int U, int Hn) {
    return kind == PILCO_POLICY_MLP ? (U + E) * HEAD_BLOCK + mlp_par_doubles(E, U, Hn) : 0;
}

// The MLP policy's hidden unit at a state (element e: x[e * stride]) from row j of W1 (w1 [E]) and b1_j, and its adjoint factor
// from column j of W2 (element k: w2[k * ldw]), as EVERY kernel evaluates them (docs/particle_mlp.md): a_j by fma over e
// ascending from 0, then + b1_j; h_j = tanh(a_j); delta_j = (1 - h_j^2) sum_k W2_kj ds_k, k ascending (ds element k:
// ds[k * dstride]), 1 - h^2 as one fma.  The operands come from LDS: a dependent chain of loads from global memory per term
// costs the kernels their time (docs/particle_mlp.md, "Measured times"); four terms' loads are issued before their fmas
#if defined(__HIPCC__)
__device__ __forceinline__ double mlp_hidden(const double* w1, double b1j, const double* x, int stride, int E) {
    double acc = 0.0;
    int e = 0;
    for (; e + 4 <= E; e += 4) {
        const double w0 = w1[e], wa = w1[e + 1], wb = w1[e + 2], wc = w1[e + 3];
        const double x0 = x[e * stride], xa = x[(e + 1) * stride], xb = x[(e + 2) * stride], xc = x[(e + 3) * stride];
        acc = fma(w0, x0, acc);
        acc = fma(wa, xa, acc);
        acc = fma(wb, xb, acc);
        acc = fma(wc, xc, acc);
    }
    for (; e < E; ++e) acc = fma(w1[e], x[e * stride], acc);
    acc += b1j;
    return tanh(acc);
}
__device__ __forceinline__ double mlp_delta(const double* w2, int ldw, double h, const double* ds, int dstride, int U) {
    double t = 0.0;
    for (int k = 0; k < U; ++k) t = fma(w2[k * ldw], ds[k * dstride], t);
    return fma(-h, h, 1.0) * t;
}
// the workgroup's copy of the parameters (before a barrier)
__device__ __forceinline__ void mlp_stage(const ParticleHeadArgs& a, double* w, int tid, int nthreads) {
    const int n = a.Hn * (a.E + 1) + a.U * (a.Hn + 1);
    for (int q = tid; q < n; q += nthreads) w[q] = a.W1[q];
}
#endif

struct ParticleReward {
    int kind;
    double coef;
    const double *W, *t;   // exponential: [E][E], [E]; linear: [E]
};

struct ParticleTailArgs {
    const double* x;        // [P][E] the step's states
    double* xn;             // [P][E] the next states
    const double *mu, *var; // [E][ldt] posterior of the chunk
    const double* noise;    // [E] likelihood variances (observation_noise), or nullptr
    const double* eps_in;   // [P][E] the step's draws, or nullptr: generated here
    double* eps_out;        // [P][E] the draws used, or nullptr
    double* rew;            // [P] reward of the pre-step state
    unsigned long long seed;
    int t, p0, ntc, ldt, E, n_rewards;
    ParticleReward rw[MAX_REWARD_TERMS];
};

// the reward terms at zero covariance at the state xr [E]; A: the arguments of a step kernel (E, n_rewards, rw)
#if defined(__HIPCC__)
template <class A>
__device__ __forceinline__ double particle_reward(const A& a, const double* xr) {
    const int E = a.E;
    double total = 0.0;
    for (int k = 0; k < a.n_rewards; ++k) {
        const ParticleReward& r = a.rw[k];
        double v = 0.0;
        if (r.kind == PILCO_REWARD_EXPONENTIAL) {
            double q = 0.0;
            for (int i = 0; i < E; ++i) {
                double row = 0.0;
                for (int j = 0; j < E; ++j) row = fma(r.W[i * E + j], xr[j] - r.t[j], row);
                q = fma(xr[i] - r.t[i], row, q);
            }
            v = exp(-0.5 * q);
        } else {
            for (int i = 0; i < E; ++i) v = fma(r.W[i], xr[i], v);
        }
        total = fma(r.coef, v, total);
    }
    return total;
}
#endif

struct ParticleStatArgs {
    const double* x;     // [P][E]
    const double* rew;   // [P], or nullptr (the last states: no reward)
    double* part;        // [nblk][Q] partial sums, Q = E + E*E + 1
    double* out;         // [Q] mean | cov | mean reward
    int P, E, nblk;
};

struct ParticleEventArgs {
    const double* x;     // [P][E] the states after t steps
    int* first_hit;      // [P][K] the first t with a hit, -1 so far; or nullptr
    int* part;           // [nblk][K] the blocks' counts
    long long* counts;   // [K] row t of the counts
    int P, E, K, t, nblk;
    pilco_event ev[PILCO_MAX_EVENTS];   // the table travels in the kernel arguments (832 bytes)
};

// ---- the reverse sweep of the particle gradient (kernels in particles_grad.hip), shared with the function-sample gradient
// (particles_fn_grad.hip), which feeds it its own step matrices

constexpr int PG_RB = 64;   // particles (threads) per workgroup of the reverse kernel

struct PgReverseArgs {
    ParticleHeadArgs pol;   // the policy (x: the states of step t, [P][E]; p0: the group's first particle; ntc: its particles)
    const double* A;        // [E][D][ldg] the step's matrices, or nullptr: lam_in is zero (t = H - 1)
    const double* lam_in;   // [E][ldg]
    double* lam_out;        // [E][ldg]
    double* ds;             // [U][ldg] cotangents of the sines' arguments
    int ldg, n_rewards;
    ParticleReward rw[MAX_REWARD_TERMS];
};

// dynamic LDS: [3 E + U][PG_RB] the particle's lam, x, lam' and g_u / ds (a column per thread), then 1 / lengthscale [U][E];
// MLP policy: then [U][PG_RB] the pre-squash sums and the workgroup's copy of the parameters
inline int pg_reverse_lds_doubles(int E, int U, int kind, int Hn) {
    return (3 * E + U) * PG_RB + U * E + (kind == PILCO_POLICY_MLP ? U * PG_RB + mlp_par_doubles(E, U, Hn) : 0);
}

struct PgParamArgs {
    ParticleHeadArgs pol;   // as PgReverseArgs
    const double* ds;       // [U][ldg]
    double* part;           // [blocks of all particles][Q] the blocks' cells
    int ldg, Q;
};

// quantities of a policy: LinearController dW [U][E] | db [U]; RbfController dbeta [U][bf] | dC [bf][E] | dl [U][E];
// MLP policy (bf: its hidden units) dW1 [bf][E] | db1 [bf] | dW2 [U][bf] | db2 [U]
inline int pg_quantities(int kind, int E, int U, int bf) {
    if (kind == PILCO_POLICY_MLP) return bf * (E + 1) + U * (bf + 1);
    return kind == PILCO_POLICY_RBF ? U * bf + bf * E + U * E : U * E + U;
}

// k_pg_param_partials, MLP policy: the block's h, then delta, in tiles of PG_MLP_TILE hidden units, [PT_BLOCK][PG_MLP_TILE + 1]
// (dynamic LDS; the odd row length keeps a thread's row off its neighbours' banks), then the tile's parameters: rows of W1
// [PG_MLP_TILE][E], b1 [PG_MLP_TILE], columns of W2 [U][PG_MLP_TILE]
constexpr int PG_MLP_TILE = 64;
inline int pg_param_lds_doubles(int kind, int E, int U) {
    return kind == PILCO_POLICY_MLP ? PT_BLOCK * (PG_MLP_TILE + 1) + PG_MLP_TILE * (E + 1 + U) : 0;
}

}  // namespace pilco

// the launches of the reverse sweep: the reward sums of the blocks b0 .. b0 + nb - 1 at step t (k_pg_reward_partials), one
// reverse step over the group a.pol.p0 .. + a.pol.ntc - 1 (k_pg_reverse), its parameter sums (k_pg_param_partials), and the
// blocks' cells in block order over P (k_pg_finish)
void launch_pg_reward_partials(hipStream_t st, const double* rew, double* part, int P, int b0, int nb, int t, int H);
void launch_pg_reverse(hipStream_t st, const pilco::PgReverseArgs& a);
void launch_pg_param_partials(hipStream_t st, const pilco::PgParamArgs& a);
void launch_pg_finish(hipStream_t st, const double* part, double* out, int nblk, int Q, int P);
// doubles of stored step matrices per group: PILCO_PARTICLE_GRAD_BUDGET, read at every call, or 2^27
size_t pg_group_budget();
// the refusals of the gradient entry points, before any launch or upload; who: the entry point without "pilco_" and "_rbf"
// entry: the policy kind the entry point differentiates (PILCO_POLICY_LINEAR also takes no policy)
int check_particle_grad_call(pilco_ctx* ctx, const char* who, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                             const double* x0, int P, int H, const double* reward, int entry);

struct StreamDrain {   // the staging vectors of a call are locals: nothing of the stream may outlive them
    hipStream_t st;
    ~StreamDrain() { (void)hipStreamSynchronize(st); }
};

// k_particle_head over the chunk a.p0 .. a.p0 + a.ntc - 1 (a.ldt columns), k_particle_tail over its a.ntc particles
void launch_particle_head(hipStream_t st, const pilco::ParticleHeadArgs& a);
void launch_particle_tail(hipStream_t st, const pilco::ParticleTailArgs& a);
// the statistics of one state over all particles (k_particle_partials, k_particle_finish) and its events (k_particle_events,
// k_particle_events_finish): ParticleFrame::state launches them for every forward rollout
void launch_particle_stats(hipStream_t st, const pilco::ParticleStatArgs& a);
void launch_particle_events(hipStream_t st, const pilco::ParticleEventArgs& a);
// what pilco_rollout_particles refuses about the slot, the context, P and H; about the policy and the reward terms (in this
// order, with its null-pointer refusals between the two)
int check_particle_state(pilco_ctx* ctx, int P, int H);
int check_particle_terms(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards);
// the policy against the dynamics slot (and, RbfController, the policy slot)
int check_policy(pilco_ctx* ctx, const pilco_policy* policy);
// doubles of the staging vector hp: W[U*E] b[U] maxact[U], then per reward W[E*E] t[E] (exponential) or W[E] (linear); an MLP
// policy of Hn hidden units (0: none) puts W1[Hn*E] b1[Hn] W2[U*Hn] b2[U] in the place of W, b
inline size_t particle_par_doubles(int E, int U, int Hn) {
    return (size_t)U * E + 2 * U + (size_t)MAX_REWARD_TERMS * (E * E + E) + 8 + (size_t)Hn * (E + 1) + (size_t)U * (Hn + 1);
}
// the hidden units of the policy's network (0 for every other kind)
inline int policy_mlp_hidden(const pilco_ctx* ctx, const pilco_policy* policy) { return policy->kind == PILCO_POLICY_MLP ? ctx->mlp.Hn : 0; }
// the policy's parameters into hp (from off on) and the action kernel's arguments; dev: where hp goes
void stage_policy(pilco_ctx* ctx, const pilco_policy* policy, std::vector<double>& hp, size_t& off, const double* dev,
                  pilco::ParticleHeadArgs& ha);
// the reward terms into hp (from off on) and rw[0 .. n_rewards - 1]
void stage_rewards(const pilco_reward_term* rewards, int n_rewards, int E, std::vector<double>& hp, size_t& off, const double* dev,
                   pilco::ParticleReward* rw);

// ---- the forward frame.  Call order of a driver: check, its own refusals, open, its own buffers, upload, state(0, nullptr),
// its steps with state(t + 1, rew) behind each (or every state after the last step), download, download_events, its own
// downloads, the synchronisation, its host copies, finish.

struct ParticleCall {   // the arguments the forward entry points share
    const pilco_policy* policy;
    const pilco_reward_term* rewards;
    int n_rewards;
    const double* x0;
    int P, H;
    const double* eps;
    unsigned long long seed;
    int observation_noise;
    double *mean, *cov, *reward_steps, *particles, *eps_out;
    const pilco_event* events;
    int n_events;
    long long* counts;
    int* first_hit;
};

// hipSetDevice, the factorisation if it is stale, the dynamics slot's PredictWork (created on first use)
int particle_work(pilco_ctx* ctx, PredictWork*& work);

struct ParticleFrame {
    pilco_ctx* ctx;
    const ParticleCall c;
    PredictWork* work = nullptr;   // set by open; from then on the destructor drains the stream (hp and hstats are its staging)
    hipStream_t st = nullptr;
    int E = 0, D = 0, U = 0, Q = 0, K = 0, nblk = 0, nslab = 0;   // Q = E + E*E + 1 statistics per state, K events
    size_t PE = 0, eps_doubles = 0, fh_bytes = 0;
    std::vector<double> hp, hstats;   // parameters (particle_par_doubles), statistics [H+1][Q]
    pilco::ParticleHeadArgs ha{};     // the staged policy
    pilco::ParticleStatArgs sa{};
    pilco::ParticleEventArgs ea{};
    ~ParticleFrame() { if (work) (void)hipStreamSynchronize(st); }
    // the refusals every entry makes first, before any device call; who: the entry point without "pilco_"
    int check(const char* who);
    // device, factorisation, PredictWork; pt_x [nslab][P][E], pt_eps [eps_doubles] (0: none), pt_part, pt_stats, pt_par, pt_ev_*;
    // policy and rewards staged into hp (rw: the step kernel's reward terms); the statistics' and events' arguments
    int open(int nslab, size_t eps_doubles, pilco::ParticleReward* rw);
    // one upload: parameters, initial particles, the caller's draws (where pt_eps is kept)
    int upload();
    double* slab(int t) const { return work->pt_x.p + (size_t)(nslab > c.H ? t : (t & 1)) * PE; }
    // moments and events of the states after t steps; rew [P]: the rewards of step t - 1, nullptr for t = 0 (which first sets
    // every first hit to -1)
    int state(int t, const double* rew);
    // the copies back, enqueued: statistics into hstats, pt_x into particles, pt_eps into eps_out (nullptr: not wanted);
    // the events' counts and first hits
    int download(double* particles, double* eps_out);
    int download_events(long long* counts, int* first_hit);
    // after the synchronisation: hstats into the caller's mean, cov and reward_steps
    void finish();
};

// ---- the gradient frame.  Call order: (attach,) open, the forward's own buffers, upload, its set-up, sweep, finish_enqueue,
// the driver's own downloads, the synchronisation, finish.

struct PgPlan {   // groups of Pg particles (a multiple of PT_BLOCK, or all P), ldg columns of stored matrices, per_particle doubles each
    size_t per_particle;
    int Pg, ldg, nblk;
};
PgPlan pg_plan(int P, int H, int E, int D, size_t budget);

struct ParticleGradFrame {
    pilco_ctx* ctx;
    const pilco_policy* policy;
    const pilco_reward_term* rewards;
    int n_rewards;
    const double* x0;
    int P, H;
    double* dreturn_dx0;
    int E, D, U, Q;   // Q: pg_quantities of the policy (0 without controls)
    size_t PE;
    PredictWork* work = nullptr;   // as ParticleFrame
    hipStream_t st = nullptr;
    PgPlan pl{};
    std::vector<double> hp, hout, hlam;   // parameters, [H] rewards | [Q] parameter sums, lam_0 of a group [E][ldg]
    pilco::PgReverseArgs ra{};
    pilco::PgParamArgs pa{};
    pilco::ParticleHeadArgs ha{};   // the staged policy, for the forward
    // the dimensions; par: sized to Q and zeroed.  Touches no device
    ParticleGradFrame(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards, const double* x0, int P,
                      int H, double* dreturn_dx0, std::vector<double>& par);
    ~ParticleGradFrame() { if (work) (void)hipStreamSynchronize(st); }
    int attach() { st = ctx->st; return particle_work(ctx, work); }
    // H > 0.  The plan, the pt_* and pg_* buffers (pt_eps: eps_doubles, 0: none), policy and rewards staged (rw: the forward
    // kernel's reward terms); one upload: parameters, initial particles, the draws (nullptr: none), the parameter cells zeroed
    int open(size_t eps_doubles, pilco::ParticleReward* rw);
    int upload(const double* eps);
    double* slab(int t) const { return work->pt_x.p + (size_t)t * PE; }
    // per group: step(g0, ng, t), t = 0 .. H-1 -- the forward launches of the group's ng particles from g0 -- each followed
    // by its reward sums; the reverse sweep t = H-1 .. 0; lam_0 into dreturn_dx0
    int sweep(const std::function<int(int g0, int ng, int t)>& step);
    // the blocks' cells in block order and their download, enqueued; after the synchronisation: J in step order, par
    int finish_enqueue();
    void finish(double* reward, double* reward_steps, std::vector<double>& par);
};

// what the four gradient entry points do around their rollout (which fills par); who: the entry point without "pilco_" and
// "_rbf".  LinearController or none: the refusal of null dW, db and par = dW | db.  RbfController: the refusals, the
// singularity probe, and dbeta | dC | dl through beta_k = (K_k + noise_k I)^-1 Y_k into dX, dY and dls
using PgRollout = std::function<int(std::vector<double>& par)>;
int pg_linear_entry(pilco_ctx* ctx, const char* who, const pilco_policy* policy, double* dW, double* db, const PgRollout& rollout);
// MLP policy: the refusal of null dW1, db1, dW2, db2 and par = dW1 | db1 | dW2 | db2
int pg_mlp_entry(pilco_ctx* ctx, const char* who, const pilco_policy* policy, double* dW1, double* db1, double* dW2, double* db2,
                 const PgRollout& rollout);
int pg_rbf_entry(pilco_ctx* ctx, const char* who, const pilco_policy* policy, const double* Xp, const double* Yp, const double* lsp,
                 const double* noisep, int bf, double* dX, double* dY, double* dls, const PgRollout& rollout);
