// What the particle rollout (particles.hip) shares with its gradient (particles_grad.hip): the arguments of the action and
// draw kernels, their launches, and the policy / reward checks and staging.  The kernels themselves live in particles.hip.
#pragma once
#include "predict.h"

namespace pilco {

constexpr int PT_BLOCK = 128;

struct ParticleHeadArgs {
    const double* x;   // [P][E] the step's states
    double* Xt;        // [D][ldt] the chunk's test points [x, u], transposed; zero past ntc
    int p0, ntc, ldt, E, U, kind, squash;
    const double *W, *b, *maxact;             // LinearController [U][E], [U]; scale of the squash [U]
    const double *pc, *pls, *pvar, *pbeta;    // RbfController (policy slot): centres [E][pnpad], lengthscales [U][E], variances [U], beta [U][pnpad]
    int pn, pnpad;
};

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

}  // namespace pilco

struct StreamDrain {   // the staging vectors of a call are locals: nothing of the stream may outlive them
    hipStream_t st;
    ~StreamDrain() { (void)hipStreamSynchronize(st); }
};

// k_particle_head over the chunk a.p0 .. a.p0 + a.ntc - 1 (a.ldt columns), k_particle_tail over its a.ntc particles
void launch_particle_head(hipStream_t st, const pilco::ParticleHeadArgs& a);
void launch_particle_tail(hipStream_t st, const pilco::ParticleTailArgs& a);
// what pilco_rollout_particles refuses about the slot, the context, P and H; about the policy and the reward terms (in this
// order, with its null-pointer refusals between the two)
int check_particle_state(pilco_ctx* ctx, int P, int H);
int check_particle_terms(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards);
// the policy against the dynamics slot (and, RbfController, the policy slot)
int check_policy(pilco_ctx* ctx, const pilco_policy* policy);
// doubles of the staging vector hp: W[U*E] b[U] maxact[U], then per reward W[E*E] t[E] (exponential) or W[E] (linear)
inline size_t particle_par_doubles(int E, int U) { return (size_t)U * E + 2 * U + (size_t)MAX_REWARD_TERMS * (E * E + E) + 8; }
// the policy's parameters into hp (from off on) and the action kernel's arguments; dev: where hp goes
void stage_policy(pilco_ctx* ctx, const pilco_policy* policy, std::vector<double>& hp, size_t& off, const double* dev,
                  pilco::ParticleHeadArgs& ha);
// the reward terms into hp (from off on) and rw[0 .. n_rewards - 1]
void stage_rewards(const pilco_reward_term* rewards, int n_rewards, int E, std::vector<double>& hp, size_t& off, const double* dev,
                   pilco::ParticleReward* rw);
