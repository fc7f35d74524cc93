// Particle rollouts through the learned dynamics: pilco_rollout_particles.  DESIGN.md section 13, docs/particles.md.
// P sampled trajectories of H steps, device resident, to hold against the Gaussians the moment matching propagates.
// One step, per chunk of particles (the chunks of pilco_gp_predict_points: at most PP_KS_BUDGET doubles of cross-covariance):
//   k_particle_head   the action u = policy(x) of every particle and the transposed, padded block [x, u] launch_gram reads
//   predict_points_device (predict.hip)   the posterior (mu_e, v_e) of every output at [x, u]: two launches
//   k_particle_tail   the draw (given, or Philox4x32-10 + Box-Muller: philox_normal.h), x'_e = x_e + mu_e + sqrt(max(v_e, 0)) eps,
//                     and the reward of the pre-step state
// and then, over ALL particles of the step at once (so nothing of it depends on the chunking):
//   k_particle_partials / k_particle_finish   mean, covariance and mean reward
// Every kernel up to the tail works on a particle with that particle's own row and draws only: a trajectory has the same bits
// alone or in any batch (k_predict_points gives every test point a fixed order of its own).
//
// ORDER OF THE SUMS behind mean, cov and reward_steps (no floating-point atomics anywhere): the particles are cut into blocks
// of PT_BLOCK = 128 consecutive indices; inside a block one thread per quantity adds the particles in index order; the
// blocks' partial sums are added in block order.  The moments are taken about c = the step's particle 0 (shifted data: no
// cancellation against |x|^2): S1_a = sum (x_a - c_a), S2_ab = sum (x_a - c_a)(x_b - c_b);
//   mean_a = c_a + S1_a / P,   cov_ab = S2_ab / P - (S1_a / P)(S1_b / P),   reward = (sum r_p) / P.
// The same particles in the same order give the same bits, whatever P is chunked into; P = 1 gives a zero covariance exactly.
//
// EVENTS (pilco_rollout_particles_events; the predicate: particle_events.h).  Behind the statistics of every state t = 0..H,
// over all particles of the step:
//   k_particle_events / k_particle_events_finish   per event the number of particles that hit it, and every particle's first hit
// Integer counts: a block of PT_BLOCK particles counts by wave ballot, the blocks' counts are added in block order; no atomics.
#include "particle_events.h"
#include "particles.h"
#include "philox_normal.h"

namespace pilco {

static_assert(HEAD_BLOCK == 256, "k_particle_head: one thread per particle, 256 per workgroup");
__global__ __launch_bounds__(256) void k_particle_head(ParticleHeadArgs a) {
    extern __shared__ double head_lds[];   // MLP policy: [U][HEAD_BLOCK] the pre-squash sums, [E][HEAD_BLOCK] the states, the parameters
    const int E = a.E, U = a.U, ldt = a.ldt;
    __shared__ double il_s[MAX_D * MAX_D / 4];   // RbfController: 1 / lengthscale [U][E]  (U + E <= MAX_D)
    if (a.kind == PILCO_POLICY_RBF)
        for (int q = threadIdx.x; q < U * E; q += 256) il_s[q] = 1.0 / a.pls[q];
    if (a.kind == PILCO_POLICY_MLP) mlp_stage(a, head_lds + (U + E) * HEAD_BLOCK, threadIdx.x, HEAD_BLOCK);
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ldt) return;
    if (i >= a.ntc) {
        for (int d = 0; d < E + U; ++d) a.Xt[(long)d * ldt + i] = 0.0;
        return;
    }
    const double* xr = a.x + (long)(a.p0 + i) * E;
    for (int e = 0; e < E; ++e) a.Xt[(long)e * ldt + i] = xr[e];
    if (a.kind == PILCO_POLICY_MLP) {   // s_k by fma over j ascending, then + b2_k; the weights are wave-uniform LDS reads
        const int Hn = a.Hn;
        double* sc = head_lds + threadIdx.x;
        double* xs = sc + U * HEAD_BLOCK;
        const double *W1 = head_lds + (U + E) * HEAD_BLOCK, *b1 = W1 + Hn * E, *W2 = b1 + Hn, *b2 = W2 + U * Hn;
        for (int e = 0; e < E; ++e) xs[e * HEAD_BLOCK] = xr[e];
        for (int k = 0; k < U; ++k) sc[k * HEAD_BLOCK] = 0.0;
        for (int j = 0; j < Hn; ++j) {
            const double h = mlp_hidden(W1 + j * E, b1[j], xs, HEAD_BLOCK, E);
            for (int k = 0; k < U; ++k) sc[k * HEAD_BLOCK] = fma(W2[k * Hn + j], h, sc[k * HEAD_BLOCK]);
        }
        for (int k = 0; k < U; ++k) {
            const double s = sc[k * HEAD_BLOCK] + b2[k];
            a.Xt[(long)(E + k) * ldt + i] = a.squash ? a.maxact[k] * sin(s) : s;
        }
        return;
    }
    for (int k = 0; k < U; ++k) {
        double s = 0.0, scale = a.maxact[k];
        if (a.kind == PILCO_POLICY_LINEAR) {
            for (int e = 0; e < E; ++e) s = fma(xr[e], a.W[k * E + e], s);
            s += a.b[k];
        } else {
            const double vk = a.pvar[k];
            for (int c = 0; c < a.pn; ++c) {
                double r2 = 0.0;
                for (int e = 0; e < E; ++e) {
                    const double d = (xr[e] - a.pc[(long)e * a.pnpad + c]) * il_s[k * E + e];
                    r2 = fma(d, d, r2);
                }
                s = fma(a.pbeta[(long)k * a.pnpad + c], vk * exp(-0.5 * r2), s);
            }
            scale *= exp(-0.5e-6);   // squash_sin of a variance of 1e-6: S - diag(variance - 1e-6) at s = 0
        }
        a.Xt[(long)(E + k) * ldt + i] = a.squash ? scale * sin(s) : s;
    }
}

__global__ __launch_bounds__(256) void k_particle_tail(ParticleTailArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.ntc) return;
    const int E = a.E, ldt = a.ldt;
    const long p = a.p0 + i;
    const double* xr = a.x + p * E;
    double* xn = a.xn + p * E;
    for (int j = 0; 2 * j < E; ++j) {
        double z[2];
        if (a.eps_in) {
            z[0] = a.eps_in[p * E + 2 * j];
            z[1] = (2 * j + 1 < E) ? a.eps_in[p * E + 2 * j + 1] : 0.0;
        } else {
            philox_normal_pair(a.seed, (uint32_t)a.t, (uint32_t)p, (uint32_t)j, &z[0], &z[1]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = 2 * j + h;
            if (e >= E) break;
            double v = a.var[(long)e * ldt + i];
            if (a.noise) v += a.noise[e];
            const double sd = sqrt(fmax(v, 0.0));
            xn[e] = (xr[e] + a.mu[(long)e * ldt + i]) + sd * z[h];
            if (a.eps_out) a.eps_out[p * E + e] = z[h];
        }
    }
    a.rew[p] = particle_reward(a, xr);
}

// block b: particles PT_BLOCK b .. ; thread q adds quantity q over them in index order
__global__ __launch_bounds__(PT_BLOCK) void k_particle_partials(ParticleStatArgs a) {
    const int E = a.E, Q = E + E * E + 1, ldx = E + 2;
    __shared__ double xs[PT_BLOCK * (MAX_D + 2)];   // [particle][x - c | reward]
    const int i = threadIdx.x;
    const long p = (long)blockIdx.x * PT_BLOCK + i;
    for (int e = 0; e < E; ++e) xs[i * ldx + e] = (p < a.P) ? a.x[p * E + e] - a.x[e] : 0.0;
    xs[i * ldx + E] = (p < a.P && a.rew) ? a.rew[p] : 0.0;
    __syncthreads();
    for (int q = threadIdx.x; q < Q; q += PT_BLOCK) {
        double s = 0.0;
        if (q < E || q == Q - 1) {
            const int col = q < E ? q : E;
            for (int k = 0; k < PT_BLOCK; ++k) s += xs[k * ldx + col];
        } else {
            const int ab = q - E, ca = ab / E, cb = ab - ca * E;
            for (int k = 0; k < PT_BLOCK; ++k) s = fma(xs[k * ldx + ca], xs[k * ldx + cb], s);
        }
        a.part[(long)blockIdx.x * Q + q] = s;
    }
}

// thread q: the blocks' partial sums of quantity q in block order, then the moment it stands for
__global__ __launch_bounds__(PT_BLOCK) void k_particle_finish(ParticleStatArgs a) {
    const int E = a.E, Q = E + E * E + 1;
    const int q = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (q >= Q) return;
    auto total = [&](int col) {
        double s = 0.0;
        for (int b = 0; b < a.nblk; ++b) s += a.part[(long)b * Q + col];
        return s;
    };
    const double n = (double)a.P;
    if (q < E) {
        a.out[q] = a.x[q] + total(q) / n;
    } else if (q == Q - 1) {
        a.out[q] = total(q) / n;
    } else {
        const int ab = q - E, ca = ab / E, cb = ab - ca * E;
        const double ma = total(ca) / n, mb = total(cb) / n;
        a.out[q] = total(q) / n - ma * mb;
    }
}

// block b: particles PT_BLOCK b .. , one thread per particle; a wave counts its hits by ballot, thread k adds the two waves
__global__ __launch_bounds__(PT_BLOCK) void k_particle_events(ParticleEventArgs a) {
    __shared__ int wave_hits[PT_BLOCK / 64][PILCO_MAX_EVENTS];
    const int i = threadIdx.x, K = a.K;
    const long p = (long)blockIdx.x * PT_BLOCK + i;
    const bool live = p < a.P;
    const double* xr = a.x + (live ? p : 0) * a.E;
    for (int k = 0; k < K; ++k) {
        const bool hit = live && event_hit(a.ev[k], xr);
        const unsigned long long votes = __ballot(hit);
        if ((i & 63) == 0) wave_hits[i >> 6][k] = __popcll(votes);
        if (hit && a.first_hit && a.first_hit[p * K + k] < 0) a.first_hit[p * K + k] = a.t;
    }
    __syncthreads();
    if (i < K) {
        int s = 0;
        for (int w = 0; w < PT_BLOCK / 64; ++w) s += wave_hits[w][i];
        a.part[(long)blockIdx.x * K + i] = s;
    }
}

// thread k: the blocks' counts of event k in block order
__global__ __launch_bounds__(64) void k_particle_events_finish(ParticleEventArgs a) {
    const int k = threadIdx.x;
    if (k >= a.K) return;
    long long s = 0;
    for (int b = 0; b < a.nblk; ++b) s += a.part[(long)b * a.K + k];
    a.counts[k] = s;
}

}  // namespace pilco

using namespace pilco;

void launch_particle_head(hipStream_t st, const ParticleHeadArgs& a) {
    const size_t lds_bytes = sizeof(double) * particle_head_lds_doubles(a.kind, a.E, a.U, a.Hn);
    launch_lds<k_particle_head>(dim3((a.ldt + 255) / 256), dim3(256), lds_bytes, st, a);
}
void launch_particle_tail(hipStream_t st, const ParticleTailArgs& a) {
    hipLaunchKernelGGL(k_particle_tail, dim3((a.ntc + 255) / 256), dim3(256), 0, st, a);
}
void launch_particle_stats(hipStream_t st, const ParticleStatArgs& a) {
    const int Q = a.E + a.E * a.E + 1;
    hipLaunchKernelGGL(k_particle_partials, dim3(a.nblk), dim3(PT_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_particle_finish, dim3((Q + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, st, a);
}
void launch_particle_events(hipStream_t st, const ParticleEventArgs& a) {
    hipLaunchKernelGGL(k_particle_events, dim3(a.nblk), dim3(PT_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_particle_events_finish, dim3(1), dim3(64), 0, st, a);
}

// pilco_rollout_particles and pilco_rollout_particles_events: with n_events == 0 exactly the launches of the former.  The frame
// (particle_frame.hip) holds what surrounds the step loop
static int rollout_particles(pilco_ctx* ctx, const ParticleCall& c) {
    ParticleFrame f{ctx, c};
    if (int r = f.check("rollout_particles")) return r;
    const int E = f.E, D = f.D, P = c.P, H = c.H;
    const size_t PE = f.PE;
    ParticleTailArgs ta{};
    if (int r = f.open(c.particles ? H + 1 : 2, (H > 0 && (c.eps || c.eps_out)) ? (size_t)H * PE : 0, ta.rw)) return r;
    PredictWork& pw = *f.work;
    hipStream_t st = f.st;
    const PredictModel md = predict_model_of(ctx->slot[PILCO_SLOT_DYNAMICS], 0, E);
    const int npad = md.npad;
    const int ntc_max = std::min(round_up(P, 64), predict_chunk_cap(E, npad));
    ENSURE(pw.Xt, (size_t)D * ntc_max);
    ENSURE(pw.Ks, (size_t)E * ntc_max * npad);
    ENSURE(pw.out, (size_t)2 * E * ntc_max);
    ENSURE(pw.pt_rew, (size_t)P);
    if (int r = f.upload()) return r;

    ParticleHeadArgs& ha = f.ha;
    ta.n_rewards = c.n_rewards; ta.E = E; ta.seed = c.seed;
    ta.noise = c.observation_noise ? ctx->slot[PILCO_SLOT_DYNAMICS].noise.p : nullptr;
    ta.rew = pw.pt_rew.p;
    if (int r = f.state(0, nullptr)) return r;
    for (int t = 0; t < H; ++t) {
        ha.x = ta.x = f.slab(t);
        ta.xn = f.slab(t + 1);
        ta.t = t;
        ta.eps_in = c.eps ? pw.pt_eps.p + (size_t)t * PE : nullptr;
        ta.eps_out = (!c.eps && c.eps_out) ? pw.pt_eps.p + (size_t)t * PE : nullptr;
        for (int p0 = 0; p0 < P; p0 += ntc_max) {
            const int ntc = std::min(ntc_max, P - p0), ldt = round_up(ntc, 64);
            double *out_mean = pw.out.p, *out_var = pw.out.p + (size_t)E * ldt;
            ha.Xt = pw.Xt.p; ha.p0 = p0; ha.ntc = ntc; ha.ldt = ldt;
            launch_particle_head(st, ha);
            if (int r = predict_points_device(ctx, md, pw.Xt.p, ntc, ldt, pw.Ks.p, out_mean, out_var)) return r;
            ta.mu = out_mean; ta.var = out_var; ta.p0 = p0; ta.ntc = ntc; ta.ldt = ldt;
            launch_particle_tail(st, ta);
        }
        if (int r = f.state(t + 1, pw.pt_rew.p)) return r;
    }
    // one download, one synchronisation
    if (int r = f.download(c.particles, c.eps ? nullptr : c.eps_out)) return r;
    if (int r = f.download_events(c.counts, c.first_hit)) return r;
    HIPCHK(hipStreamSynchronize(st));
    if (c.eps_out && c.eps && H > 0) memcpy(c.eps_out, c.eps, sizeof(double) * H * PE);
    f.finish();
    return PILCO_OK;
}

extern "C" int pilco_rollout_particles(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                       const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                       int observation_noise, double* mean, double* cov, double* reward_steps, double* particles,
                                       double* eps_out) {
    return rollout_particles(ctx, {policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, mean, cov, reward_steps, particles,
                                   eps_out, nullptr, 0, nullptr, nullptr});
}

extern "C" int pilco_rollout_particles_events(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards,
                                              int n_rewards, const double* x0, int P, int H, const double* eps,
                                              unsigned long long seed, int observation_noise, double* mean, double* cov,
                                              double* reward_steps, double* particles, double* eps_out, const pilco_event* events,
                                              int n_events, long long* counts, int* first_hit) {
    return rollout_particles(ctx, {policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, mean, cov, reward_steps, particles,
                                   eps_out, events, n_events, counts, first_hit});
}

extern "C" int pilco_debug_particle_actions(pilco_ctx* ctx, const pilco_policy* policy, const double* x, int P, double* u) {
    if (int r = check_slot(ctx, PILCO_SLOT_DYNAMICS)) return r;
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    if (!s.has_data) return fail(ctx, PILCO_E_STATE, "particle_actions needs set_data first");
    if (int r = check_policy(ctx, policy)) return r;
    const int E = s.E, D = s.D, U = D - E;
    if (P <= 0 || !x || (U > 0 && !u)) return fail(ctx, PILCO_E_SHAPE, "particle_actions: null pointer or P <= 0");
    if (U == 0) return PILCO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    if (!s.pred) s.pred = new PredictWork();
    PredictWork& pw = *s.pred;
    const int ldt = round_up(P, 64);
    std::vector<double> hp(particle_par_doubles(E, U, policy_mlp_hidden(ctx, policy)), 0.0);
    ENSURE(pw.pt_x, (size_t)P * E);
    ENSURE(pw.Xt, (size_t)D * ldt);
    ENSURE(pw.pt_par, hp.size());
    ParticleHeadArgs ha{};
    size_t off = 0;
    stage_policy(ctx, policy, hp, off, pw.pt_par.p, ha);
    ha.x = pw.pt_x.p; ha.Xt = pw.Xt.p; ha.p0 = 0; ha.ntc = P; ha.ldt = ldt;
    StreamDrain drain{ctx->st};
    HIPCHK(hipMemcpyAsync(pw.pt_par.p, hp.data(), sizeof(double) * hp.size(), hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(pw.pt_x.p, x, sizeof(double) * P * E, hipMemcpyHostToDevice, ctx->st));
    launch_particle_head(ctx->st, ha);
    HIPCHK(hipGetLastError());
    std::vector<double> ut((size_t)U * ldt);
    HIPCHK(hipMemcpyAsync(ut.data(), pw.Xt.p + (size_t)E * ldt, sizeof(double) * ut.size(), hipMemcpyDeviceToHost, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < U; ++k) u[(size_t)p * U + k] = ut[(size_t)k * ldt + p];
    return PILCO_OK;
}
