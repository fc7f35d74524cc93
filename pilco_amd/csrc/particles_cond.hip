// Particle rollouts conditioned on their own path: pilco_rollout_particles_cond.  docs/particle_conditioned.md.
// The increments f(xt_0), .., f(xt_{H-1}) of one particle and one output are jointly Gaussian under the posterior; they are
// sampled one step at a time, step t conditioned on the particle's own earlier visited points (xt = [x, u]):
//   c_ts = k_e(xt_t, xt_s) - w_t . w_s                    exact GP,  w = L^{-1} k*(xt)
//   c_ts = k_e(xt_t, xt_s) - w0_t . w0_s + w1_t . w1_s    FITC,  w0 = Luu^{-1} ku*,  w1 = sqrt(sn2) iAt ku*   (docs/predict_cov.md)
//   row t of the path factor Lam (Lam Lam^T = C + j_e I, j_e = jitter sf2_e):
//     l_s = (c_ts - sum_{r<s} l_r Lam_sr) / Lam_ss   s = 0 .. t-1,      d = (c_tt + j_e) - sum_{s<t} l_s^2,   Lam_tt = sqrt(d)
//   f_t = mu_t + sum_{s<t} l_s z_s + Lam_tt z_t,     x'_e = x_e + f_t [+ sqrt(sn2_e) zeta_t]
// One step of a group of particles (the group is one chunk of pilco_gp_predict_points):
//   k_particle_head          the actions and the transposed points, written into slab t of the point history Xh [H][D][ldt]
//   predict_points_device    Ks and the mean mu (pilco_gp_predict_points' bits)
//   predict_points_w_device  W = Op K*, written into slab t of the row history Wh [H][nops][E][ldt][npad]
//   k_particle_cond_step     the t + 1 signed dot products, the kernel values, the factor row, the draw, the update, the reward
// A group runs all H steps, then the next group; the statistics and events of every state run after the last group over all
// particles, by the frame every forward rollout stands on (ParticleFrame::state, particle_frame.hip): grouping changes no bit.
//
// ORDER OF THE SUMS (a function of (npad, nops, t) only; no atomics of any kind).
//   dot product of two rows: lane l of the wave owns the element pairs (2 q, 2 q + 1), q = l + 64 m, m = 0, 1, ..; it adds
//     its products to one accumulator in increasing index order, the first operator then the second (whose products enter
//     negated, the sign on one factor: exact); the 64 lane sums meet in a butterfly, v += v(lane ^ m), m = 32, 16, 8, 4, 2, 1
//     (an addition commutes, so every lane holds the same bits).  c_ts = k - that sum; c_tt is the same routine at s = t.
//   k_e(xt_t, xt_s) = sf2 exp(-0.5 sum_d ((xt_td - xt_sd) fl(1 / l_d))^2), d ascending: k_gram's formula and order.
//   forward substitution: a_r = c_tr; for s = 0 .. t-1 in turn: l_s = a_s / Lam_ss, then a_r = fma(-l_s, Lam_rs, a_r) for r > s,
//     d = fma(-l_s, l_s, d) from d = c_tt + j_e, f = fma(l_s, z_s, f) from f = mu_t; last f = fma(Lam_tt, z_t, f).
// Nothing of a particle looks at another particle: one wave owns one (particle, output), and its history lives in the
// particle's own rows.
#include "particle_events.h"
#include "particles.h"
#include "particles_cond_plan.h"
#include "philox_normal.h"

namespace pilco {

constexpr int PC2_ROWS = 4;   // history rows in flight per wave

struct ParticleCondArgs {
    const double* Wh;     // [H][nops][E][ldt][npad] the rows of every step so far; slab t: this step's
    const double* Xh;     // [H][D][ldt] the visited points, transposed
    double* Lam;          // [ldt][E][tri] the factor, packed by columns: Lam_rs at cond_col(H, s) + r - s
    double* Cov;          // nullptr, or c_rs in the same layout (without jitter)
    const double* mu;     // [E][ldt] the posterior mean of the step
    const double* x;      // [P][E] the step's states
    double* xn;           // [P][E] the next states
    double* eps;          // [H][P][E] the step draws z: slabs < t are read, slab t is read (given) or written
    double* zeta;         // nullptr (no observation noise), or [H][P][E]: slab t is read (given) or written
    const double *ls, *sf2, *noise;   // [E][D], [E], [E]
    double* rew;          // [P] reward of the pre-step state
    int* info;            // [ldt][E]: 0, or 1 + the first step whose pivot was not positive
    unsigned long long seed;
    double jitter;
    int t, H, P, p0, ntc, ldt, E, D, npad, nops, eps_given, zeta_given, n_rewards;
    ParticleReward rw[MAX_REWARD_TERMS];
};

__device__ __forceinline__ double pc2_wave_sum(double v) {
    v += __shfl_xor(v, 32);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// One wave: one (particle i of the group, output e).  Dynamic LDS: the wave's new row, [nops][npad] doubles per wave.
__global__ __launch_bounds__(256) void k_particle_cond_step(ParticleCondArgs a) {
    extern __shared__ double pc2_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int E = a.E, D = a.D, npad = a.npad, nops = a.nops, ldt = a.ldt, t = a.t, H = a.H;
    const long q = (long)blockIdx.x * waves + w;
    const bool live = q < (long)a.ntc * E;
    const int i = live ? (int)(q / E) : 0, e = live ? (int)(q - (long)i * E) : 0;
    const long rowlen = (long)nops * npad;
    double* row = pc2_lds + w * rowlen;
    const long sE = (long)ldt * npad, sOp = (long)E * sE, sT = (long)nops * sOp;   // strides of Wh
    const double* Wpe = a.Wh + (long)e * sE + (long)i * npad;                      // row of (i, e) in slab 0, operator 0
    if (live)
        for (int op = 0; op < nops; ++op) {
            const double* src = Wpe + (long)t * sT + (long)op * sOp;
            for (int k = 2 * lane; k < npad; k += 128)
                *reinterpret_cast<double2*>(row + (long)op * npad + k) = *reinterpret_cast<const double2*>(src + k);
        }
    __syncthreads();
    if (!live) return;
    const long p = a.p0 + i;

    // the kernel values of the lane's rows s = lane and s = lane + 64
    double kv0 = 0.0, kv1 = 0.0;
    {
        double r20 = 0.0, r21 = 0.0;
        const int s0 = min(lane, t), s1 = min(lane + 64, t);
        for (int d = 0; d < D; ++d) {
            const double il = 1.0 / a.ls[(long)e * D + d];
            const double xt = a.Xh[((long)t * D + d) * ldt + i];
            const double d0 = (xt - a.Xh[((long)s0 * D + d) * ldt + i]) * il;
            const double d1 = (xt - a.Xh[((long)s1 * D + d) * ldt + i]) * il;
            r20 = fma(d0, d0, r20);
            r21 = fma(d1, d1, r21);
        }
        kv0 = a.sf2[e] * exp(-0.5 * r20);
        kv1 = a.sf2[e] * exp(-0.5 * r21);
    }

    // c_ts, s = 0 .. t: PC2_ROWS history rows at a time (a request past row t reads row t again and is dropped)
    double c0 = 0.0, c1 = 0.0;
    for (int sb = 0; sb <= t; sb += PC2_ROWS) {
        double acc[PC2_ROWS];
        const double* hr[PC2_ROWS];
#pragma unroll
        for (int r = 0; r < PC2_ROWS; ++r) {
            acc[r] = 0.0;
            hr[r] = Wpe + (long)min(sb + r, t) * sT;
        }
        for (int op = 0; op < nops; ++op) {
            const double* rw = row + (long)op * npad;
            const long o = (long)op * sOp;
#pragma unroll 2
            for (int k = 2 * lane; k < npad; k += 128) {
                double2 av = *reinterpret_cast<const double2*>(rw + k);
                if (op) { av.x = -av.x; av.y = -av.y; }   // (exact: the sign)
                double2 bv[PC2_ROWS];
#pragma unroll
                for (int r = 0; r < PC2_ROWS; ++r) bv[r] = *reinterpret_cast<const double2*>(hr[r] + o + k);
#pragma unroll
                for (int r = 0; r < PC2_ROWS; ++r) {
                    acc[r] = fma(av.x, bv[r].x, acc[r]);
                    acc[r] = fma(av.y, bv[r].y, acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < PC2_ROWS; ++r) {
            const int s = sb + r;
            const double v = pc2_wave_sum(acc[r]);
            if (s <= t && lane == (s & 63)) {
                if (s >> 6) c1 = kv1 - v; else c0 = kv0 - v;
            }
        }
    }
    const long tri = (long)H * (H + 1) / 2;
    const long pe = ((long)i * E + e) * tri;
    auto col = [&](int s) { return (long)s * H - (long)s * (s - 1) / 2; };
    if (a.Cov) {
        if (lane <= t) a.Cov[pe + col(lane) + (t - lane)] = c0;
        if (lane + 64 <= t) a.Cov[pe + col(lane + 64) + (t - lane - 64)] = c1;
    }

    // the factor row by forward substitution; lane r holds the running sums of rows r and r + 64
    const double je = a.jitter * a.sf2[e];
    double acc0 = c0, acc1 = c1;
    double d = __shfl((t >> 6) ? c1 : c0, t & 63) + je;
    double f = a.mu[(long)e * ldt + i];
    const double z0 = (lane < t) ? a.eps[((long)lane * a.P + p) * E + e] : 0.0;
    const double z1 = (lane + 64 < t) ? a.eps[((long)(lane + 64) * a.P + p) * E + e] : 0.0;
    double* Lpe = a.Lam + pe;
    for (int s = 0; s < t; ++s) {
        const double* cs = Lpe + col(s) - s;   // cs[r] = Lam_rs, r = s .. t - 1
        const double lam0 = (lane >= s && lane < t) ? cs[lane] : 0.0;
        const double lam1 = (lane + 64 >= s && lane + 64 < t) ? cs[lane + 64] : 0.0;
        const bool hi = (s >> 6) != 0;
        const double ls = __shfl((hi ? acc1 : acc0) / (hi ? lam1 : lam0), s & 63);
        const double zs = __shfl(hi ? z1 : z0, s & 63);
        if (lane > s) acc0 = fma(-ls, lam0, acc0);
        if (lane + 64 > s) acc1 = fma(-ls, lam1, acc1);
        d = fma(-ls, ls, d);
        f = fma(ls, zs, f);
        if (lane == 0) Lpe[col(s) + (t - s)] = ls;
    }
    const bool bad = !(d > 0.0);   // (NaN included)
    const double ltt = sqrt(d);

    // the draws: z_t of the step stream (domain 0), zeta_t of the observation stream (domain 6)
    const long ze = ((long)t * a.P + p) * E + e;
    double zt;
    if (a.eps_given) {
        zt = a.eps[ze];
    } else {
        double n0, n1;
        philox_normal_pair(a.seed, (uint32_t)t, (uint32_t)p, (uint32_t)(e >> 1), &n0, &n1);
        zt = (e & 1) ? n1 : n0;
    }
    f = fma(ltt, zt, f);
    double xnew = a.x[p * E + e] + f;
    double zo = 0.0;
    if (a.zeta) {
        if (a.zeta_given) {
            zo = a.zeta[ze];
        } else {
            double n0, n1;
            philox_domain_normal_pair(a.seed, (uint32_t)p, (uint32_t)t, (uint32_t)(e >> 1), PHILOX_COND_OBS, &n0, &n1);
            zo = (e & 1) ? n1 : n0;
        }
        xnew += sqrt(a.noise[e]) * zo;
    }
    if (lane == 0) {
        Lpe[col(t)] = ltt;
        a.xn[p * E + e] = xnew;
        if (!a.eps_given) a.eps[ze] = zt;
        if (a.zeta && !a.zeta_given) a.zeta[ze] = zo;
        if (bad && a.info[(long)i * E + e] == 0) a.info[(long)i * E + e] = t + 1;
        if (e == 0) a.rew[p] = particle_reward(a, a.x + p * E);
    }
}

}  // namespace pilco

using namespace pilco;

namespace {

size_t cond_budget() {
    if (const char* v = getenv("PILCO_PARTICLE_COND_BUDGET")) {
        const long long n = atoll(v);
        if (n > 0) return (size_t)n;
    }
    return PC2_BUDGET;
}

// the packed columns of one (particle, output) -> the lower triangle of an (H, H) matrix (the upper triangle: zero)
void cond_unpack(const double* packed, int H, double* full) {
    std::fill(full, full + (size_t)H * H, 0.0);
    for (int s = 0; s < H; ++s)
        for (int r = s; r < H; ++r) full[(size_t)r * H + s] = packed[cond_col(H, s) + (r - s)];
}

}  // namespace

extern "C" int pilco_rollout_particles_cond(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                            const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                            int observation_noise, double* mean, double* cov, double* reward_steps, double* particles,
                                            double* eps_out, const pilco_event* events, int n_events, long long* counts,
                                            int* first_hit, double jitter, const double* eps_obs, const pilco_cond_out* out) {
    // everything the caller gets back is staged here: nothing is written unless every pivot was positive.  (Before the frame,
    // which drains the stream when it leaves)
    std::vector<double> h_parts, h_eps, h_zeta, h_lam, h_cov;
    std::vector<int> h_info, h_first;
    std::vector<long long> h_counts;
    ParticleFrame f{ctx, {policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, mean, cov, reward_steps, particles, eps_out,
                          events, n_events, counts, first_hit}};
    if (int r = f.check("rollout_particles_cond")) return r;
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    const int E = f.E, D = f.D, K = f.K;
    if (H > PILCO_MAX_COND_STEPS) return fail(ctx, PILCO_E_SHAPE, "rollout_particles_cond: H must be at most 128 (PILCO_MAX_COND_STEPS)");
    if (!(jitter >= 0.0) || !std::isfinite(jitter)) return fail(ctx, PILCO_E_SHAPE, "rollout_particles_cond: jitter must be finite and >= 0");
    const bool noisy = observation_noise != 0, sparse = s.M > 0;
    const int nops = sparse ? 2 : 1, npad_m = sparse ? round_up(s.M, 64) : round_up(s.N, 64);
    double* o_zeta = (out && noisy) ? out->eps_obs : nullptr;
    double* o_cov = out ? out->path_cov : nullptr;
    double* o_fac = out ? out->path_factor : nullptr;
    if (nops * npad_m > PC2_MAX_ROW)
        return fail(ctx, PILCO_E_SHAPE, "rollout_particles_cond: more than 8192 (exact GP) or 4096 (FITC) padded points are not supported");
    const size_t budget = cond_budget();
    const CondPlan pl = cond_plan(P, H, nops, E, D, npad_m, o_cov != nullptr, budget, predict_chunk_cap(E, npad_m));
    if (pl.G == 0)
        return fail(ctx, PILCO_E_SHAPE, "rollout_particles_cond: a group of 64 particles needs " + std::to_string(pl.footprint) +
                                            " doubles, over the budget of " + std::to_string(budget) +
                                            " (PILCO_PARTICLE_COND_BUDGET); the largest H that fits is " + std::to_string(pl.H_fit));
    const size_t PE = f.PE, tri = cond_tri(H);
    ParticleCondArgs ca{};
    if (int r = f.open(H + 1, std::max((size_t)H * PE, (size_t)1), ca.rw)) return r;
    PredictWork& pw = *f.work;
    hipStream_t st = f.st;
    const PredictModel md = predict_model_of(s, 0, E);
    const int npad = md.npad;
    if (npad != npad_m || predict_jac_nops(md) != nops) return fail(ctx, PILCO_E_STATE, "rollout_particles_cond: the model's padding changed under the plan");
    const int G = pl.G;
    if (noisy) ENSURE(pw.pc2_zeta, std::max((size_t)H * PE, (size_t)1));
    ENSURE(pw.pc2_rew, std::max((size_t)H * P, (size_t)1));
    if (H > 0) {
        ENSURE(pw.Ks, (size_t)E * G * npad);
        ENSURE(pw.out, (size_t)2 * E * G);
        ENSURE(pw.pc2_Wh, (size_t)H * nops * E * G * npad);
        ENSURE(pw.pc2_Xh, (size_t)H * D * G);
        ENSURE(pw.pc2_lam, (size_t)G * E * tri);
        if (o_cov) ENSURE(pw.pc2_cov, (size_t)G * E * tri);
        ENSURE(pw.pc2_info, (sizeof(int) * (size_t)G * E + 7) / 8);
    }
    h_parts.resize(particles ? (size_t)(H + 1) * PE : 0); h_eps.resize((eps_out && !eps) ? (size_t)H * PE : 0);
    h_zeta.resize((o_zeta && !eps_obs) ? (size_t)H * PE : 0);
    h_lam.resize(o_fac ? PE * tri : 0); h_cov.resize(o_cov ? PE * tri : 0);
    h_info.resize(H > 0 ? PE : 0); h_first.resize(first_hit ? (size_t)P * K : 0);
    h_counts.resize((size_t)(H + 1) * K);
    if (int r = f.upload()) return r;
    if (noisy && eps_obs && H > 0) HIPCHK(hipMemcpyAsync(pw.pc2_zeta.p, eps_obs, sizeof(double) * H * PE, hipMemcpyHostToDevice, st));

    ParticleHeadArgs& ha = f.ha;
    ca.n_rewards = n_rewards;
    ca.H = H; ca.P = P; ca.E = E; ca.D = D; ca.npad = npad; ca.nops = nops; ca.seed = seed; ca.jitter = jitter;
    ca.ls = md.ls; ca.sf2 = md.sf2; ca.noise = md.sn2;
    ca.eps = pw.pt_eps.p; ca.eps_given = eps ? 1 : 0;
    ca.zeta = noisy ? pw.pc2_zeta.p : nullptr; ca.zeta_given = (noisy && eps_obs) ? 1 : 0;
    ca.Lam = pw.pc2_lam.p; ca.Cov = o_cov ? pw.pc2_cov.p : nullptr;
    ca.info = reinterpret_cast<int*>(pw.pc2_info.p);
    const int waves = std::max(1, std::min(4, PC2_MAX_ROW / (nops * npad)));
    const size_t lds = sizeof(double) * (size_t)waves * nops * npad;
    for (int g0 = 0; g0 < P && H > 0; g0 += G) {
        const int ntc = std::min(G, P - g0), ldt = round_up(ntc, 64);
        const size_t sX = (size_t)D * ldt, sW = (size_t)nops * E * ldt * npad;
        double *out_mean = pw.out.p, *out_var = pw.out.p + (size_t)E * ldt;
        HIPCHK(hipMemsetAsync(pw.pc2_info.p, 0, sizeof(int) * (size_t)ldt * E, st));
        ha.p0 = ca.p0 = g0; ha.ntc = ca.ntc = ntc; ha.ldt = ca.ldt = ldt;
        ca.Wh = pw.pc2_Wh.p; ca.Xh = pw.pc2_Xh.p; ca.mu = out_mean;
        for (int t = 0; t < H; ++t) {
            ha.x = ca.x = f.slab(t);
            ca.xn = f.slab(t + 1);
            ca.t = t;
            ca.rew = pw.pc2_rew.p + (size_t)t * P;
            ha.Xt = pw.pc2_Xh.p + (size_t)t * sX;
            launch_particle_head(st, ha);
            if (int r = predict_points_device(ctx, md, ha.Xt, ntc, ldt, pw.Ks.p, out_mean, out_var)) return r;
            if (int r = predict_points_w_device(ctx, md, ntc, ldt, pw.Ks.p, pw.pc2_Wh.p + (size_t)t * sW)) return r;
            const unsigned nb = (unsigned)(((size_t)ntc * E + waves - 1) / waves);
            hipLaunchKernelGGL(k_particle_cond_step, dim3(nb), dim3(64 * waves), lds, st, ca);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_info.data() + (size_t)g0 * E, pw.pc2_info.p, sizeof(int) * (size_t)ntc * E, hipMemcpyDeviceToHost, st));
        if (o_fac)
            HIPCHK(hipMemcpyAsync(h_lam.data() + (size_t)g0 * E * tri, pw.pc2_lam.p, sizeof(double) * ntc * E * tri, hipMemcpyDeviceToHost, st));
        if (o_cov)
            HIPCHK(hipMemcpyAsync(h_cov.data() + (size_t)g0 * E * tri, pw.pc2_cov.p, sizeof(double) * ntc * E * tri, hipMemcpyDeviceToHost, st));
    }

    // the statistics and events of every state, over all particles: the launches and the order of pilco_rollout_particles
    for (int t = 0; t <= H; ++t)
        if (int r = f.state(t, t > 0 ? pw.pc2_rew.p + (size_t)(t - 1) * P : nullptr)) return r;
    // one download into staging memory, one synchronisation
    if (int r = f.download(particles ? h_parts.data() : nullptr, h_eps.empty() ? nullptr : h_eps.data())) return r;
    if (!h_zeta.empty()) HIPCHK(hipMemcpyAsync(h_zeta.data(), pw.pc2_zeta.p, sizeof(double) * H * PE, hipMemcpyDeviceToHost, st));
    if (int r = f.download_events(h_counts.data(), h_first.data())) return r;
    HIPCHK(hipStreamSynchronize(st));
    // the earliest step with a pivot that was not positive; at that step the lowest particle, then the lowest output
    long bad = -1;
    for (size_t k = 0; k < h_info.size(); ++k)
        if (h_info[k] != 0 && (bad < 0 || h_info[k] < h_info[bad])) bad = (long)k;
    if (bad >= 0) {
        ctx->not_pd = (int)(bad % E);
        return fail(ctx, PILCO_E_NOT_PD, "rollout_particles_cond: the path covariance + jitter*sf2*I of particle " + std::to_string(bad / E) +
                                             ", output " + std::to_string(bad % E) + " is not positive definite at step " +
                                             std::to_string(h_info[bad] - 1));
    }
    if (particles) memcpy(particles, h_parts.data(), sizeof(double) * h_parts.size());
    if (eps_out && H > 0) memcpy(eps_out, eps ? eps : h_eps.data(), sizeof(double) * H * PE);
    if (o_zeta && H > 0) memcpy(o_zeta, eps_obs ? eps_obs : h_zeta.data(), sizeof(double) * H * PE);
    if (K > 0) {
        memcpy(counts, h_counts.data(), sizeof(long long) * h_counts.size());
        if (first_hit) memcpy(first_hit, h_first.data(), f.fh_bytes);
    }
    for (size_t k = 0; k < PE && H > 0; ++k) {
        if (o_fac) cond_unpack(h_lam.data() + k * tri, H, o_fac + k * (size_t)H * H);
        if (o_cov) cond_unpack(h_cov.data() + k * tri, H, o_cov + k * (size_t)H * H);
    }
    f.finish();
    return PILCO_OK;
}
