// Policy gradients through particle rollouts: pilco_rollout_particles_grad / _grad_rbf.  docs/particle_gradients.md.
// With fixed initial particles and fixed draws the particle return J = sum_t (1/P) sum_p r(x_t^p) is a smooth function of the
// controller parameters; this is its pathwise (reparameterisation) gradient, by a reverse sweep over stored step matrices.
//
// FORWARD, per step t and per chunk of particles: the launches of pilco_rollout_particles (k_particle_head,
// predict_points_device, k_particle_tail: the same states and rewards, bit for bit) and, for t < H - 1,
//   predict_points_jac_device (predict_jac.hip)   d mu / d z, d v / d z at z = [x, u]: two launches
//   k_pg_fold        A_t[e][d] = [e == d] + d mu_e / d z_d + g_e d v_e / d z_d,  g_e = eps_e / (2 sd_e) where v~_e > 0, else 0,
//                    stored [t][e][d][particle]: the particle index fastest
//   k_pg_reward_partials   the blocks' reward sums of the step (the sums of k_particle_partials)
// REVERSE, t = H-1 .. 0, one launch over the group's particles, one thread per particle, its vectors parked in LDS:
//   k_pg_reverse     g_u = A[:, E:]^T lam,  ds_k = g_u[k] scale_k cos(s_k),  lam' = A[:, :E]^T lam + (ds/dx)^T ds + grad r(x_t)
//                    (step H - 1 meets lam_H = 0: its matrix is neither computed nor read)
//   k_pg_param_partials   (t <= H - 2) per block of PT_BLOCK particles and per parameter the block's sum, added to the block's cell
// and after the last group  k_pg_finish: the blocks' cells in block order, divided by P.
// An MLP policy (pilco_rollout_particles_grad_mlp; docs/particle_mlp.md) has a branch of its own in the reverse step (compiled
// into k_pg_reverse_mlp, an instance of k_pg_reverse's body) and in
// k_pg_param_partials; its hidden units are evaluated by mlp_hidden (particles.h), the statements of k_particle_head, on LDS copies of the parameters.
// The host side of a call -- plan, buffers, staging, the sweep over the groups, the finish -- is ParticleGradFrame
// (particle_frame.hip); the driver here passes it the forward launches of one step of a group.
//
// ORDER OF THE PARAMETER SUMS (no floating-point atomics): the particles are cut into blocks of PT_BLOCK = 128 consecutive
// indices; one thread per quantity adds a block's particles of one step in index order (from zero) and adds that sum to the
// block's cell, steps in the order t = H-2 .. 0; the blocks' cells are added in block order; one division by P.  The reward sums
// are those of pilco_rollout_particles.  Neither depends on the chunks or on the groups.
//
// GROUPS: the stored matrices take (H-1) P E D doubles.  Above the budget (PG_BUDGET doubles; PILCO_PARTICLE_GRAD_BUDGET in the
// environment, read at every call) the particles run in groups of a multiple of PT_BLOCK particles, each forward then reverse;
// the particles are independent and a block never straddles two groups, so every output has the bits of the one-group run.
#include "particles.h"

namespace pilco {

constexpr size_t PG_BUDGET = size_t(1) << 27;   // doubles of stored step matrices per group (1 GiB)

struct PgFoldArgs {
    const double *dmean, *dvar;   // [E][ldt][D] of the chunk
    const double* var;            // [E][ldt]
    const double* noise;          // [E] or nullptr
    const double* eps;            // [P][E] the step's draws
    double* A;                    // [E][D][ldg] the step's matrices of the group
    int p0, l0, ntc, ldt, ldg, E, D;   // p0: first particle of the chunk, l0: its index in the group
};

// thread (i, e): row e of particle i's step matrix
__global__ __launch_bounds__(256) void k_pg_fold(PgFoldArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
    if (i >= a.ntc) return;
    const int D = a.D;
    double v = a.var[(long)e * a.ldt + i];
    if (a.noise) v += a.noise[e];
    // the clamp sd = sqrt(max(v, 0)) has no derivative at v <= 0
    const double g = v > 0.0 ? a.eps[(long)(a.p0 + i) * a.E + e] / (2.0 * sqrt(v)) : 0.0;
    const double* dm = a.dmean + ((long)e * a.ldt + i) * D;
    const double* dv = a.dvar + ((long)e * a.ldt + i) * D;
    double* A = a.A + (long)e * D * a.ldg + a.l0 + i;
    for (int d = 0; d < D; ++d) A[(long)d * a.ldg] = fma(g, dv[d], dm[d] + (d == e ? 1.0 : 0.0));
}

// thread b: the reward sum of block b0 + b at step t, the particles in index order (zeros past P, as k_particle_partials).
// part [blocks][H]
__global__ __launch_bounds__(64) void k_pg_reward_partials(const double* rew, double* part, int P, int b0, int nb, int t, int H) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    const long p0 = (long)(b0 + b) * PT_BLOCK;
    double s = 0.0;
    for (int k = 0; k < PT_BLOCK; ++k) s += (p0 + k < P) ? rew[p0 + k] : 0.0;
    part[(long)(b0 + b) * H + t] = s;
}

// MLP: the instance that holds the MLP policy's branch (k_pg_reverse_mlp).  With the branch inside k_pg_reverse the kernel takes
// 98 registers and kinds 0-2 lose a wave per SIMD (5 -> 4), so launch_pg_reverse picks the kernel by kind
template <bool MLP>
__device__ __forceinline__ void pg_reverse_body(const PgReverseArgs& a) {
    extern __shared__ double pg_lds[];
    const ParticleHeadArgs& po = a.pol;
    const int E = po.E, U = po.U, D = E + U, tid = threadIdx.x, ldg = a.ldg;
    double* lam = pg_lds + tid;               // element e: lam[e * PG_RB]
    double* xs = lam + E * PG_RB;
    double* ln = xs + E * PG_RB;
    double* du = ln + E * PG_RB;
    double* il_s = pg_lds + (3 * E + U) * PG_RB;
    double* sc = il_s + U * E + tid;          // MLP policy: the pre-squash sums, element k: sc[k * PG_RB]; then the parameters
    const double* mlp_w = il_s + U * E + U * PG_RB;
    if (po.kind == PILCO_POLICY_RBF)
        for (int q = tid; q < U * E; q += PG_RB) il_s[q] = 1.0 / po.pls[q];
    if (MLP && po.kind == PILCO_POLICY_MLP) mlp_stage(po, il_s + U * E + U * PG_RB, tid, PG_RB);
    __syncthreads();
    const int l = blockIdx.x * PG_RB + tid;
    if (l >= po.ntc) return;
    const double* xr = po.x + (long)(po.p0 + l) * E;
    for (int e = 0; e < E; ++e) xs[e * PG_RB] = xr[e];
    if (a.A) {
        for (int e = 0; e < E; ++e) lam[e * PG_RB] = a.lam_in[(long)e * ldg + l];
        const double* A = a.A + l;
        for (int d = 0; d < D; ++d) {
            double acc = 0.0;
            for (int e = 0; e < E; ++e) acc = fma(A[((long)e * D + d) * ldg], lam[e * PG_RB], acc);
            if (d < E) ln[d * PG_RB] = acc; else du[(d - E) * PG_RB] = acc;
        }
    } else {
        for (int e = 0; e < E; ++e) ln[e * PG_RB] = 0.0;
        for (int k = 0; k < U; ++k) du[k * PG_RB] = 0.0;
    }
    // the MLP policy: ds_k = g_u[k] d u_k / d s_k into du, then delta_j and lam'_e += sum_j W1_je delta_j, j ascending; every
    // h_j comes from mlp_hidden twice with the same bits (no barrier below: a thread touches its own columns only)
    if (MLP && po.kind == PILCO_POLICY_MLP) {
        const int Hn = po.Hn;
        const double *W1 = mlp_w, *b1 = W1 + Hn * E, *W2 = b1 + Hn, *b2 = W2 + U * Hn;
        if (po.squash) {
            for (int k = 0; k < U; ++k) sc[k * PG_RB] = 0.0;
            for (int j = 0; j < Hn; ++j) {
                const double h = mlp_hidden(W1 + j * E, b1[j], xs, PG_RB, E);
                for (int k = 0; k < U; ++k) sc[k * PG_RB] = fma(W2[k * Hn + j], h, sc[k * PG_RB]);
            }
            for (int k = 0; k < U; ++k) {
                const double s = sc[k * PG_RB] + b2[k];
                du[k * PG_RB] = du[k * PG_RB] * (po.maxact[k] * cos(s));
            }
        }
        for (int j = 0; j < Hn; ++j) {
            const double dj = mlp_delta(W2 + j, Hn, mlp_hidden(W1 + j * E, b1[j], xs, PG_RB, E), du, PG_RB, U);
            for (int e = 0; e < E; ++e) ln[e * PG_RB] = fma(W1[j * E + e], dj, ln[e * PG_RB]);
        }
        for (int k = 0; k < U; ++k) a.ds[(long)k * ldg + l] = du[k * PG_RB];
    }
    // the policy: ds_k = g_u[k] d u_k / d s_k, lam' += (ds / dx)^T ds
    const int Uk = (MLP && po.kind == PILCO_POLICY_MLP) ? 0 : U;   // (the MLP policy: done above)
    for (int k = 0; k < Uk; ++k) {
        const double gu = du[k * PG_RB];
        double dsk = gu;
        if (po.kind == PILCO_POLICY_LINEAR) {
            if (po.squash) {
                double s = 0.0;
                for (int e = 0; e < E; ++e) s = fma(xs[e * PG_RB], po.W[k * E + e], s);
                s += po.b[k];
                dsk = gu * (po.maxact[k] * cos(s));
            }
            for (int e = 0; e < E; ++e) ln[e * PG_RB] = fma(po.W[k * E + e], dsk, ln[e * PG_RB]);
        } else if (po.kind == PILCO_POLICY_RBF) {
            const double vk = po.pvar[k];
            if (po.squash) {
                double s = 0.0;
                for (int c = 0; c < po.pn; ++c) {
                    double r2 = 0.0;
                    for (int e = 0; e < E; ++e) {
                        const double d = (xs[e * PG_RB] - po.pc[(long)e * po.pnpad + c]) * il_s[k * E + e];
                        r2 = fma(d, d, r2);
                    }
                    s = fma(po.pbeta[(long)k * po.pnpad + c], vk * exp(-0.5 * r2), s);
                }
                dsk = gu * (po.maxact[k] * exp(-0.5e-6) * cos(s));
            }
            for (int c = 0; c < po.pn; ++c) {
                double r2 = 0.0;
                for (int e = 0; e < E; ++e) {
                    const double d = (xs[e * PG_RB] - po.pc[(long)e * po.pnpad + c]) * il_s[k * E + e];
                    r2 = fma(d, d, r2);
                }
                const double w = dsk * po.pbeta[(long)k * po.pnpad + c] * (vk * exp(-0.5 * r2));
                for (int e = 0; e < E; ++e) {
                    const double il = il_s[k * E + e];
                    ln[e * PG_RB] = fma(-w, (xs[e * PG_RB] - po.pc[(long)e * po.pnpad + c]) * (il * il), ln[e * PG_RB]);
                }
            }
        }
        a.ds[(long)k * ldg + l] = dsk;
    }
    // the reward of the pre-step state: exponential grad r = -r/2 (W + W^T)(x - t), linear grad r = W
    for (int k = 0; k < a.n_rewards; ++k) {
        const ParticleReward& r = a.rw[k];
        if (r.kind == PILCO_REWARD_EXPONENTIAL) {
            double q = 0.0;
            for (int i = 0; i < E; ++i) {
                double row = 0.0;
                for (int j = 0; j < E; ++j) row = fma(r.W[i * E + j], xs[j * PG_RB] - r.t[j], row);
                q = fma(xs[i * PG_RB] - r.t[i], row, q);
            }
            const double c = -0.5 * r.coef * exp(-0.5 * q);
            for (int i = 0; i < E; ++i) {
                double row = 0.0;
                for (int j = 0; j < E; ++j) row = fma(r.W[i * E + j] + r.W[j * E + i], xs[j * PG_RB] - r.t[j], row);
                ln[i * PG_RB] = fma(c, row, ln[i * PG_RB]);
            }
        } else {
            for (int i = 0; i < E; ++i) ln[i * PG_RB] = fma(r.coef, r.W[i], ln[i * PG_RB]);
        }
    }
    for (int e = 0; e < E; ++e) a.lam_out[(long)e * ldg + l] = ln[e * PG_RB];
}

__global__ __launch_bounds__(PG_RB) void k_pg_reverse(PgReverseArgs a) { pg_reverse_body<false>(a); }
__global__ __launch_bounds__(PG_RB) void k_pg_reverse_mlp(PgReverseArgs a) { pg_reverse_body<true>(a); }

// block b of the group: particles PT_BLOCK b .. ; thread q adds quantity q over them in index order
__global__ __launch_bounds__(PT_BLOCK) void k_pg_param_partials(PgParamArgs a) {
    const ParticleHeadArgs& po = a.pol;
    const int E = po.E, U = po.U, Q = a.Q, bf = po.pn;
    __shared__ double sh[PT_BLOCK * MAX_D];        // [particle][x] then [particle][ds]
    __shared__ double il_s[MAX_D * MAX_D / 4];     // RbfController: 1 / lengthscale [U][E]  (U + E <= MAX_D)
    extern __shared__ double pt_tile[];            // MLP policy: [PT_BLOCK][PG_MLP_TILE + 1] the block's h, then delta, of a tile
    double* xs = sh;
    double* dss = sh + PT_BLOCK * E;
    const int i = threadIdx.x;
    const int l = blockIdx.x * PT_BLOCK + i;
    const int nv = min(PT_BLOCK, po.ntc - blockIdx.x * PT_BLOCK);   // the block's particles
    if (i < nv) {
        for (int e = 0; e < E; ++e) xs[i * E + e] = po.x[(long)(po.p0 + l) * E + e];
        for (int k = 0; k < U; ++k) dss[i * U + k] = a.ds[(long)k * a.ldg + l];
    }
    if (po.kind == PILCO_POLICY_RBF)
        for (int q = i; q < U * E; q += PT_BLOCK) il_s[q] = 1.0 / po.pls[q];
    __syncthreads();
    double* cell = a.part + (long)(po.p0 / PT_BLOCK + blockIdx.x) * Q;
    // the MLP policy, cells dW1 [Hn][E] | db1 [Hn] | dW2 [U][Hn] | db2 [U]: per tile of hidden units one tanh per (unit,
    // particle) -- thread i stages particle i's row -- then a thread per quantity over the particles in index order.  Every
    // thread reaches every barrier (five per tile): the bounds of the tile loop are uniform and nothing returns early
    if (po.kind == PILCO_POLICY_MLP) {
        const int Hn = po.Hn, ld = PG_MLP_TILE + 1;
        double *c_b1 = cell + Hn * E, *c_W2 = c_b1 + Hn, *c_b2 = c_W2 + U * Hn;
        double *w1 = pt_tile + PT_BLOCK * ld, *b1 = w1 + PG_MLP_TILE * E, *w2 = b1 + PG_MLP_TILE;   // the tile's parameters
        for (int j0 = 0; j0 < Hn; j0 += PG_MLP_TILE) {
            const int nj = min(PG_MLP_TILE, Hn - j0);
            __syncthreads();   // the readers of the tile before
            for (int q = i; q < nj * E; q += PT_BLOCK) w1[q] = po.W1[j0 * E + q];
            for (int q = i; q < nj; q += PT_BLOCK) b1[q] = po.b1[j0 + q];
            for (int q = i; q < U * nj; q += PT_BLOCK) w2[(q / nj) * PG_MLP_TILE + q % nj] = po.W2[(q / nj) * Hn + j0 + q % nj];
            __syncthreads();
            if (i < nv)
                for (int jj = 0; jj < nj; ++jj) pt_tile[i * ld + jj] = mlp_hidden(w1 + jj * E, b1[jj], xs + i * E, 1, E);
            __syncthreads();
            for (int q = i; q < U * nj; q += PT_BLOCK) {              // d W2_kj = sum ds_k h_j
                const int k = q / nj, jj = q - k * nj;
                double s = 0.0;
                for (int j = 0; j < nv; ++j) s = fma(dss[j * U + k], pt_tile[j * ld + jj], s);
                c_W2[k * Hn + j0 + jj] += s;
            }
            __syncthreads();
            if (i < nv)
                for (int jj = 0; jj < nj; ++jj)
                    pt_tile[i * ld + jj] = mlp_delta(w2 + jj, PG_MLP_TILE, pt_tile[i * ld + jj], dss + i * U, 1, U);
            __syncthreads();
            for (int q = i; q < nj * (E + 1); q += PT_BLOCK) {        // d W1_je = sum delta_j x_e, d b1_j = sum delta_j
                const int jj = q / (E + 1), e = q - jj * (E + 1);
                double s = 0.0;
                if (e < E) {
                    for (int j = 0; j < nv; ++j) s = fma(pt_tile[j * ld + jj], xs[j * E + e], s);
                    cell[(j0 + jj) * E + e] += s;
                } else {
                    for (int j = 0; j < nv; ++j) s += pt_tile[j * ld + jj];
                    c_b1[j0 + jj] += s;
                }
            }
        }
        for (int k = i; k < U; k += PT_BLOCK) {                       // d b2_k = sum ds_k
            double s = 0.0;
            for (int j = 0; j < nv; ++j) s += dss[j * U + k];
            c_b2[k] += s;
        }
        return;
    }
    // k_kc of particle j: the basis function as k_particle_head evaluates it
    auto basis = [&](int j, int k, int c) {
        double r2 = 0.0;
        for (int e = 0; e < E; ++e) {
            const double d = (xs[j * E + e] - po.pc[(long)e * po.pnpad + c]) * il_s[k * E + e];
            r2 = fma(d, d, r2);
        }
        return po.pvar[k] * exp(-0.5 * r2);
    };
    for (int q = i; q < Q; q += PT_BLOCK) {
        double s = 0.0;
        if (po.kind == PILCO_POLICY_LINEAR) {
            if (q < U * E) {
                const int k = q / E, e = q - k * E;
                for (int j = 0; j < nv; ++j) s = fma(dss[j * U + k], xs[j * E + e], s);
            } else {
                const int k = q - U * E;
                for (int j = 0; j < nv; ++j) s += dss[j * U + k];
            }
        } else if (q < U * bf) {                     // d beta_kc = sum ds_k k_kc
            const int k = q / bf, c = q - k * bf;
            for (int j = 0; j < nv; ++j) s = fma(dss[j * U + k], basis(j, k, c), s);
        } else if (q < U * bf + bf * E) {            // d C_ce = sum_k w_kc (x_e - c_ce) / l_ke^2
            const int ce = q - U * bf, c = ce / E, e = ce - c * E;
            const double cc = po.pc[(long)e * po.pnpad + c];
            for (int j = 0; j < nv; ++j)
                for (int k = 0; k < U; ++k) {
                    const double w = dss[j * U + k] * po.pbeta[(long)k * po.pnpad + c] * basis(j, k, c);
                    const double il = il_s[k * E + e];
                    s = fma(w, (xs[j * E + e] - cc) * (il * il), s);
                }
        } else {                                     // d l_ke = sum_c w_kc (x_e - c_ce)^2 / l_ke^3
            const int ke = q - U * bf - bf * E, k = ke / E, e = ke - k * E;
            const double il = il_s[ke], il3 = il * il * il;
            for (int j = 0; j < nv; ++j)
                for (int c = 0; c < bf; ++c) {
                    const double w = dss[j * U + k] * po.pbeta[(long)k * po.pnpad + c] * basis(j, k, c);
                    const double d = xs[j * E + e] - po.pc[(long)e * po.pnpad + c];
                    s = fma(w, d * d * il3, s);
                }
        }
        cell[q] += s;
    }
}

// thread q: the blocks' cells of quantity q in block order, over P.  part [nblk][Q] -> out [Q]
__global__ __launch_bounds__(PT_BLOCK) void k_pg_finish(const double* part, double* out, int nblk, int Q, int P) {
    const int q = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (q >= Q) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(long)b * Q + q];
    out[q] = s / (double)P;
}

}  // namespace pilco

using namespace pilco;

size_t pg_group_budget() {
    if (const char* v = getenv("PILCO_PARTICLE_GRAD_BUDGET")) {
        const long long n = atoll(v);
        if (n > 0) return (size_t)n;
    }
    return PG_BUDGET;
}

void launch_pg_reward_partials(hipStream_t st, const double* rew, double* part, int P, int b0, int nb, int t, int H) {
    hipLaunchKernelGGL(k_pg_reward_partials, dim3((nb + 63) / 64), dim3(64), 0, st, rew, part, P, b0, nb, t, H);
}

void launch_pg_reverse(hipStream_t st, const PgReverseArgs& a) {
    const int lds_bytes = (int)sizeof(double) * pg_reverse_lds_doubles(a.pol.E, a.pol.U, a.pol.kind, a.pol.Hn);
    const dim3 grid((a.pol.ntc + PG_RB - 1) / PG_RB);
    if (a.pol.kind == PILCO_POLICY_MLP) launch_lds<k_pg_reverse_mlp>(grid, dim3(PG_RB), lds_bytes, st, a);
    else launch_lds<k_pg_reverse>(grid, dim3(PG_RB), lds_bytes, st, a);
}

void launch_pg_param_partials(hipStream_t st, const PgParamArgs& a) {
    const size_t lds_bytes = sizeof(double) * pg_param_lds_doubles(a.pol.kind, a.pol.E, a.pol.U);
    launch_lds<k_pg_param_partials>(dim3((a.pol.ntc + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), lds_bytes, st, a);
}

void launch_pg_finish(hipStream_t st, const double* part, double* out, int nblk, int Q, int P) {
    hipLaunchKernelGGL(k_pg_finish, dim3((Q + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, st, part, out, nblk, Q, P);
}

namespace {

// The three entry points.  par: LinearController dW (U,E) | db (U); RbfController dbeta (U,bf) | dC (bf,E) | dl (U,E); MLP policy
// dW1 (Hn,E) | db1 (Hn) | dW2 (U,Hn) | db2 (U), over P.
// The frame (particle_frame.hip) holds what surrounds the forward pass
int rollout_particles_grad(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards, const double* x0,
                           int P, int H, const double* eps, unsigned long long seed, int observation_noise, double* reward,
                           double* reward_steps, std::vector<double>& par, double* dreturn_dx0) {
    ParticleGradFrame g(ctx, policy, rewards, n_rewards, x0, P, H, dreturn_dx0, par);
    const int E = g.E, D = g.D;
    const size_t PE = g.PE;
    if (H == 0) {
        *reward = 0.0;
        if (dreturn_dx0) std::fill(dreturn_dx0, dreturn_dx0 + PE, 0.0);
        return PILCO_OK;
    }
    ParticleTailArgs ta{};
    if (int r = g.open((size_t)H * PE, ta.rw)) return r;
    PredictWork& pw = *g.work;
    hipStream_t st = g.st;
    Slot& s = ctx->slot[PILCO_SLOT_DYNAMICS];
    const PredictModel md = predict_model_of(s, 0, E);
    const int npad = md.npad, ldg = g.pl.ldg;
    const int ntc_max = std::min(ldg, predict_chunk_cap(E, npad));
    ENSURE(pw.Xt, (size_t)D * ntc_max);
    ENSURE(pw.Ks, (size_t)E * ntc_max * npad);
    ENSURE(pw.out, (size_t)2 * E * ntc_max);
    if (H > 1) {
        ENSURE(pw.jac, (size_t)2 * E * ntc_max * D);
        ENSURE(pw.jacW, (size_t)predict_jac_nops(md) * E * ntc_max * npad);
    }
    if (int r = g.upload(eps)) return r;
    ParticleHeadArgs& ha = g.ha;
    ta.n_rewards = n_rewards; ta.E = E; ta.seed = seed;
    ta.noise = observation_noise ? s.noise.p : nullptr;
    ta.rew = pw.pt_rew.p;
    PgFoldArgs fa{};
    fa.noise = ta.noise; fa.ldg = ldg; fa.E = E; fa.D = D;
    auto step = [&](int g0, int ng, int t) {
        const bool jac = t < H - 1;
        double* eps_t = pw.pt_eps.p + (size_t)t * PE;
        ha.x = ta.x = g.slab(t);
        ta.xn = g.slab(t + 1);
        ta.t = t;
        ta.eps_in = eps ? eps_t : nullptr;
        ta.eps_out = eps ? nullptr : eps_t;
        for (int l0 = 0; l0 < ng; l0 += ntc_max) {
            const int p0 = g0 + l0, ntc = std::min(ntc_max, ng - l0), ldt = round_up(ntc, 64);
            double *out_mean = pw.out.p, *out_var = pw.out.p + (size_t)E * ldt;
            ha.Xt = pw.Xt.p; ha.p0 = p0; ha.ntc = ntc; ha.ldt = ldt;
            launch_particle_head(st, ha);
            if (int r = predict_points_device(ctx, md, pw.Xt.p, ntc, ldt, pw.Ks.p, out_mean, out_var)) return r;
            ta.mu = out_mean; ta.var = out_var; ta.p0 = p0; ta.ntc = ntc; ta.ldt = ldt;
            launch_particle_tail(st, ta);
            if (!jac) continue;
            double *dm = pw.jac.p, *dv = pw.jac.p + (size_t)E * ldt * D;
            if (int r = predict_points_jac_device(ctx, md, pw.Xt.p, ntc, ldt, pw.Ks.p, pw.jacW.p, dm, dv)) return r;
            fa.dmean = dm; fa.dvar = dv; fa.var = out_var; fa.eps = eps_t;
            fa.A = pw.pg_A.p + (size_t)t * E * D * ldg;
            fa.p0 = p0; fa.l0 = l0; fa.ntc = ntc; fa.ldt = ldt;
            hipLaunchKernelGGL(k_pg_fold, dim3((ntc + 255) / 256, E), dim3(256), 0, st, fa);
        }
        return (int)PILCO_OK;
    };
    if (int r = g.sweep(step)) return r;
    if (int r = g.finish_enqueue()) return r;
    HIPCHK(hipStreamSynchronize(st));
    g.finish(reward, reward_steps, par);
    return PILCO_OK;
}

}  // namespace

// the refusals of both entry points, before any launch or upload
int check_particle_grad_call(pilco_ctx* ctx, const char* who, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards, const double* x0, int P,
                    int H, const double* reward, int entry) {
    if (int r = check_particle_state(ctx, P, H)) return r;
    if (!x0 || !reward) return fail(ctx, PILCO_E_SHAPE, std::string(who) + ": null x0 or reward");
    if (int r = check_particle_terms(ctx, policy, rewards, n_rewards)) return r;
    if (entry != (policy->kind == PILCO_POLICY_NONE ? PILCO_POLICY_LINEAR : policy->kind))
        return fail(ctx, PILCO_E_SHAPE, std::string(who) + ": no policy or a LinearController (pilco_" + who + "), an "
                                        "RbfController (pilco_" + who + "_rbf), an MLP policy (pilco_" + who + "_mlp)");
    return PILCO_OK;
}

extern "C" int pilco_rollout_particles_grad(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards, int n_rewards,
                                            const double* x0, int P, int H, const double* eps, unsigned long long seed,
                                            int observation_noise, double* reward, double* reward_steps, double* dW, double* db,
                                            double* dreturn_dx0) {
    if (!ctx) return PILCO_E_SHAPE;
    if (int r = check_particle_grad_call(ctx, "rollout_particles_grad", policy, rewards, n_rewards, x0, P, H, reward, PILCO_POLICY_LINEAR)) return r;
    return pg_linear_entry(ctx, "rollout_particles_grad", policy, dW, db, [&](std::vector<double>& par) {
        return rollout_particles_grad(ctx, policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, reward, reward_steps, par,
                                      dreturn_dx0);
    });
}

extern "C" int pilco_rollout_particles_grad_rbf(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards,
                                                int n_rewards, const double* x0, int P, int H, const double* eps,
                                                unsigned long long seed, int observation_noise, const double* Xp, const double* Yp,
                                                const double* lsp, const double* noisep, int bf, double* reward, double* reward_steps,
                                                double* dX, double* dY, double* dls, double* dreturn_dx0) {
    if (!ctx) return PILCO_E_SHAPE;
    if (int r = check_particle_grad_call(ctx, "rollout_particles_grad", policy, rewards, n_rewards, x0, P, H, reward, PILCO_POLICY_RBF)) return r;
    return pg_rbf_entry(ctx, "rollout_particles_grad", policy, Xp, Yp, lsp, noisep, bf, dX, dY, dls, [&](std::vector<double>& par) {
        return rollout_particles_grad(ctx, policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, reward, reward_steps, par,
                                      dreturn_dx0);
    });
}

extern "C" int pilco_rollout_particles_grad_mlp(pilco_ctx* ctx, const pilco_policy* policy, const pilco_reward_term* rewards,
                                                int n_rewards, const double* x0, int P, int H, const double* eps,
                                                unsigned long long seed, int observation_noise, double* reward, double* reward_steps,
                                                double* dW1, double* db1, double* dW2, double* db2, double* dreturn_dx0) {
    if (!ctx) return PILCO_E_SHAPE;
    if (int r = check_particle_grad_call(ctx, "rollout_particles_grad", policy, rewards, n_rewards, x0, P, H, reward, PILCO_POLICY_MLP)) return r;
    return pg_mlp_entry(ctx, "rollout_particles_grad", policy, dW1, db1, dW2, db2, [&](std::vector<double>& par) {
        return rollout_particles_grad(ctx, policy, rewards, n_rewards, x0, P, H, eps, seed, observation_noise, reward, reward_steps, par,
                                      dreturn_dx0);
    });
}
