// What the function-sample rollout (particles_fn.hip) shares with its gradient (particles_fn_grad.hip): the arguments and the
// body of the step kernel -- ONE statement of the value arithmetic, which k_particle_fn_step instantiates without and
// k_particle_fn_step_jac with the Jacobian sums -- and the host side of a call's set-up (the checks of the draws and of the
// budget, the set-up launches, the return of the draws).  The set-up kernels themselves live in particles_fn.hip.
#pragma once
#include "particles.h"
#include "philox_normal.h"

namespace pilco {

constexpr int FN_TILE = 64;
constexpr int FN_WAVES = 8;                  // waves of a step workgroup
constexpr int FN_SHARE = FN_TILE / FN_WAVES;   // indices of a tile per wave

struct ParticleFnArgs {
    const double* x;        // [P][E] the step's states
    double* xn;             // [P][E] the next states
    const double* Xq;       // [D][ldq] the step's [x, u] of the particles p0 .., transposed (k_particle_head)
    const double* Xt;       // [D][npad] training points
    const double *ls, *sf2; // [E][D], [E]
    const double* noise;    // [E] likelihood variances (observation_noise), or nullptr
    const double *om, *ph;  // [E][L][D], [E][L]
    const double* Wt;       // [E][Lpad][Ppad]
    const double* V;        // [E][npad][Ppad]
    const double* eps_in;   // [P][E] the step's draws (observation_noise), or nullptr: generated here
    double* eps_out;        // [P][E] the draws used, or nullptr
    double* rew;            // [P] reward of the pre-step state
    unsigned long long seed;
    int t, P, Ppad, E, D, N, npad, L, Lpad, n_rewards;
    int p0, ldq;            // the launch's first particle (a multiple of 64) and the leading dimension of Xq
    ParticleReward rw[MAX_REWARD_TERMS];
};

// the Jacobian half of k_particle_fn_step_jac: row e of the step matrices of the launch's particles
struct ParticleFnJac {
    double* A;   // [E][D][ldg] the step's matrices of the group; particle p at column p - p0
    int ldg;
};

constexpr int FN_JR = FN_WAVES;   // inputs d per round of the Jacobian's wave sums: wave w adds input 8 r + w in round r

#if defined(__HIPCC__)
// LDS of a step workgroup.  JAC adds the lengthscales' reciprocals (uniform over the workgroup: they leave the registers)
// and one round of the Jacobian's wave sums.
template <int DM, bool JAC>
struct FnJacLds {};
template <int DM>
struct FnJacLds<DM, true> {
    double il[DM];                        // 1 / lengthscale [D]
    double jred[FN_JR][FN_WAVES][64];     // [d of the round][wave][lane]
};
template <int DM, bool JAC>
struct FnStepLds {
    double tile[FN_TILE * DM];        // [index][D]: training points, then frequencies
    double tph[FN_TILE];              // phases of the feature tile
    double red[2][FN_WAVES][64];      // the waves' sums [K | F][wave][lane]
    FnJacLds<DM, JAC> j;
};

// The waves' Jacobian sums J[d] of one phase, combined in wave order: round r parks the inputs 8 r .. 8 r + 7 of every wave
// in LDS and wave w adds input d = 8 r + w over the waves 0 .. 7 into out[r].  Every wave arrives (barriers inside).
template <int DM>
__device__ __forceinline__ void fn_jac_combine(double (&jred)[FN_JR][FN_WAVES][64], const double (&J)[DM], double (&out)[(DM + FN_JR - 1) / FN_JR],
                                               int D, int w, int lane) {
#pragma unroll
    for (int r = 0; r < (DM + FN_JR - 1) / FN_JR; ++r) {
        out[r] = 0.0;
        if (r * FN_JR < D) {   // (uniform)
            __syncthreads();
#pragma unroll
            for (int j = 0; j < FN_JR; ++j)
                if (r * FN_JR + j < DM) jred[j][w][lane] = J[r * FN_JR + j];
            __syncthreads();
            if (r * FN_JR + w < DM) {
                double s = jred[w][0][lane];
#pragma unroll
                for (int q = 1; q < FN_WAVES; ++q) s += jred[w][q][lane];   // wave order
                out[r] = s;
            }
        }
    }
}

// The step of 64 particles and ONE output e by a workgroup of FN_WAVES waves: the head of particles_fn.hip has the walk and
// the order of the value sums.  DM: the register build, D <= DM (the arithmetic of a particle is the same in every build: the
// loops over d run to D).  JAC: also row e of the particle's step matrix (docs/particle_fn_gradients.md), accumulated beside
// sK and sF -- per term i:  JK[d] = fma(exp(..) v_i, xt_d - X_id, JK[d]);  per term l:  JF[d] = fma(w_l sin(arg_l), omega_ld,
// JF[d]) -- in ONE array of D sums that serves the kernel phase, is combined over the waves and then serves the feature
// phase.  Nothing of JAC enters an operation of the value: states and rewards have the bits of the plain build.
template <int DM, bool JAC>
__device__ __forceinline__ void fn_step_body(const ParticleFnArgs& a, const ParticleFnJac& ja, FnStepLds<DM, JAC>& sh) {
    constexpr int NR = (DM + FN_JR - 1) / FN_JR;
    double (&tile)[FN_TILE * DM] = sh.tile;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int e = blockIdx.y, D = a.D, N = a.N, L = a.L, npad = a.npad, Ppad = a.Ppad;
    const long q0 = (long)blockIdx.x * 64 + lane;   // column of Xq (and of A)
    const long p = a.p0 + q0;                       // < Ppad
    [[maybe_unused]] double xt[DM], il[JAC ? 1 : DM], J[JAC ? DM : 1], JKs[JAC ? NR : 1];
#pragma unroll
    for (int d = 0; d < DM; ++d) {
        xt[d] = d < D ? a.Xq[(long)d * a.ldq + q0] : 0.0;
        if constexpr (JAC) J[d] = 0.0;
        else il[d] = d < D ? 1.0 / a.ls[e * D + d] : 0.0;
    }
    if constexpr (JAC)
        if (tid < DM) sh.j.il[tid] = tid < D ? 1.0 / a.ls[e * D + tid] : 0.0;   // (the first barrier of the walk publishes it)
    double sK = 0.0, sF = 0.0;
    const double* Ve = a.V + (long)e * npad * Ppad + p;
    for (int i0 = 0; i0 < N; i0 += FN_TILE) {
        __syncthreads();
        for (int q = tid; q < FN_TILE * D; q += 64 * FN_WAVES) {   // (i0 + ii < npad: the slot pads its points with zeros)
            const int d = q >> 6, ii = q & 63;
            tile[ii * D + d] = a.Xt[(long)d * npad + i0 + ii];
        }
        __syncthreads();
        const int end = min(FN_SHARE * (w + 1), N - i0);
#pragma unroll 1
        for (int k0 = FN_SHARE * w; k0 < end; k0 += 4) {   // (wave-uniform bounds; the loops inside unroll: xt, il, v stay in registers)
            double v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = Ve[(long)(i0 + k0 + k) * Ppad];   // rows < npad exist (zero past N)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ii = k0 + k;
                if (ii < end) {
                    double r2 = 0.0;
#pragma unroll
                    for (int d = 0; d < DM; ++d)
                        if (d < D) {
                            double ild;
                            if constexpr (JAC) ild = sh.j.il[d]; else ild = il[d];
                            const double s = (xt[d] - tile[ii * D + d]) * ild;
                            r2 = fma(s, s, r2);
                        }
                    const double ek = exp(-0.5 * r2);
                    sK = fma(ek, v[k], sK);
                    if constexpr (JAC) {
                        const double g = ek * v[k];
#pragma unroll
                        for (int d = 0; d < DM; ++d)
                            if (d < D) J[d] = fma(g, xt[d] - tile[ii * D + d], J[d]);
                    }
                }
            }
        }
    }
    if constexpr (JAC) {
        fn_jac_combine<DM>(sh.j.jred, J, JKs, D, w, lane);
#pragma unroll
        for (int d = 0; d < DM; ++d) J[d] = 0.0;
    }
    const double* We = a.Wt + (long)e * a.Lpad * Ppad + p;
    for (int l0 = 0; l0 < L; l0 += FN_TILE) {
        __syncthreads();
        for (int q = tid; q < FN_TILE * D; q += 64 * FN_WAVES) {
            const int ll = q / D, d = q - ll * D;
            tile[q] = (l0 + ll < L) ? a.om[((long)e * L + l0 + ll) * D + d] : 0.0;
        }
        if (tid < FN_TILE) sh.tph[tid] = (l0 + tid < L) ? a.ph[e * L + l0 + tid] : 0.0;
        __syncthreads();
        const int end = min(FN_SHARE * (w + 1), L - l0);
#pragma unroll 1
        for (int k0 = FN_SHARE * w; k0 < end; k0 += 4) {
            double v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = We[(long)(l0 + k0 + k) * Ppad];   // rows < Lpad exist (zero past L)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ll = k0 + k;
                if (ll < end) {
                    double arg = sh.tph[ll];
#pragma unroll
                    for (int d = 0; d < DM; ++d)
                        if (d < D) arg = fma(tile[ll * D + d], xt[d], arg);
                    sF = fma(v[k], cos(arg), sF);
                    if constexpr (JAC) {
                        const double g = v[k] * sin(arg);
#pragma unroll
                        for (int d = 0; d < DM; ++d)
                            if (d < D) J[d] = fma(g, tile[ll * D + d], J[d]);
                    }
                }
            }
        }
    }
    if constexpr (JAC) {
        // A[e][d] = [e == d] + fma(-(sf2 il_d^2), JK_d, -(A_e JF_d)) by the wave that combined input d
        double JFs[NR];
        fn_jac_combine<DM>(sh.j.jred, J, JFs, D, w, lane);
        const double sf2 = a.sf2[e], amp = sqrt(2.0 * sf2 / (double)L);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int d = r * FN_JR + w;
            if (d < D && p < a.P) {
                const double ild = sh.j.il[d];
                const double df = fma(-(sf2 * (ild * ild)), JKs[r], -(amp * JFs[r]));
                ja.A[((long)e * D + d) * ja.ldg + q0] = (d == e ? 1.0 : 0.0) + df;
            }
        }
    }
    sh.red[0][w][lane] = sK;
    sh.red[1][w][lane] = sF;
    __syncthreads();
    if (w != 0 || p >= a.P) return;
    double K = sh.red[0][0][lane], F = sh.red[1][0][lane];
#pragma unroll
    for (int q = 1; q < FN_WAVES; ++q) {   // wave order
        K += sh.red[0][q][lane];
        F += sh.red[1][q][lane];
    }
    const double sf2 = a.sf2[e];
    const double f = fma(sqrt(2.0 * sf2 / (double)L), F, sf2 * K);
    const int E = a.E;
    const double* xr = a.x + p * E;
    double xe = xr[e] + f;
    if (a.noise) {
        double z;
        if (a.eps_in) {
            z = a.eps_in[p * E + e];
        } else {
            double z0, z1;
            philox_normal_pair(a.seed, (uint32_t)a.t, (uint32_t)p, (uint32_t)(e >> 1), &z0, &z1);
            z = (e & 1) ? z1 : z0;
        }
        xe += sqrt(fmax(a.noise[e], 0.0)) * z;
        if (a.eps_out) a.eps_out[p * E + e] = z;
    }
    a.xn[p * E + e] = xe;
    if (e == 0) a.rew[p] = particle_reward(a, xr);
}
#endif

}  // namespace pilco

// ---- the host side of a function-sample call, shared by pilco_rollout_particles_fn and pilco_rollout_particles_fn_grad[_rbf]

// the sizes of a call, settled by fn_plan
struct FnPlan {
    int E, D, N, npad, L, Lpad, P, Ppad;
    bool own;                                // the caller gave the four draws
    size_t n_om, n_ph, n_w, n_xi, n_Wt, n_V;
};
// host staging of the draws a call returns (alive until the call's synchronisation)
struct FnDrawsStage {
    std::vector<double> w, xi, v;
};

// what pilco_rollout_particles_fn refuses about the slot, the draws and the budget, in its order; who: the message's prefix
int fn_plan(pilco_ctx* ctx, const char* who, const pilco_function_draws* draws, int P, FnPlan& pl);
// the fn_* buffers, the upload of the caller's draws and the set-up launches (features, weights, Phi(X), residuals, V)
int fn_setup(pilco_ctx* ctx, const FnPlan& pl, const pilco_function_draws* draws, const pilco_function_draws_out* draws_out,
             unsigned long long seed);
// the draws used: the downloads (before the call's synchronisation) and their way to the caller's layout (after it)
int fn_draws_download(pilco_ctx* ctx, const FnPlan& pl, const pilco_function_draws_out* draws_out, FnDrawsStage& stage);
void fn_draws_finish(const FnPlan& pl, const pilco_function_draws* draws, const pilco_function_draws_out* draws_out,
                     const FnDrawsStage& stage);
// k_particle_fn_step over the particles a.p0 .. a.p0 + count - 1 (count rounded up to 64 columns of Xq)
void launch_fn_step(hipStream_t st, const pilco::ParticleFnArgs& a, int count);
