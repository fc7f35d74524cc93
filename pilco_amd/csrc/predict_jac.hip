// Input Jacobians of the GP posterior at deterministic test inputs: pilco_gp_predict_points_jac.  DESIGN.md section 12,
// docs/predict_jacobians.md.  With k_i = sf2 exp(-0.5 sum_d (X_id - x_d)^2 / l_d^2) and a = iK k*:
//   d mean / d x_d =      sum_i beta_i k_i (X_id - x_d) / l_d^2
//   d var  / d x_d = -2 * sum_i a_i    k_i (X_id - x_d) / l_d^2
// a = iK k* is formed through the triangular factors, never through the explicit matrix (whose rounding, cond(K) eps, reaches the
// result): exact GP  a = L^{-T} (L^{-1} k*);  FITC, iK = Kuu^{-1} - sn2 iAt^T iAt (smgpr.py:43-44),  a = Luu^{-T} (Luu^{-1} k*) -
// sn2 iAt^T (iAt k*) -- the factors predict.hip's variance is evaluated with.  The cross-covariances K* of the chunk are the
// ones predict_points_device left in Ks.  Two kernels on v_mfma_f64_16x16x4_f64:
//   k_predict_points_w    W_op = Op K* for Op = L^{-1} (and iAt, scaled by -sn2), the lower-triangular walk of k_predict_points,
//                         the product tiles stored instead of squared;
//   k_predict_points_jac  walks the 64-row groups of Op^T (upper triangular: k chunks from the group's diagonal on) over W_op,
//                         keeps the tiles of A = sum_op Op^T W_op in registers, multiplies every element by its k_it and
//                         contracts it against (X_id - x_td) / l_d^2, one input dimension at a time; the sums of a wave's
//                         units are parked in LDS, which serves every D the slot accepts without a register array indexed by d.
#include "predict.h"
#include "mm_device.h"

namespace pilco {

constexpr int PJ_CT = 2;                    // 16-point column tiles per workgroup: 32 test points
constexpr int PJ_RB = 4;                    // 16-row blocks per work unit: 64 rows
constexpr int PJ_PTS = 16 * PJ_CT;
constexpr int PJ_DB = 4;                    // input dimensions per pass of the mean unit

struct PredictJacArgs {
    const double* Ks;     // [Eu][ldt][npad]: k(test point t, training / inducing point i); zero past n and past the chunk
    long sKs;
    const double* L;      // [Eu][npad][npad] L^{-1} (lower; only tiles on or below the diagonal are read)
    const double* iAt;    // FITC: [Eu][npad][npad] Am^{-1} Luu^{-1} (lower), nullptr for the exact GP
    long sL;
    const double* noise;  // [Eu] likelihood variance (FITC)
    double* W;            // [nops][Eu][ldt][npad]: W_op[t][i] = (Op K*)_it, the second operator's times -sn2
    const double* beta;   // [Eu][npad]
    const double* Pt;     // [D][npad] points, transposed (per output: + e * sP)
    long sP;
    const double* ls;     // [Eu][D]
    const double* Xt;     // [D][ldt] the chunk's test points, transposed
    double* dmean;        // [Eu][ldt][D]
    double* dvar;
    int n, npad, G, ntc, ldt, D;
    int w_cov;            // k_predict_points_w: 0 the Jacobians' scaling above; 1 the covariance's (predict_cov.hip): the second operator's times sqrt(sn2)
};

// doubles of dynamic LDS: [4 waves][D][32 points] variance sums, [D][32] mean sums, [D] 1 / l_d^2
inline int predict_jac_lds_doubles(int D) { return 5 * D * PJ_PTS + D; }

// sum over the four row groups h of a tile column (lanes c, c + 16, c + 32, c + 48): (h0 + h1) + (h2 + h3) in every lane
// (the two operands of each addition only change places between lanes)
__device__ __forceinline__ double pj_sum_h(double v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// W_op = Op K*: a workgroup owns 32 test points of one output; its units, the 64-row groups of every operator block, are
// dealt over the four waves.  The walk of k_predict_points (k chunks up to the group's diagonal, the A operand zeroed above
// the diagonal and past n); every product tile is stored, all npad = 64 G rows of it, so nothing of W stays from an earlier call.
__global__ __launch_bounds__(256) void k_predict_points_w(PredictJacArgs a) {
    const int e = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 15, h = lane >> 4;
    const int t0 = blockIdx.x * PJ_PTS;
    const int n = a.n, npad = a.npad, G = a.G;
    const double* Ks = a.Ks + (long)e * a.sKs + (long)(t0 + c) * npad + 4 * h;
    const int nops = a.iAt ? 2 : 1;
    const int nkc = (n + 15) / 16;
    for (int u = w; u < nops * G; u += 4) {
        const int op = u / G, g = G - 1 - (u - op * G);
        const double* A = (op ? a.iAt : a.L) + (long)e * a.sL;
        const int i0 = 64 * g + c;
        const double* Arow = A + (long)i0 * npad + 4 * h;
        d4 acc[PJ_RB][PJ_CT];
#pragma unroll
        for (int rb = 0; rb < PJ_RB; ++rb)
#pragma unroll
            for (int ct = 0; ct < PJ_CT; ++ct) acc[rb][ct] = d4{0.0, 0.0, 0.0, 0.0};
        const int kcend = min(4 * g + 4, nkc);
        for (int kc = 0; kc < kcend; ++kc) {
            const int k0 = 16 * kc + 4 * h;
            d4 av[PJ_RB], kv[PJ_CT];
#pragma unroll
            for (int rb = 0; rb < PJ_RB; ++rb) av[rb] = *reinterpret_cast<const d4*>(Arow + (long)16 * rb * npad + 16 * kc);
#pragma unroll
            for (int ct = 0; ct < PJ_CT; ++ct) kv[ct] = *reinterpret_cast<const d4*>(Ks + (long)16 * ct * npad + 16 * kc);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int rb = 0; rb < PJ_RB; ++rb) {
                    const int i = i0 + 16 * rb;
                    const double x = (k0 + s <= i && i < n) ? av[rb][s] : 0.0;
#pragma unroll
                    for (int ct = 0; ct < PJ_CT; ++ct) {
                        acc[rb][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, kv[ct][s], acc[rb][ct], 0, 0, 0);
                        MFMA_KEEP_ALIVE(x);   // (the first MFMA of a chain has a constant-zero accumulator)
                        MFMA_KEEP_ALIVE(kv[ct][s]);
                    }
                }
        }
        // result register r of the lane: row 64 g + 16 rb + h + 4 r, point t0 + 16 ct + c
        const double sc = op ? (a.w_cov ? sqrt(a.noise[e]) : -a.noise[e]) : 1.0;
        double* Wt = a.W + (((long)op * gridDim.y + e) * a.ldt + t0 + c) * npad + 64 * g + h;
#pragma unroll
        for (int rb = 0; rb < PJ_RB; ++rb)
#pragma unroll
            for (int ct = 0; ct < PJ_CT; ++ct) {
                MFMA_RESULT_FENCE(acc[rb][ct]);
#pragma unroll
                for (int r = 0; r < 4; ++r) Wt[(long)16 * ct * npad + 16 * rb + 4 * r] = sc * acc[rb][ct][r];
            }
    }
}

// One workgroup: 32 test points of one output.  Work units: the G 64-row groups of A = sum_op Op^T W_op, then the mean unit; dealt over the
// four waves in index order.  A row-group unit runs its MFMA chain over the k chunks from its diagonal on, operator after operator, then, per input dimension d, each
// lane adds its sixteen elements a_it k_it (X_id - x_td) of a point in a fixed order (row blocks, then result registers),
// the four row groups h of the tile meet by lane exchange, and the wave adds the unit's sum to its own LDS cell (d, t):
// units in index order.  The mean unit does the same with beta_i in place of a_i (no product needed), PJ_DB dimensions
// per walk over the k chunks.  At the end the waves' sums are added in wave order.  No atomics; a test point's results
// depend on its own column of K* and its own coordinates only.
__global__ __launch_bounds__(256) void k_predict_points_jac(PredictJacArgs a) {
    extern __shared__ double pj_lds[];
    const int e = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 15, h = lane >> 4;
    const int t0 = blockIdx.x * PJ_PTS;
    const int n = a.n, npad = a.npad, G = a.G, D = a.D, ldt = a.ldt;
    const double* Ks = a.Ks + (long)e * a.sKs + (long)(t0 + c) * npad + 4 * h;   // lane's row of tile 0; tile ct: + 16 ct npad
    const double* beta = a.beta + (long)e * npad;
    const double* Pt = a.Pt + (long)e * a.sP + 4 * h;
    const double* Kse = a.Ks + (long)e * a.sKs + (long)(t0 + c) * npad + h;     // epilogue: element h + 4 r of a 16-row block
    const double* Pte = a.Pt + (long)e * a.sP + h;
    const double* Xt = a.Xt + t0 + c;                                             // dimension d, tile ct: + d ldt + 16 ct
    double* dv = pj_lds + w * D * PJ_PTS;
    double* dm = pj_lds + 4 * D * PJ_PTS;
    double* il2 = dm + D * PJ_PTS;
    for (int q = lane; q < D * PJ_PTS; q += 64) dv[q] = 0.0;
    if (threadIdx.x < D) {
        const double l = a.ls[(long)e * D + threadIdx.x];
        il2[threadIdx.x] = 1.0 / (l * l);
    }
    __syncthreads();
    const int units = G + 1;
    const int nops = a.iAt ? 2 : 1;
    const int nkc = (n + 15) / 16;
    for (int u = w; u < units; u += 4) {
        if (u == G) {   // the mean: weights beta_i k_it
            for (int d0 = 0; d0 < D; d0 += PJ_DB) {
                double s[PJ_DB][PJ_CT], x[PJ_DB][PJ_CT];
                const double* Pd[PJ_DB];
#pragma unroll
                for (int j = 0; j < PJ_DB; ++j) {
                    const int d = min(d0 + j, D - 1);   // (past D: the last dimension again, not stored)
                    Pd[j] = Pt + (long)d * npad;
#pragma unroll
                    for (int ct = 0; ct < PJ_CT; ++ct) {
                        s[j][ct] = 0.0;
                        x[j][ct] = Xt[(long)d * ldt + 16 * ct];
                    }
                }
                for (int kc = 0; kc < nkc; ++kc) {
                    const int k0 = 16 * kc + 4 * h;
                    const d4 bv = *reinterpret_cast<const d4*>(beta + k0);
                    d4 gk[PJ_CT];
#pragma unroll
                    for (int ct = 0; ct < PJ_CT; ++ct) {
                        const d4 kv = *reinterpret_cast<const d4*>(Ks + (long)16 * ct * npad + 16 * kc);
#pragma unroll
                        for (int r = 0; r < 4; ++r) gk[ct][r] = (k0 + r < n) ? bv[r] * kv[r] : 0.0;
                    }
#pragma unroll
                    for (int j = 0; j < PJ_DB; ++j) {
                        const d4 pv = *reinterpret_cast<const d4*>(Pd[j] + 16 * kc);
#pragma unroll
                        for (int ct = 0; ct < PJ_CT; ++ct)
#pragma unroll
                            for (int r = 0; r < 4; ++r) s[j][ct] = fma(gk[ct][r], pv[r] - x[j][ct], s[j][ct]);
                    }
                }
#pragma unroll
                for (int j = 0; j < PJ_DB; ++j) {
                    const int d = min(d0 + j, D - 1);
#pragma unroll
                    for (int ct = 0; ct < PJ_CT; ++ct) {
                        const double v = pj_sum_h(s[j][ct] * il2[d]);
                        if (h == 0 && d0 + j < D) dm[d * PJ_PTS + 16 * ct + c] = v;
                    }
                }
            }
            continue;
        }
        const int i0 = 64 * u + c;   // the lane's row in row block 0 of the group
        d4 acc[PJ_RB][PJ_CT];
#pragma unroll
        for (int rb = 0; rb < PJ_RB; ++rb)
#pragma unroll
            for (int ct = 0; ct < PJ_CT; ++ct) acc[rb][ct] = d4{0.0, 0.0, 0.0, 0.0};
        for (int op = 0; op < nops; ++op) {
            // A operand: Op^T, element (i, k) = Op[k][i] (the lanes c of a row block read neighbours of one row of Op)
            const double* At = (op ? a.iAt : a.L) + (long)e * a.sL + (long)(4 * h) * npad + i0;
            const double* Wt = a.W + (((long)op * gridDim.y + e) * ldt + t0 + c) * npad + 4 * h;
            for (int kc = 4 * u; kc < nkc; ++kc) {   // upper triangular: k >= the group's first row
                const int k0 = 16 * kc + 4 * h;
                double av[PJ_RB][4];
                d4 kv[PJ_CT];
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int rb = 0; rb < PJ_RB; ++rb) av[rb][s] = At[(long)(16 * kc + s) * npad + 16 * rb];
#pragma unroll
                for (int ct = 0; ct < PJ_CT; ++ct) kv[ct] = *reinterpret_cast<const d4*>(Wt + (long)16 * ct * npad + 16 * kc);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int rb = 0; rb < PJ_RB; ++rb) {
                        // below the diagonal of Op^T (never written by the factorisation) and past n (padding): zero
                        const double x = (k0 + s >= i0 + 16 * rb && k0 + s < n) ? av[rb][s] : 0.0;
#pragma unroll
                        for (int ct = 0; ct < PJ_CT; ++ct) {
                            acc[rb][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, kv[ct][s], acc[rb][ct], 0, 0, 0);
                            MFMA_KEEP_ALIVE(x);   // (the first MFMA of a chain has a constant-zero accumulator)
                            MFMA_KEEP_ALIVE(kv[ct][s]);
                        }
                    }
            }
        }
        // acc[rb][ct][r] = a_it of row i = 64 u + 16 rb + h + 4 r (the f64 result layout: row = (lane >> 4) + 4 * register),
        // point t = t0 + 16 ct + c: times k_it, from the row of Ks the lane reads its B operand from
#pragma unroll
        for (int rb = 0; rb < PJ_RB; ++rb)
#pragma unroll
            for (int ct = 0; ct < PJ_CT; ++ct) {
                MFMA_RESULT_FENCE(acc[rb][ct]);
                const double* kp = Kse + (long)16 * ct * npad + 64 * u + 16 * rb;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[rb][ct][r] *= kp[4 * r];
            }
        for (int d = 0; d < D; ++d) {
            d4 pv[PJ_RB];
#pragma unroll
            for (int rb = 0; rb < PJ_RB; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) pv[rb][r] = Pte[(long)d * npad + 64 * u + 16 * rb + 4 * r];
            const double sc = il2[d];
#pragma unroll
            for (int ct = 0; ct < PJ_CT; ++ct) {
                const double x = Xt[(long)d * ldt + 16 * ct];
                double s = 0.0;
#pragma unroll
                for (int rb = 0; rb < PJ_RB; ++rb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s = fma(acc[rb][ct][r], pv[rb][r] - x, s);   // the difference itself: no cancelling expansion
                s = pj_sum_h(s * sc);
                if (h == 0) dv[d * PJ_PTS + 16 * ct + c] += s;
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < PJ_PTS * D; q += 256) {
        const int tl = q / D, d = q - tl * D;
        if (t0 + tl >= a.ntc) continue;
        const int cell = d * PJ_PTS + tl;
        double sv = 0.0;
        for (int ww = 0; ww < 4; ++ww) sv += pj_lds[ww * D * PJ_PTS + cell];
        const long o = ((long)e * ldt + t0 + tl) * D + d;
        a.dmean[o] = dm[cell];
        a.dvar[o] = -2.0 * sv;
    }
}

}  // namespace pilco

using namespace pilco;

int predict_points_jac_device(pilco_ctx* ctx, const PredictModel& m, const double* Xt, int ntc, int ldt, const double* Ks,
                              double* W, double* dmean, double* dvar) {
    PredictJacArgs a{};
    a.Ks = Ks; a.sKs = (long)ldt * m.npad;
    a.L = m.L; a.iAt = m.iAt; a.sL = (long)m.npad * m.npad; a.noise = m.sn2; a.W = W;
    a.beta = m.beta; a.Pt = m.Pt; a.sP = m.sP; a.ls = m.ls; a.Xt = Xt;
    a.dmean = dmean; a.dvar = dvar;
    a.n = m.n; a.npad = m.npad; a.G = (m.n + 63) / 64; a.ntc = ntc; a.ldt = ldt; a.D = m.D;
    hipLaunchKernelGGL(k_predict_points_w, dim3(ldt / PJ_PTS, m.Eu), dim3(256), 0, ctx->st, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_predict_points_jac, dim3(ldt / PJ_PTS, m.Eu), dim3(256), sizeof(double) * predict_jac_lds_doubles(m.D),
                       ctx->st, a);
    HIPCHK(hipGetLastError());
    return PILCO_OK;
}

int predict_points_w_device(pilco_ctx* ctx, const PredictModel& m, int ntc, int ldt, const double* Ks, double* W) {
    PredictJacArgs a{};
    a.Ks = Ks; a.sKs = (long)ldt * m.npad;
    a.L = m.L; a.iAt = m.iAt; a.sL = (long)m.npad * m.npad; a.noise = m.sn2; a.W = W;
    a.n = m.n; a.npad = m.npad; a.G = (m.n + 63) / 64; a.ntc = ntc; a.ldt = ldt; a.D = m.D;
    a.w_cov = 1;
    hipLaunchKernelGGL(k_predict_points_w, dim3(ldt / PJ_PTS, m.Eu), dim3(256), 0, ctx->st, a);
    HIPCHK(hipGetLastError());
    return PILCO_OK;
}

extern "C" int pilco_gp_predict_points_jac(pilco_ctx* ctx, int slot, const double* Xs, int Nt, int output, const double* Z_all,
                                           double* mean, double* var, double* dmean, double* dvar) {
    if (int r = check_slot(ctx, slot)) return r;
    Slot& s = ctx->slot[slot];
    if (ctx->nranks != 1 || ctx->comm || s.shW > 1) return fail(ctx, PILCO_E_STATE, "predict_points_jac: single rank only");
    if (!s.has_data || !s.has_hyp) return fail(ctx, PILCO_E_STATE, "predict_points_jac needs set_data and set_hyp first");
    if (!Xs || !dmean || !dvar || Nt <= 0) return fail(ctx, PILCO_E_SHAPE, "predict_points_jac: null pointer or Nt <= 0");
    if (output < -1 || output >= s.E)
        return fail(ctx, PILCO_E_SHAPE, "predict_points_jac: output must be -1 (all) or 0 <= output < E");
    if (Z_all && s.M == 0) return fail(ctx, PILCO_E_SHAPE, "predict_points_jac: Z_all given for an exact GP slot");
    if (s.user_factors)
        return fail(ctx, PILCO_E_STATE,
                    "predict_points_jac: the slot holds factors set by pilco_gp_set_factors, not its own factorisation");
    HIPCHK(hipSetDevice(ctx->device));
    if (!s.factor_valid)
        if (int r = pilco_gp_factorize(ctx, slot)) return r;
    if (!s.pred) s.pred = new PredictWork();
    PredictWork& pw = *s.pred;
    hipStream_t st = ctx->st;
    const int D = s.D, Eu = output < 0 ? s.E : 1, e0 = output < 0 ? 0 : output;
    PredictModel md = predict_model_of(s, e0, Eu);
    if (Z_all) {
        if (int r = factorize_own_z(ctx, s, pw, Z_all, e0, Eu)) return r;
        const Slot& f = pw.fitc;
        md.Pt = f.Zt.p; md.sP = f.Zstride;
        md.L = f.Linv.p; md.iAt = f.iAt.p; md.beta = f.beta.p;
    }
    const int npad = md.npad;
    const int ntc_max = std::min(round_up(Nt, 64), predict_chunk_cap(Eu, npad));
    ENSURE(pw.raw, (size_t)ntc_max * D);
    ENSURE(pw.Xt, (size_t)D * ntc_max);
    ENSURE(pw.Ks, (size_t)Eu * ntc_max * npad);
    ENSURE(pw.out, (size_t)2 * Eu * ntc_max);
    ENSURE(pw.jac, (size_t)2 * Eu * ntc_max * D);
    ENSURE(pw.jacW, (size_t)predict_jac_nops(md) * Eu * ntc_max * npad);
    for (int t0 = 0; t0 < Nt; t0 += ntc_max) {
        const int ntc = std::min(ntc_max, Nt - t0), ldt = round_up(ntc, 64);
        double *out_mean = pw.out.p, *out_var = pw.out.p + (size_t)Eu * ldt;
        double *out_dm = pw.jac.p, *out_dv = pw.jac.p + (size_t)Eu * ldt * D;
        HIPCHK(hipMemcpyAsync(pw.raw.p, Xs + (size_t)t0 * D, sizeof(double) * ntc * D, hipMemcpyHostToDevice, st));
        launch_transpose_points(st, pw.raw.p, ntc, D, pw.Xt.p, ldt);
        // the values with the bits of pilco_gp_predict_points: its own launches, whose cross-covariances the Jacobians reuse
        if (int r = predict_points_device(ctx, md, pw.Xt.p, ntc, ldt, pw.Ks.p, out_mean, out_var)) return r;
        if (int r = predict_points_jac_device(ctx, md, pw.Xt.p, ntc, ldt, pw.Ks.p, pw.jacW.p, out_dm, out_dv)) return r;
        if (mean)
            HIPCHK(hipMemcpy2DAsync(mean + t0, sizeof(double) * Nt, out_mean, sizeof(double) * ldt, sizeof(double) * ntc, Eu,
                                    hipMemcpyDeviceToHost, st));
        if (var)
            HIPCHK(hipMemcpy2DAsync(var + t0, sizeof(double) * Nt, out_var, sizeof(double) * ldt, sizeof(double) * ntc, Eu,
                                    hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpy2DAsync(dmean + (size_t)t0 * D, sizeof(double) * Nt * D, out_dm, sizeof(double) * ldt * D,
                                sizeof(double) * ntc * D, Eu, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpy2DAsync(dvar + (size_t)t0 * D, sizeof(double) * Nt * D, out_dv, sizeof(double) * ldt * D,
                                sizeof(double) * ntc * D, Eu, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));   // (the chunk's buffers are reused by the next)
    }
    return PILCO_OK;
}
