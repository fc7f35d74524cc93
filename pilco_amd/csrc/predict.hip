// GP posterior at deterministic test inputs (GPflow GPR.predict_f / GPRFITC.predict_f, full_cov = False):
// pilco_gp_predict_points.  DESIGN.md section 12.
//   exact GP:  mean = K*^T beta,   var = sf2 - || L^{-1} K* ||^2
//   FITC:      mean = Ku*^T beta,  var = sf2 - || Luu^{-1} Ku* ||^2 + sn2 || iAt Ku* ||^2   (iAt = Am^{-1} Luu^{-1}, smgpr.py:36-37)
// The cross-covariances of a chunk of test points are built by launch_gram; one kernel then walks the row blocks of the stacked
// operator [L^{-1}; (iAt;) beta^T] on v_mfma_f64_16x16x4_f64 and squares and sums every product tile in registers: the product
// W = L^{-1} K* never leaves the chip.
// predict_points_device is that pair of launches, device to device and without a wait (predict.h): pilco_gp_predict_points
// wraps it in upload, download and synchronisation; the particle rollout (particles.hip) calls it per chunk of particles.
#include "predict.h"
#include "mm_device.h"

namespace pilco {

constexpr int PP_CT = 2;                    // 16-point column tiles per workgroup: 32 test points
constexpr int PP_RB = 4;                    // 16-row blocks per work unit: 64 operator rows
constexpr int PP_PTS = 16 * PP_CT;

struct PredictArgs {
    const double* Ks;     // [Eu][ldt][npad]: k(test point t, training / inducing point k); zero past n and past the chunk
    long sKs;
    const double* L;      // [Eu][npad][npad] L^{-1} (lower; only tiles on or below the diagonal are read)
    const double* iAt;    // FITC: [Eu][npad][npad] Am^{-1} Luu^{-1} (lower), nullptr for the exact GP
    long sL;
    const double* beta;   // [Eu][npad]
    const double* var;    // [Eu] kernel variance
    const double* noise;  // [Eu] likelihood variance (FITC)
    double* out_mean;     // [Eu][ldt]
    double* out_var;
    int n, npad, G, ntc, ldt;   // points of the operator, its padding, 64-row groups, test points in the chunk, their padding
};

// One workgroup: 32 test points of one output.  The work units -- 64-row groups of every operator block, and the beta row --
// are dealt over the four waves in a fixed order (largest groups first); each unit runs its own MFMA chain over the k
// chunks up to its diagonal, and the squares of its product tiles are added in a fixed order.  The waves' partial sums
// meet in LDS and are added in wave order: every test point's result depends on its own column of K* only.
__global__ __launch_bounds__(256) void k_predict_points(PredictArgs a) {
    const int e = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 15, h = lane >> 4;
    const int t0 = blockIdx.x * PP_PTS;
    const int n = a.n, npad = a.npad, G = a.G;
    const double* Ks = a.Ks + (long)e * a.sKs + (long)(t0 + c) * npad + 4 * h;   // lane's row of tile 0; tile ct: + 16 ct npad
    const double* beta = a.beta + (long)e * npad;
    const int nops = a.iAt ? 2 : 1;
    const int units = nops * G + 1;
    const int nkc = (n + 15) / 16;
    double sq0[PP_CT], sq1[PP_CT], mu[PP_CT];
#pragma unroll
    for (int ct = 0; ct < PP_CT; ++ct) sq0[ct] = sq1[ct] = mu[ct] = 0.0;
    for (int u = w; u < units; u += 4) {
        if (u == nops * G) {   // the beta row (in all 16 rows of the A operand): the mean
            d4 acc[PP_CT];
#pragma unroll
            for (int ct = 0; ct < PP_CT; ++ct) acc[ct] = d4{0.0, 0.0, 0.0, 0.0};
            for (int kc = 0; kc < nkc; ++kc) {
                const int k0 = 16 * kc + 4 * h;
                const d4 bv = *reinterpret_cast<const d4*>(beta + k0);
                d4 kv[PP_CT];
#pragma unroll
                for (int ct = 0; ct < PP_CT; ++ct) kv[ct] = *reinterpret_cast<const d4*>(Ks + (long)16 * ct * npad + 16 * kc);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const double av = (k0 + s < n) ? bv[s] : 0.0;
#pragma unroll
                    for (int ct = 0; ct < PP_CT; ++ct) {
                        acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, kv[ct][s], acc[ct], 0, 0, 0);
                        MFMA_KEEP_ALIVE(av);   // (the first MFMA of a chain has a constant-zero accumulator)
                        MFMA_KEEP_ALIVE(kv[ct][s]);
                    }
                }
            }
#pragma unroll
            for (int ct = 0; ct < PP_CT; ++ct) {
                MFMA_RESULT_FENCE(acc[ct]);
                mu[ct] = acc[ct][0];
            }
            continue;
        }
        const int op = u / G, g = G - 1 - (u - op * G);
        const double* A = (op ? a.iAt : a.L) + (long)e * a.sL;
        const int i0 = 64 * g + c;   // the lane's row in row block 0 of the group
        const double* Arow = A + (long)i0 * npad + 4 * h;
        d4 acc[PP_RB][PP_CT];
#pragma unroll
        for (int rb = 0; rb < PP_RB; ++rb)
#pragma unroll
            for (int ct = 0; ct < PP_CT; ++ct) acc[rb][ct] = d4{0.0, 0.0, 0.0, 0.0};
        const int kcend = min(4 * g + 4, nkc);   // lower triangular: k <= the group's last row
        for (int kc = 0; kc < kcend; ++kc) {
            const int k0 = 16 * kc + 4 * h;
            d4 av[PP_RB], kv[PP_CT];
#pragma unroll
            for (int rb = 0; rb < PP_RB; ++rb) av[rb] = *reinterpret_cast<const d4*>(Arow + (long)16 * rb * npad + 16 * kc);
#pragma unroll
            for (int ct = 0; ct < PP_CT; ++ct) kv[ct] = *reinterpret_cast<const d4*>(Ks + (long)16 * ct * npad + 16 * kc);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int rb = 0; rb < PP_RB; ++rb) {
                    const int i = i0 + 16 * rb;
                    // above the diagonal (never written by the factorisation) and past n (padding): zero
                    const double x = (k0 + s <= i && i < n) ? av[rb][s] : 0.0;
#pragma unroll
                    for (int ct = 0; ct < PP_CT; ++ct) {
                        acc[rb][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, kv[ct][s], acc[rb][ct], 0, 0, 0);
                        MFMA_KEEP_ALIVE(x);
                        MFMA_KEEP_ALIVE(kv[ct][s]);
                    }
                }
        }
#pragma unroll
        for (int rb = 0; rb < PP_RB; ++rb)
#pragma unroll
            for (int ct = 0; ct < PP_CT; ++ct) {
                MFMA_RESULT_FENCE(acc[rb][ct]);
                double q = op ? sq1[ct] : sq0[ct];
#pragma unroll
                for (int r = 0; r < 4; ++r) q = fma(acc[rb][ct][r], acc[rb][ct][r], q);
                if (op) sq1[ct] = q; else sq0[ct] = q;
            }
    }
    __shared__ double red[4][2][PP_PTS][4];   // [wave][operator block][test point][row group h of the tile]
    __shared__ double redm[4][PP_PTS];
#pragma unroll
    for (int ct = 0; ct < PP_CT; ++ct) {
        red[w][0][16 * ct + c][h] = sq0[ct];
        red[w][1][16 * ct + c][h] = sq1[ct];
        if (h == 0) redm[w][16 * ct + c] = mu[ct];   // (every row of the beta tile holds the mean)
    }
    __syncthreads();
    const int tl = threadIdx.x;
    if (tl < PP_PTS && t0 + tl < a.ntc) {
        double s0 = 0.0, s1 = 0.0, m = 0.0;
        for (int ww = 0; ww < 4; ++ww) {
            s0 += (red[ww][0][tl][0] + red[ww][0][tl][1]) + (red[ww][0][tl][2] + red[ww][0][tl][3]);
            s1 += (red[ww][1][tl][0] + red[ww][1][tl][1]) + (red[ww][1][tl][2] + red[ww][1][tl][3]);
            m += redm[ww][tl];
        }
        double v = a.var[e] - s0;
        if (a.iAt) v = fma(a.noise[e], s1, v);
        a.out_mean[(long)e * a.ldt + t0 + tl] = m;
        a.out_var[(long)e * a.ldt + t0 + tl] = v;
    }
}

}  // namespace pilco

using namespace pilco;

void predict_release(Slot& s) {
    if (!s.pred) return;
    PredictWork& p = *s.pred;
    for (DevBuf* b : {&p.raw, &p.Xt, &p.Ks, &p.out, &p.jac, &p.jacW, &p.pt_x, &p.pt_eps, &p.pt_rew, &p.pt_part, &p.pt_stats, &p.pt_par,
                      &p.pt_ev_first, &p.pt_ev_part, &p.pt_ev_counts, &p.pg_A, &p.pg_lam, &p.pg_ds, &p.pg_part, &p.pg_rew, &p.pg_out,
                      &p.fn_om, &p.fn_ph, &p.fn_Wt, &p.fn_phix, &p.fn_R, &p.fn_V, &p.fn_xi, &p.fn_raw,
                      &p.pc_cov, &p.pc_fac, &p.pc_linv, &p.pc_z, &p.pc_f, &p.pc_zraw, &p.pc_smp,
                      &p.pc2_Wh, &p.pc2_Xh, &p.pc2_lam, &p.pc2_cov, &p.pc2_zeta, &p.pc2_rew, &p.pc2_info})
        b->release();
    Slot& f = p.fitc;
    for (ChainGraph* cg : {&f.g_fact, &f.g_fitc, &f.g_fitc_nlml}) chain_graph_release(*cg);
    for (DevBuf* b : {&f.Xt, &f.Yt, &f.Zt, &f.ls, &f.var, &f.noise, &f.K, &f.Linv, &f.iK, &f.beta, &f.Tscr, &f.ksplit_ws, &f.vec,
                      &f.Kmn, &f.V2, &f.Am, &f.AmInv, &f.iAt, &f.G, &f.own, &f.ft_Z})
        b->release();
    delete s.pred;
    s.pred = nullptr;
}

static void view(DevBuf& b, double* p) {
    b.release();
    b.p = p;
    b.cap = 0;
    b.borrowed = true;
}

// FITC operands (Luu^{-1}, iAt, beta) of outputs e0 .. e0 + Eu - 1, each on its own inducing inputs Z_all[e] (host (E, M, D)):
// pilco_factorize_fitc on the prediction slot, whose Zt holds one point set per output
int factorize_own_z(pilco_ctx* ctx, Slot& s, PredictWork& pw, const double* Z_all, int e0, int Eu) {
    Slot& f = pw.fitc;
    const int D = s.D, M = s.M, Mp = s.npad;
    f.N = s.N; f.D = D; f.E = Eu; f.M = M; f.Npad = s.Npad; f.npad = Mp; f.n = M;
    f.has_data = f.has_hyp = true;
    view(f.Xt, s.Xt.p);
    view(f.Yt, s.Yt.p + (size_t)e0 * s.Npad);
    view(f.ls, s.ls.p + (size_t)e0 * D);
    view(f.var, s.var.p + e0);
    view(f.noise, s.noise.p + e0);
    f.Zstride = (long)D * Mp;
    ENSURE(f.ft_Z, (size_t)Eu * M * D);
    ENSURE(f.Zt, (size_t)Eu * D * Mp);
    HIPCHK(hipMemcpyAsync(f.ft_Z.p, Z_all + (size_t)e0 * M * D, sizeof(double) * Eu * M * D, hipMemcpyHostToDevice, ctx->st));
    launch_transpose_points(ctx->st, f.ft_Z.p, M, D, f.Zt.p, Mp, Eu, (long)M * D, (long)D * Mp);
    ctx->not_pd = -1;
    if (int r = pilco_factorize_fitc(ctx, &f)) {
        if (ctx->not_pd >= 0) ctx->not_pd += e0;
        return r;
    }
    return PILCO_OK;
}

PredictModel predict_model_of(const Slot& s, int e0, int Eu) {
    const bool sparse = s.M > 0;
    PredictModel m{};
    m.n = sparse ? s.M : s.N;
    m.npad = sparse ? s.npad : s.Npad;
    m.D = s.D;
    m.Eu = Eu;
    const long mat = (long)m.npad * m.npad;
    m.Pt = sparse ? s.Zt.p : s.Xt.p;
    m.sP = 0;
    m.ls = s.ls.p + (size_t)e0 * s.D;
    m.sf2 = s.var.p + e0;
    m.sn2 = s.noise.p + e0;
    m.L = s.Linv.p + e0 * mat;
    m.iAt = sparse ? s.iAt.p + e0 * mat : nullptr;
    m.beta = s.beta.p + (size_t)e0 * m.npad;
    return m;
}

int predict_points_device(pilco_ctx* ctx, const PredictModel& m, const double* Xt, int ntc, int ldt, double* Ks, double* out_mean,
                          double* out_var) {
    hipStream_t st = ctx->st;
    launch_gram(st, Xt, ldt, ntc, m.Pt, m.npad, m.n, m.D, m.ls, m.sf2, m.Eu, Ks, ldt, m.npad, 0, nullptr, 0.0, 0, m.sP);
    PredictArgs a{};
    a.Ks = Ks; a.sKs = (long)ldt * m.npad;
    a.L = m.L; a.iAt = m.iAt; a.sL = (long)m.npad * m.npad;
    a.beta = m.beta; a.var = m.sf2; a.noise = m.sn2;
    a.out_mean = out_mean; a.out_var = out_var;
    a.n = m.n; a.npad = m.npad; a.G = (m.n + 63) / 64; a.ntc = ntc; a.ldt = ldt;
    hipLaunchKernelGGL(k_predict_points, dim3(ldt / PP_PTS, m.Eu), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    return PILCO_OK;
}

extern "C" int pilco_gp_predict_points(pilco_ctx* ctx, int slot, const double* Xs, int Nt, int output, const double* Z_all,
                                       double* mean, double* var) {
    if (int r = check_slot(ctx, slot)) return r;
    Slot& s = ctx->slot[slot];
    if (ctx->nranks != 1 || ctx->comm || s.shW > 1) return fail(ctx, PILCO_E_STATE, "predict_points: single rank only");
    if (!s.has_data || !s.has_hyp) return fail(ctx, PILCO_E_STATE, "predict_points needs set_data and set_hyp first");
    if (!Xs || !mean || !var || Nt <= 0) return fail(ctx, PILCO_E_SHAPE, "predict_points: null pointer or Nt <= 0");
    if (output < -1 || output >= s.E) return fail(ctx, PILCO_E_SHAPE, "predict_points: output must be -1 (all) or 0 <= output < E");
    if (Z_all && s.M == 0) return fail(ctx, PILCO_E_SHAPE, "predict_points: Z_all given for an exact GP slot");
    if (s.user_factors)
        return fail(ctx, PILCO_E_STATE, "predict_points: the slot holds factors set by pilco_gp_set_factors, not its own factorisation");
    HIPCHK(hipSetDevice(ctx->device));
    if (!s.factor_valid)   // (pilco_gp_nlml / pilco_gp_fitc_nlml use the factorisation's buffers as scratch)
        if (int r = pilco_gp_factorize(ctx, slot)) return r;
    if (!s.pred) s.pred = new PredictWork();
    PredictWork& pw = *s.pred;
    hipStream_t st = ctx->st;
    const int D = s.D, Eu = output < 0 ? s.E : 1, e0 = output < 0 ? 0 : output;
    // the operator blocks and the points of the cross-covariance, for outputs e0 ..
    PredictModel md = predict_model_of(s, e0, Eu);
    if (Z_all) {
        if (int r = factorize_own_z(ctx, s, pw, Z_all, e0, Eu)) return r;
        const Slot& f = pw.fitc;
        md.Pt = f.Zt.p; md.sP = f.Zstride;
        md.L = f.Linv.p; md.iAt = f.iAt.p; md.beta = f.beta.p;
    }
    const int npad = md.npad;
    // chunks of test points: the cross-covariance of a chunk is at most PP_KS_BUDGET doubles
    const int ntc_max = std::min(round_up(Nt, 64), predict_chunk_cap(Eu, npad));
    ENSURE(pw.raw, (size_t)ntc_max * D);
    ENSURE(pw.Xt, (size_t)D * ntc_max);
    ENSURE(pw.Ks, (size_t)Eu * ntc_max * npad);
    ENSURE(pw.out, (size_t)2 * Eu * ntc_max);
    for (int t0 = 0; t0 < Nt; t0 += ntc_max) {
        const int ntc = std::min(ntc_max, Nt - t0), ldt = round_up(ntc, 64);
        double *out_mean = pw.out.p, *out_var = pw.out.p + (size_t)Eu * ldt;
        HIPCHK(hipMemcpyAsync(pw.raw.p, Xs + (size_t)t0 * D, sizeof(double) * ntc * D, hipMemcpyHostToDevice, st));
        launch_transpose_points(st, pw.raw.p, ntc, D, pw.Xt.p, ldt);
        if (int r = predict_points_device(ctx, md, pw.Xt.p, ntc, ldt, pw.Ks.p, out_mean, out_var)) return r;
        HIPCHK(hipMemcpy2DAsync(mean + t0, sizeof(double) * Nt, out_mean, sizeof(double) * ldt, sizeof(double) * ntc, Eu,
                                hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpy2DAsync(var + t0, sizeof(double) * Nt, out_var, sizeof(double) * ldt, sizeof(double) * ntc, Eu,
                                hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));   // (the chunk's buffers are reused by the next)
    }
    return PILCO_OK;
}
