// The full posterior covariance between test points and joint samples of the latent functions there (GPflow GPR.predict_f /
// GPRFITC.predict_f with full_cov = True, predict_f_samples): pilco_gp_predict_points_cov, pilco_gp_sample_points.
// DESIGN.md section 12, docs/predict_cov.md.  Per output, with w_a = L^{-1} k*(x_a):
//   exact GP:  cov_ab = k(x_a, x_b) - w_a . w_b
//   FITC:      cov_ab = k(x_a, x_b) - w0_a . w0_b + sn2 w1_a . w1_b,   w0 = Luu^{-1} ku*(x_a),  w1 = iAt ku*(x_a)
//   samples    f[s, :, e] = mean[:, e] + C_e z[s, :, e],   C_e C_e^T = cov_e + jitter I
// The cross-covariances and the mean are predict_points_device's (the mean's bits are pilco_gp_predict_points'), W = Op K* is
// k_predict_points_w's (predict_jac.hip) with the second operator scaled by sqrt(sn2) -- the same factor on both sides of the
// product, so that cov_ab and cov_ba are the same sums.  k_predict_cov contracts W against itself over all pairs of test points.
#include "predict.h"
#include "mm_device.h"
#include "lds_layout.h"
#include "philox_normal.h"

namespace pilco {

struct PredictCovArgs {
    const double* W;     // [nops][Eu][ldt][npad]: W_op[a][i] (rows past n and test points past nt: zero)
    const double* Xt;    // [D][ldt] the test points, transposed
    const double* ls;    // [Eu][D]
    const double* var;   // [Eu] kernel variance
    double* cov;         // [Eu][ldt][ldt]
    double* fac;         // nullptr, or [Eu][ldt][ldt]: cov + jitter I on the real diagonal, the tiles on and below the diagonal only
    double jitter;
    int nops, n, npad, nt, ldt, D;
};

// One workgroup: one 64 x 64 tile (bi >= bj) of one output's covariance; wave w owns the 32 x 32 quarter (w >> 1, w & 1) as
// 2 x 2 MFMA tiles.  Both operands are rows of W, read as k_predict_points reads its operands: the lane's d4 of row c at
// k = 16 kc + 4 h.  ONE accumulator chain per element: the operator rows of the first operator in index order, then (FITC)
// those of the second with the A operand negated; k(x_a, x_b) is formed in the epilogue, the sum over d in k_gram's order,
// and the chain's sum is subtracted from it last.  Element (a, b) is a function of rows a and b of W and of the two points only (a product commutes, the
// squared difference does not see the order): the same bits wherever the two points stand, for any nt, and for (b, a).
// Rows and columns past nt hold the identity.  The tile below the diagonal is turned around in LDS and stored as full rows
// of its mirror image.
__global__ __launch_bounds__(256) void k_predict_cov(PredictCovArgs a) {
    constexpr PredictCovLds lds = predict_cov_lds();
    __shared__ double sm[lds.total];
    const int bi = blockIdx.y, bj = blockIdx.x, e = blockIdx.z;
    if (bi < bj) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int c = lane & 15, h = lane >> 4;
    const int i0 = bi * PCOV_TILE + (w >> 1) * 32, j0 = bj * PCOV_TILE + (w & 1) * 32;
    const int npad = a.npad, ldt = a.ldt, D = a.D, Eu = gridDim.z;
    double* il = sm + lds.il;
    if (t < D) il[t] = 1.0 / a.ls[(long)e * D + t];
    d4 acc[2][2];
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[ra][cb] = d4{0.0, 0.0, 0.0, 0.0};
    const int nkc = (a.n + 15) / 16;
    // the lane's operands of chunk kc: two d4 of the A rows, two of the B rows
    auto fetch = [&](const double* Wa, const double* Wb, int kc, d4* av, d4* bv) {
#pragma unroll
        for (int ra = 0; ra < 2; ++ra) av[ra] = *reinterpret_cast<const d4*>(Wa + (long)16 * ra * npad + 16 * kc);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) bv[cb] = *reinterpret_cast<const d4*>(Wb + (long)16 * cb * npad + 16 * kc);
    };
    auto multiply = [&](const d4* av, const d4* bv, bool neg) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int ra = 0; ra < 2; ++ra) {
                const double x = neg ? -av[ra][s] : av[ra][s];   // (exact: the sign)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    acc[ra][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, bv[cb][s], acc[ra][cb], 0, 0, 0);
                    MFMA_KEEP_ALIVE(x);   // (the first MFMA of a chain has a constant-zero accumulator)
                    MFMA_KEEP_ALIVE(bv[cb][s]);
                }
            }
    };
    // acc = sum w0_a w0_b - sum (sqrt(sn2) w1_a) (sqrt(sn2) w1_b): the sign sits on the SECOND operator's A operand (the exact GP
    // negates nothing), the covariance is k - acc.  The next chunk's operands are requested before this chunk is multiplied
    // (two register sets in turn); a request past the last chunk reads the last chunk again.
    for (int op = 0; op < a.nops; ++op) {
        const double* Wo = a.W + ((long)op * Eu + e) * ldt * npad + 4 * h;
        const double* Wa = Wo + (long)(i0 + c) * npad;
        const double* Wb = Wo + (long)(j0 + c) * npad;
        const bool neg = op != 0;
        d4 av0[2], bv0[2], av1[2], bv1[2];
        fetch(Wa, Wb, 0, av0, bv0);
        for (int kc = 0; kc < nkc; kc += 2) {
            fetch(Wa, Wb, min(kc + 1, nkc - 1), av1, bv1);
            multiply(av0, bv0, neg);
            fetch(Wa, Wb, min(kc + 2, nkc - 1), av0, bv0);
            if (kc + 1 < nkc) multiply(av1, bv1, neg);
        }
    }
    __syncthreads();   // il
    // result register r of the lane: row i0 + 16 ra + h + 4 r, column j0 + 16 cb + c
    double r2[2][2][4];
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) r2[ra][cb][r] = 0.0;
    for (int d = 0; d < D; ++d) {
        const double* Xd = a.Xt + (long)d * ldt;
        const double ild = il[d];
        double xb[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) xb[cb] = Xd[j0 + 16 * cb + c];
#pragma unroll
        for (int ra = 0; ra < 2; ++ra)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double xa = Xd[i0 + 16 * ra + h + 4 * r];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const double diff = (xa - xb[cb]) * ild;
                    r2[ra][cb][r] = fma(diff, diff, r2[ra][cb][r]);
                }
            }
    }
    const double va = a.var[e];
    double* cov = a.cov + (long)e * ldt * ldt;
    double* fac = a.fac ? a.fac + (long)e * ldt * ldt : nullptr;
    double* tile = sm + lds.tile;
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            MFMA_RESULT_FENCE(acc[ra][cb]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ia = i0 + 16 * ra + h + 4 * r, ib = j0 + 16 * cb + c;
                double v;
                if (ia < a.nt && ib < a.nt)
                    v = va * exp(-0.5 * r2[ra][cb][r]) - acc[ra][cb][r];
                else
                    v = ia == ib ? 1.0 : 0.0;
                cov[(long)ia * ldt + ib] = v;
                if (fac) fac[(long)ia * ldt + ib] = (ia == ib && ia < a.nt) ? v + a.jitter : v;
                tile[(ib - bj * PCOV_TILE) * PCOV_TP + ia - bi * PCOV_TILE] = v;
            }
        }
    if (bi != bj) {
        __syncthreads();
        for (int q = t; q < PCOV_TILE * PCOV_TILE; q += 256)
            cov[(long)(bj * PCOV_TILE + (q >> 6)) * ldt + bi * PCOV_TILE + (q & 63)] = tile[(q >> 6) * PCOV_TP + (q & 63)];
    }
}

struct CovDrawArgs {
    const double* z_in;   // nullptr (Philox domain 5) or the caller's normals [S][Nt][Eu]
    double* z_raw;        // nullptr or [S][Nt][Eu]: the normals used, in the caller's layout
    double* Z;            // [Eu][ldt][Spad], zeroed before the launch
    unsigned long long seed;
    int S, Spad, nt, ldt, Eu, e0;
};
// one thread per (sample, test point, output): the normal of output e = e0 + el is half e & 1 of the block {s, a, e >> 1, 5}
__global__ __launch_bounds__(256) void k_cov_draws(CovDrawArgs a) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)a.S * a.nt * a.Eu) return;
    const int el = (int)(q % a.Eu), pt = (int)((q / a.Eu) % a.nt), s = (int)(q / ((long)a.Eu * a.nt));
    double z;
    if (a.z_in) {
        z = a.z_in[q];
    } else {
        const int e = a.e0 + el;
        double z0, z1;
        philox_domain_normal_pair(a.seed, (uint32_t)s, (uint32_t)pt, (uint32_t)(e >> 1), PHILOX_COV_Z, &z0, &z1);
        z = (e & 1) ? z1 : z0;
    }
    if (a.z_raw) a.z_raw[q] = z;
    a.Z[((long)el * a.ldt + pt) * a.Spad + s] = z;
}

// samples[s][a][el] = mean[el][a] + (C z)[el][a][s]
__global__ __launch_bounds__(256) void k_cov_samples(const double* __restrict__ F, const double* __restrict__ mean, double* __restrict__ out,
                                                     int S, int Spad, int nt, int ldt, int Eu) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)S * nt * Eu) return;
    const int el = (int)(q % Eu), pt = (int)((q / Eu) % nt), s = (int)(q / ((long)Eu * nt));
    out[q] = mean[(long)el * ldt + pt] + F[((long)el * ldt + pt) * Spad + s];
}

}  // namespace pilco

using namespace pilco;

namespace {

constexpr size_t PCOV_BUDGET = size_t(1) << 30;   // doubles of device memory a call may hold (8 GB)

size_t cov_budget() {
    if (const char* v = getenv("PILCO_PREDICT_COV_BUDGET")) {
        const long long n = atoll(v);
        if (n > 0) return (size_t)n;
    }
    return PCOV_BUDGET;
}

// doubles a call holds at Ntpad = ldt test points: the cross-covariances and W of every operator, nmat matrices of
// [Eu][ldt][ldt], and (samples) the normals and products [Eu][ldt][Spad] with their copies in the caller's layout
size_t cov_footprint(int nops, int Eu, int npad, size_t ldt, int nmat, int Spad) {
    return (size_t)(nops + 1) * Eu * ldt * npad + (size_t)nmat * Eu * ldt * ldt + (size_t)4 * Eu * ldt * Spad;
}

struct CovCall {
    Slot* s;
    PredictWork* pw;
    PredictModel md;
    int Eu, e0, D, ldt, nops;
    double *mean, *var;   // device, [Eu][ldt]
    PredictCovArgs args;  // of the covariance launch
};

// Checks, budget, factorisation, upload; then the mean (predict_points_device), W and the covariance kernel, all enqueued.
// nmat: matrices of [Eu][ldt][ldt] the call holds (1: the covariance; 3: its copy with the jitter and the factor's block
// inverses as well, which the launch then fills through `fac`).
int cov_enqueue(pilco_ctx* ctx, int slot, const char* who, const double* Xs, int Nt, int output, const double* Z_all, int nmat, int Spad,
                double jitter, CovCall& c) {
    const std::string pre = std::string(who) + ": ";
    if (int r = check_slot(ctx, slot)) return r;
    Slot& s = ctx->slot[slot];
    if (ctx->nranks != 1 || ctx->comm || s.shW > 1) return fail(ctx, PILCO_E_STATE, pre + "single rank only");
    if (!s.has_data || !s.has_hyp) return fail(ctx, PILCO_E_STATE, pre + "needs set_data and set_hyp first");
    if (!Xs || Nt <= 0) return fail(ctx, PILCO_E_SHAPE, pre + "null pointer or Nt <= 0");
    if (output < -1 || output >= s.E) return fail(ctx, PILCO_E_SHAPE, pre + "output must be -1 (all) or 0 <= output < E");
    if (Z_all && s.M == 0) return fail(ctx, PILCO_E_SHAPE, pre + "Z_all given for an exact GP slot");
    if (s.user_factors)
        return fail(ctx, PILCO_E_STATE, pre + "the slot holds factors set by pilco_gp_set_factors, not its own factorisation");
    const int Eu = output < 0 ? s.E : 1, e0 = output < 0 ? 0 : output;
    if (nmat > 1 && Eu > 64) return fail(ctx, PILCO_E_SHAPE, pre + "at most 64 outputs per call");
    const bool sparse = s.M > 0;
    const int npad_m = sparse ? round_up(s.M, 64) : round_up(s.N, 64), nops = sparse ? 2 : 1;
    const size_t budget = cov_budget();
    if ((size_t)Nt > (size_t)1 << 24 || cov_footprint(nops, Eu, npad_m, (size_t)round_up(Nt, 64), nmat, Spad) > budget) {
        size_t fit = 0;
        while (fit + 64 <= ((size_t)1 << 24) && cov_footprint(nops, Eu, npad_m, fit + 64, nmat, Spad) <= budget) fit += 64;
        return fail(ctx, PILCO_E_SHAPE, pre + "the covariance of " + std::to_string(Nt) + " test points needs " +
                                            std::to_string(cov_footprint(nops, Eu, npad_m, (size_t)round_up(std::min(Nt, 1 << 24), 64), nmat, Spad)) +
                                            " doubles, over the budget of " + std::to_string(budget) +
                                            " (PILCO_PREDICT_COV_BUDGET); the largest Nt that fits is " + std::to_string(fit));
    }
    HIPCHK(hipSetDevice(ctx->device));
    if (!s.factor_valid)
        if (int r = pilco_gp_factorize(ctx, slot)) return r;
    if (!s.pred) s.pred = new PredictWork();
    PredictWork& pw = *s.pred;
    hipStream_t st = ctx->st;
    const int D = s.D;
    PredictModel md = predict_model_of(s, e0, Eu);
    if (Z_all) {
        if (int r = factorize_own_z(ctx, s, pw, Z_all, e0, Eu)) return r;
        const Slot& f = pw.fitc;
        md.Pt = f.Zt.p; md.sP = f.Zstride;
        md.L = f.Linv.p; md.iAt = f.iAt.p; md.beta = f.beta.p;
    }
    const int npad = md.npad, ldt = round_up(Nt, 64);
    const size_t mat = (size_t)Eu * ldt * ldt;
    ENSURE(pw.raw, (size_t)ldt * D);
    ENSURE(pw.Xt, (size_t)D * ldt);
    ENSURE(pw.Ks, (size_t)Eu * ldt * npad);
    ENSURE(pw.out, (size_t)2 * Eu * ldt);
    ENSURE(pw.jacW, (size_t)predict_jac_nops(md) * Eu * ldt * npad);
    ENSURE(pw.pc_cov, mat);
    if (nmat > 1) {
        ENSURE(pw.pc_fac, mat);
        ENSURE(pw.pc_linv, mat);
    }
    c.s = &s; c.pw = &pw; c.md = md; c.Eu = Eu; c.e0 = e0; c.D = D; c.ldt = ldt; c.nops = predict_jac_nops(md);
    c.mean = pw.out.p; c.var = pw.out.p + (size_t)Eu * ldt;
    HIPCHK(hipMemcpyAsync(pw.raw.p, Xs, sizeof(double) * Nt * D, hipMemcpyHostToDevice, st));
    launch_transpose_points(st, pw.raw.p, Nt, D, pw.Xt.p, ldt);
    if (int r = predict_points_device(ctx, md, pw.Xt.p, Nt, ldt, pw.Ks.p, c.mean, c.var)) return r;
    if (int r = predict_points_w_device(ctx, md, Nt, ldt, pw.Ks.p, pw.jacW.p)) return r;
    PredictCovArgs a{};
    a.W = pw.jacW.p; a.Xt = pw.Xt.p; a.ls = md.ls; a.var = md.sf2;
    a.cov = pw.pc_cov.p; a.fac = nmat > 1 ? pw.pc_fac.p : nullptr; a.jitter = jitter;
    a.nops = c.nops; a.n = md.n; a.npad = npad; a.nt = Nt; a.ldt = ldt; a.D = D;
    if (nmat > 1) HIPCHK(hipMemsetAsync(pw.pc_fac.p, 0, sizeof(double) * mat, st));   // (the factor's tiles above the diagonal: zero)
    hipLaunchKernelGGL(k_predict_cov, dim3(ldt / PCOV_TILE, ldt / PCOV_TILE, Eu), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    c.args = a;
    return PILCO_OK;
}

// [Eu][ldt][ldt] on the device -> [Eu][Nt][Nt] on the host
int cov_download(pilco_ctx* ctx, const double* dev, int Eu, int Nt, int ldt, double* host) {
    for (int e = 0; e < Eu; ++e)
        HIPCHK(hipMemcpy2DAsync(host + (size_t)e * Nt * Nt, sizeof(double) * Nt, dev + (size_t)e * ldt * ldt, sizeof(double) * ldt,
                                sizeof(double) * Nt, Nt, hipMemcpyDeviceToHost, ctx->st));
    return PILCO_OK;
}

}  // namespace

extern "C" int pilco_gp_predict_points_cov(pilco_ctx* ctx, int slot, const double* Xs, int Nt, int output, const double* Z_all,
                                           double* mean, double* cov) {
    if (!ctx) return PILCO_E_SHAPE;
    if (!cov) return fail(ctx, PILCO_E_SHAPE, "predict_points_cov: null pointer or Nt <= 0");
    CovCall c{};
    if (int r = cov_enqueue(ctx, slot, "predict_points_cov", Xs, Nt, output, Z_all, 1, 0, 0.0, c)) return r;
    hipStream_t st = ctx->st;
    if (mean)
        HIPCHK(hipMemcpy2DAsync(mean, sizeof(double) * Nt, c.mean, sizeof(double) * c.ldt, sizeof(double) * Nt, c.Eu, hipMemcpyDeviceToHost, st));
    if (int r = cov_download(ctx, c.pw->pc_cov.p, c.Eu, Nt, c.ldt, cov)) return r;
    HIPCHK(hipStreamSynchronize(st));
    return PILCO_OK;
}

extern "C" int pilco_gp_sample_points(pilco_ctx* ctx, int slot, const double* Xs, int Nt, int output, const double* Z_all, int S,
                                      unsigned long long seed, const double* z_in, double jitter, double* samples, double* mean,
                                      double* cov, double* chol, double* z_out) {
    if (!ctx) return PILCO_E_SHAPE;
    if (!samples) return fail(ctx, PILCO_E_SHAPE, "sample_points: null pointer or Nt <= 0");
    if (S <= 0) return fail(ctx, PILCO_E_SHAPE, "sample_points: S <= 0");
    if (!(jitter >= 0.0) || !std::isfinite(jitter)) return fail(ctx, PILCO_E_SHAPE, "sample_points: jitter must be finite and >= 0");
    const int Spad = round_up(S, 64);
    CovCall c{};
    if (int r = cov_enqueue(ctx, slot, "sample_points", Xs, Nt, output, Z_all, 3, Spad, jitter, c)) return r;
    PredictWork& pw = *c.pw;
    hipStream_t st = ctx->st;
    const int Eu = c.Eu, ldt = c.ldt;
    const size_t nz = (size_t)S * Nt * Eu, nzp = (size_t)Eu * ldt * Spad, mat = (size_t)ldt * ldt;
    ENSURE(pw.pc_z, nzp);
    ENSURE(pw.pc_f, nzp);
    ENSURE(pw.pc_zraw, nz);
    ENSURE(pw.pc_smp, nz);
    HIPCHK(hipMemsetAsync(ctx->d_info, 0, sizeof(int) * 64, st));
    launch_potrf(st, pw.pc_fac.p, ldt, Eu, pw.pc_linv.p, ctx->d_info, false);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(pw.pc_z.p, 0, sizeof(double) * nzp, st));
    if (z_in) HIPCHK(hipMemcpyAsync(pw.pc_zraw.p, z_in, sizeof(double) * nz, hipMemcpyHostToDevice, st));
    CovDrawArgs da{};
    da.z_in = z_in ? pw.pc_zraw.p : nullptr;
    da.z_raw = z_in ? nullptr : pw.pc_zraw.p;
    da.Z = pw.pc_z.p; da.seed = seed; da.S = S; da.Spad = Spad; da.nt = Nt; da.ldt = ldt; da.Eu = Eu; da.e0 = c.e0;
    const unsigned nblk = (unsigned)((nz + 255) / 256);
    hipLaunchKernelGGL(k_cov_draws, dim3(nblk), dim3(256), 0, st, da);
    HIPCHK(hipGetLastError());
    GemmDesc g{};   // C z: the factor is lower triangular, k < i0 + 64
    g.A = pw.pc_fac.p; g.lda = ldt; g.sA = (long)mat;
    g.B = pw.pc_z.p; g.ldb = Spad; g.sB = (long)ldt * Spad;
    g.C = pw.pc_f.p; g.ldc = Spad; g.sC = (long)ldt * Spad;
    g.M = ldt; g.N = Spad; g.K = ldt; g.alpha = 1.0; g.beta = 0.0; g.tile_mode = 0; g.k_mode = 3;
    launch_gemm(st, g, false, false, Eu);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_cov_samples, dim3(nblk), dim3(256), 0, st, pw.pc_f.p, c.mean, pw.pc_smp.p, S, Spad, Nt, ldt, Eu);
    HIPCHK(hipGetLastError());
    // one download into staging memory, one synchronisation: the caller's arrays are written only when every factor exists
    const size_t n_mean = mean ? (size_t)Eu * Nt : 0, n_cov = cov ? (size_t)Eu * Nt * Nt : 0, n_chol = chol ? (size_t)Eu * Nt * Nt : 0;
    const size_t n_zo = (z_out && !z_in) ? nz : 0;
    std::vector<double> host(nz + n_mean + n_cov + n_chol + n_zo);
    double *h_smp = host.data(), *h_mean = h_smp + nz, *h_cov = h_mean + n_mean, *h_chol = h_cov + n_cov, *h_zo = h_chol + n_chol;
    int info[64];
    HIPCHK(hipMemcpyAsync(info, ctx->d_info, sizeof(int) * Eu, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_smp, pw.pc_smp.p, sizeof(double) * nz, hipMemcpyDeviceToHost, st));
    if (mean)
        HIPCHK(hipMemcpy2DAsync(h_mean, sizeof(double) * Nt, c.mean, sizeof(double) * ldt, sizeof(double) * Nt, Eu, hipMemcpyDeviceToHost, st));
    if (cov)
        if (int r = cov_download(ctx, pw.pc_cov.p, Eu, Nt, ldt, h_cov)) return r;
    if (chol)
        if (int r = cov_download(ctx, pw.pc_fac.p, Eu, Nt, ldt, h_chol)) return r;
    if (n_zo) HIPCHK(hipMemcpyAsync(h_zo, pw.pc_zraw.p, sizeof(double) * nz, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int el = 0; el < Eu; ++el)
        if (info[el] != 0) {
            ctx->not_pd = c.e0 + el;
            return fail(ctx, PILCO_E_NOT_PD, "sample_points: Cholesky failed: the posterior covariance + jitter*I of output " +
                                                 std::to_string(c.e0 + el) + " is not positive definite (pivot " + std::to_string(info[el]) + ")");
        }
    memcpy(samples, h_smp, sizeof(double) * nz);
    if (mean) memcpy(mean, h_mean, sizeof(double) * n_mean);
    if (cov) memcpy(cov, h_cov, sizeof(double) * n_cov);
    if (chol) memcpy(chol, h_chol, sizeof(double) * n_chol);
    if (z_out) memcpy(z_out, z_in ? z_in : h_zo, sizeof(double) * nz);
    return PILCO_OK;
}

#ifdef PILCO_DEV
namespace pilco {
// the yardstick's add: out = Kss - G0 (+ G1), elementwise
__global__ __launch_bounds__(256) void k_cov_parts_add(const double* __restrict__ Kss, const double* __restrict__ G0,
                                                       const double* __restrict__ G1, double* __restrict__ out, long n) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q < n) out[q] = G1 ? (Kss[q] - G0[q]) + G1[q] : Kss[q] - G0[q];
}
}  // namespace pilco
#endif

extern "C" int pilco_debug_predict_cov_timed(pilco_ctx* ctx, int slot, const double* Xs, int Nt, int reps, float* ms_fused, float* ms_parts,
                                             double* max_diff) {
    if (!ctx) return PILCO_E_SHAPE;
#ifndef PILCO_DEV
    (void)slot; (void)Xs; (void)Nt; (void)reps; (void)ms_fused; (void)ms_parts; (void)max_diff;
    return fail(ctx, PILCO_E_STATE, "predict_cov_timed: the yardstick exists in -DPILCO_DEV builds only");
#else
    if (!ms_fused || !ms_parts || !max_diff || reps <= 0) return fail(ctx, PILCO_E_SHAPE, "predict_cov_timed: null pointer or reps <= 0");
    CovCall c{};
    if (int r = cov_enqueue(ctx, slot, "predict_cov_timed", Xs, Nt, -1, nullptr, 4, 0, 0.0, c)) return r;   // (four matrices: cov, K**, G0, the sum)
    PredictWork& pw = *c.pw;
    hipStream_t st = ctx->st;
    const int Eu = c.Eu, ldt = c.ldt, npad = c.md.npad;
    const size_t mat = (size_t)Eu * ldt * ldt;
    ENSURE(pw.pc_z, mat);
    ENSURE(pw.pc_f, mat);
    PredictCovArgs a = c.args;
    a.fac = nullptr;
    double *Kss = pw.pc_fac.p, *G0 = pw.pc_linv.p, *G1 = c.nops > 1 ? pw.pc_z.p : nullptr, *sum = pw.pc_f.p;
    auto parts = [&]() {
        launch_gram(st, pw.Xt.p, ldt, Nt, pw.Xt.p, ldt, Nt, c.D, c.md.ls, c.md.sf2, Eu, Kss, ldt, ldt, 0, nullptr, 0.0);
        for (int op = 0; op < c.nops; ++op) {
            GemmDesc g{};   // W W^T, the tiles on and below the diagonal computed, their mirror images stored
            g.A = pw.jacW.p + (size_t)op * Eu * ldt * npad; g.lda = npad; g.sA = (long)ldt * npad;
            g.B = g.A; g.ldb = npad; g.sB = g.sA;
            g.C = op ? G1 : G0; g.ldc = ldt; g.sC = (long)ldt * ldt;
            g.M = ldt; g.N = ldt; g.K = npad; g.alpha = 1.0; g.beta = 0.0; g.tile_mode = 2; g.k_mode = 0;
            launch_gemm(st, g, false, true, Eu);
        }
        hipLaunchKernelGGL(k_cov_parts_add, dim3((unsigned)((mat + 255) / 256)), dim3(256), 0, st, Kss, G0, G1, sum, (long)mat);
    };
    auto fused = [&]() { hipLaunchKernelGGL(k_predict_cov, dim3(ldt / PCOV_TILE, ldt / PCOV_TILE, Eu), dim3(256), 0, st, a); };
    fused();
    parts();   // warm
    HIPCHK(hipEventRecord(ctx->ev0, st));
    for (int i = 0; i < reps; ++i) fused();
    HIPCHK(hipEventRecord(ctx->ev1, st));
    HIPCHK(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *ms_fused = ms / reps;
    HIPCHK(hipEventRecord(ctx->ev0, st));
    for (int i = 0; i < reps; ++i) parts();
    HIPCHK(hipEventRecord(ctx->ev1, st));
    HIPCHK(hipEventSynchronize(ctx->ev1));
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *ms_parts = ms / reps;
    HIPCHK(hipGetLastError());
    std::vector<double> h0((size_t)Eu * Nt * Nt), h1((size_t)Eu * Nt * Nt);
    if (int r = cov_download(ctx, pw.pc_cov.p, Eu, Nt, ldt, h0.data())) return r;
    if (int r = cov_download(ctx, sum, Eu, Nt, ldt, h1.data())) return r;
    HIPCHK(hipStreamSynchronize(st));
    double d = 0.0;
    for (size_t i = 0; i < h0.size(); ++i) d = std::max(d, std::fabs(h0[i] - h1[i]));
    *max_diff = d;
    return PILCO_OK;
#endif
}
