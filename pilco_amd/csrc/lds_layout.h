// The dynamic-LDS layouts of the reverse pass and the reverse chain, each defined once for the host and the device: for every
// role a workgroup can play in k_mm_bwd_pair / _head / _post / _fin, k_mm_jac_rec / _fin, k_rev_step and k_rev_chain one
// function that returns the offsets of the role's regions (in doubles from the kernel's `sm`) and their `total`.  The device
// function of the role carves with it, the launcher sizes with it; a launch whose workgroups play several roles takes the
// largest total (lds_launch_*, below the roles).  A `slack` term is what a launch has always asked for beyond its last
// region: the totals decide how many workgroups a CU holds and stay as they were.
// (The serial link's layout is glue_lds_carve, glue_device.h: host and device as well.)
// Plain C++ apart from the __host__ __device__ marks: tests/test_lds_layout_cpu.py compiles this header into a host probe.
#pragma once
#include "grad_layout.h"
#include "link_predicates.h"   // PILCO_HD

namespace pilco {

PILCO_HD constexpr int lds_max(int a, int b) { return a > b ? a : b; }

// ------------------------------------------------------------------ the reverse sweep (bwd.hip: k_mm_bwd_pair)
constexpr int BWD_CH = 64;   // columns staged per LDS chunk (one wave-wide row segment)
constexpr int BWD_SCR_H = 40, BWD_SCR_R = 72, BWD_SCR_W = 4 * BWD_SCR_R;   // column-sum scratch of a wave (doubles): half / register strides, size
PILCO_HD constexpr int bwd_tp(int kp) { return kp <= 16 ? 17 : kp + 1; }   // pitch of the staged column-major tile (doubles): operand rows + 1 (odd: conflict-free)
PILCO_HD constexpr int bwd_stage_doubles(int kp) { return BWD_CH * bwd_tp(kp) + 2 * BWD_CH; }   // one staging buffer: the tile | beta_b | v
// stride of a wave's column-sum slice: the widest of the njs column splits, in whole 16-column tiles
PILCO_HD inline int sweep_jws(int npad, int njs) { return 16 * ((npad / 16 + njs - 1) / njs); }
constexpr int SWEEP_STATIC_BYTES = 2048;   // k_mm_bwd_pair's static LDS beside the dynamic: the exp table
struct SweepLds {
    int csl;   // [4][jws]   the four waves' column sums
    int stg;   // [2][bwd_stage_doubles]   (the epilogue's [4][256] reduction buffer afterwards)
    int scr;   // [4][BWD_SCR_W]   read back with 16-byte accesses
    int total;
};
PILCO_HD inline SweepLds sweep_lds(int jws, int kp) {
    SweepLds l;
    l.csl = 0;
    l.stg = l.csl + 4 * jws;
    l.scr = l.stg + 2 * bwd_stage_doubles(kp);
    l.total = l.scr + 4 * BWD_SCR_W;
    return l;
}
// bwd_head: the D x D inverses of a step (spare workgroups of the sweep, k_mm_bwd_head)
struct HeadLds {
    int G0, G1;   // [D][2D] each: the Gauss-Jordan's ping and pong
    int lam;      // [D]
    int total;
};
PILCO_HD inline HeadLds head_lds(int D) {
    HeadLds l;
    l.G0 = 0;
    l.G1 = l.G0 + 2 * D * D;
    l.lam = l.G1 + 2 * D * D;
    l.total = l.lam + D;
    return l;
}

// ------------------------------------------------------------------ k_mm_bwd_post / k_mm_bwd_fin
struct PairPostLds {   // bwd_pair_post<NMT>, GW = 16 NMT
    int Gs, Gc;   // [GW][GW] each
    int red;      // [4][256]
    int total;
};
PILCO_HD constexpr PairPostLds pair_post_lds(int nmt) {
    return PairPostLds{0, 256 * nmt * nmt, 2 * 256 * nmt * nmt, 2 * 256 * nmt * nmt + 4 * 256};
}
struct MeanPartialLds {   // bwd_mean_partial
    int T;        // [D][D]
    int zs;       // [64][D | 1]
    int lv, lq;   // [64] each
    int u;        // [D + 2]
    int total;
};
PILCO_HD inline MeanPartialLds mean_partial_lds(int D) {
    MeanPartialLds l;
    l.T = 0;
    l.zs = l.T + D * D;
    l.lv = l.zs + 64 * (D | 1);
    l.lq = l.lv + 64;
    l.u = l.lq + 64;
    l.total = l.u + D + 2;
    return l;
}
struct MeanFinalLds {   // bwd_mean_final
    int T;     // [D][D]
    int u;     // [D + 2]
    int sc;    // [2]
    int Th;    // [D]
    int red;   // [D*D + 2 D + 1]
    int TH;    // [D][D]
    int total;
};
PILCO_HD inline MeanFinalLds mean_final_lds(int D) {
    MeanFinalLds l;
    l.T = 0;
    l.u = l.T + D * D;
    l.sc = l.u + D + 2;
    l.Th = l.sc + 2;
    l.red = l.Th + D;
    l.TH = l.red + D * D + 2 * D + 1;
    l.total = l.TH + D * D + 3;   // (slack: 3)
    return l;
}
struct FinPairsLds {   // bwd_fin_pairs
    int Pm;    // [D][D]
    int lam;   // [D + 2]
    int Iv;    // [1 + D + D*D]
    int PI;    // [D][D]
    int total;
};
PILCO_HD inline FinPairsLds fin_pairs_lds(int D) {
    FinPairsLds l;
    l.Pm = 0;
    l.lam = l.Pm + D * D;
    l.Iv = l.lam + D + 2;
    l.PI = l.Iv + 1 + D + D * D;
    l.total = l.PI + D * D;
    return l;
}

// ------------------------------------------------------------------ the Jacobian tape's records (k_mm_jac_rec / k_mm_jac_fin)
struct JacRecLds {   // the fused record role: bwd_pair_post<1>'s regions first, the pair's sums and its head record behind them
    PairPostLds post;
    int Iv;    // [1 + D + D*D]   (bwd_pair_post<1>'s output)
    int Pm;    // [D][D]
    int lam;   // [D + 2]
    int PI;    // [2][D][D]
    int cjl;   // [npad]   read with 16-byte accesses: an even offset
    int total;
};
PILCO_HD inline JacRecLds jac_rec_lds(int D, int npad) {
    JacRecLds l;
    l.post = pair_post_lds(1);
    l.Iv = l.post.total;
    l.Pm = l.Iv + 1 + D + D * D;
    l.lam = l.Pm + D * D;
    l.PI = l.lam + D + 2;
    const int end = l.PI + 2 * D * D + 1;   // (+ 1: room for the rounding below)
    l.cjl = end & ~1;
    l.total = end + npad;
    return l;
}
constexpr int JAC_MT = 8;   // row tiles of the moment product: D1 (D1 + 1) / 2 <= 128 pairs (D <= 14)
struct MeanMomentsLds {   // bwd_mean_moments_mfma
    int T;      // [16][16]
    int zs;     // [64][17]
    int lv;     // [64]
    int qp;     // [4][256]
    int ptab;   // [16 JAC_MT] ints
    int total;
};
PILCO_HD constexpr MeanMomentsLds mean_moments_lds() {
    return MeanMomentsLds{0, 256, 256 + 64 * 17, 256 + 64 * 17 + 64, 256 + 64 * 17 + 64 + 4 * 256,
                          256 + 64 * 17 + 64 + 4 * 256 + 8 * JAC_MT + 2};   // (slack: 2)
}
struct JacFinOutputLds {   // jac_fin_output
    int T;         // [D][D]
    int Hs;        // [NS], NS = (D + 1)(D + 2)(D + 3) / 6
    int Th;        // [D]
    int TH, THT;   // [D][D] each
    int W3, Z3;    // [D][D][D] each
    int total;
};
PILCO_HD inline JacFinOutputLds jac_fin_output_lds(int D) {
    const int nI = D * D;
    JacFinOutputLds l;
    l.T = 0;
    l.Hs = l.T + nI;
    l.Th = l.Hs + (D + 1) * (D + 2) * (D + 3) / 6;
    l.TH = l.Th + D;
    l.THT = l.TH + nI;
    l.W3 = l.THT + nI;
    l.Z3 = l.W3 + nI * D;
    l.total = l.Z3 + nI * D;
    return l;
}

// ------------------------------------------------------------------ the reverse chain (rev_local.h, rev.hip)
// loc [H][rev_loc_size]: the trajectory-only quantities of a step (rev_local_step writes them, k_rev_step keeps them in LDS)
PILCO_HD inline int rev_loc_size(int E, int U) { return E + E * E + 2 * U * E + 2 * U + 9 * U * U; }
struct RevLocalLds {   // rev_local_step
    int mx, sx;   // [E] | [E][E]
    int dm, dS;   // [E] | [E][E]
    int v, dTi, d;   // [E] each
    int G0, G1;   // [E][2E] each; afterwards, from G0: T1 (U,E) | T2 (U,E) | mu0 (U)
    int total;
};
PILCO_HD inline RevLocalLds rev_local_lds(int E, int U) {
    RevLocalLds l;
    l.mx = 0;
    l.sx = l.mx + E;
    l.dm = l.sx + E * E;
    l.dS = l.dm + E;
    l.v = l.dS + E * E;
    l.dTi = l.v + E;
    l.d = l.dTi + E;
    l.G0 = l.d + E;
    l.G1 = l.G0 + 2 * E * E;
    l.total = l.G0 + lds_max(4 * E * E, 2 * U * E + U) + 8;   // (slack: 8)
    return l;
}
constexpr int REVS_SPLIT = 4;   // workgroups per step of k_rev_step (column ranges of [A; B]); a flag each
constexpr int REV_NT = 512;     // threads of k_rev_chain's workgroup
// a step's reverse map in memory (RevArgs::amat): [A; B] by columns | r | flags
PILCO_HD inline size_t rev_mat_doubles(int E, int U, int D) {
    const RevDims d = rev_dims(E, U, D);
    return (size_t)d.NX * d.NR + d.NX + REVS_SPLIT;
}
struct RevStepLds {   // k_rev_step
    int M1;     // [NX][NOUT]
    int s1;     // (E,D)
    int Mg;     // (E)
    int Vg;     // (D,E)
    int mx;     // (E)
    int sx;     // (E,E)
    int loc;    // [rev_loc_size]
    int Wl;     // (U,E)
    int gcol;   // [NX][U + U*U]
    int pab;    // [P] ints
    int total;
};
PILCO_HD inline RevStepLds rev_step_lds(int E, int U, int D) {
    const RevDims d = rev_dims(E, U, D);
    RevStepLds l;
    l.M1 = 0;
    l.s1 = l.M1 + d.NX * d.NOUT;
    l.Mg = l.s1 + E * D;
    l.Vg = l.Mg + E;
    l.mx = l.Vg + E * D;
    l.sx = l.mx + E;
    l.loc = l.sx + E * E;
    l.Wl = l.loc + rev_loc_size(E, U);
    l.gcol = l.Wl + U * E;
    l.pab = l.gcol + d.NX * (U + U * U);
    l.total = l.pab + (d.P + 1) / 2 + 2;   // (slack: 2)
    return l;
}
struct RevChainLds {   // k_rev_chain
    int nch;    // column chunks of the matrix-vector product: REV_NT / NR
    int x;      // [NX + 1]   (one zero behind x: the coefficient of a slot past a thread's share)
    int part;   // [nch][NR]
    int total;
};
PILCO_HD inline RevChainLds rev_chain_lds(int E, int U, int D) {
    const RevDims d = rev_dims(E, U, D);
    RevChainLds l;
    l.nch = REV_NT / d.NR;
    l.x = 0;
    l.part = l.x + d.NX + 1;
    l.total = l.part + l.nch * d.NR;
    return l;
}

// ------------------------------------------------------------------ the posterior covariance (predict_cov.hip: k_predict_cov)
// static LDS, the same for every launch: the finished 64 x 64 tile turned around for its mirror image, the reciprocal lengthscales
constexpr int PCOV_TILE = 64, PCOV_TP = 65;   // tile edge; pitch of the turned tile (odd: conflict-free both ways)
struct PredictCovLds {
    int tile;   // [PCOV_TILE][PCOV_TP]   element (b, a) of the tile (a, b)
    int il;     // [32]   1 / l_d
    int total;
};
PILCO_HD constexpr PredictCovLds predict_cov_lds() { return PredictCovLds{0, PCOV_TILE * PCOV_TP, PCOV_TILE * PCOV_TP + 32}; }

// ------------------------------------------------------------------ what a launch asks for (doubles): the largest of its roles
PILCO_HD inline int lds_launch_sweep(int npad, int njs, int kp, int D) { return lds_max(sweep_lds(sweep_jws(npad, njs), kp).total, head_lds(D).total); }
PILCO_HD inline int lds_launch_bwd_post(int D) { return lds_max(pair_post_lds((D + 16) / 16).total, mean_partial_lds(D).total); }
PILCO_HD inline int lds_launch_bwd_fin(int D) { return lds_max(mean_final_lds(D).total, fin_pairs_lds(D).total); }
PILCO_HD inline int lds_launch_jac_rec(int D, int npad) { return lds_max(jac_rec_lds(D, npad).total, mean_moments_lds().total); }
// local: the launch carries the reverse chain's extra workgroup per step (rev_local_step for E states and U controls)
PILCO_HD inline int lds_launch_jac_fin(int D, bool local, int E, int U) {
    return lds_max(jac_fin_output_lds(D).total, local ? rev_local_lds(E, U).total : 0);
}

}  // namespace pilco
