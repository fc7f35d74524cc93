// The branch predicates of the step's serial link, in one place and callable from the host: which squash code a shape
// takes (glue_body / squash_inplace) and whether an RbfController is evaluated inline.  (Which device path a reward weight
// goes down: reward_factor.h.)  Plain C++ apart from the __host__ __device__ marks: tests/test_link_edges_cpu.py compiles
// this header into a host probe and holds its Python mirror (tests/helpers/link_cases.py) to it over the whole shape range.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PILCO_HD __host__ __device__
#else
#define PILCO_HD
#endif
namespace pilco {

// The two squash predicates are EXPRESSIONS (macros) that glue_device.h expands in place, and functions of the same text
// for the host: with a call at either site -- inlined or not -- this compiler allocates k_glue's and the fused heads'
// registers differently (several hundred instructions move), and the link's instruction stream is the step's critical path.
// Expanded in place the link compiles to the instructions it had before the predicates moved here.
//
// squash_inplace: slots of one round of evaluations in the link's own scratch (t1 .. js: 4 nm^2 + nm doubles), in whole
// items -- an item is 5 slots (a control uses 3 of its 5)
#define PILCO_SQUASH_ROUND_CAP(nm) (((4 * (nm) * (nm) + (nm)) / 5) * 5)
// LinearController + squash inside a rollout: the 5 (U^2 + U) evaluations fit ONE nm x nm buffer (t2), so the link stops
// behind them and write_joint_lin_squash combines them
#define PILCO_SQUASH_LIN_FUSED_FITS(U, nm) (5 * ((U) * (U) + (U)) <= (nm) * (nm))
PILCO_HD inline int squash_round_cap(int nm) { return PILCO_SQUASH_ROUND_CAP(nm); }
PILCO_HD inline bool squash_lin_fused_fits(int U, int nm) { return PILCO_SQUASH_LIN_FUSED_FITS(U, nm); }

// LDS layout (offsets in doubles) of the inline RbfController evaluation (glue_device.h: rbf_policy_inline)
struct RbfInlineLayout {
    int ctr, bet, il, var, lvar, aug0, aug1, piv, T, Q, det, pt, red, red3, total;
};
PILCO_HD inline RbfInlineLayout rbf_inline_layout(int E, int U, int bf) {
    const int P = U * (U + 1) / 2, nmat = U + P;
    RbfInlineLayout l;
    int o = 0;
    l.ctr = o; o += bf * E;                 // centred centres  zeta_i = c_i - m
    l.bet = o; o += U * bf;                 // beta of every output
    l.il = o;  o += U * E;                  // 1 / lengthscale
    l.var = o; o += U;
    l.lvar = o; o += U;                     // log of the signal variances (phase 3's exponents)
    l.aug0 = o; o += nmat * E * 2 * E;      // augmented matrices of the batched Gauss-Jordan (ping)
    l.aug1 = o; o += nmat * E * 2 * E;      //                                                (pong)
    l.piv = o; o += nmat * E;               // pivots -> determinants
    l.T = o;   o += U * E * E;              // T_u = (s + Lambda_u^2)^-1
    l.Q = o;   o += P * E * E;              // Q_uv = R_uv^-1 s / 2
    l.det = o; o += nmat;                   // det B_u | det R_uv
    l.pt = o;  o += bf * (2 * E + 2) + bf * 16;   // per point of the current pair: u_i, v_i, p_i = 2 Q z_i, w_i | 16 doubles of scratch per point
    l.red = o; o += 4 * (E + 2);            // wave partials (mean part)
    l.red3 = o; o += 4;                     // wave partials (covariance part: it may run beside the mean part)
    l.total = (o + 1) & ~1;
    return l;
}

// doubles of LDS the inline evaluation needs, or 0 when the controller is not eligible for it
PILCO_HD inline int link_rbf_inline_lds_doubles(int E, int U, int bf) {
    if (E < 1 || E > 16 || U < 1 || U > 4 || bf < 1 || bf > 256) return 0;
    const int P = U * (U + 1) / 2;
    if ((long)P * bf * bf > 16384) return 0;   // the O(bf^2) sums run redundantly in every workgroup of the head: keep them short
    const RbfInlineLayout lay = rbf_inline_layout(E, U, bf);
    return lay.total <= 8192 ? lay.total : 0;
}

}  // namespace pilco
