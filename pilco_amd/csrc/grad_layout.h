// The data formats of a value-and-gradient rollout, each defined once for the host and the device: the dimensions of the
// reverse chain and of a step's Jacobian records (RevDims), the tape record, the geometry of the sharded records'
// all-gather and the reverse chain's output vector.  rollout.hip, grad_route.hip, grad.hip, bwd.hip (mm_jac_rec_size) and
// rev.hip take them from here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace pilco {

// x = (mbar (E) | sbar packed, P entries in the pairs' dealing order) is the reverse chain's state (NX), theta = (W (U,E) | b (U))
// its parameters (NP), NR = NX + NP the rows of a step's reverse map.  A step's Jacobian records (bwd.hip: k_mm_jac_fin):
//   pair record   (recp doubles): N_ab | d / d m (D) | d / d s packed (NT2)
//   output record (reco doubles): dM/dm (D) | sym dM/ds (NT2) | dV/dm (D,D) | dV/ds (D,NT2)
struct RevDims {
    int E, U, D, P, NX, NP, NR, NOUT, NT2, nI, recp, reco;
};
__host__ __device__ inline RevDims rev_dims(int E, int U, int D) {
    RevDims d;
    d.E = E; d.U = U; d.D = D; d.P = E * (E + 1) / 2;
    d.NX = E + d.P; d.NP = U * E + U; d.NR = d.NX + d.NP;
    d.NT2 = D * (D + 1) / 2; d.NOUT = D + d.NT2; d.nI = D * D;
    d.recp = 1 + d.NOUT; d.reco = d.NOUT + d.nI + D * d.NT2;
    return d;
}
// one rank's records of one step: its PL pair records, then the E output records (mm_jac_rec_size)
__host__ __device__ inline size_t jac_rec_size(int D, int E, int PL) {
    const RevDims d = rev_dims(E, D - E, D);
    return (size_t)PL * d.recp + (size_t)E * d.reco;
}

// The tape record of a step (GlueArgs::tape, pilco_rollout_tape): the joint Gaussian handed to the dynamics GP and its
// outputs, m_j (D) | s_j (D,D) | s1 (E,D) | M (E) | S (E,E) | V (D,E).  Field offsets and the record's size, in doubles.
struct TapeRec {
    size_t m_j, s_j, s1, M, S, V, size;
};
__host__ __device__ inline TapeRec tape_rec(int D, int E) {
    TapeRec r;
    r.m_j = 0;
    r.s_j = r.m_j + (size_t)D;
    r.s1 = r.s_j + (size_t)D * D;
    r.M = r.s1 + (size_t)E * D;
    r.S = r.M + (size_t)E;
    r.V = r.S + (size_t)E * E;
    r.size = r.V + (size_t)D * E;
    return r;
}

// Sharded value-and-gradient rollout over W ranks: every rank compacts its records of the H steps into one block of gblk
// doubles -- per step (gstep) its pair records padded to PLcap, then the E output records at out_off -- and the W blocks are
// all-gathered.  Pair kk of the dealing order lives in rank kk % W's block as its pair kk / W; the output records are taken
// from rank 0's block (every rank WITH pairs computes them all; rank 0 always has pairs).  JSg: one step's records of the
// WHOLE model, [P pair records | E output records], as the host chain reads them.
struct JacGather {
    int W, P, PLcap;
    size_t gstep, gblk, out_off, JSg;
};
__host__ __device__ inline JacGather jac_gather(int D, int E, int W, int H) {
    const RevDims d = rev_dims(E, D - E, D);
    JacGather g;
    g.W = W; g.P = d.P; g.PLcap = (d.P + W - 1) / W;
    g.out_off = (size_t)g.PLcap * d.recp;
    g.gstep = g.out_off + (size_t)E * d.reco;
    g.gblk = (size_t)(H > 1 ? H : 1) * g.gstep;
    g.JSg = jac_rec_size(D, E, d.P);
    return g;
}

// The reverse chain's output vector (RevArgs::out, written by k_rev_chain): dW (U,E) | db (U) | status (0 fine, 1: a step
// with a singular matrix in its records or rewards) | d objective / d (m_0, S_0 packed) (NX) | the rollout's reward.
struct RevOut {
    size_t dW, db, status, x0, reward, size;
};
__host__ __device__ inline RevOut rev_out(int E, int U) {
    const RevDims d = rev_dims(E, U, E + U);
    RevOut o;
    o.dW = 0;
    o.db = (size_t)U * E;
    o.status = (size_t)d.NP;
    o.x0 = o.status + 1;
    o.reward = o.x0 + (size_t)d.NX;
    o.size = o.reward + 1;
    return o;
}

}  // namespace pilco
