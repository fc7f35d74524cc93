// The memory plan of the path-conditioned particle rollout (particles_cond.hip, docs/particle_conditioned.md): how many
// particles run together.  Plain C++ without a HIP include: tests/test_particle_cond_cpu.py compiles this header into a host
// probe and holds a Python mirror to it.
//   per particle   H nops E npad  (the history of W rows)  +  E H (H + 1) / 2  (the factor; twice with path_cov)  +  H D  (the
//                  visited points)  +  E npad + 2 E  (the chunk's cross-covariances, mean and variance)      doubles
//   group          the largest multiple of 64 particles whose footprint is within the budget, at most P rounded up to 64 and at
//                  most one chunk of pilco_gp_predict_points (chunk_cap); below 64 the call is refused and H_fit is the
//                  largest horizon a group of 64 can hold (-1: none)
#pragma once
#include <algorithm>
#include <cstddef>

namespace pilco {

constexpr int PC2_MAX_STEPS = 128;                 // PILCO_MAX_COND_STEPS
constexpr size_t PC2_BUDGET = size_t(1) << 29;     // doubles (4 GB); PILCO_PARTICLE_COND_BUDGET overrides it
constexpr int PC2_MAX_ROW = 8192;                  // nops * npad: the new row of one (particle, output) sits in 64 KB of LDS

inline size_t cond_tri(int H) { return (size_t)H * (H + 1) / 2; }
// offset of column s of the packed lower triangle (rows s .. H - 1 of the column, one after the other)
inline size_t cond_col(int H, int s) { return (size_t)s * H - (size_t)s * (s - 1) / 2; }

inline size_t cond_per_particle(int H, int nops, int E, int D, int npad, bool want_cov) {
    return (size_t)H * nops * E * npad + (want_cov ? 2 : 1) * E * cond_tri(H) + (size_t)H * D + (size_t)E * npad + 2 * (size_t)E;
}

struct CondPlan {
    int G;                 // particles per group (a multiple of 64), 0: refused
    int ngroups;
    size_t per_particle;   // doubles
    size_t footprint;      // per_particle * G (refused: of a group of 64)
    int H_fit;             // refused: the largest H that fits a group of 64, or -1
};

inline CondPlan cond_plan(int P, int H, int nops, int E, int D, int npad, bool want_cov, size_t budget, int chunk_cap) {
    CondPlan pl{};
    pl.per_particle = cond_per_particle(H, nops, E, D, npad, want_cov);
    const size_t fit = budget / pl.per_particle / 64 * 64;
    const size_t cap = std::min((size_t)((P + 63) / 64 * 64), (size_t)chunk_cap);
    if (fit < 64) {
        pl.G = 0;
        pl.ngroups = 0;
        pl.footprint = pl.per_particle * 64;
        pl.H_fit = -1;
        for (int h = 0; h < H; ++h)
            if (cond_per_particle(h, nops, E, D, npad, want_cov) * 64 <= budget) pl.H_fit = h;
        return pl;
    }
    pl.G = (int)std::min(fit, cap);
    pl.ngroups = (P + pl.G - 1) / pl.G;
    pl.footprint = pl.per_particle * pl.G;
    pl.H_fit = H;
    return pl;
}

}  // namespace pilco
