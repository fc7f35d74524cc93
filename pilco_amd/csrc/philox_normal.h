// The random stream of the particle rollouts (particles.hip): Philox4x32-10 (Salmon et al., "Parallel random numbers: as
// easy as 1, 2, 3", SC'11; the Random123 known answers are held in tests/test_particles_cpu.py) and the Box-Muller map
// from one block of four words to two standard-normal draws.  Plain C++ apart from the __host__ __device__ marks:
// tests/test_particles_cpu.py compiles this header into a host probe and holds the Python restatement
// (tests/helpers/particles_restatement.py) to it.
//   key     {seed & 0xffffffff, seed >> 32}
//   counter {p, t, j, 0}  ->  words w0 .. w3  ->  draws 2j, 2j + 1 of particle p at step t
//   u1 = 1 - ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53  in (0, 1],   u2 = ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53  in [0, 1)
//   r = sqrt(-2 ln u1),   z_2j = r cos(2 pi u2),   z_2j+1 = r sin(2 pi u2)
// A draw depends on (seed, t, p, e) only: not on the particle count, not on how the particles are chunked.
// The counter's fourth word is a domain: 0 above; 1..4 below, the function-sample rollout (particles_fn.hip); 5, the joint
// posterior samples at test points (predict_cov.hip); 6, the observation noise of the path-conditioned rollout
// (particles_cond.hip).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PILCO_PHILOX_HD __host__ __device__
#else
#define PILCO_PHILOX_HD
#endif
namespace pilco {

struct PhiloxWords {
    uint32_t w[4];
};

PILCO_PHILOX_HD inline PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    return PhiloxWords{{c0, c1, c2, c3}};
}

PILCO_PHILOX_HD inline PhiloxWords philox_particle_words(unsigned long long seed, uint32_t t, uint32_t p, uint32_t j) {
    return philox4x32_10(p, t, j, 0u, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
}

// the two uniforms of a block: 53 bits each, u1 never 0 (its logarithm is taken), u2 never 1
PILCO_PHILOX_HD inline void philox_uniforms(const PhiloxWords& b, double* u1, double* u2) {
    const double two26 = 67108864.0, twom53 = 1.0 / 9007199254740992.0;
    *u1 = 1.0 - ((double)(b.w[0] >> 5) * two26 + (double)(b.w[1] >> 6)) * twom53;
    *u2 = ((double)(b.w[2] >> 5) * two26 + (double)(b.w[3] >> 6)) * twom53;
}

// draws 2j and 2j + 1 of particle p at step t
PILCO_PHILOX_HD inline void philox_normal_pair(unsigned long long seed, uint32_t t, uint32_t p, uint32_t j, double* z0, double* z1) {
    double u1, u2;
    philox_uniforms(philox_particle_words(seed, t, p, j), &u1, &u2);
    const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586476925 * u2;
    *z0 = r * cos(a);
    *z1 = r * sin(a);
}

// The streams of the function-sample rollout (particles_fn.hip, docs/particle_functions.md).  The counter's fourth word
// selects a domain; domain 0 is the step draws above, whose functions and bits stay as they are.  Key and Box-Muller map as
// above; a draw depends on (seed, indices) only.
//   domain 1  {l, e, j, 1}  normals 2j, 2j + 1: z_el,2j, z_el,2j+1 (the frequency of feature l of output e is z / lengthscale)
//   domain 2  {l, e, 0, 2}  u2: the phase b_el = 2 pi u2
//   domain 3  {p, l, j, 3}  normals: the weights w_p,2j,l, w_p,2j+1,l of particle p (outputs 2j, 2j + 1, feature l)
//   domain 4  {p, i, j, 4}  normals: the noise draws xi_p,2j,i, xi_p,2j+1,i (outputs 2j, 2j + 1, training point i)
//   domain 5  {s, a, j, 5}  normals: z_s,a,2j, z_s,a,2j+1 of pilco_gp_sample_points (sample s, test point a, outputs 2j, 2j + 1)
//   domain 6  {p, t, j, 6}  normals: zeta_t,p,2j, zeta_t,p,2j+1, the observation noise of pilco_rollout_particles_cond
enum PhiloxDomain : uint32_t {
    PHILOX_STEP = 0u, PHILOX_FN_FREQ = 1u, PHILOX_FN_PHASE = 2u, PHILOX_FN_WEIGHT = 3u, PHILOX_FN_XI = 4u, PHILOX_COV_Z = 5u,
    PHILOX_COND_OBS = 6u
};

PILCO_PHILOX_HD inline PhiloxWords philox_domain_words(unsigned long long seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t domain) {
    return philox4x32_10(c0, c1, c2, domain, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
}

// the two normals of the block {c0, c1, c2, domain}
PILCO_PHILOX_HD inline void philox_domain_normal_pair(unsigned long long seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t domain,
                                                      double* z0, double* z1) {
    double u1, u2;
    philox_uniforms(philox_domain_words(seed, c0, c1, c2, domain), &u1, &u2);
    const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586476925 * u2;
    *z0 = r * cos(a);
    *z1 = r * sin(a);
}

// the phase of feature l of output e, in [0, 2 pi)
PILCO_PHILOX_HD inline double philox_fn_phase(unsigned long long seed, uint32_t l, uint32_t e) {
    double u1, u2;
    philox_uniforms(philox_domain_words(seed, l, e, 0u, PHILOX_FN_PHASE), &u1, &u2);
    return 6.283185307179586476925 * u2;
}

}  // namespace pilco
