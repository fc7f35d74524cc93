// psd_factor: which device path an exponential reward's weight goes down (stage_rewards, rollout.hip; the reverse chains'
// reward adjoint, grad.hip).  Host only, plain C++: tests/test_link_edges_cpu.py compiles it into its probe.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace pilco {

// W (E x E, symmetric PSD) = F F^T with F (E x rank) from a cyclic Jacobi eigen-decomposition.
// Returns rank, or -1 when W is not symmetric PSD (the general pivoted device path is used then).
inline int psd_factor(const double* W, int E, std::vector<double>& F) {
    double scale = 0.0;
    for (int i = 0; i < E * E; ++i) scale = std::max(scale, std::fabs(W[i]));
    if (scale == 0.0) { F.clear(); return 0; }
    for (int i = 0; i < E; ++i)
        for (int j = 0; j < i; ++j)
            if (std::fabs(W[i * E + j] - W[j * E + i]) > 1e-13 * scale) return -1;
    std::vector<double> A(W, W + E * E), V(E * E, 0.0);
    for (int i = 0; i < E; ++i) V[i * E + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < E; ++i)
            for (int j = 0; j < i; ++j) off += A[i * E + j] * A[i * E + j];
        if (off <= 1e-32 * scale * scale) break;
        for (int p = 0; p < E; ++p)
            for (int q = p + 1; q < E; ++q) {
                const double apq = A[p * E + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * E + q] - A[p * E + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < E; ++k) {
                    const double akp = A[k * E + p], akq = A[k * E + q];
                    A[k * E + p] = c * akp - sn * akq;
                    A[k * E + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < E; ++k) {
                    const double apk = A[p * E + k], aqk = A[q * E + k];
                    A[p * E + k] = c * apk - sn * aqk;
                    A[q * E + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < E; ++k) {
                    const double vkp = V[k * E + p], vkq = V[k * E + q];
                    V[k * E + p] = c * vkp - sn * vkq;
                    V[k * E + q] = sn * vkp + c * vkq;
                }
            }
    }
    double lmax = 0.0;
    for (int i = 0; i < E; ++i) lmax = std::max(lmax, A[i * E + i]);
    for (int i = 0; i < E; ++i)
        if (A[i * E + i] < -1e-12 * std::max(lmax, scale)) return -1;
    std::vector<int> keep;
    for (int i = 0; i < E; ++i)
        if (A[i * E + i] > 1e-15 * lmax) keep.push_back(i);
    const int r = (int)keep.size();
    F.assign((size_t)E * std::max(r, 1), 0.0);
    for (int k = 0; k < r; ++k) {
        const double sq = std::sqrt(A[keep[k] * E + keep[k]]);
        for (int e = 0; e < E; ++e) F[(size_t)e * r + k] = V[e * E + keep[k]] * sq;
    }
    return r;
}

}  // namespace pilco
