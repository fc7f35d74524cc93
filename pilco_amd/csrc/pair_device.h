// Device code of the O(N^2) pair sums shared by the pair kernels (pair.hip) and the one-launch small step of the fused head
// (prep_device.h): the per-wave tile loop (pair_wave) and the closed forms of the stream-K work split.  Internal; gfx950 only.
#pragma once
#include "mm_device.h"

namespace pilco {

// ------------------------------------------------------------------ pair kernel, MFMA
// Work item of a workgroup: (local pair, 64-row tile, column block); the four
// waves take consecutive column sub-ranges of JW columns.  Per 16-column step a
// wave issues 4*KC MFMAs (four 16-row tiles) and 16 exps per lane.
//
// a != b : S_num += beta_a,i beta_b,j L_ij; 16 per-row accumulators, beta_a applied at the end.
// a == b : L_aa and (beta beta^T - iK_a) are symmetric, so only column steps at or right of the
//          64x64 diagonal block are evaluated (weight 2 right of it): half the exps and half the
//          iK stream.  S_num += (beta_i beta_j - iK_ij) L_ij, one accumulator per result register.
#ifndef PAIR_RT
#define PAIR_RT 2      // 16-row MFMA tiles per wave (rows per work item = 16 * PAIR_RT); 2 measured best
#endif
// ablation switches for kernel experiments (tools/): never defined in product builds
#if !defined(PILCO_DEV) && defined(PAIR_ABL)
#error "PAIR_ABL is a developer experiment: build with -DPILCO_DEV (tools/ only)"
#endif
#ifndef PAIR_ABL
#define PAIR_ABL 0
#endif
#if PAIR_ABL == 2
#define PAIR_ABL_TAB(v) (1.0 + 1e-9 * (double)(__double2loint(tt[i]) & (FEXP_TN - 1)))
#else
#define PAIR_ABL_TAB(v) (v)
#endif
#if PAIR_ABL == 3
#define PAIR_ABL_MFMA(a_, b_, e_) (d4{e_[0] + a_ * b_, e_[1] - a_, e_[2] + b_, e_[3] * 0.5})
#else
#define PAIR_ABL_MFMA(a_, b_, e_) __builtin_amdgcn_mfma_f64_16x16x4f64(a_, b_, e_, 0, 0, 0)
#endif
#ifndef PAIR_PF
#define PAIR_PF 2      // operand prefetch distance in 16-column steps
#endif
#ifndef PAIR_FAIR
#define PAIR_FAIR 1    // the stream-K waves lower their issue priority as they advance (WaveProgress); 0: A/B builds
#endif
#ifndef PAIR_MINW
#define PAIR_MINW 1    // __launch_bounds__ min waves per SIMD for the pair kernel
#endif
// FENCE: an s_nop between the MFMA chain of a tile and the first VALU read of its result (MFMA_RESULT_FENCE, mm_device.h).
// The pair kernels do not need it (the compiler keeps 7 + p slots there); inside the fused head, under its register
// budget, the same source has been seen scheduled with reads of destination pairs 2 and 3 one slot early
// (tools/mfma_hazard_check.py, tests/test_build_isa.py), so that host asks for the fence.
// Operands in global memory (po: the layout of MMWork::At / Wt): every row of the column operand is reached through ONE buffer
// resource (base po.Wt) and a per-lane row offset computed once per call -- the w rows of the pair's column block, the ones,
// v_j, the zeros --, so the hot loop is what it was when every pair had its own copy of all KP rows.
// LDSOP (the one-launch step of small models, prep_device.h): the operands never went to memory -- At / Bt / vcol point into
// the workgroup's LDS, At as [k][lda] over the workgroup's own rows (row i0 is its row i0l), Bt as [k][ldb] over all columns
// (all KP rows materialised there); po is not used.
// The exp table of a pair kernel's workgroup, on its way from memory while the first tile's operands are requested: the
// kernel REQUESTS its entry (one per thread) at its very top and hands it to the first pair_wave call of each wave, which
// stores it and meets the other waves at the workgroup's barrier only after its own operand requests have left (the table is
// first read by the first exp, a whole MFMA chain later).  Loading table -> barrier -> operands in sequence was two memory
// round trips in a row at the start of every launch.
struct TabArrival {
    static constexpr int NV = (FEXP_TN + 255) / 256;   // entries per thread of a 256-thread workgroup
    double v[NV];    // this thread's table entries (requested, perhaps not yet arrived)
    double* lds;     // the table in LDS
    bool pending;    // not stored yet (wave-uniform)
#ifdef PAIR_START_STAMP   // developer build (tools/pair_start.py): where this lane stamps "first operand requests issued", or nullptr
    unsigned long long* stamp;
#endif
    __device__ __forceinline__ void request(const double* __restrict__ g, double* l) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = (FEXP_TN % 256 == 0 || threadIdx.x + 256 * k < FEXP_TN) ? g[threadIdx.x + 256 * k] : 0.0;
        lds = l;
        pending = true;
#ifdef PAIR_START_STAMP
        stamp = nullptr;
#endif
    }
    __device__ __forceinline__ void land() {
        if (pending) {
#pragma unroll
            for (int k = 0; k < NV; ++k)
                if (FEXP_TN % 256 == 0 || threadIdx.x + 256 * k < FEXP_TN) lds[threadIdx.x + 256 * k] = v[k];
            __syncthreads();
            pending = false;
        }
    }
};
// Progress of a stream-K wave through its share of the line, turned into its issue priority.  The SIMD's arbiter serves the
// OLDEST wave first: of the three waves a SIMD hosts the first finished after 24 us, the second after 38, the third after 50
// (tools/pair_waves.py) -- and a lone wave cannot keep the fp64 pipe busy (dependent MFMA -> exp -> accumulate chains), so the
// last quarter of every launch ran at two thirds of the rate.  A wave that is ahead now yields: priority 3 for the first
// quarter of its steps down to 0 for the last, so the waves of a SIMD stay within a quarter of each other and the pipe has
// work from all of them until the end (headline 409 -> 417 rollouts/s in one A/B call).  Finer slices -- the four
// priorities cycled 8, 16, 32 times per share -- measured WORSE (410, 409, 399): waves in lock-step want the matrix cores
// and the VALU at the same moments.
#ifndef PAIR_FAIR_LEVELS
#define PAIR_FAIR_LEVELS 4     // priority levels used (2..4): level = L - 1 - floor(L done / total)
#endif
struct WaveProgress {
    int done, total, level;
    __device__ __forceinline__ void tick(int steps) {
        done += steps;
        const int lv = (PAIR_FAIR_LEVELS - 1) - min(PAIR_FAIR_LEVELS - 1, (PAIR_FAIR_LEVELS * done) / max(total, 1));
        if (lv != level) {   // (wave-uniform)
            level = lv;
            if (lv == 3) __builtin_amdgcn_s_setprio(3);
            else if (lv == 2) __builtin_amdgcn_s_setprio(2);
            else if (lv == 1) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
    }
};
// BTAB: the exp table is the biased one (exponent inserted into the table value, fexp_finish: the pair kernels); false: the
// unbiased copy the fused head keeps in LDS (fexp_finish_ub, see fexp_table_unbias in mm_device.h)
template <int KC, bool DIAG, bool VSEP, bool FENCE = false, bool LDSOP = false, bool BTAB = true>
__device__ __forceinline__ double pair_wave(const PairOps& po, const double* __restrict__ At, const double* __restrict__ Bt,
                                            const double* __restrict__ vcol,
                                            const double* __restrict__ beta_a, const double* __restrict__ beta_b,
                                            const double* __restrict__ iKa, const double* __restrict__ tab, int npad, int i0,
                                            int jbeg, int jend, int lane, int lda = 0, int ldb = 0, int i0l = 0, TabArrival* ta = nullptr, WaveProgress* wp = nullptr) {
    constexpr int NE = 4 * PAIR_RT;  // exponent values per lane per 16-column step
    static_assert(PAIR_PF == 2, "the column loop is unrolled over a two-slot operand ring");
    const int lr = lane >> 4, lc = lane & 15;
    double af[PAIR_RT][KC];
#pragma unroll
    for (int rt = 0; rt < PAIR_RT; ++rt)
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            if (LDSOP) af[rt][c] = At[(4 * c + lr) * lda + i0l + 16 * rt + lc];
            else af[rt][c] = po.At[(long)(4 * c + lr) * npad + i0 + 16 * rt + lc];
        }
    double acc[NE];
    double bi[NE];
    unsigned ik_off[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        acc[i] = 0.0;
        const int row = i0 + 16 * (i >> 2) + lr + 4 * (i & 3);
        bi[i] = beta_a[row];
        ik_off[i] = ((unsigned)(row - i0) * (unsigned)npad + (unsigned)lc) * 8u;   // relative to row i0: < 32 rows
    }
    unsigned b_off[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        b_off[c] = ((unsigned)(4 * c + lr) * (unsigned)npad + (unsigned)lc) * 8u;   // relative to the pair's column block (po.w0 rides in the scalar offset)
        if (!VSEP && !LDSOP && 4 * c + lr == po.D + 1) b_off[c] = po.v0 - po.w0 + (unsigned)lc * 8u;   // the lanes of row D + 1: the pair's own v_j
    }
    const unsigned bb_off = (unsigned)lc * 8u;
    const unsigned sB = LDSOP ? 0u : po.w0, sV = LDSOP ? 0u : po.v0;   // scalar byte offsets of the column block / of v_j (VSEP) in the resource
    const __amdgpu_buffer_rsrc_t rB = buf_rsrc(LDSOP ? beta_b : po.Wt), rbeta = buf_rsrc(beta_b);   // (LDSOP: rB is never used)
    const __amdgpu_buffer_rsrc_t rIK = buf_rsrc(DIAG ? iKa + (long)i0 * npad : beta_b);
    if (DIAG && jbeg < i0) jbeg = i0;  // columns left of the diagonal block are mirrored by the transposed tile
    double total = 0.0;
    // software pipeline: the operands of the column step two ahead are requested while this one is
    // evaluated (a first touch of Bt / beta misses the XCD's L2: ~2 us, more than one step)
    double ring[2][KC + 2];   // column operand fragments, beta_b,j and (VSEP) v_j
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int c = 0; c <= KC + 1; ++c) ring[p][c] = 0.0;
        if (jbeg + 16 * p < jend) {
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                if (LDSOP) ring[p][c] = Bt[(4 * c + lr) * ldb + jbeg + 16 * p + lc];
                else ring[p][c] = buf_ld(rB, b_off[c], sB + (unsigned)(jbeg + 16 * p) * 8u);
            }
            ring[p][KC] = buf_ld(rbeta, bb_off, (unsigned)(jbeg + 16 * p) * 8u);
            if (VSEP) {
                if (LDSOP) ring[p][KC + 1] = vcol[jbeg + 16 * p + lc];
                else ring[p][KC + 1] = buf_ld(rB, bb_off, sV + (unsigned)(jbeg + 16 * p) * 8u);
            }
        }
    }
#ifdef PAIR_START_STAMP
    if (ta && ta->pending && ta->stamp) *ta->stamp = wall_clock64();
#endif
    if (ta) ta->land();   // (the requests above are in flight; see TabArrival)
    // one 16-column step on ring slot rg; the slot is refilled with the operands of column step j0 + 32
    auto step = [&](double (&rg)[KC + 2], const int j0) {
        double bf[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) bf[c] = rg[c];
        const double bb = rg[KC];
        const double vv = rg[KC + 1];
        double ik[NE];
        if (DIAG) {
#pragma unroll
            for (int i = 0; i < NE; ++i) ik[i] = buf_ld(rIK, ik_off[i], (unsigned)j0 * 8u);
        }
        // exponent tiles: C/D layout of the f64 MFMA is col = lane & 15, row = (lane >> 4) + 4 * reg
        double x[NE], tt[NE], tv[NE], pm[NE];
#pragma unroll
        for (int rt = 0; rt < PAIR_RT; ++rt) {
            d4 e = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int c = 0; c < KC; ++c) e = PAIR_ABL_MFMA(af[rt][c], bf[c], e);
            MFMA_KEEP_ALIVE(af[rt][0]);   // (first MFMA of the chain: constant-zero accumulator, see mm_device.h)
            MFMA_KEEP_ALIVE(bf[0]);
            if (FENCE) MFMA_RESULT_FENCE(e);
#pragma unroll
            for (int r = 0; r < 4; ++r) x[4 * rt + r] = VSEP ? e[r] + vv : e[r];   // C/D column = lane & 15: one v_j per lane
        }
        if (PAIR_ABL != 4 && j0 + 32 < jend) {
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                if (LDSOP) rg[c] = Bt[(4 * c + lr) * ldb + j0 + 32 + lc];
                else rg[c] = buf_ld(rB, b_off[c], sB + (unsigned)(j0 + 32) * 8u);
            }
            rg[KC] = buf_ld(rbeta, bb_off, (unsigned)(j0 + 32) * 8u);
            if (VSEP) {
                if (LDSOP) rg[KC + 1] = vcol[j0 + 32 + lc];
                else rg[KC + 1] = buf_ld(rB, bb_off, sV + (unsigned)(j0 + 32) * 8u);
            }
        }
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            x[i] = fexp_clamp(x[i]);
            tt[i] = fexp_t(x[i]);
        }
#pragma unroll
        for (int i = 0; i < NE; ++i) tv[i] = PAIR_ABL_TAB(tab[__double2loint(tt[i]) & (FEXP_TN - 1)]);
#if !(PAIR_OPT & 4)
        __builtin_amdgcn_sched_barrier(0);
#endif
        // Horner stages across all NE elements at once: NE independent fp64 chains per wave
        double rr[NE];
#pragma unroll
        for (int i = 0; i < NE; ++i) rr[i] = fma(tt[i] - FEXP_MAGIC, -FEXP_LN2_64, x[i]);
        if (FEXP_DEG == 5) {
#pragma unroll
            for (int i = 0; i < NE; ++i) pm[i] = fma(rr[i], 1.0 / 120.0, 1.0 / 24.0);
#pragma unroll
            for (int i = 0; i < NE; ++i) pm[i] = fma(rr[i], pm[i], 1.0 / 6.0);
#pragma unroll
            for (int i = 0; i < NE; ++i) pm[i] = fma(rr[i], pm[i], 0.5);
        } else if (FEXP_DEG == 4) {
#pragma unroll
            for (int i = 0; i < NE; ++i) pm[i] = fma(rr[i], 1.0 / 24.0, 1.0 / 6.0);
#pragma unroll
            for (int i = 0; i < NE; ++i) pm[i] = fma(rr[i], pm[i], 0.5);
        } else {
#pragma unroll
            for (int i = 0; i < NE; ++i) pm[i] = fma(rr[i], 1.0 / 6.0, 0.5);
        }
#pragma unroll
        for (int i = 0; i < NE; ++i) pm[i] = fma(rr[i], pm[i], 1.0);
#pragma unroll
        for (int i = 0; i < NE; ++i) pm[i] = rr[i] * pm[i];
        __builtin_amdgcn_sched_barrier(0);
#if PAIR_ABL == 1
#pragma unroll
        for (int i = 0; i < NE; ++i) { tv[i] = x[i]; pm[i] = 0.0; tt[i] = 0.0; }
#define FEXP_FINISH(a_, b_, c_) (a_)
#else
#define FEXP_FINISH(a_, b_, c_) (BTAB ? fexp_finish(a_, b_, c_) : fexp_finish_ub(a_, b_, c_))
#endif
        if (DIAG) {
            double st[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < NE; ++i)
                st[i & 3] = fma(fma(bi[i], bb, -ik[i]), FEXP_FINISH(tv[i], pm[i], tt[i]), st[i & 3]);
            const double wgt = (j0 >= i0 + 16 * PAIR_RT) ? 2.0 : 1.0;
            total = fma(wgt, (st[0] + st[1]) + (st[2] + st[3]), total);
        } else {
#pragma unroll
            for (int i = 0; i < NE; ++i) acc[i] = fma(bb, FEXP_FINISH(tv[i], pm[i], tt[i]), acc[i]);
        }
    };
    for (int j0 = jbeg; j0 < jend; j0 += 32) {
        if (wp) wp->tick(2);
        step(ring[0], j0);
        if (j0 + 16 < jend) step(ring[1], j0 + 16);
    }
    if (!DIAG) {
#pragma unroll
        for (int i = 0; i < NE; ++i) total = fma(bi[i], acc[i], total);
    }
    return total;
}

// Stream-K form of the same computation: the column steps of all local (pair, row tile)
// rows are laid out on one line and cut into sk_waves equal ranges, so that every resident
// wave does the same number of 16-column steps (no tail, no per-tile launch overhead).
// A range touches at most two pairs; each wave writes one partial per touched pair.
// first column step of wave w: the cost line (diagonal steps weigh sk_ud units, the others sk_uo)
// is cut into sk_waves equal parts; a step belongs to the wave in whose part it starts.
// floor(a / b) for 0 <= a < 2^52, 0 < b: one fp64 division and an exact integer fix-up (the emulated 64-bit integer
// division is ~10x slower, and these quotients sit at the head of the glue kernel's critical path)
__host__ __device__ inline long div_floor(long a, long b) {
    long q = (long)((double)a / (double)b);
    while (q * b > a) --q;
    while ((q + 1) * b <= a) ++q;
    return q;
}
__host__ __device__ inline int sk_boundary_of(int w, int waves, int nd_steps, int total, int ud, int uo) {
    const long Ud = (long)nd_steps * ud;
    const long C = Ud + (long)(total - nd_steps) * uo;
    if (w >= waves) return total;
    const long x = div_floor((long)w * C, waves);
    if (x <= Ud) return (int)div_floor(x + ud - 1, ud);
    return nd_steps + (int)div_floor(x - Ud + uo - 1, uo);
}
// inverse: the last wave whose first step is <= x  (boundary(w) <= x  <=>  floor(w C / waves) <= cost(x))
__host__ __device__ inline int sk_wave_of(long x, int waves, int nd_steps, int total, int ud, int uo) {
    const long Ud = (long)nd_steps * ud;
    const long C = Ud + (long)(total - nd_steps) * uo;
    const long cx = (x <= nd_steps) ? x * ud : Ud + (x - nd_steps) * uo;
    long w = div_floor((cx + 1) * waves + C - 1, C) - 1;
    if (w > waves - 1) w = waves - 1;
    return (int)w;
}
// waves holding partials of local pair k: first wave, its slot for this pair, last wave
__host__ __device__ inline void sk_pair_waves(int k, int waves, int nd, int tdiag, int toff, int total, int ud, int uo,
                                              int& wlo, int& fslot, int& whi) {
    const long S0 = (k < nd) ? (long)k * tdiag : (long)nd * tdiag + (long)(k - nd) * toff;
    const long S1 = S0 + ((k < nd) ? tdiag : toff);
    const int nd_steps = nd * tdiag;
    wlo = sk_wave_of(S0, waves, nd_steps, total, ud, uo);
    fslot = sk_boundary_of(wlo, waves, nd_steps, total, ud, uo) < S0 ? 1 : 0;   // a wave that starts before the pair holds it second
    whi = sk_wave_of(S1 - 1, waves, nd_steps, total, ud, uo);
}
// the most local pairs one wave's range touches (sk_wave_range keeps the sums of two): a cut that exceeds two loses sums
inline int sk_max_pairs_per_wave(int waves, int nd, int tdiag, int toff, int n_pairs, int ud, int uo) {
    const int nd_steps = nd * tdiag, total = nd_steps + (n_pairs - nd) * toff;
    auto pair_of = [&](int step) { return step < nd_steps ? step / tdiag : nd + (step - nd_steps) / toff; };
    int most = 0;
    for (int w = 0; w < waves; ++w) {
        const int b0 = sk_boundary_of(w, waves, nd_steps, total, ud, uo), b1 = sk_boundary_of(w + 1, waves, nd_steps, total, ud, uo);
        const int n = pair_of(b1 - 1) - pair_of(b0) + 1;
        if (b1 > b0 && n > most) most = n;
    }
    return most;
}
// ---- the same cut without a division (SkCut, moment.h).  Everything the cut divides by is a constant of the workspace, so
// the host makes, per divisor d >= 2, the multiplier m = ceil(2^(32 + sh) / d) with 2^sh < d <= 2^(sh + 1): then
// floor(n / d) = mulhi(n, m) >> sh for every n <= 2^31 (the error term n (m d - 2^(32 + sh)) stays below 2^(32 + sh)), and
// m < 2^32.  sk_cut_make checks every range the forms below rely on and clears `fast` where one does not hold (a divisor of 1,
// a cost line of 2^31 or more, more than 46340 waves: w cr would pass 2^31, more points than the root forms are tested for:
// npad > 8192); the kernel then keeps the division forms.
// tests/test_sk_cut_fast_cpu.py compares every form with the ones above over all shapes.
#ifndef SK_SQRTF   // the square root of the two closed forms: one v_sqrt_f32 (1 ulp) on the device; both have an integer fix-up
#ifdef __HIP_DEVICE_COMPILE__
#define SK_SQRTF(x_) __builtin_amdgcn_sqrtf(x_)
#else
#define SK_SQRTF(x_) sqrtf(x_)
#endif
#endif
__host__ __device__ inline unsigned sk_mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
__host__ __device__ inline unsigned sk_div(unsigned n, unsigned m, unsigned sh) { return sk_mulhi(n, m) >> sh; }
inline bool sk_magic_make(unsigned d, unsigned& m, unsigned& sh) {
    m = 0;
    sh = 0;
    if (d < 2 || d > (1u << 30)) return false;
    while ((2u << sh) < d) ++sh;
    m = (unsigned)((((unsigned long long)1 << (32 + sh)) + d - 1) / d);
    return true;
}
inline SkCut sk_cut_make(int waves, int nd, int tdiag, int toff, int total, int ud, int uo, int npad) {
    SkCut c{};
    c.waves = waves; c.total = total; c.nd = nd; c.tdiag = tdiag; c.toff = toff; c.ud = ud; c.uo = uo;
    const long nd_steps = (long)nd * tdiag;
    const long Ud = nd_steps * ud;
    const long C = Ud + ((long)total - nd_steps) * uo;
    c.nd_steps = (unsigned)nd_steps;
    c.ns = (unsigned)(npad / 16);
    const SkCut slow = c;
    if (waves < 2 || waves > 46340 || C <= 0 || C + ud + uo >= (1L << 31) || total <= 0 || npad < 32 || npad % 16) return slow;
    // the two closed forms with a root work on integers that fp32 must hold exactly: b^2 and 2 PAIR_RT q (q < tdiag) below 2^24
    // (npad <= 65504; tests/test_sk_cut_fast_cpu.py runs them over all arguments up to npad = 8192), 8 q + 1 of a pair index likewise
    {
        const double b = (double)(npad / 16) + 0.5 * PAIR_RT;
        if (b * b > 16777216.0 || 2.0 * PAIR_RT * (double)tdiag > 16777216.0 || npad > 8192) return slow;
    }
    unsigned sw, sud, suo, std_, sto, sns;
    bool ok = sk_magic_make((unsigned)waves, c.m_waves, sw);
    ok = sk_magic_make((unsigned)ud, c.m_ud, sud) && ok;
    ok = sk_magic_make((unsigned)uo, c.m_uo, suo) && ok;
    ok = sk_magic_make((unsigned)tdiag, c.m_tdiag, std_) && ok;
    ok = sk_magic_make((unsigned)toff, c.m_toff, sto) && ok;
    ok = sk_magic_make((unsigned)(npad / 16), c.m_ns, sns) && ok;
    if (!ok) return slow;
    // the inverse: the wave of a cost x is ceil((x + 1) waves / C) - 1; ((x + 1) m_inv) >> s is less than one below
    // (x + 1) waves / C as long as C < 2^s, and the product stays below 2^63
    int s = 47;
    while (s > 0 && (((unsigned long long)waves << s) / (unsigned long long)C) >> 32) --s;
    if (C >= (1L << s)) return slow;
    c.m_inv = (unsigned)(((unsigned long long)waves << s) / (unsigned long long)C);
    c.cq = (unsigned)(C / waves);
    c.cr = (unsigned)(C % waves);
    c.Ud = (unsigned)Ud;
    c.sh0 = sw | sud << 8 | suo << 16 | std_ << 24;
    c.sh1 = sto | sns << 8 | (unsigned)s << 16;
    c.fast = 1;
    return c;
}
// floor(w C / waves), w <= waves
__host__ __device__ inline unsigned sk_cost_of_wave(const SkCut& c, unsigned w) {
    return w * c.cq + sk_div(w * c.cr, c.m_waves, c.sh0 & 255u);
}
__host__ __device__ inline int sk_boundary_fast(const SkCut& c, int w) {
    if (w >= c.waves) return c.total;
    const unsigned x = sk_cost_of_wave(c, (unsigned)w);
    if (x <= c.Ud) return (int)sk_div(x + (unsigned)c.ud - 1u, c.m_ud, (c.sh0 >> 8) & 255u);
    return (int)(c.nd_steps + sk_div(x - c.Ud + (unsigned)c.uo - 1u, c.m_uo, (c.sh0 >> 16) & 255u));
}
// sk_wave_of: the last wave whose first step is <= x -- an estimate from the inverse multiplier, at most one above, then down
// along the forward form (exactly the wave the division form names: floor(w C / waves) <= cost(x) is its definition)
__host__ __device__ inline int sk_wave_of_fast(const SkCut& c, unsigned x) {
    const int waves = c.waves;
    const unsigned cx = (x <= c.nd_steps) ? x * (unsigned)c.ud : c.Ud + (x - c.nd_steps) * (unsigned)c.uo;
    unsigned w = (unsigned)(((unsigned long long)(cx + 1u) * c.m_inv) >> ((c.sh1 >> 16) & 255u)) + 1u;
    if (w > (unsigned)waves - 1u) w = (unsigned)waves - 1u;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (sk_cost_of_wave(c, w) > cx) --w;   // (never below 0: the cost of wave 0 is 0)
    return (int)w;
}
// first step of local pair k on the line
__host__ __device__ inline unsigned sk_pair_start(const SkCut& c, int k) {
    return (k < c.nd) ? (unsigned)k * (unsigned)c.tdiag : c.nd_steps + (unsigned)(k - c.nd) * (unsigned)c.toff;
}
// row tile of column step q of a diagonal pair: tile t starts at P(t) = t ns - PAIR_RT t (t - 1) / 2 (its row lost the columns
// left of its diagonal block), so t = floor((b - sqrt(b^2 - 2 PAIR_RT q)) / PAIR_RT), b = ns + PAIR_RT / 2 -- all integers
// below 2^24, exact in fp32 up to the root itself -- and one step of integer fix-up either way
__host__ __device__ inline int sk_tile_start(int t, int ns) { return t * ns - PAIR_RT * (t * (t - 1) / 2); }
__host__ __device__ inline int sk_row_tile(int q, int ns) {
    const float b = (float)ns + 0.5f * (float)PAIR_RT;
    const float disc = b * b - (float)(2 * PAIR_RT) * (float)q;
    int t = (int)((b - SK_SQRTF(disc > 0.0f ? disc : 0.0f)) * (1.0f / (float)PAIR_RT));
    if (t < 0) t = 0;
    if (sk_tile_start(t, ns) > q) --t;
    if (sk_tile_start(t + 1, ns) <= q) ++t;
    return t;
}
// decode of a step of the line: local pair, row tile, column step of the row and the steps left in the row
__host__ __device__ inline void sk_decode_fast(const SkCut& c, int step, int& pl, int& ti, int& sidx, int& cnt) {
    const int ns = (int)c.ns, nd = c.nd, tdiag = c.tdiag, toff = c.toff;
    if ((unsigned)step < c.nd_steps) {
        pl = (int)sk_div((unsigned)step, c.m_tdiag, (c.sh0 >> 24) & 255u);
        int q = step - pl * tdiag;
        ti = sk_row_tile(q, ns);
        q -= sk_tile_start(ti, ns);
        sidx = ti * PAIR_RT + q;
        cnt = ns - PAIR_RT * ti - q;
    } else {
        const unsigned r = (unsigned)step - c.nd_steps;
        const unsigned k = sk_div(r, c.m_toff, c.sh1 & 255u);
        const unsigned q = r - k * (unsigned)toff;
        pl = nd + (int)k;
        ti = (int)sk_div(q, c.m_ns, (c.sh1 >> 8) & 255u);
        sidx = (int)q - ti * ns;
        cnt = ns - sidx;
    }
}
// the division form of the same decode (what sk_wave_range did inline; kept for shapes with fast == 0 and as the reference)
__host__ __device__ inline void sk_decode_ref(const SkCut& g, int step, int& pl, int& ti, int& sidx, int& cnt) {
    const int NS = (int)g.ns, nd = g.nd, tdiag = g.tdiag, toff = g.toff, nd_steps = (int)g.nd_steps;
    int q;
    if (step < nd_steps) {
        pl = step / tdiag;
        q = step - pl * tdiag;
        ti = 0;
        int c = NS;
        while (q >= c) {
            q -= c;
            ++ti;
            c -= PAIR_RT;
        }
        sidx = ti * PAIR_RT + q;
        cnt = c - q;
    } else {
        const int r = step - nd_steps;
        pl = nd + r / toff;
        q = r - (pl - nd) * toff;
        ti = q / NS;
        sidx = q - ti * NS;
        cnt = NS - sidx;
    }
}
// outputs (a >= b) of order index kk (local_pair_ab without its loop): a (a - 1) / 2 <= kk - E < a (a + 1) / 2
__host__ __device__ inline void sk_pair_ab_fast(int kk, int E, int& a, int& b) {
    if (kk < E) {
        a = b = kk;
        return;
    }
    const int q = kk - E;
    int t = (int)((1.0f + SK_SQRTF((float)(8 * q + 1))) * 0.5f);
    if (t < 1) t = 1;
    if (t * (t - 1) / 2 > q) --t;
    if ((t + 1) * t / 2 <= q) ++t;
    a = t;
    b = q - t * (t - 1) / 2;
}
inline SkMagic sk_magic_of(const SkCut& c) {
    SkMagic m{};
    m.fast = c.fast; m.cq = c.cq; m.cr = c.cr; m.Ud = c.Ud; m.m_waves = c.m_waves; m.m_ud = c.m_ud; m.m_uo = c.m_uo;
    m.m_tdiag = c.m_tdiag; m.m_toff = c.m_toff; m.m_ns = c.m_ns; m.m_inv = c.m_inv; m.sh0 = c.sh0; m.sh1 = c.sh1;
    return m;
}
// The kernel's copy of the cut: read from the kernel-argument segment of a kernel with the parameters (MMModel, MMWork, ...)
// -- uniform loads that hit the scalar cache: kernarg_warm has requested the lines -- every time it is asked for: at the wave's
// start, at a segment change, at the wave's end.  None of its words is held across the column loop.
typedef const __attribute__((address_space(4))) char* SkArgPtr;
__device__ __forceinline__ SkArgPtr sk_cut_argptr() { return (SkArgPtr)__builtin_amdgcn_kernarg_segment_ptr(); }
__device__ __forceinline__ SkCut sk_cut_arg(SkArgPtr ka) {
    asm volatile("" : "+s"(ka));   // (a read of its own: not merged with an earlier one whose registers would have to live on)
    typedef const __attribute__((address_space(4))) int* IP;
    typedef const __attribute__((address_space(4))) unsigned* UP;
    // LAYOUT: the kernel's first two parameters are (MMModel, MMWork) BY VALUE -- k_mm_pair_sk and k_sk_cut_probe (pair.hip) say so
    // at their heads; the argument segment holds them in order at their natural alignment (tests/test_gpu_sk_cut.py reads the
    // result back through the probe)
    static_assert(std::is_standard_layout<MMModel>::value && std::is_standard_layout<MMWork>::value, "offsetof into the argument segment");
    static_assert(std::is_trivially_copyable<MMModel>::value && std::is_trivially_copyable<MMWork>::value, "passed by value, bit for bit");
    static_assert(alignof(MMModel) == 8 && alignof(MMWork) == 8, "the second parameter starts at round_up(sizeof(MMModel), 8)");
    static_assert(sizeof(MMWork) - (offsetof(MMWork, skm) + sizeof(SkMagic)) < alignof(MMWork) && offsetof(MMWork, skm) % 4 == 0, "SkMagic is the last block of MMWork");
    static_assert(sizeof(((MMWork*)nullptr)->sk_waves) == 4 && sizeof(((MMModel*)nullptr)->npad) == 4, "read as 32-bit words");
    constexpr size_t WK = (sizeof(MMModel) + alignof(MMWork) - 1) / alignof(MMWork) * alignof(MMWork);   // the second parameter
    SkCut c;
    c.waves = *(IP)(ka + WK + offsetof(MMWork, sk_waves));
    c.total = *(IP)(ka + WK + offsetof(MMWork, sk_total));
    c.nd = *(IP)(ka + WK + offsetof(MMWork, sk_nd));
    c.tdiag = *(IP)(ka + WK + offsetof(MMWork, sk_tdiag));
    c.toff = *(IP)(ka + WK + offsetof(MMWork, sk_toff));
    c.ud = *(IP)(ka + WK + offsetof(MMWork, sk_ud));
    c.uo = *(IP)(ka + WK + offsetof(MMWork, sk_uo));
    c.ns = (unsigned)(*(IP)(ka + offsetof(MMModel, npad))) >> 4;
    c.nd_steps = (unsigned)(c.nd * c.tdiag);
    const UP m = (UP)(ka + WK + offsetof(MMWork, skm));
    c.fast = m[0]; c.cq = m[1]; c.cr = m[2]; c.Ud = m[3]; c.m_waves = m[4]; c.m_ud = m[5]; c.m_uo = m[6];
    c.m_tdiag = m[7]; c.m_toff = m[8]; c.m_ns = m[9]; c.m_inv = m[10]; c.sh0 = m[11]; c.sh1 = m[12];
    return c;
}
__host__ __device__ inline int sk_boundary(const SkCut& c, int w) {
    if (c.fast) return sk_boundary_fast(c, w);
    return sk_boundary_of(w, c.waves, (int)c.nd_steps, c.total, c.ud, c.uo);
}
__host__ __device__ inline void sk_decode(const SkCut& c, int step, int& pl, int& ti, int& sidx, int& cnt) {
    if (c.fast) sk_decode_fast(c, step, pl, ti, sidx, cnt);
    else sk_decode_ref(c, step, pl, ti, sidx, cnt);
}
// slot of a wave's FIRST touched pair p0 in the slot-major partial array: w - (first wave of the pair)
__host__ __device__ inline int sk_first_slot(const SkCut& c, int w, int p0) {
    if (c.fast) return w - sk_wave_of_fast(c, sk_pair_start(c, p0));
    const long S0 = (p0 < c.nd) ? (long)p0 * c.tdiag : (long)c.nd * c.tdiag + (long)(p0 - c.nd) * c.toff;
    return w - sk_wave_of(S0, c.waves, (int)c.nd_steps, c.total, c.ud, c.uo);
}
// One wave's share of the stream-K line (see k_mm_pair_sk): the 16-column steps [boundary(w), boundary(w + 1)) of the
// cost line, touching at most two local pairs p0, p1 (-1: none) with the sums out0, out1 (before the wave reduction).
template <int KC, bool VSEP, bool FENCE = false>
__device__ __forceinline__ void sk_wave_range(const MMModel& md, const MMWork& wk, SkArgPtr skp, const double* __restrict__ tab, int w, int lane,
                                              double& out0, double& out1, int& p0, int& p1, TabArrival* ta = nullptr, bool fair = false) {
    const int npad = md.npad;
    SkCut c = sk_cut_arg(skp);
    int step = sk_boundary(c, w);
    const int end = sk_boundary(c, w + 1);
    WaveProgress prog{0, end - step, -1};
    WaveProgress* wp = fair ? &prog : nullptr;
    out0 = 0.0;
    out1 = 0.0;
    p0 = -1;
    p1 = -1;
    double cur = 0.0;
    int cur_pl = -1;
    while (step < end) {
        int pl, ti, sidx, cnt;
        const bool dg = step < (int)c.nd_steps;
        sk_decode(c, step, pl, ti, sidx, cnt);
        const int seg = (cnt < end - step) ? cnt : (end - step);
        if (pl != cur_pl) {
            if (cur_pl >= 0) {  // a range touches at most two pairs
                out0 = cur;
                p0 = cur_pl;
            }
            cur_pl = pl;
            cur = 0.0;
        }
        int a, b;
        if (c.fast) sk_pair_ab_fast(pl * wk.nranks + wk.rank, md.E, a, b);
        else local_pair_ab(wk, md.E, pl, a, b);
        const PairOps po = pair_ops(wk, md.D, npad, pl, b);
        const double* beta_a = md.beta + mm_beta_row(md, a) * npad;
        const double* beta_b = md.beta + mm_beta_row(md, b) * npad;
        const int i0 = ti * 16 * PAIR_RT, jbeg = sidx * 16, jend = jbeg + seg * 16;
        if (dg)
            cur += pair_wave<KC, true, VSEP, FENCE>(po, nullptr, nullptr, nullptr, beta_a, beta_b, md.iK + mm_ik_blk(md, a) * npad * npad, tab, npad, i0, jbeg, jend, lane, 0, 0, 0, ta, wp);
        else
            cur += pair_wave<KC, false, VSEP, FENCE>(po, nullptr, nullptr, nullptr, beta_a, beta_b, nullptr, tab, npad, i0, jbeg, jend, lane, 0, 0, 0, ta, wp);
        step += seg;
        if (step < end) c = sk_cut_arg(skp);   // (the next segment's decode: read again behind the column loop)
    }
    if (cur_pl >= 0) {
        if (p0 < 0) {
            out0 = cur;
            p0 = cur_pl;
        } else {
            out1 = cur;
            p1 = cur_pl;
        }
    }
}

}  // namespace pilco
